"""Times the two sweeps of clustering.whiten at the size of a real view -- 1M x 1024 fp32 rows on the device -- against the
K = 256 assign sweep over the same rows in the same process, which reads the same n d 4 bytes once.

    python tools/bench_whiten.py [--n 1000000] [--d 1024] [--repeat 20] [--segments 1,1000] [--out profiles/whiten_1gpu.json]

Prints one JSON line:
  colstats_ms[segments]   acav_colstats (the tile sweep, the fold, the copy of the moments back): median wall time of a call,
                          which returns when the results are in place, once per segment count (equal segments of n / segments rows)
  rows_scale_ms           acav_rows_scale in place (reads and writes the bytes): median wall time of a call
  assign_ms               acav_kmeans_assign with mean_dist == NULL between acav_kmeans_timer_begin / _end: median
  *_of_assign             the ratios the sweeps are judged by (stats <= 1.5, scale <= 3), *_GBps the bytes they move over the time
Every shape is warmed up with three calls first; medians of --repeat calls."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--segments", default="1,1000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd import _lib
    from acav100m_amd.clustering import ColumnMoments, KMeans, whiten_
    n, d, K = args.n, args.d, args.k
    gen = torch.Generator(device="cuda").manual_seed(7)
    cen = torch.randn(K, d, device="cuda", generator=gen)
    comp = torch.randint(0, K, (n,), device="cuda", generator=gen)
    x = torch.empty(n, d, device="cuda")
    for s in range(0, n, 65536):
        e = min(n, s + 65536)
        x[s:e] = cen[comp[s:e]] + 0.3 * torch.randn(e - s, d, device="cuda", generator=gen)
    torch.cuda.synchronize()
    lib = _lib.load_library()
    nbytes = n * d * 4
    row = {"n": n, "d": d, "K": K, "repeat": args.repeat, "colstats_ms": {}, "colstats_of_assign": {}, "colstats_GBps": {}}

    def median_ms(fn):
        for _ in range(3):
            fn()
        times = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times)

    # the yardstick: the assign sweep of a trained K-centre clustering over the same rows
    acav100m_amd.manual_seed(3)
    km = KMeans(None, d, K).to("cuda:0")
    km.train_epoch(x[:262144], 32, lr=0.01)
    lab = torch.empty(n, dtype=torch.long, device="cuda")

    def assign():
        _lib.check(lib.acav_kmeans_timer_begin(km._h))
        _lib.check(lib.acav_kmeans_assign(km._h, _lib.ptr(x), n, _lib.ptr(lab), None))
        ms = C.c_float(0)
        _lib.check(lib.acav_kmeans_timer_end(km._h, C.byref(ms)))
        return ms.value
    for _ in range(3):
        assign()
    row["assign_ms"] = statistics.median(assign() for _ in range(args.repeat))
    row["assign_GBps"] = nbytes / row["assign_ms"] / 1e6

    std = None
    for nseg in (int(v) for v in args.segments.split(",")):
        prefix = np.linspace(0, n, nseg + 1).astype(np.int64)
        moments = np.empty((nseg, 2, d), np.float64)

        def stats():
            _lib.check(lib.acav_colstats(0, _lib.ptr(x), n, d, _lib.ptr(prefix), nseg, _lib.ptr(moments), None))
        ms = median_ms(stats)
        row["colstats_ms"][str(nseg)] = ms
        row["colstats_of_assign"][str(nseg)] = ms / row["assign_ms"]
        row["colstats_GBps"][str(nseg)] = nbytes / ms / 1e6
        cm = ColumnMoments(d, "cuda:0")
        for s in range(nseg):
            cm.add_segment(int(prefix[s + 1] - prefix[s]), moments[s, 0], moments[s, 1])
        std = cm.std()
    ones = np.ones(d, np.float32)  # dividing by 1 costs what dividing by std costs, and the rows stay what they are
    row["rows_scale_ms"] = median_ms(lambda: whiten_(x, ones))
    row["rows_scale_of_assign"] = row["rows_scale_ms"] / row["assign_ms"]
    row["rows_scale_GBps"] = 2 * nbytes / row["rows_scale_ms"] / 1e6
    row["std_min_max"] = [float(std.min()), float(std.max())]
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
