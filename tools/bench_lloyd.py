"""Times one iteration of clustering.algorithm=lloyd at the size of a real view -- 1M x 1024 fp32 rows on the device -- split
into its assign sweep, its accumulate sweep (acav_lloyd_accumulate) and its host part, against the acav_colstats sweep over the
same rows in the same process: the project's read-once HBM-bound pass, which reads the same n d 4 bytes.

    python tools/bench_lloyd.py [--n 1000000] [--d 1024] [--ks 256,1024] [--repeat 10] [--out profiles/lloyd_1gpu.json]

Prints one JSON line.  Per K and label shape ("even": the labels a Gaussian mixture of K components gets from its own centres,
"skewed": the same with half of all rows moved into cluster 0):
  assign_ms       acav_kmeans_assign with mean_dist == NULL between acav_kmeans_timer_begin / _end (lloyd hyper-parameters)
  accumulate_ms   acav_lloyd_accumulate into int64 tables on the device: wall time of a call, which returns when the tables are
                  up to date (histogram, host scan, index, chunked sums)
  host_ms         the centre step, wall time of lloyd.finish_iteration: acav_lloyd_centers on the device tables and a device-to-
                  device copy into the handle (with an empty cluster: the tables to the host, centres in float64, the
                  empty-cluster rule, upload);  host_ms_min / host_ms_max: the extremes of the same --repeat calls
  iteration_ms    their sum;  accumulate_of_colstats: the ratio the accumulate sweep is judged by;  *_GBps: n d 4 bytes over the time
  absmax_ms       the read-once sweep before the first iteration (acav_rows_absmax), once per run
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
    ap.add_argument("--ks", default="256,1024")
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd import _lib
    from acav100m_amd.clustering import KMeans, accumulate, fixed_point_shift, rows_absmax
    from acav100m_amd.clustering.lloyd import finish_iteration
    n, d = args.n, args.d
    ks = [int(v) for v in args.ks.split(",")]
    lib = _lib.load_library()
    nbytes = n * d * 4
    row = {"n": n, "d": d, "repeat": args.repeat, "runs": {}}

    def median_ms(fn):
        for _ in range(3):
            fn()
        times = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
        median_ms.last = times
        return statistics.median(times)

    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.empty(n, d, device="cuda")
    for K in ks:
        cen = torch.randn(K, d, device="cuda", generator=gen)
        comp = torch.randint(0, K, (n,), device="cuda", generator=gen)
        for s in range(0, n, 65536):
            e = min(n, s + 65536)
            x[s:e] = cen[comp[s:e]] + 0.3 * torch.randn(e - s, d, device="cuda", generator=gen)
        torch.cuda.synchronize()
        if "colstats_ms" not in row:  # the yardstick and the pre-pass, once: neither depends on K
            prefix = np.array([0, n], np.int64)
            moments = np.empty((1, 2, d), np.float64)
            row["colstats_ms"] = median_ms(lambda: _lib.check(lib.acav_colstats(0, _lib.ptr(x), n, d, _lib.ptr(prefix), 1, _lib.ptr(moments), None)))
            row["colstats_GBps"] = nbytes / row["colstats_ms"] / 1e6
            row["absmax_ms"] = median_ms(lambda: rows_absmax(x))
            row["absmax_GBps"] = nbytes / row["absmax_ms"] / 1e6
        shift = fixed_point_shift(rows_absmax(x), n)
        km = KMeans(None, d, K).to_lloyd(cen.cpu().numpy()).to("cuda:0")
        lab = torch.empty(n, dtype=torch.long, device="cuda")

        def assign():
            _lib.check(lib.acav_kmeans_timer_begin(km._h))
            _lib.check(lib.acav_kmeans_assign(km._h, _lib.ptr(x), n, _lib.ptr(lab), None))
            ms = C.c_float(0)
            _lib.check(lib.acav_kmeans_timer_end(km._h, C.byref(ms)))
            return ms.value
        for _ in range(3):
            assign()
        assign_ms = statistics.median(assign() for _ in range(args.repeat))
        even = lab.clone()
        skewed = even.clone()
        skewed[torch.randperm(n, device="cuda", generator=gen)[:n // 2]] = 0
        for name, labels in (("even", even), ("skewed", skewed)):
            sums = torch.zeros((K, d), dtype=torch.int64, device="cuda")
            counts = torch.zeros(K, dtype=torch.int64, device="cuda")

            def acc():
                sums.zero_()
                counts.zero_()
                accumulate(x, labels, shift, sums, counts)
            acc_ms = median_ms(acc)
            acc()
            state = km.state_arrays()
            host_ms = median_ms(lambda: finish_iteration(km, sums, counts, shift))
            host_min, host_max = min(median_ms.last), max(median_ms.last)
            km.load_state_arrays(*state)
            sizes = counts.cpu().numpy()
            row["runs"]["K%d_%s" % (K, name)] = {
                "assign_ms": assign_ms, "accumulate_ms": acc_ms, "host_ms": host_ms, "host_ms_min": host_min, "host_ms_max": host_max, "iteration_ms": assign_ms + acc_ms + host_ms,
                "accumulate_of_colstats": acc_ms / row["colstats_ms"], "accumulate_GBps": nbytes / acc_ms / 1e6,
                "assign_GBps": nbytes / assign_ms / 1e6, "largest_cluster": int(sizes.max()), "median_cluster": float(np.median(sizes))}
        del km
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
