"""Times acav_rows_normalize (clustering.normalize) against acav_rows_scale -- the other in-place row sweep, which moves the same
bytes: 4 read and 4 written per element -- on the same tensor in the same process, at the sizes of two real views, and a whole
spherical Lloyd iteration (clustering.spherical) on unit rows: its assign sweep, its accumulate sweep and its centre step with
the renormalisation of the [K, d] centre table.

    python tools/bench_normalize.py [--shapes 1000000x1024,262144x2304] [--ks 256,1024] [--repeat 10] [--out profiles/normalize_1gpu.json]

Prints one JSON line:
  shapes[NxD]   rows_scale_ms, rows_normalize_ms: median wall time of a call, which returns when the rows are done;
                normalize_of_scale: the ratio the kernel is judged by (<= 1.25); *_min_max_ms: the spread of the calls;
                *_GBps: 2 n d 4 bytes over the time
  spherical[K]  on the first shape, rows normalised: assign_ms (acav_kmeans_assign between the handle's timers), accumulate_ms
                (acav_lloyd_accumulate), finish_ms / finish_plain_ms (lloyd.finish_iteration with and without spherical=True on the
                same tables), iteration_ms = assign + accumulate + finish, iteration_plain_ms with the plain centre step
Every figure: three warm-up calls, then the median of --repeat calls."""
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
    ap.add_argument("--shapes", default="1000000x1024,262144x2304")
    ap.add_argument("--ks", default="256,1024")
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd import _lib
    from acav100m_amd.clustering import KMeans, accumulate, fixed_point_shift, normalize_, rows_absmax, whiten_
    from acav100m_amd.clustering.lloyd import finish_iteration
    lib = _lib.load_library()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    ks = [int(v) for v in args.ks.split(",")] if args.ks else []
    row = {"repeat": args.repeat, "shapes": {}, "spherical": {}}

    def median_ms(fn):
        for _ in range(3):
            fn()
        times = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
        median_ms.spread = [min(times), max(times)]
        return statistics.median(times)

    gen = torch.Generator(device="cuda").manual_seed(7)
    first = None
    for n, d in shapes:
        x = torch.empty(n, d, device="cuda")
        for s in range(0, n, 65536):
            e = min(n, s + 65536)
            x[s:e] = torch.randn(e - s, d, device="cuda", generator=gen) * (10.0 ** torch.empty(e - s, 1, device="cuda").uniform_(-3, 3, generator=gen))
        torch.cuda.synchronize()
        ones = np.ones(d, np.float32)  # dividing by 1 costs what dividing by a std costs, and the rows stay what they are
        nbytes = 2 * n * d * 4
        scale_ms = median_ms(lambda: whiten_(x, ones))
        scale_spread = median_ms.spread
        norm_ms = median_ms(lambda: normalize_(x))  # (rows that are already unit cost what any rows cost)
        row["shapes"]["%dx%d" % (n, d)] = {"rows_scale_ms": scale_ms, "rows_normalize_ms": norm_ms, "normalize_of_scale": norm_ms / scale_ms,
                                           "rows_scale_min_max_ms": scale_spread, "rows_normalize_min_max_ms": median_ms.spread,
                                           "rows_scale_GBps": nbytes / scale_ms / 1e6, "rows_normalize_GBps": nbytes / norm_ms / 1e6}
        if first is None:
            first = x
        del x
    if ks:
        x = first
        n, d = x.shape
        shift = fixed_point_shift(rows_absmax(x), n)
        for K in ks:
            cen = x[torch.randperm(n, device="cuda", generator=gen)[:K]].cpu().numpy()
            km = KMeans(None, d, K).to_lloyd(cen, spherical=True).to("cuda:0")
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
            sums = torch.zeros((K, d), dtype=torch.int64, device="cuda")
            counts = torch.zeros(K, dtype=torch.int64, device="cuda")

            def acc():
                sums.zero_()
                counts.zero_()
                accumulate(x, lab, shift, sums, counts)
            acc_ms = median_ms(acc)
            acc()
            state = km.state_arrays()
            finish_ms = median_ms(lambda: finish_iteration(km, sums, counts, shift, spherical=True))
            plain_ms = median_ms(lambda: finish_iteration(km, sums, counts, shift))
            km.load_state_arrays(*state)
            row["spherical"]["K%d" % K] = {"n": n, "d": d, "assign_ms": assign_ms, "accumulate_ms": acc_ms, "finish_ms": finish_ms,
                                           "finish_plain_ms": plain_ms, "iteration_ms": assign_ms + acc_ms + finish_ms,
                                           "iteration_plain_ms": assign_ms + acc_ms + plain_ms, "empty_clusters": int((counts == 0).sum())}
            del km
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
