"""Times the k-means++ seeding (clustering.init=kmeans++, acav_kmeanspp_seed) on device-resident samples and shows what it buys
the Lloyd loop.

    python tools/bench_kmeanspp.py [--shapes 65536x1024x256,262144x1024x1024,8192x64x32] [--repeat 5]
                                   [--stream-bench tools/exp/stream_bench] [--ceiling-GBps 7100] [--out profiles/kmeanspp_1gpu.json]

Prints one JSON line.  Per shape (m, d, K) and T = 1 and 'auto' (min(16, 2 + floor(ln K))):
  seed_ms          wall time of one acav_kmeanspp_seed call (K picks, one synchronisation at its end); the shift is computed before
  us_per_pick      seed_ms / K: the sample, sweep and select kernels of a pick and the block-sum memset between them
  pick_GBps        m d 4 bytes over the time of a pick: the sweep's effective read rate INSIDE the seeding loop (a lower bound of
                   the sweep's own rate: the pick's two small kernels are in the time)
  sweep_ms, sweep_GBps   one acav_kmeanspp_weights call for T candidate rows into a device buffer (launch and one synchronisation
                   included), and m d 4 bytes over it
  regime           'cache': the sample fits the 256 MB Infinity Cache and is re-read from it pick after pick; 'hbm': it does not
  lloyd_iteration_ms   one Lloyd iteration at the same shape (assign sweep, accumulate sweep, host part), K centres
  seed_of_iteration    seed_ms / lloyd_iteration_ms
  ceiling_GBps     the read ceiling: the best read-only `flat` stream of tools/exp/stream_bench on this device when
                   --stream-bench names the built program, else --ceiling-GBps (the figure recorded with it,
                   profiles/r03_stream_bench.txt); copy_GBps: the 6.29 TB/s float4 copy figure of the MI355X
"quality": on a fixed seeded mixture (65 536 rows, d = 64, 256 components of unequal weight, Zipf-like), Lloyd from random rows,
from k-means++ seeds with T = 1 and with T = 'auto' (sample = all rows): inertia (mean squared distance to the nearest centre)
after iteration 1 and at convergence, and the number of iterations (at most --max-iters).
Every timing is warmed up with two calls first; medians of --repeat calls."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L3_BYTES = 256 << 20


def stream_ceiling(program, n, d):
    """the largest 'TB/s (med)' figure among the program's `flat` streams, in GB/s"""
    out = subprocess.run([program, str(n), str(d)], capture_output=True, text=True, timeout=600).stdout
    rates = [float(m.group(1)) for line in out.splitlines() if line.startswith("flat ")
             for m in re.finditer(r"([0-9.]+) TB/s \(med\)", line)]
    if not rates:
        raise RuntimeError("no 'TB/s (med)' line in the output of {}".format(program))
    return max(rates) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x1024x256,262144x1024x1024,8192x64x32")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-iters", type=int, default=60)
    ap.add_argument("--stream-bench", default=None)
    ap.add_argument("--ceiling-GBps", type=float, default=7100.0)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd import _lib
    from acav100m_amd.clustering import KMeans, fixed_point_shift, kmeanspp, rows_absmax
    from acav100m_amd.clustering.lloyd import finish_iteration, lloyd_update
    from acav100m_amd.rng import Generator
    lib = _lib.load_library()

    def median_ms(fn):
        for _ in range(2):
            fn()
        times = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times)

    ceiling = stream_ceiling(args.stream_bench, 262144, 1024) if args.stream_bench else args.ceiling_GBps
    row = {"repeat": args.repeat, "ceiling_GBps": ceiling, "ceiling_from": "stream_bench on this device" if args.stream_bench else "given",
           "copy_GBps": 6290.0, "shapes": {}}
    gen = torch.Generator(device="cuda").manual_seed(7)
    for shape in args.shapes.split(","):
        m, d, K = (int(v) for v in shape.split("x"))
        cen = torch.randn(K, d, device="cuda", generator=gen)
        x = torch.empty(m, d, device="cuda")
        for s in range(0, m, 65536):
            e = min(m, s + 65536)
            x[s:e] = cen[torch.randint(0, K, (e - s,), device="cuda", generator=gen)] + 0.3 * torch.randn(e - s, d, device="cuda", generator=gen)
        torch.cuda.synchronize()
        nbytes = m * d * 4
        t = kmeanspp.weight_shift(rows_absmax(x), m, d)
        res = {"m": m, "d": d, "K": K, "sample_MB": nbytes / 1e6, "regime": "cache" if nbytes <= L3_BYTES else "hbm", "shift": t}
        # one Lloyd iteration at this shape
        km = KMeans(None, d, K).to_lloyd(cen.cpu().numpy()).to("cuda:0")
        shift = fixed_point_shift(rows_absmax(x), m)
        state = km.state_arrays()

        def iteration():
            _labels, sums, counts = lloyd_update(km, x, shift)
            finish_iteration(km, sums, counts, shift)
            km.load_state_arrays(*state)
        res["lloyd_iteration_ms"] = median_ms(iteration)
        del km
        for name in ("1", "auto"):
            T = kmeanspp.trials_for(K, 1 if name == "1" else "auto")
            u = kmeanspp.uniforms(Generator(5), 1 + (K - 1) * T)
            rows, pot = np.empty(K, np.int64), np.empty(K, np.int64)

            def seed():
                _lib.check(lib.acav_kmeanspp_seed(0, _lib.ptr(x), m, d, K, T, _lib.ptr(u), t, _lib.ptr(rows), _lib.ptr(pot), None))
            seed_ms = median_ms(seed)
            cand = np.ascontiguousarray(rows[:T] if T <= K else np.resize(rows, T), np.int64)
            out = torch.empty((T, m), dtype=torch.int64, device="cuda")

            def sweep():
                _lib.check(lib.acav_kmeanspp_weights(0, _lib.ptr(x), m, d, _lib.ptr(cand), T, t, _lib.ptr(out), None))
            sweep_ms = median_ms(sweep)
            res["T" + name] = {"T": T, "seed_ms": seed_ms, "us_per_pick": seed_ms * 1e3 / K, "pick_GBps": nbytes / (seed_ms / K) / 1e6,
                               "sweep_ms": sweep_ms, "sweep_GBps": nbytes / sweep_ms / 1e6,
                               "pick_of_ceiling": nbytes / (seed_ms / K) / 1e6 / ceiling,
                               "seed_of_iteration": seed_ms / res["lloyd_iteration_ms"],
                               "potential_first": int(pot[0]), "potential_last": int(pot[-1])}
            del out
        row["shapes"][shape] = res
        del x
    if not args.no_quality:
        row["quality"] = quality(args, torch, np)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def quality(args, torch, np):
    from acav100m_amd.clustering import KMeans, fixed_point_shift, kmeanspp, rows_absmax
    from acav100m_amd.clustering.lloyd import finish_iteration, lloyd_update
    from acav100m_amd.rng import Generator
    n, d, K = 65536, 64, 256
    gen = torch.Generator(device="cuda").manual_seed(11)
    cen = torch.randn(K, d, device="cuda", generator=gen)
    weight = 1.0 / torch.arange(1, K + 1, device="cuda", dtype=torch.float32)  # Zipf-like: the last components hold ~40 rows
    comp = torch.multinomial(weight, n, replacement=True, generator=gen)
    x = cen[comp] + 0.3 * torch.randn(n, d, device="cuda", generator=gen)
    shift = fixed_point_shift(rows_absmax(x), n)

    def inertia(centers):
        c = torch.from_numpy(centers).cuda().double()
        total = 0.0
        for s in range(0, n, 8192):
            total += float(torch.cdist(x[s:s + 8192].double(), c).min(dim=1).values.pow(2).sum())
        return total / n

    out = {"n": n, "d": d, "K": K, "max_iters": args.max_iters}
    for name, trials in (("random", None), ("kmeans++_T1", 1), ("kmeans++_Tauto", "auto")):
        g = Generator(3)
        perm = g.randperm(n)
        t0 = time.perf_counter()
        if trials is None:
            start = perm[:K]
        else:
            start, _pot = kmeanspp.seed(x, K, trials, generator=g)
        seed_ms = (time.perf_counter() - t0) * 1e3
        km = KMeans(None, d, K, generator=g).to_lloyd(x[torch.from_numpy(start).cuda()].cpu().numpy()).to("cuda:0")
        prev, first, iters, splits = None, None, 0, 0
        for _it in range(args.max_iters):
            labels, sums, counts = lloyd_update(km, x, shift)
            changed = n if prev is None else int((labels != prev).sum())
            splits += finish_iteration(km, sums, counts, shift)
            prev, iters = labels, iters + 1
            if first is None:
                first = inertia(km.centers.numpy())
            if changed == 0:
                break
        out[name] = {"seed_ms": seed_ms, "inertia_after_1": first, "inertia_final": inertia(km.centers.numpy()), "iterations": iters,
                     "converged": changed == 0, "splits": splits}
        del km
    return out


if __name__ == "__main__":
    main()
