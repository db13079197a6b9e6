"""Times KMeans.quality (acav_kmeans_quality: float64 distances on the f64 matrix core) on resident rows, beside the exact
fp32 assign sweep on the same rows.

    python tools/bench_kmeans_quality.py [--n 1000000] [--d 1024] [--k 256,1024] [--repeat 3]

Per K one JSON line: wall time of a quality call without and with row_stats (best of --repeat after a warm-up call; the
call returns when its results are in place), of calc_best with the mean (the exact sweep) and without (filter + re-check),
the f64 FLOP rate 2 n K d / t and its share of the MI355X's public 78.6 TFLOP/s f64 matrix peak, and the row bytes per second.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MATRIX_PEAK = 78.6e12


def best_of(fn, repeat):
    fn()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", default="256,1024")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import torch
    import acav100m_amd
    from acav100m_amd.clustering import KMeans
    acav100m_amd.configure_runtime(quiet=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    for K in [int(v) for v in a.k.split(",")]:
        cen = torch.randn(K, a.d, device="cuda", generator=g)
        x = torch.empty(a.n, a.d, device="cuda")
        for s in range(0, a.n, 65536):  # mixture rows, built in pieces
            e = min(a.n, s + 65536)
            x[s:e] = cen[torch.randint(0, K, (e - s,), device="cuda", generator=g)] + 0.5 * torch.randn(e - s, a.d, device="cuda", generator=g)
        km = KMeans(None, a.d, K).to("cuda:0")
        counts = np.full(K, 100.0, np.float32)
        counts[::8] = 1.0  # some under-used clusters: the discount is live
        km.load_state_arrays(cen.cpu().numpy(), counts, 100 * K, 0)
        labels, _ = km.calc_best(x, need_mean=False)
        t_q = best_of(lambda: km.quality(x, labels), a.repeat)
        t_qr = best_of(lambda: km.quality(x, labels, rows=True), a.repeat)
        t_exact = best_of(lambda: km.calc_best(x, need_mean=True), a.repeat)
        t_filter = best_of(lambda: km.calc_best(x, need_mean=False), a.repeat)
        flop = 2.0 * a.n * K * a.d
        print(json.dumps({"n": a.n, "d": a.d, "K": K, "quality_ms": round(t_q * 1e3, 3), "quality_rows_ms": round(t_qr * 1e3, 3),
                          "assign_exact_ms": round(t_exact * 1e3, 3), "assign_filter_ms": round(t_filter * 1e3, 3),
                          "f64_tflops": round(flop / t_q / 1e12, 2), "f64_matrix_peak_share": round(flop / t_q / F64_MATRIX_PEAK, 3),
                          "row_gbytes_per_s": round(4.0 * a.n * a.d / t_q / 1e9, 1)}), flush=True)
        del x, km


if __name__ == "__main__":
    main()
