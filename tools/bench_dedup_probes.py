"""Times the multi-probe dedup -- acav_kmeans_probes (the m nearest centres of every row) and acav_rows_probedup (the earlier rows
of the m probed clusters, every pair in float64 on the f64 matrix core) -- at the scale the `dedup` verb is run at, beside the
figures it is to be read against, measured in the same process: acav_rows_neardup's pair rate (the stage loop is the same one)
and acav_kmeans_quality's time (the probes kernel is its sweep plus the lists).

    python tools/bench_dedup_probes.py [--n 1000000] [--d 1024] [--k 256,1024] [--m 1,2,4,8] [--window 0.5] [--rounds 2]
                                       [--out profiles/dedup_probes_1gpu.json]

Rows are randn, the centres k of the rows plus 0.25 randn (a Lloyd state: the labels are the nearest centres), the lists
KMeans.probe_centers'.  Every shape is warmed up with one call, then timed with device events over windows of at least --window
seconds of back-to-back calls; the rounds alternate between all shapes of a k.  A call includes everything the entry point does
(checks, the host's sort of the entries, the norms, the sweep, the fold).

Prints one JSON line; per k: neardup, quality, probes_m<M> (the kernel at the largest m) and probedup_m<m>, each with
  ms          the window's time / its calls, per round
  pairs       the pairs compared (dedup.probe_pairs; neardup: sum_c n_c (n_c - 1) / 2)
  pair_rate   pairs * 2 d / time in Tflop/s: the useful multiply-adds
  plan        the entry point's _plan for this device; blocks_vs_neardup = its blocks / (m x neardup's blocks)"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", default="256,1024")
    ap.add_argument("--m", default="1,2,4,8")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd import _lib
    from acav100m_amd.clustering import KMeans
    from acav100m_amd.clustering.dedup import probe_pairs
    lib = _lib.load_library()
    cus = C.c_int(0)
    _lib.check(lib.acav_device_info(0, None, 0, C.byref(cus), None))
    n, d = args.n, args.d
    ks, ms = [int(v) for v in args.k.split(",")], [int(v) for v in args.m.split(",")]
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(n, d, device="cuda", generator=gen)
    best = torch.empty(n, dtype=torch.float64, device="cuda")
    partner = torch.empty(n, dtype=torch.int64, device="cuda")
    before = np.arange(n, dtype=np.int64)
    row = {"n": n, "d": d, "cus": cus.value, "window_s": args.window, "k": {}}

    def window(call):
        """ms per call over a window of at least args.window seconds, by device events around the (blocking) calls"""
        calls, total = 0, 0.0
        while total < args.window * 1e3:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            total += e0.elapsed_time(e1)
            calls += 1
        return total / calls, calls

    for k in ks:
        pick = torch.randperm(n, device="cuda", generator=gen)[:k]
        centres = (x[pick] + 0.25 * torch.randn(k, d, device="cuda", generator=gen)).cpu().numpy()
        km = KMeans(None, d, k).to_lloyd(centres).to("cuda:0")
        labels, _ = km.calc_best(x, need_mean=False)
        lab = labels.cpu().numpy().astype(np.int64)
        hist = np.bincount(lab, minlength=k).astype(np.int64)
        plan = (C.c_int64 * 6)()
        _lib.check(lib.acav_rows_neardup_plan(_lib.ptr(hist), k, d, cus.value, plan, None, 0))
        base_blocks = int(plan[2])
        h = km._require_handle()
        stats = np.empty((k, 6), np.float64)
        rows = torch.empty(n, 2, dtype=torch.float64, device="cuda")
        lists = torch.empty(n, max(ms), dtype=torch.int64, device="cuda")
        dist = torch.empty(n, max(ms), dtype=torch.float64, device="cuda")
        qplan, pplan = (C.c_int64 * 4)(), (C.c_int64 * 4)()
        _lib.check(lib.acav_kmeans_quality_plan(n, k, cus.value, qplan))
        _lib.check(lib.acav_kmeans_probes_plan(n, k, cus.value, pplan))
        shapes = [
            ("neardup", lambda: _lib.check(lib.acav_rows_neardup(0, _lib.ptr(x), n, d, _lib.ptr(labels), k, _lib.ptr(best),
                                                                 _lib.ptr(partner), None)),
             int((hist * (hist - 1) // 2).sum()), {"plan": [int(v) for v in plan]}),
            ("quality", lambda: _lib.check(lib.acav_kmeans_quality(h, _lib.ptr(x), n, _lib.ptr(labels), _lib.ptr(stats), _lib.ptr(rows))),
             None, {"plan": [int(v) for v in qplan]}),
            ("probes_m{}".format(max(ms)), lambda: _lib.check(lib.acav_kmeans_probes(h, _lib.ptr(x), n, _lib.ptr(labels), max(ms),
                                                                                      _lib.ptr(lists), _lib.ptr(dist))),
             None, {"plan": [int(v) for v in pplan]}),
        ]
        full = km.probe_centers(x, max(ms), labels)
        for m in ms:
            pr = np.ascontiguousarray(full[:, :m])
            each = torch.empty(n, m, dtype=torch.float64, device="cuda")
            pplan6 = (C.c_int64 * 6)()
            _lib.check(lib.acav_rows_probedup_plan(_lib.ptr(pr), n, m, _lib.ptr(lab), n, _lib.ptr(before), k, d, cus.value, pplan6, None, 0))

            def call(pr=pr, m=m, each=each):
                _lib.check(lib.acav_rows_probedup(0, _lib.ptr(x), n, _lib.ptr(x), n, d, _lib.ptr(pr), m, _lib.ptr(lab), _lib.ptr(before), k,
                                                  _lib.ptr(best), _lib.ptr(partner), _lib.ptr(each), None))
            shapes.append(("probedup_m{}".format(m), call, probe_pairs(pr, lab, before),
                           {"plan": [int(v) for v in pplan6], "blocks_vs_neardup": pplan6[2] / (m * base_blocks)}))
        out = row["k"][str(k)] = {"largest_cluster_share": float(hist.max() / n)}
        for name, call, pairs, info in shapes:  # warm up every shape
            call()
            out[name] = dict(info, pairs=pairs, rounds=[])
        for r in range(args.rounds):  # all shapes of this k alternate
            for name, call, pairs, _info in shapes:
                t, calls = window(call)
                entry = {"ms": t, "calls": calls}
                if pairs is not None:
                    entry["pair_rate_tflops"] = pairs * 2.0 * d / t / 1e9
                out[name]["rounds"].append(entry)
                print("k {} round {} {:<14} {:10.3f} ms  {}  ({} calls)".format(
                    k, r, name, t, "{:7.2f} Tflop/s".format(entry["pair_rate_tflops"]) if pairs is not None else "", calls),
                    file=sys.stderr, flush=True)
        del km, lists, dist, rows
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
