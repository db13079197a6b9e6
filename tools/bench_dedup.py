"""Times acav_rows_neardup -- for every row the largest cosine to an earlier row of its cluster, every such pair in float64 on the
f64 matrix core -- at the scale the `dedup` verb is run at, beside its yardstick: acav_rows_silhouette at M = 32 768 (the set-up
of tools/bench_silhouette.py: Gaussian-mixture rows, labels = the component), the same operand path with more work per pair.

    python tools/bench_dedup.py [--n 1000000] [--d 1024] [--k 256] [--cfg5_k 1024] [--window 1.0] [--rounds 3]
                                [--out profiles/dedup_1gpu.json]

Label histograms at (n, d, k): `balanced` (labels uniform over k) and `zipf` (cluster c drawn with weight 1 / (c + s), s chosen so
that the largest cluster holds about 10 % of the rows: the balance of the tile list shows here); `cfg5` is the balanced histogram
at --cfg5_k, skipped when the rows do not fit on the device.  Every shape is warmed up with one call, then timed with device
events on the stream the library runs on, over windows of at least --window seconds of back-to-back calls; --rounds rounds
alternate between the dedup shapes and the silhouette yardstick in the same process.  A call includes everything the entry point
does: the label and value checks, the host's sort of the positions, the norms and the sweep.

Prints one JSON line; per shape and round:
  ms          the window's time / its calls
  pairs       the (row, earlier row of the same cluster) pairs of the histogram = sum_c n_c (n_c - 1) / 2; the silhouette's: M^2
  pair_rate   pairs * 2 d / time, in Tflop/s: the useful multiply-adds (the kernel computes whole 64-column blocks: `blocks` of
              the plan times tile height times 64 is what it multiplies)
  plan        acav_rows_neardup_plan / acav_rows_silhouette_plan for this device"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def zipf_weights(k, top_share):
    """weights 1 / (c + s) over c = 0 ... k - 1 with s (by bisection) such that the largest holds top_share of the mass"""
    import numpy as np
    c = np.arange(k, dtype=np.float64)
    lo, hi = 1e-6, 1e6
    for _ in range(200):
        s = (lo * hi) ** 0.5
        w = 1.0 / (c + s)
        lo, hi = (s, hi) if w[0] / w.sum() > top_share else (lo, s)
    return w / w.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--cfg5_k", type=int, default=1024)
    ap.add_argument("--sil_m", type=int, default=32768)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd import _lib
    lib = _lib.load_library()
    cus = C.c_int(0)
    _lib.check(lib.acav_device_info(0, None, 0, C.byref(cus), None))
    n, d = args.n, args.d
    gen = torch.Generator(device="cuda").manual_seed(7)
    free, _total = torch.cuda.mem_get_info()
    row = {"n": n, "d": d, "cus": cus.value, "window_s": args.window, "shapes": {}}
    if 4 * n * d + 4 * args.sil_m * d + (1 << 30) > free:
        raise SystemExit("{} rows x {} columns do not fit on the device ({} bytes free)".format(n, d, free))
    x = torch.randn(n, d, device="cuda", generator=gen)
    best = torch.empty(n, dtype=torch.float64, device="cuda")
    partner = torch.empty(n, dtype=torch.int64, device="cuda")

    def window(call):
        """ms per call over a window of at least args.window seconds, by device events on the library's stream"""
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

    shapes = []
    for name, k, weights in (("balanced", args.k, None), ("zipf", args.k, zipf_weights(args.k, 0.10)), ("cfg5", args.cfg5_k, None)):
        if weights is None:
            labels = torch.randint(0, k, (n,), device="cuda", generator=gen)
        else:
            labels = torch.multinomial(torch.from_numpy(weights).to("cuda", torch.float32), n, replacement=True, generator=gen)
        hist = np.bincount(labels.cpu().numpy(), minlength=k).astype(np.int64)
        plan = (C.c_int64 * 6)()
        _lib.check(lib.acav_rows_neardup_plan(_lib.ptr(hist), k, d, cus.value, plan, None, 0))
        pairs = int((hist * (hist - 1) // 2).sum())

        def call(labels=labels, k=k):
            _lib.check(lib.acav_rows_neardup(0, _lib.ptr(x), n, d, _lib.ptr(labels), k, _lib.ptr(best), _lib.ptr(partner), None))
        shapes.append(("dedup_" + name, call, pairs, d,
                       {"k": k, "largest_cluster_share": float(hist.max() / n), "plan": [int(v) for v in plan]}))
    # the yardstick: tools/bench_silhouette.py's set-up at M = 32 768
    m, sk = args.sil_m, args.k
    slab = torch.randint(0, sk, (m,), device="cuda", generator=gen)
    centres = torch.randn(sk, d, device="cuda", generator=gen)
    sx = (centres[slab] + 0.6 * torch.randn(m, d, device="cuda", generator=gen)).contiguous()
    stats = torch.empty(m, 2, dtype=torch.float64, device="cuda")
    splan = (C.c_int64 * 9)()
    _lib.check(lib.acav_rows_silhouette_plan(m, d, sk, cus.value, splan))

    def sil():
        _lib.check(lib.acav_rows_silhouette(0, _lib.ptr(sx), m, d, _lib.ptr(slab), sk, _lib.ptr(stats), None))
    shapes.append(("silhouette_{}".format(m), sil, m * m, d, {"k": sk, "plan": [int(v) for v in splan]}))
    torch.cuda.synchronize()
    for name, call, pairs, dd, info in shapes:  # warm up every shape
        call()
        row["shapes"][name] = dict(info, pairs=pairs, rounds=[])
    for r in range(args.rounds):  # the dedup shapes and the yardstick alternate
        for name, call, pairs, dd, _info in shapes:
            ms, calls = window(call)
            rate = pairs * 2.0 * dd / ms / 1e9
            row["shapes"][name]["rounds"].append({"ms": ms, "calls": calls, "pair_rate_tflops": rate})
            print("round {} {:<18} {:10.3f} ms  {:.4g} pairs  {:7.2f} Tflop/s ({} calls)".format(r, name, ms, float(pairs), rate, calls),
                  file=sys.stderr, flush=True)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
