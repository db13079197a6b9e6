"""Times acav_rows_crossdup -- for every row of a pool piece the largest cosine to a row of a resident held-out set, every pair in
float64 on the f64 matrix core -- at the scale `dedup --dedup.against_path` is run at, beside two yardsticks taken in the same
process: acav_rows_neardup on the pool piece (balanced labels at --k: the same stage loop over a triangle) and
acav_rows_silhouette at M = 32 768 (the set-up of tools/bench_silhouette.py).

    python tools/bench_dedup_against.py [--n 1000000] [--d 1024] [--k 256] [--held 16384,131072] [--held_blocked 1000000]
                                        [--window 1.0] [--rounds 3] [--out profiles/dedup_against_1gpu.json]

Shapes: `against_<m>` -- no blocking, the pool piece of n rows against the first m rows of the held-out set, n m pairs;
`against_blocked_<m>` -- both sets labelled uniformly over --k clusters, sum_c n_c m_c pairs.  Every shape is warmed up with one
call, then timed with device events on the stream the library runs on, over windows of at least --window seconds of back-to-back
calls; --rounds rounds alternate between the shapes and the yardsticks.  A call includes everything the entry point does: the
label and value checks of both sets, the host's sorts, the norms of both sets and the sweep.

Prints one JSON line; per shape and round:
  ms          the window's time / its calls
  pairs       the pairs the definition compares (neardup: sum_c n_c (n_c - 1) / 2; the silhouette's: M^2)
  pair_rate   pairs * 2 d / time, in Tflop/s: the useful multiply-adds (the kernels compute whole 64-column blocks: `blocks` of
              the plan times tile height times 64 is what they multiply)
  plan        acav_rows_crossdup_plan / acav_rows_neardup_plan / acav_rows_silhouette_plan for this device"""
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
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--held", default="16384,131072")
    ap.add_argument("--held_blocked", type=int, default=1000000)
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
    n, d, k = args.n, args.d, args.k
    held = [int(v) for v in args.held.split(",") if v]
    m_all = max(held + [args.held_blocked])
    gen = torch.Generator(device="cuda").manual_seed(7)
    free, _total = torch.cuda.mem_get_info()
    row = {"n": n, "d": d, "cus": cus.value, "window_s": args.window, "shapes": {}}
    if 4 * (n + m_all + args.sil_m) * d + (1 << 30) > free:
        raise SystemExit("{} + {} rows x {} columns do not fit on the device ({} bytes free)".format(n, m_all, d, free))
    x = torch.randn(n, d, device="cuda", generator=gen)
    y = torch.randn(m_all, d, device="cuda", generator=gen)
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

    def cross_plan(hist_x, hist_y):
        plan = (C.c_int64 * 6)()
        _lib.check(lib.acav_rows_crossdup_plan(_lib.ptr(hist_x), _lib.ptr(hist_y), len(hist_x), d, cus.value, plan, None, 0))
        return [int(v) for v in plan]

    shapes = []
    for m in held:
        def call(m=m):
            _lib.check(lib.acav_rows_crossdup(0, _lib.ptr(x), n, _lib.ptr(y), m, d, None, None, 1, _lib.ptr(best), _lib.ptr(partner), None))
        shapes.append(("against_{}".format(m), call, n * m, d,
                       {"m": m, "k": 1, "plan": cross_plan(np.array([n], np.int64), np.array([m], np.int64))}))
    labels_x = torch.randint(0, k, (n,), device="cuda", generator=gen)
    hist_x = np.bincount(labels_x.cpu().numpy(), minlength=k).astype(np.int64)
    if args.held_blocked:
        mb = args.held_blocked
        labels_y = torch.randint(0, k, (mb,), device="cuda", generator=gen)
        hist_y = np.bincount(labels_y.cpu().numpy(), minlength=k).astype(np.int64)

        def blocked():
            _lib.check(lib.acav_rows_crossdup(0, _lib.ptr(x), n, _lib.ptr(y), mb, d, _lib.ptr(labels_x), _lib.ptr(labels_y), k,
                                              _lib.ptr(best), _lib.ptr(partner), None))
        shapes.append(("against_blocked_{}".format(mb), blocked, int((hist_x * hist_y).sum()), d,
                       {"m": mb, "k": k, "plan": cross_plan(hist_x, hist_y)}))
    # the yardsticks: tools/bench_dedup.py's balanced shape on the pool piece, tools/bench_silhouette.py's set-up at M = 32 768
    nplan = (C.c_int64 * 6)()
    _lib.check(lib.acav_rows_neardup_plan(_lib.ptr(hist_x), k, d, cus.value, nplan, None, 0))

    def neardup():
        _lib.check(lib.acav_rows_neardup(0, _lib.ptr(x), n, d, _lib.ptr(labels_x), k, _lib.ptr(best), _lib.ptr(partner), None))
    shapes.append(("neardup_balanced", neardup, int((hist_x * (hist_x - 1) // 2).sum()), d, {"k": k, "plan": [int(v) for v in nplan]}))
    sm = args.sil_m
    slab = torch.randint(0, k, (sm,), device="cuda", generator=gen)
    centres = torch.randn(k, d, device="cuda", generator=gen)
    sx = (centres[slab] + 0.6 * torch.randn(sm, d, device="cuda", generator=gen)).contiguous()
    stats = torch.empty(sm, 2, dtype=torch.float64, device="cuda")
    splan = (C.c_int64 * 9)()
    _lib.check(lib.acav_rows_silhouette_plan(sm, d, k, cus.value, splan))

    def sil():
        _lib.check(lib.acav_rows_silhouette(0, _lib.ptr(sx), sm, d, _lib.ptr(slab), k, _lib.ptr(stats), None))
    shapes.append(("silhouette_{}".format(sm), sil, sm * sm, d, {"k": k, "plan": [int(v) for v in splan]}))
    torch.cuda.synchronize()
    for name, call, pairs, dd, info in shapes:  # warm up every shape
        call()
        row["shapes"][name] = dict(info, pairs=pairs, rounds=[])
    for r in range(args.rounds):  # the shapes and the yardsticks alternate
        for name, call, pairs, dd, _info in shapes:
            ms, calls = window(call)
            rate = pairs * 2.0 * dd / ms / 1e9
            row["shapes"][name]["rounds"].append({"ms": ms, "calls": calls, "pair_rate_tflops": rate})
            print("round {} {:<26} {:10.3f} ms  {:.4g} pairs  {:7.2f} Tflop/s ({} calls)".format(r, name, ms, float(pairs), rate, calls),
                  file=sys.stderr, flush=True)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
