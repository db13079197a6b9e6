"""Times acav_rows_neardup_pairs -- every pair of a cluster at cosine >= threshold, a count sweep and an emit sweep over the
tiles that hold a pair -- at the scale the `dedup` verb is run at, beside its yardstick: acav_rows_neardup on the same rows
(untouched code; the count sweep is its stage loop plus one compare per walked element), and acav_pairs_components on the host.

    python tools/bench_dedup_groups.py [--n 1000000] [--d 1024] [--k 256] [--threshold 0.9] [--window 1.0] [--rounds 3]
                                       [--out profiles/dedup_groups_1gpu.json]

Rows: standard normal, labels uniform over k (tools/bench_dedup.py's `balanced`): no pair reaches the threshold, so a call of
acav_rows_neardup_pairs is its count sweep alone.  Every shape is warmed up with one call, then timed with device events on the
stream the library runs on, over windows of at least --window seconds of back-to-back calls; --rounds rounds alternate between
acav_rows_neardup and the count sweep in the same process: `spread` is (max - min) / median of a shape's rounds.  Then 0.1 %,
1 % and 10 % of the rows (cumulatively) become bitwise copies of a source row with its label, in groups of 2 ... 50 rows; per
share the call is timed with room for every pair (count + emit) and with cap = 0 (count alone) on the same rows, alternating:
  emit_ms            their difference: the emit sweep, the upload of the offsets and of its tile list
  emit_tile_share    the tiles the emit sweep launches / the tiles of the count sweep (acav_rows_neardup_pairs_plan)
  emit_block_share   likewise for the column blocks they walk: the share of the count sweep's work the emit sweep repeats
  components_ms      acav_pairs_components on the host at that pair count (best of three)
Outputs are device buffers, so no pair crosses the bus inside the timed calls.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=0.9)
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
    n, d, k, thr = args.n, args.d, args.k, args.threshold
    gen = torch.Generator(device="cuda").manual_seed(7)
    free, _total = torch.cuda.mem_get_info()
    if 4 * n * d + (1 << 30) > free:
        raise SystemExit("{} rows x {} columns do not fit on the device ({} bytes free)".format(n, d, free))
    x = torch.randn(n, d, device="cuda", generator=gen)
    labels = torch.randint(0, k, (n,), device="cuda", generator=gen)
    best = torch.empty(n, dtype=torch.float64, device="cuda")
    partner = torch.empty(n, dtype=torch.int64, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    row = {"n": n, "d": d, "k": k, "cus": cus.value, "threshold": thr, "window_s": args.window, "shapes": {}, "planted": []}

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

    def nearest():
        _lib.check(lib.acav_rows_neardup(0, _lib.ptr(x), n, d, _lib.ptr(labels), k, _lib.ptr(best), _lib.ptr(partner), None))

    def pairs(cap=0, pair_j=None, pair_cos=None):
        _lib.check(lib.acav_rows_neardup_pairs(0, _lib.ptr(x), n, d, _lib.ptr(labels), k, thr, _lib.ptr(best), _lib.ptr(partner),
                                               _lib.ptr(offsets), cap, _lib.ptr(pair_j), _lib.ptr(pair_cos), None))

    def spread(rounds):
        ms = sorted(r["ms"] for r in rounds)
        return (ms[-1] - ms[0]) / ms[len(ms) // 2]

    torch.cuda.synchronize()
    shapes = (("neardup", nearest), ("pairs_count", pairs))
    for name, call in shapes:  # warm up
        call()
        row["shapes"][name] = {"rounds": []}
    if int(offsets[n]) != 0:
        raise SystemExit("the unplanted rows hold {} pairs at {}: raise --threshold".format(int(offsets[n]), thr))
    for r in range(args.rounds):  # the yardstick and the count sweep alternate
        for name, call in shapes:
            ms, calls = window(call)
            row["shapes"][name]["rounds"].append({"ms": ms, "calls": calls})
            print("round {} {:<12} {:10.3f} ms ({} calls)".format(r, name, ms, calls), file=sys.stderr, flush=True)
    for name, _call in shapes:
        row["shapes"][name]["spread"] = spread(row["shapes"][name]["rounds"])

    rs = np.random.RandomState(7)
    free_rows = rs.permutation(n)  # every row is planted at most once, as a source or as a copy
    used, planted = 0, 0
    for share in (0.001, 0.01, 0.1):
        src, dst = [], []
        while planted < int(share * n):
            g = int(rs.randint(2, 51))
            rows = free_rows[used:used + g]
            used += g
            src.extend([int(rows.min())] * (g - 1))
            dst.extend(int(v) for v in rows if v != rows.min())
            planted += g
        src_t, dst_t = torch.tensor(src, device="cuda"), torch.tensor(dst, device="cuda")
        x[dst_t] = x[src_t]
        labels[dst_t] = labels[src_t]
        torch.cuda.synchronize()
        pairs()  # the count call: how much room the pairs need
        total = int(offsets[n])
        pair_j = torch.empty(total, dtype=torch.int64, device="cuda")
        pair_cos = torch.empty(total, dtype=torch.float64, device="cuda")
        full = lambda: pairs(total, pair_j, pair_cos)  # noqa: E731
        full()
        both, count = [], []
        for r in range(args.rounds):
            both.append(window(full)[0])
            count.append(window(pairs)[0])
        off = offsets.cpu().numpy()
        hist = np.bincount(labels.cpu().numpy(), minlength=k).astype(np.int64)
        plain = (C.c_int64 * 6)()
        _lib.check(lib.acav_rows_neardup_plan(_lib.ptr(hist), k, d, cus.value, plain, None, 0))
        perm = np.argsort(labels.cpu().numpy(), kind='stable')
        flags = np.zeros(plain[1], np.uint8)
        flags[np.flatnonzero(np.diff(off)[perm] > 0) // plain[0]] = 1
        plan = (C.c_int64 * 7)()
        _lib.check(lib.acav_rows_neardup_pairs_plan(_lib.ptr(hist), k, d, cus.value, _lib.ptr(flags), plan, None, 0))
        pj = pair_j.cpu().numpy()
        root = np.empty(n, np.int64)
        comp_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            _lib.check(lib.acav_pairs_components(n, _lib.ptr(off), _lib.ptr(pj), _lib.ptr(root)))
            comp_ms.append(1e3 * (time.perf_counter() - t0))
        size = np.bincount(root, minlength=n)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        entry = {"share": share, "planted_rows": planted, "pairs": total, "groups": int((size >= 2).sum()),
                 "removed": int(n - (size >= 1).sum()), "full_ms": both, "count_ms": count, "emit_ms": med(both) - med(count),
                 "emit_tile_share": plan[3] / plan[1], "emit_block_share": plan[4] / plan[2], "emit_share_of_count_ms": (med(both) - med(count)) / med(count),
                 "components_ms": min(comp_ms), "plan": [int(v) for v in plan]}
        row["planted"].append(entry)
        print("planted {:>5.1%}: {} pairs, {} groups; count {:.3f} ms, count + emit {:.3f} ms; emit tiles {:.1%}, blocks {:.1%}; "
              "components {:.3f} ms".format(share, total, entry["groups"], med(count), med(both), entry["emit_tile_share"],
                                            entry["emit_block_share"], entry["components_ms"]), file=sys.stderr, flush=True)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
