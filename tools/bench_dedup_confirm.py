"""Times acav_pairs_cosine -- the cosines of a pair list in a second view, the confirmation step of `dedup --dedup.confirm_view=`
-- at the scale the verb is run at, beside the emit sweep of acav_rows_neardup_pairs that produced the list, in the same process.

    python tools/bench_dedup_confirm.py [--n 1000000] [--d 1024] [--k 256] [--db 1024,2304] [--threshold 0.9] [--window 1.0]
                                        [--rounds 3] [--ceiling_tbs <TB/s>] [--out profiles/dedup_confirm_1gpu.json]

View A: tools/bench_dedup_groups.py's generator -- standard normal rows, labels uniform over k, then 0.1 %, 1 % and 10 % of the
rows (cumulatively) become bitwise copies of a source row with its label, in groups of 2 ... 50 rows.  Per share the pair list
of view A is taken once (acav_rows_neardup_pairs with room for every pair) and
  emit_ms     median(count + emit) - median(count alone) of that entry on the same rows, alternating: the sweep that wrote the list
  confirm     per width dB of view B: acav_pairs_cosine on the [R, dB] buffer of the R rows that occur in a pair (standard normal:
              the time does not depend on the values) with the pairs re-indexed into it (dedup.pair_rows), lists and cosines on
              the device -- what the verb calls.  ms: the whole call (index and value checks, the norms, the kernel);
              gather_gbs = pairs x 2 x 4 dB bytes / ms, the roof's traffic (rows that consecutive pairs share and L2 hits only
              help); ceiling_share = gather_gbs / --ceiling_tbs, the coalesced read ceiling tools/exp/stream_bench reports on
              the same device (not given: left out).
Every shape is warmed up with one call, then timed with device events over windows of at least --window seconds of back-to-back
calls, --rounds rounds alternating between the shapes; the medians are reported beside every round.  On view A's own compact
rows the cosines are compared with the list's pair_cos: bitwise_equal must be true.  Prints one JSON line."""
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
    ap.add_argument("--db", default="1024,2304")
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ceiling_tbs", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd import _lib
    from acav100m_amd.clustering.dedup import pair_rows
    lib = _lib.load_library()
    cus = C.c_int(0)
    _lib.check(lib.acav_device_info(0, None, 0, C.byref(cus), None))
    n, d, k, thr = args.n, args.d, args.k, args.threshold
    widths = [int(w) for w in args.db.split(",")]
    gen = torch.Generator(device="cuda").manual_seed(7)
    free, _total = torch.cuda.mem_get_info()
    if 4 * n * d + (1 << 30) > free:
        raise SystemExit("{} rows x {} columns do not fit on the device ({} bytes free)".format(n, d, free))
    x = torch.randn(n, d, device="cuda", generator=gen)
    labels = torch.randint(0, k, (n,), device="cuda", generator=gen)
    best = torch.empty(n, dtype=torch.float64, device="cuda")
    partner = torch.empty(n, dtype=torch.int64, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    row = {"n": n, "d": d, "k": k, "cus": cus.value, "threshold": thr, "window_s": args.window, "ceiling_tbs": args.ceiling_tbs,
           "planted": []}

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
        return total / calls

    def pairs(cap=0, pair_j=None, pair_cos=None):
        _lib.check(lib.acav_rows_neardup_pairs(0, _lib.ptr(x), n, d, _lib.ptr(labels), k, thr, _lib.ptr(best), _lib.ptr(partner),
                                               _lib.ptr(offsets), cap, _lib.ptr(pair_j), _lib.ptr(pair_cos), None))

    def cosines(rows_b, ci, cj, out):
        _lib.check(lib.acav_pairs_cosine(0, _lib.ptr(rows_b), rows_b.shape[0], rows_b.shape[1], _lib.ptr(ci), _lib.ptr(cj), ci.shape[0],
                                         _lib.ptr(out), None))

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
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
        _later, occ, ci, cj = pair_rows(offsets.cpu().numpy(), pair_j.cpu().numpy())
        ci_t, cj_t = torch.from_numpy(ci).cuda(), torch.from_numpy(cj).cuda()
        out = torch.empty(total, dtype=torch.float64, device="cuda")
        compact_a = x[torch.from_numpy(occ).cuda()]
        cosines(compact_a, ci_t, cj_t, out)
        bitwise = bool(torch.equal(out.view(torch.int64), pair_cos.view(torch.int64)))
        del compact_a
        views = [torch.randn(len(occ), w, device="cuda", generator=gen) for w in widths]
        for b in views:  # warm up
            cosines(b, ci_t, cj_t, out)
        both, count, confirm = [], [], [[] for _ in widths]
        for _r in range(args.rounds):
            both.append(window(full))
            count.append(window(pairs))
            for w, b in enumerate(views):
                confirm[w].append(window(lambda b=b: cosines(b, ci_t, cj_t, out)))
        plan = (C.c_int64 * 6)()
        _lib.check(lib.acav_pairs_cosine_plan(total, widths[0], cus.value, plan))
        entry = {"share": share, "planted_rows": planted, "pairs": total, "rows_in_pairs": int(len(occ)), "bitwise_equal": bitwise,
                 "full_ms": both, "count_ms": count, "emit_ms": med(both) - med(count), "plan": [int(v) for v in plan], "confirm": []}
        for w, ms in zip(widths, confirm):
            gbs = total * 2 * 4 * w / med(ms) * 1e-6
            c = {"db": w, "ms_rounds": ms, "ms": med(ms), "gather_bytes": total * 2 * 4 * w, "gather_gbs": gbs,
                 "ms_over_emit_ms": med(ms) / (med(both) - med(count))}
            if args.ceiling_tbs:
                c["ceiling_share"] = gbs / (1e3 * args.ceiling_tbs)
            entry["confirm"].append(c)
        row["planted"].append(entry)
        print("planted {:>5.1%}: {} pairs over {} rows; emit {:.3f} ms; confirm ".format(share, total, len(occ), entry["emit_ms"])
              + "; ".join("dB {}: {:.3f} ms = {:.0f} GB/s".format(c["db"], c["ms"], c["gather_gbs"]) for c in entry["confirm"])
              + "; bitwise equal on view A: {}".format(bitwise), file=sys.stderr, flush=True)
        del views
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
