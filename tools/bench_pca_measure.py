"""Times the two kernels of the PCA selection measures at the size of a real run -- V = 10^6 clips, D = 10 projected views,
p = 64 and 256 columns, the combination (P = 45) and bipartite (P = 25) pairings -- on rows resident on the device.

    python tools/bench_pca_measure.py [--n 1000000] [--views 10] [--p 64,256] [--repeat 20] [--k 200000]
                                      [--stream-bench tools/exp/stream_bench] [--ceiling-GBps 7100] [--out profiles/pca_measure_1gpu.json]

Prints one JSON line:
  pair_scores[p][pairing][distance]   acav_pair_scores: median over --repeat calls of the time between two events on the call's
                                      stream (ms), the wall time of the call (ms, includes the upload of the pointer table and the
                                      pair list and the final synchronisation), GBps = n D p 4 bytes (every clip's rows read once:
                                      the kernel's floor) over the event time, and of_ceiling = GBps / the read ceiling
  rank_desc                           acav_rank_desc of the n scores, k = --k: the same two times
  ceiling_GBps                        the read ceiling: the best read-only stream of tools/exp/stream_bench on THIS box when
                                      --stream-bench names the built program (hipcc --offload-arch=gfx950 -O3 -o tools/exp/stream_bench
                                      tools/exp/stream_bench.hip), else --ceiling-GBps (default: the
                                      figure the project recorded with it, profiles/r03_stream_bench.txt)
Every shape is warmed up with three calls first."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stream_ceiling(program, n, d):
    """the largest 'TB/s (med)' figure among the program's `flat` streams (plain coalesced 16-byte loads of the whole matrix,
    read once from HBM), in GB/s"""
    out = subprocess.run([program, str(n), str(d)], capture_output=True, text=True, timeout=600).stdout
    rates = [float(m.group(1)) for line in out.splitlines() if line.startswith("flat ")
             for m in re.finditer(r"([0-9.]+) TB/s \(med\)", line)]
    if not rates:
        raise RuntimeError("no 'TB/s (med)' line in the output of {}".format(program))
    return max(rates) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--p", default="64,256")
    ap.add_argument("--k", type=int, default=200_000)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--stream-bench", default=None)
    ap.add_argument("--ceiling-GBps", type=float, default=7100.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import itertools
    import torch
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd.subset_selection.measures.pca import DISTANCE_CODES, pair_scores, rank_desc
    n, D = args.n, args.views
    pairings = {"combination": list(itertools.combinations(range(D), 2)),
                "bipartite": list(itertools.product(range(D // 2), range(D // 2, D)))}
    ceiling = stream_ceiling(args.stream_bench, n, 1024) if args.stream_bench else args.ceiling_GBps
    row = {"n": n, "views": D, "repeat": args.repeat, "ceiling_GBps": ceiling,
           "ceiling_from": "stream_bench on this device" if args.stream_bench else "given", "pair_scores": {}}

    def timed(fn):
        for _ in range(3):
            fn()
        ev, wall = [], []
        for _ in range(args.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        return statistics.median(ev), statistics.median(wall)

    gen = torch.Generator(device="cuda").manual_seed(11)
    scores = None
    for p in (int(v) for v in args.p.split(",")):
        views = [torch.randn(n, p, device="cuda", generator=gen) for _ in range(D)]
        nbytes = n * D * p * 4
        row["pair_scores"][str(p)] = {}
        for pname, pairs in pairings.items():
            cell = row["pair_scores"][str(p)][pname] = {"pairs": len(pairs)}
            for kind in DISTANCE_CODES:
                ev, wall = timed(lambda: pair_scores(views, pairs, kind))
                cell[kind] = {"event_ms": ev, "wall_ms": wall, "GBps": nbytes / ev / 1e6, "of_ceiling": nbytes / ev / 1e6 / ceiling}
        scores = pair_scores(views, pairings["combination"], "cosine_similarity")
        del views
    k = min(args.k, n)
    ev, wall = timed(lambda: rank_desc(scores, k))
    row["rank_desc"] = {"k": k, "event_ms": ev, "wall_ms": wall}
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
