"""batch_mi with batch.sampler=permutation and batch.sampler=draw, in one process, on the same data.

    python tools/bench_mi_draw.py [--out FILE] [--reps N] [--quick]

Every shape: one warm-up call of each sampler (code objects loaded, buffers at their final size), then N timed calls each,
alternating permutation / draw / permutation / ...  A call is timed with the host clock around run_greedy /
run_greedy_multi, which end in a device synchronise and the read-back; the handles are rebuilt (init) before every call,
outside the timed window.  Reported per shape and sampler: seconds and us per iteration (of one chunk) as median, min and max.

Shapes: bench.py's selection (V = 10^6, C = 256, P = 1, B / k = 20 / 4, subset 2 10^5); the same at B / k = 100 / 25; P = 45 at
V = 10^5; 125 chunks of 10^5 at width 1 and 16; the draw sampler alone at L = 10^5, 10^6, 10^7 with the iteration count fixed
(does an iteration's time depend on L?).  Quality: five seeds per sampler at V = 10^5, score_subset's mutual information of
each selection.  --quick: every shape a hundred times smaller (a rehearsal of the script, not a measurement).
Prints one JSON line per result and writes all of them to FILE (default profiles/mi_draw_1gpu.json)."""
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acav100m_amd.rng import Generator  # noqa: E402
from acav100m_amd.subset_selection import get_measure  # noqa: E402

argv, out_path, reps, quick = sys.argv[1:], None, 3, False
while argv:
    x = argv.pop(0)
    if x == "--out":
        out_path = argv.pop(0)
    elif x == "--reps":
        reps = int(argv.pop(0))
    elif x == "--quick":
        quick = True
    else:
        raise SystemExit("unknown argument " + x)
if out_path is None:
    out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mi_draw_1gpu.json")
SCALE = 100 if quick else 1
SAMPLERS = ("permutation", "draw")
results = []


def emit(rec):
    results.append(rec)
    print(json.dumps(rec), flush=True)


def make_data(seed, v, c, dd):
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, c, v)
    a = np.stack([np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, v)) for _ in range(dd)], 1).astype(np.int64)
    a[0] = c - 1
    return a, rs.permutation(v).astype(np.int64)


def make_measure(a, c, B, k, sampler, seed):
    return get_measure("batch_mi")(a, ncentroids=c, batch_size=B, selection_size=k, device="cuda:0", keep_unselected=True,
                                   generator=Generator(seed), sampler=sampler)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def quiet(fn, *a, **kw):
    """the measures print their progress lines: keep them out of the JSON stream"""
    saved, sys.stdout = sys.stdout, open(os.devnull, "w")
    try:
        return fn(*a, **kw)
    finally:
        sys.stdout.close()
        sys.stdout = saved


def timed_single(m, pairs, cand, subset):
    m.init(pairs, cand[1:])
    t0 = time.perf_counter()
    S, G, _, _ = quiet(m.run_greedy, subset, cand[:1])
    return time.perf_counter() - t0, S, len(G) // m.k


def bench_single(name, v, c, dd, B, k, subset, samplers=SAMPLERS):
    a, cand = make_data(0, v, c, dd)
    pairs = list(itertools.combinations(range(dd), 2))
    ms = {s: make_measure(a, c, B, k, s, 11) for s in samplers}
    for s in samplers:  # warm-up
        timed_single(ms[s], pairs, cand, min(subset, 50 * k))
    times, iters = {s: [] for s in samplers}, 0
    for rep in range(reps):
        for s in samplers:
            dt, S, iters = timed_single(ms[s], pairs, cand, subset)
            assert len(set(S)) == len(S) == subset
            times[s].append(dt)
    for s in samplers:
        emit({"shape": name, "sampler": s, "V": v, "C": c, "P": len(pairs), "B": B, "k": k, "subset": subset, "iterations": iters,
              "reps": reps, "seconds": spread(times[s]), "us_per_iteration": spread([t / iters * 1e6 for t in times[s]])})
    if len(samplers) == 2:
        p, d = statistics.median(times["permutation"]), statistics.median(times["draw"])
        emit({"shape": name, "summary": True, "permutation_over_draw": p / d, "draw_is_faster": bool(d < p)})


def bench_chunks(n, v, c, dd, B, k, subset, widths):
    cls = get_measure("batch_mi")
    pairs = list(itertools.combinations(range(dd), 2))
    data = [make_data(100 + i, v, c, dd) for i in range(n)]
    ms = {s: [make_measure(a, c, B, k, s, 500 + i) for i, (a, _) in enumerate(data)] for s in SAMPLERS}

    def run(sampler, width, sub):
        for m, (_, cand) in zip(ms[sampler], data):
            m.init(pairs, cand[1:])
        t0 = time.perf_counter()
        for g0 in range(0, n, width):
            group = list(range(g0, min(g0 + width, n)))
            if width == 1:
                quiet(ms[sampler][g0].run_greedy, sub, data[g0][1][:1])
            else:
                quiet(cls.run_greedy_multi, [ms[sampler][i] for i in group], [sub] * len(group), [data[i][1][:1] for i in group])
        return time.perf_counter() - t0

    iters = -(-subset // k)
    for width in widths:
        for s in SAMPLERS:
            run(s, width, 50 * k)
        times = {s: [] for s in SAMPLERS}
        for rep in range(reps):
            for s in SAMPLERS:
                times[s].append(run(s, width, subset))
        for s in SAMPLERS:
            emit({"shape": "chunks", "sampler": s, "chunks": n, "width": width, "V": v, "C": c, "P": len(pairs), "B": B, "k": k,
                  "subset": subset, "iterations_per_chunk": iters, "reps": reps, "seconds": spread(times[s]),
                  "us_per_chunk_iteration": spread([t / iters / n * 1e6 for t in times[s]])})
        p, d = statistics.median(times["permutation"]), statistics.median(times["draw"])
        emit({"shape": "chunks", "width": width, "summary": True, "permutation_over_draw": p / d, "draw_is_faster": bool(d < p)})


def bench_quality(v, c, dd, B, k, subset, seeds):
    a, cand = make_data(7, v, c, dd)
    pairs = list(itertools.combinations(range(dd), 2))
    for s in SAMPLERS:
        mi = []
        for seed in seeds:
            m = make_measure(a, c, B, k, s, seed)
            m.init(pairs, cand[1:])
            S, _, _, _ = quiet(m.run_greedy, subset, cand[:1])
            mi.append(float(m.score_subset(S, measures=["mutual_info"])["mutual_info"]))
        emit({"shape": "quality", "sampler": s, "V": v, "C": c, "P": len(pairs), "B": B, "k": k, "subset": subset, "seeds": list(seeds),
              "selection_mutual_info": mi, "mean": statistics.mean(mi), "min": min(mi), "max": max(mi)})
    rs = np.random.RandomState(0)
    m = make_measure(a, c, B, k, "draw", 0)
    m.init(pairs, cand[1:])
    rnd = [float(m.score_subset(rs.permutation(v)[:subset], measures=["mutual_info"])["mutual_info"]) for _ in seeds]
    emit({"shape": "quality", "sampler": "none (uniform random subsets of the same size)", "selection_mutual_info": rnd,
          "mean": statistics.mean(rnd)})


bench_single("bench.py selection", 10 ** 6 // SCALE, 256, 2, 20, 4, 2 * 10 ** 5 // SCALE)
bench_single("bench.py selection, B/k = 100/25", 10 ** 6 // SCALE, 256, 2, 100, 25, 2 * 10 ** 5 // SCALE)
bench_single("P = 45", 10 ** 5 // SCALE, 32, 10, 20, 4, 2 * 10 ** 4 // SCALE)
bench_chunks(125 if not quick else 5, 10 ** 5 // SCALE, 256, 2, 20, 4, 2 * 10 ** 4 // SCALE, (1, 16))
for L in (10 ** 5, 10 ** 6, 10 ** 7):  # the same 20 000 iterations on lists of three lengths
    bench_single("draw alone, L = %d" % L, L // SCALE, 256, 2, 20, 4, 8 * 10 ** 4 // SCALE, samplers=("draw",))
bench_quality(10 ** 5 // SCALE, 256, 2, 20, 4, 2 * 10 ** 4 // SCALE, (1, 2, 3, 4, 5))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    import torch
    json.dump({"tool": "tools/bench_mi_draw.py", "device": torch.cuda.get_device_name(0), "gpus": 1, "quick": quick, "reps": reps,
               "results": results}, f, indent=1)
    f.write("\n")
