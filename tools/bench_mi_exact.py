"""Exact greedy timing: one launch per iteration, all remaining candidates scored.

    python tools/bench_mi_exact.py [V [C [D [subset]]]] [--measure NAME] [--chunks N [--sequential-only]]

NAME: any exact-greedy measure of the registry (default mem_mi; mi, ami, nmi, constant, fm, rand, arand).

--chunks N: N equal chunks of V clips each (own labels, own candidate order), selected (a) one after another, N calls of
acav_mi_run_exact, and (b) in lockstep, one call of acav_mi_run_exact_multi.  Same process, the handles rebuilt before
every run, one warm-up of each form, then two timed runs each, alternating a / b / a / b.  Prints one JSON line per run:
us per pick-iteration (wall time / picks of one chunk: what one more pick of EVERY chunk costs) and us per pick per chunk.
--sequential-only: (a) alone, through nothing but acav_mi_run_exact -- for timing a library that predates the lockstep call."""
import ctypes as C
import itertools
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acav100m_amd import _lib
from acav100m_amd.subset_selection import get_measure

argv, measure, rest, chunks, seq_only = sys.argv[1:], "mem_mi", [], 0, False
while argv:
    x = argv.pop(0)
    if x == "--measure":
        measure = argv.pop(0)
    elif x.startswith("--measure="):
        measure = x.split("=", 1)[1]
    elif x == "--chunks":
        chunks = int(argv.pop(0))
    elif x.startswith("--chunks="):
        chunks = int(x.split("=", 1)[1])
    elif x == "--sequential-only":
        seq_only = True
    else:
        rest.append(x)
argv = rest
v = int(argv[0]) if len(argv) > 0 else 100_000
c = int(argv[1]) if len(argv) > 1 else 256
dd = int(argv[2]) if len(argv) > 2 else 2
subset = int(argv[3]) if len(argv) > 3 else 5000
pairs = list(itertools.combinations(range(dd), 2))


def make_chunk(seed):
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, c, v)
    a = np.stack([np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, v)) for _ in range(dd)], 1).astype(np.int64)
    a[0] = c - 1
    return a, [int(i) for i in rs.permutation(v)]


if not chunks:
    a, cand = make_chunk(0)
    m = get_measure(measure)(a, ncentroids=c, device="cuda:0")
    m.init(pairs, cand[1:])
    m.run_greedy(10, cand[:1])  # warm-up
    m.init(pairs, cand[1:])
    t0 = time.perf_counter()
    S, G, _, _ = m.run_greedy(subset, cand[:1])
    dt = time.perf_counter() - t0
    it = len(G)
    print(json.dumps({"measure": measure, "V": v, "C": c, "D": dd, "P": len(pairs), "picks": it, "seconds": dt, "us_per_iteration": dt / it * 1e6,
                      "candidate_scores_per_s": sum(v - 1 - t for t in range(it)) * len(pairs) / dt}))
    sys.exit(0)

data = [make_chunk(s) for s in range(chunks)]
measures = [get_measure(measure)(a, ncentroids=c, device="cuda:0") for a, _ in data]
pair_measure = hasattr(measures[0], "pair_stats")  # these add their start clip to the tables first
cands = [np.ascontiguousarray(cand[1:], np.int64) for _, cand in data]
picks = max(0, min(subset - 2, v - 1))
S = [np.empty(picks + 1, np.int64) for _ in data]
G = [np.empty(picks + 1, np.float64) for _ in data]


def rebuild():
    for m, (_, cand) in zip(measures, data):
        m.init(pairs, cand[1:])
        if pair_measure:
            m.add_samples(cand[:1])
        _lib.check(_lib._lib.acav_mi_sync(m._h))


def sequential(sub):
    nsel = C.c_int64(0)
    t0 = time.perf_counter()
    for i, m in enumerate(measures):
        _lib.check(_lib._lib.acav_mi_run_exact(m._h, _lib.ptr(cands[i]), len(cands[i]), 1, sub, _lib.ptr(S[i]), _lib.ptr(G[i]),
                                               C.byref(nsel), None, None, None))
    return time.perf_counter() - t0


def parr(ptrs):
    return (C.c_void_p * chunks)(*[p.value if isinstance(p, C.c_void_p) else p for p in ptrs])


def lockstep(sub):
    L = np.full(chunks, v - 1, np.int64)
    ns = np.ones(chunks, np.int32)
    subs = np.full(chunks, sub, np.int64)
    nsel = np.zeros(chunks, np.int64)
    args = (parr([m._h for m in measures]), chunks, parr([_lib.ptr(x) for x in cands]), _lib.ptr(L), _lib.ptr(ns), _lib.ptr(subs),
            parr([_lib.ptr(x) for x in S]), parr([_lib.ptr(x) for x in G]), _lib.ptr(nsel))
    t0 = time.perf_counter()
    _lib.check(_lib._lib.acav_mi_run_exact_multi(*args))
    return time.perf_counter() - t0


forms = [("sequential", sequential)] if seq_only else [("sequential", sequential), ("lockstep", lockstep)]
for name, fn in forms:  # warm-up: code objects loaded, scratch buffers at their final size
    rebuild()
    fn(min(subset, 50))
results = {}
for rep in range(2):
    for name, fn in forms:
        rebuild()
        dt = fn(subset)
        results.setdefault(name, []).append((dt, [s[:picks].copy() for s in S], [g[:picks].copy() for g in G]))
        print(json.dumps({"form": name, "run": rep, "measure": measure, "V": v, "C": c, "D": dd, "P": len(pairs), "chunks": chunks,
                          "picks_per_chunk": picks, "seconds": dt, "us_per_pick_iteration": dt / picks * 1e6,
                          "us_per_pick_per_chunk": dt / picks / chunks * 1e6}), flush=True)
if not seq_only:
    (_, Sa, Ga), (_, Sb, Gb) = results["sequential"][0], results["lockstep"][0]
    same = all(np.array_equal(x, y) for x, y in zip(Sa, Sb)) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(Ga, Gb))
    a_runs, b_runs = [r[0] for r in results["sequential"]], [r[0] for r in results["lockstep"]]
    print(json.dumps({"summary": True, "measure": measure, "V": v, "chunks": chunks, "identical_results": bool(same),
                      "sequential_us_per_pick_per_chunk": [t / picks / chunks * 1e6 for t in a_runs],
                      "lockstep_us_per_pick_per_chunk": [t / picks / chunks * 1e6 for t in b_runs],
                      "speedup_of_means": sum(a_runs) / sum(b_runs)}), flush=True)
