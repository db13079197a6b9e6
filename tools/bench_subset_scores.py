"""Times subset scoring (EfficientBatchMI.score_subset) at the size of a real selection: n = 200 000 clips out of V = 10^6,
for (C, P) in {(256, 1), (256, 45), (1024, 45)}, with and without adjusted_mutual_info (the exact EMI).

    python tools/bench_subset_scores.py [--n 200000] [--v 1000000] [--repeat 3] [--sklearn] [--shapes 256x1,256x45,1024x45]

Per shape it prints one JSON line: the wall time of a call (best of --repeat, after one warm-up call that also builds the
ln k! table), the library's own event times of the three phases (ACAV_SCORE_TIMING: table build, marginals + per-cell sums,
EMI + finish; they arrive on stderr and are parsed from there), the number of EMI terms and the achieved terms per second, and
the label pairs per second of the table build.  --sklearn: where scikit-learn is importable, the time of its
adjusted_mutual_info_score (and the five cheap scores) on ONE pair of the same data, on the CPU.
"""
import argparse
import itertools
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_assignments(rs, v, d, c):
    comp = rs.randint(0, c, size=v)
    cols = [np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(d)]
    a = np.stack(cols, 1).astype(np.int64)
    a[0] = c - 1
    return a


def emi_terms(a, ids, pairs, c):
    """number of (cell, n_ij) terms of the exact EMI over all pairs"""
    total = 0
    n = len(ids)
    for d1, d2 in pairs:
        b = np.bincount(a[ids, d1], minlength=c)
        aa = np.bincount(a[ids, d2], minlength=c)
        b, aa = b[b > 0][:, None], aa[aa > 0][None, :]
        total += int((np.minimum(aa, b) - np.maximum(1, aa + b - n) + 1).sum())
    return total


def timed_call(m, ids, measures):
    """-> (wall seconds, {phase: ms}) of one call, the phase times parsed from the library's stderr line"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            m.score_subset(ids, measures=measures)
            wall = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode("utf-8", "replace")
    phases = {}
    for line in text.splitlines():
        if line.startswith("acav_score:"):
            for tok in line.split()[1:]:
                k, _, val = tok.partition("=")
                if k.endswith("_ms"):
                    phases[k] = float(val)
        else:
            sys.stderr.write(line + "\n")
    return wall, phases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--v", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--shapes", default="256x1,256x45,1024x45")
    ap.add_argument("--sklearn", action="store_true")
    args = ap.parse_args()
    os.environ["ACAV_SCORE_TIMING"] = "1"
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd.subset_selection.measures.batch import SCORE_NAMES, EfficientBatchMI
    cheap = [s for s in SCORE_NAMES if s != "adjusted_mutual_info"]
    for shape in args.shapes.split(","):
        c, p = (int(x) for x in shape.split("x"))
        d = 2 if p == 1 else next(k for k in range(2, 64) if k * (k - 1) // 2 >= p)
        pairs = list(itertools.combinations(range(d), 2))[:p]
        rs = np.random.RandomState(c * 1000 + p)
        a = make_assignments(rs, args.v, d, c)
        ids = rs.choice(args.v, args.n, replace=False).astype(np.int64)
        m = EfficientBatchMI(a, ncentroids=c, device="cuda:0")
        m.init(pairs, [])
        terms = emi_terms(a, ids, pairs, c)
        row = {"C": c, "P": p, "V": args.v, "n": args.n, "emi_terms": terms}
        for tag, names in (("no_ami", cheap), ("with_ami", list(SCORE_NAMES))):
            timed_call(m, ids, names)  # warm-up
            best = min((timed_call(m, ids, names) for _ in range(args.repeat)), key=lambda r: r[0])
            row[tag] = {"wall_ms": round(best[0] * 1e3, 3), **best[1]}
        build = next(v for k, v in row["with_ami"].items() if k.startswith("table_"))
        row["table_label_pairs_per_s"] = args.n * p / (build * 1e-3)
        row["emi_terms_per_s"] = terms / (row["with_ami"]["emi_finish_ms"] * 1e-3)
        if args.sklearn:
            try:
                from sklearn import metrics
                x, y = a[ids, pairs[0][0]], a[ids, pairs[0][1]]
                t0 = time.perf_counter()
                metrics.adjusted_mutual_info_score(x, y)
                row["sklearn_ami_one_pair_s"] = round(time.perf_counter() - t0, 3)
                t0 = time.perf_counter()
                for f in (metrics.mutual_info_score, metrics.normalized_mutual_info_score, metrics.adjusted_rand_score,
                          metrics.fowlkes_mallows_score, metrics.rand_score):
                    f(x, y)
                row["sklearn_other_five_one_pair_s"] = round(time.perf_counter() - t0, 3)
            except ImportError:
                row["sklearn"] = "not importable here"
        print(json.dumps(row), flush=True)
        del m


if __name__ == "__main__":
    main()
