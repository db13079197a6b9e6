"""Generator of tests/golden/subset_scores_large.npz: sklearn's scores at the sizes where the subset-scoring kernels start
splitting their work (several table-building workgroups per pair, the cap on them, the EMI's n_ij slices at their cap).
Needs scikit-learn (the tests do not); reads nothing but its own seeds and leaves tests/golden/subset_scores.npz and its
generator's random stream alone.

    python tests/golden/gen_subset_scores_large.py

The file holds no assignment matrix and no id list: per case <name> it holds <name>.seed, .V, .D, .C, .n, .repeats -- the
arguments of tests/_subset_scores_np.large_inputs, which rebuilds both -- and <name>.pairs [P, 2], <name>.prefix [q] (ending
at n), <name>.emi (0: adjusted_mutual_info is left out, its column of sk and dev is NaN), <name>.sk [q, P, 6], <name>.h
[q, P, 2] and <name>.dev [q, P, 6] as in subset_scores.npz.  `cases` lists the names.

The cases, by the launch shapes they reach (acav_score_plan):
    c7_n20000         distinct ids; a call of 3 table-building workgroups per pair (6667 ids each) and a prefix curve whose
                      second point adds 15000 ids from 5000 on in 2
    c143_n20000       the largest LDS table (81796 B) built by 3 workgroups
    c300_n20000       global adds on a grid of 79 x P
    c2_n300000        ids with repeats, P = 1: 37 workgroups, 128 lanes per column, n_ij ranges of ~1.5e5 over 1024 slices
    c2_n304097        the same clips, a list longer than V + 1: the ln k / ln k! tables of a handle that scored before grow
    c32_p45_n400000   P = 45: ceil(n / 8192) = 49 workgroups capped to 2048 / 45 = 45; without adjusted_mutual_info (its
                      restatement costs minutes at this size)
"""
import io
import itertools
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _subset_scores_np as R  # noqa: E402
from gen_subset_scores import sk_scores  # noqa: E402

TWO = [(0, 1), (0, 2)]
CASES = [
    # name, seed, V, D, C, n, repeats, pairs, prefix, emi
    ("c7_n20000", 101, 30000, 3, 7, 20000, False, TWO, [5000, 20000], True),
    ("c143_n20000", 102, 30000, 3, 143, 20000, False, TWO, None, True),
    ("c300_n20000", 103, 30000, 3, 300, 20000, False, TWO, None, True),
    ("c2_n300000", 104, 300000, 2, 2, 300000, True, [(0, 1)], None, True),
    ("c2_n304097", 104, 300000, 2, 2, 304097, True, [(0, 1)], None, True),
    ("c32_p45_n400000", 105, 50000, 10, 32, 400000, True, list(itertools.combinations(range(10), 2)), None, False),
]


def main():
    from sklearn.metrics.cluster import entropy
    out, names = {}, []
    for name, seed, V, D, C, n, repeats, pairs, prefix, with_emi in CASES:
        assign, ids = R.large_inputs(seed, V, D, C, n, repeats)
        prefix = np.asarray([n] if prefix is None else prefix, np.int64)
        pairs = np.asarray(pairs, np.int32)
        sk = np.zeros((len(prefix), len(pairs), 6))
        dev = np.zeros_like(sk)
        h = np.zeros((len(prefix), len(pairs), 2))
        for q, k in enumerate(prefix):
            sub = ids[:k]
            for p, (d1, d2) in enumerate(pairs):
                x, y = assign[sub, d1], assign[sub, d2]
                if with_emi:
                    sk[q, p] = sk_scores(x, y)
                else:
                    from sklearn import metrics
                    sk[q, p] = [metrics.mutual_info_score(x, y), metrics.normalized_mutual_info_score(x, y), np.nan,
                                metrics.adjusted_rand_score(x, y), metrics.fowlkes_mallows_score(x, y), metrics.rand_score(x, y)]
                h[q, p] = entropy(x), entropy(y)
                ours = R.compose(R.raw_stats(R.table(assign, sub, d1, d2, C), with_emi=with_emi))
                dev[q, p] = [abs(ours[m] - s) for m, s in zip(R.NAMES, sk[q, p])]
        out.update({name + ".seed": np.array(seed), name + ".V": np.array(V), name + ".D": np.array(D), name + ".C": np.array(C),
                    name + ".n": np.array(n), name + ".repeats": np.array(int(repeats)), name + ".emi": np.array(int(with_emi)),
                    name + ".pairs": pairs, name + ".prefix": prefix, name + ".sk": sk, name + ".h": h, name + ".dev": dev})
        names.append(name)
        worst = np.where(np.isnan(dev), -1.0, dev).max((0, 1))  # -1: a score the case leaves out
        print("{:<16} n={:<6} P={:<3} max dev: {}".format(name, n, len(pairs), " ".join("{:.1e}".format(v) for v in worst)))
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "subset_scores_large.npz")
    with zipfile.ZipFile(path, "w") as z:  # np.savez stamps its entries with the time of day: the same bytes on every run instead
        for key, value in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
