"""Generator of tests/golden/subset_scores.npz: sklearn's six agreement scores of label columns restricted to id lists --
the expected values of the subset-scoring tests.  Needs scikit-learn (the tests do not); reads nothing but its own seeds.

    python tests/golden/gen_subset_scores.py

Per case <name> the file holds  <name>.assign (the key of a shared assignment matrix), <name>.C, <name>.pairs [P, 2],
<name>.ids [n], <name>.prefix [q] (ending at n), <name>.sk [q, P, 6] sklearn's scores in the order of
tests/_subset_scores_np.NAMES, <name>.h [q, P, 2] sklearn's entropies of the two columns, and <name>.dev [q, P, 6]: |pure float64 restatement (tests/_subset_scores_np.py) - sklearn|,
the yardstick for the device's adjusted_mutual_info bound.  `cases` lists the names.

The cases are the smallest at which each code path can go wrong: C = 1 (the one-label case), 2 (long n_ij ranges,
a + b - n > 1), 7 (no power of two), 64 (table in LDS), 143 / 144 (the last table that fits the LDS share and the first
that does not), 300 (global adds); n = 1, 2, 3, 50, 777, 2500; P = 45; an id list with repeats; a subset that leaves labels
unused; an id list longer than V (repeats: the ln k! table must reach n); one prefix curve.
"""
import itertools
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _subset_scores_np as R  # noqa: E402


def make_assign(rs, V, D, C, agree=0.7):
    """column 1 agrees with column 0 on a share of the clips; the others are independent"""
    a = rs.randint(0, C, size=(V, D))
    same = rs.rand(V) < agree
    a[same, 1] = a[same, 0]
    a[0, :] = C - 1  # the largest label occurs: C = max + 1
    return a.astype(np.int16)


def sk_scores(x, y):
    from sklearn import metrics
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return [metrics.mutual_info_score(x, y), metrics.normalized_mutual_info_score(x, y),
                metrics.adjusted_mutual_info_score(x, y), metrics.adjusted_rand_score(x, y),
                metrics.fowlkes_mallows_score(x, y), metrics.rand_score(x, y)]


def main():
    rs = np.random.RandomState(20240607)
    out, cases = {}, []

    def add(name, akey, C, pairs, ids, prefix=None):
        assign = out[akey].astype(np.int64)
        ids = np.asarray(ids, np.int64)
        prefix = np.asarray([len(ids)] if prefix is None else prefix, np.int64)
        pairs = np.asarray(pairs, np.int32)
        from sklearn.metrics.cluster import entropy
        sk = np.zeros((len(prefix), len(pairs), 6))
        dev = np.zeros_like(sk)
        h = np.zeros((len(prefix), len(pairs), 2))
        for q, k in enumerate(prefix):
            sub = ids[:k]
            for p, (d1, d2) in enumerate(pairs):
                sk[q, p] = sk_scores(assign[sub, d1], assign[sub, d2])
                h[q, p] = entropy(assign[sub, d1]), entropy(assign[sub, d2])
                ours = R.compose(R.raw_stats(R.table(assign, sub, d1, d2, C)))
                dev[q, p] = [abs(ours[m] - s) for m, s in zip(R.NAMES, sk[q, p])]
        out.update({name + ".assign": np.array(akey), name + ".C": np.array(C), name + ".pairs": pairs,
                    name + ".ids": ids.astype(np.int32), name + ".prefix": prefix, name + ".sk": sk, name + ".h": h, name + ".dev": dev})
        cases.append(name)
        print("{:<16} n={:<5} P={:<3} max dev: {}".format(name, len(ids), len(pairs),
                                                          " ".join("{:.1e}".format(v) for v in dev.max((0, 1)))))

    V = 3000
    two = [(0, 1), (0, 2)]
    for C in (1, 2, 7, 64, 143, 144):
        out["A{}".format(C)] = make_assign(rs, V, 3, C)
    for C in (1, 2, 7, 64):
        for n in (1, 2, 3, 50, 777, 2500):
            add("c{}_n{}".format(C, n), "A{}".format(C), C, two, rs.choice(V, n, replace=False))
    for C in (143, 144):
        add("c{}_n2500".format(C), "A{}".format(C), C, two, rs.choice(V, 2500, replace=False))
    out["A300"] = make_assign(rs, 5000, 3, 300)
    add("c300_n4000", "A300", 300, two, rs.choice(5000, 4000, replace=False))
    out["A32"] = make_assign(rs, V, 10, 32)
    add("c32_p45", "A32", 32, list(itertools.combinations(range(10), 2)), rs.choice(V, 1000, replace=False))
    add("c7_repeats", "A7", 7, two, rs.randint(0, V, 777))
    add("c7_long", "A7", 7, two, rs.randint(0, V, V + 517))
    a64 = out["A64"].astype(np.int64)
    few = np.nonzero((a64[:, 0] < 10) & (a64[:, 2] < 40))[0]
    add("c64_unused", "A64", 64, two, rs.permutation(few)[:200])
    add("c7_curve", "A7", 7, two, rs.choice(V, 2500, replace=False), prefix=[1, 10, 256, 257, 2500])
    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "subset_scores.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
