#!/usr/bin/env python3
"""Generate the golden vectors of the layer-weighted clustering pairs by running the REFERENCE itself (only where the
reference is mounted; what is committed is the data it produced).

    python tests/golden/gen_golden_weights.py               # every stage
    python tests/golden/gen_golden_weights.py pairing|exact|batch

pairing  weights_pairing.json: correspondence_retrieval's get_cluster_pairing(keys, pairing, weight_type)
         (cluster_pairing.py:7-21, pair_weights.py:4-50) for ten keys named like the real pipeline's (5 SlowFast + 5 VGGish
         layers), every pairing of that function and linear / log / exp with coefficients -2 .. 2 plus onehot_0 .. onehot_4.
         Per case: the pairing and the weights (float64), or the name of the exception the reference raised.
exact    weights_exact_<case>_<measure>.npz: correspondence_retrieval's EfficientMI / EfficientMemMI (measures/efficient.py,
         mem_mi.py) with the weighted dict form, on the CPU through EfficientMI.run (candidates = range(V), one start clip,
         which joins the tables before the first pick).  Per iteration: the fp32 score vector by remaining position (row t
         holds L - t values, NaN-padded), the argmax and the top-two margin; then S and GAIN.
batch    weights_batch_<case>.npz: correspondence_retrieval's EfficientBatchMI (measures/batch.py) with the weighted dict form,
         keep_unselected=True, torch.manual_seed(seed): per iteration the batch ids, the fp32 batch scores (scores.mean(-1)),
         the top-k positions; then S and GAIN.  Sizes keep every batch at B (its calc_ids has no short-batch rule).

The reference's stages clash on top-level module names, so each stage runs in its own interpreter.
"""
import itertools
import json
import os
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
STUBS = os.path.join(HERE, "_stubs")
CODE = os.path.join(REF, "correspondence_retrieval", "code")

# the ten clusterings of the real pipeline, sorted as dataloader.format_assignments sorts them: (model, layer)
KEYS = [(m, "layer_{}".format(i)) for m in ("SlowFast", "VGGish") for i in range(5)]
PAIRINGS = ("combination", "bipartite", "diagonal", "layer_0", "penultimate")
COEFFS = ("-2", "-1", "-0.5", "0", "0.5", "1", "2")
WEIGHT_TYPES = ["{}_{}".format(f, c) for f in ("linear", "log", "exp") for c in COEFFS] + ["linear", "log", "exp"] + \
    ["onehot_{}".format(i) for i in range(5)]

# name: (seed, V, D, C, pairing, weight_type, start clip, subset)  -- D clusterings = D / 2 layers of two views
EXACT_CASES = {
    "a": (0, 160, 4, 6, "combination", "linear_1", 7, 40),
    "b": (1, 150, 10, 5, "combination", "exp_2", 11, 30),
    "c": (2, 180, 6, 8, "bipartite", "log_-1", 23, 36),
}
EXACT_MEASURES = ("mi", "mem_mi")
# name: (seed, V, D, C, pairing, weight_type, start clip, subset, B, k)
BATCH_CASES = {
    "a": (3, 400, 4, 6, "combination", "linear_2", 5, 62, 20, 4),
    "b": (4, 500, 10, 6, "combination", "exp_1", 13, 50, 20, 4),
}


def ref_keys(keys):
    return ["{}_{}".format(m, l) for m, l in keys]


def layer_keys(dd):
    return [(m, "layer_{}".format(i)) for m in ("SlowFast", "VGGish") for i in range(dd // 2)]


def correlated(seed, v, dd, c):
    """clusterings that agree on about half of the clips (the layout of gen_golden_pair.correlated)"""
    rs = np.random.RandomState(800 + seed)
    comp = rs.randint(0, c, size=v)
    cols = [np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)]
    a = np.stack(cols, 1).astype(np.int64)
    a[0] = c - 1
    return a


def gen_pairing():
    sys.path.insert(0, STUBS)
    sys.path.insert(0, CODE)
    import contextlib
    import io
    from cluster_pairing import get_cluster_pairing  # noqa: E402  (the reference)
    out = []
    for pairing in PAIRINGS:
        for wt in WEIGHT_TYPES:
            rec = dict(pairing=pairing, weight_type=wt)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    r = get_cluster_pairing(ref_keys(KEYS), pairing, wt)
                rec["pairs"] = [[int(x) for x in p] for p in r["pairing"]]
                rec["weights"] = [float(w) for w in r["weights"]]
            except Exception as exc:  # the reference's own failure: the tests expect a ValueError there
                rec["error"] = type(exc).__name__
            out.append(rec)
        with contextlib.redirect_stdout(io.StringIO()):
            plain = get_cluster_pairing(ref_keys(KEYS), pairing)
        out.append(dict(pairing=pairing, weight_type=None, pairs=[[int(x) for x in p] for p in plain]))
    path = os.path.join(HERE, "weights_pairing.json")
    with open(path, "w") as f:
        json.dump(dict(keys=[list(k) for k in KEYS], cases=out), f, separators=(",", ":"))
    print("{}: {} cases, {} reference errors, {} bytes".format(os.path.basename(path), len(out),
                                                             sum("error" in r for r in out), os.path.getsize(path)))


def _weighted(pairing, wt, dd):
    import contextlib
    import io
    from cluster_pairing import get_cluster_pairing  # noqa: E402  (the reference)
    with contextlib.redirect_stdout(io.StringIO()):
        return get_cluster_pairing(ref_keys(layer_keys(dd)), pairing, wt)


def gen_exact():
    sys.path.insert(0, STUBS)
    sys.path.insert(0, CODE)
    from measures.efficient import EfficientMI  # noqa: E402  (the reference)
    from measures.mem_mi import EfficientMemMI  # noqa: E402
    classes = dict(mi=EfficientMI, mem_mi=EfficientMemMI)
    for name, (seed, v, dd, c, pairing, wt, start, subset) in EXACT_CASES.items():
        a = correlated(seed, v, dd, c)
        comb = _weighted(pairing, wt, dd)
        for mname in EXACT_MEASURES:
            rec = dict(scores=[], idx=[], margin=[])
            orig = EfficientMI.calc_score

            def calc_score(self, *args, **kw):
                sc = self._calc_score(*args, **kw).mean(dim=-1)
                score, idx = sc.max(dim=0)
                vv = sc.cpu().numpy().astype(np.float32).copy()
                rec["scores"].append(vv)
                rec["idx"].append(int(idx.item()))
                u = np.unique(vv)
                rec["margin"].append(float(u[-1]) - float(u[-2]) if len(u) > 1 else np.inf)
                return score.item(), idx.item()

            EfficientMI.calc_score = calc_score
            try:
                clusterings = [types.SimpleNamespace(ncentroids=c, ind2cen=a[:, d].tolist()) for d in range(dd)]
                m = classes[mname](clusterings)
                m.device = "cpu"
                m.init(dict(pairing=list(comb["pairing"]), weights=list(comb["weights"])), list(range(v)))
                S, GAIN, _, _ = m.run_greedy(subset, [start])
            finally:
                EfficientMI.calc_score = orig
            w0 = len(rec["scores"][0])
            sc = np.full((len(rec["scores"]), w0), np.nan, np.float32)
            for t, row in enumerate(rec["scores"]):
                sc[t, :len(row)] = row
            out = os.path.join(HERE, "weights_exact_{}_{}.npz".format(name, mname))
            np.savez_compressed(out, assignments=a.astype(np.int16), pairs=np.array(comb["pairing"], np.int64),
                                weights=np.array(comb["weights"], np.float64), pairing=pairing, weight_type=wt, C=c,
                                start=start, subset=subset, S=np.array(S, np.int64), GAIN=np.array(GAIN, np.float64),
                                scores=sc, idx=np.array(rec["idx"], np.int64), margin=np.array(rec["margin"], np.float64))
            print("{}: {} selected, {} bytes".format(os.path.basename(out), len(S), os.path.getsize(out)))


def gen_batch():
    sys.path.insert(0, STUBS)
    sys.path.insert(0, CODE)
    import torch
    from measures.batch import EfficientBatchMI  # noqa: E402  (the reference)
    for name, (seed, v, dd, c, pairing, wt, start, subset, B, k) in BATCH_CASES.items():
        a = correlated(seed, v, dd, c)
        comb = _weighted(pairing, wt, dd)
        rec = dict(ids=[], scores=[], pos=[])
        orig_block, orig_ids = EfficientBatchMI.operate_block, EfficientBatchMI.calc_ids

        def operate_block(self, batch_range=None):
            scores, samples = orig_block(self, batch_range)
            rec["ids"].append(samples.numpy().astype(np.int64).copy())
            rec["scores"].append(scores.mean(dim=-1).numpy().astype(np.float32).copy())
            return scores, samples

        def calc_ids(self, scores):
            s, ids = orig_ids(self, scores)
            rec["pos"].append(ids.numpy().astype(np.int64).copy())
            return s, ids

        EfficientBatchMI.operate_block, EfficientBatchMI.calc_ids = operate_block, calc_ids
        try:
            clusterings = [types.SimpleNamespace(ncentroids=c, ind2cen=a[:, d].tolist()) for d in range(dd)]
            m = EfficientBatchMI(clusterings, batch_size=B, selection_size=k, device="cpu", keep_unselected=True)
            m.init(dict(pairing=list(comb["pairing"]), weights=list(comb["weights"])), list(range(v)))
            torch.manual_seed(seed)
            S, GAIN, _, _ = m.run_greedy(subset, [start])
        finally:
            EfficientBatchMI.operate_block, EfficientBatchMI.calc_ids = orig_block, orig_ids
        assert all(len(i) == B for i in rec["ids"])
        out = os.path.join(HERE, "weights_batch_{}.npz".format(name))
        np.savez_compressed(out, assignments=a.astype(np.int16), pairs=np.array(comb["pairing"], np.int64),
                            weights=np.array(comb["weights"], np.float64), pairing=pairing, weight_type=wt, C=c, seed=seed,
                            start=start, subset=subset, B=B, k=k, S=np.array(S, np.int64), GAIN=np.array(GAIN, np.float64),
                            ids=np.stack(rec["ids"]), scores=np.stack(rec["scores"]), pos=np.stack(rec["pos"]))
        print("{}: {} iterations, {} selected, {} bytes".format(os.path.basename(out), len(rec["ids"]), len(S),
                                                                os.path.getsize(out)))


STAGES = {"pairing": gen_pairing, "exact": gen_exact, "batch": gen_batch}

if __name__ == "__main__":
    which = sys.argv[1:] or list(STAGES)
    if len(which) > 1:  # one interpreter per stage
        for w in which:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), w])
    else:
        STAGES[which[0]]()
