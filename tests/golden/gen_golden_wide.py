#!/usr/bin/env python3
"""Generate the golden traces of the batch-MI greedy at WIDE batches (batch_size > 64) by running the REFERENCE itself (only
where the reference is mounted; what is committed is the data it produced).

    python tests/golden/gen_golden_wide.py

mi_wide_<a|b>.npz: subset_selection's EfficientBatchMI (measures/batch.py) on the CPU through run_greedy._run_greedy, at the
paper grid's batch setting (batch_size 100 / selection_size 25: every correspondence_retrieval search target) and at
160 / 40 with four clusterings (six pairs).  Same inputs and the same keys as gen_golden.py's mi_<name>.npz: assignments, C,
seed, ratio, shuffled (the candidate order the reference shuffled to), per iteration the batch ids, the fp32 scores
[B, P], the picked positions and their scores, and the final S and GAIN; B and k are recorded as well.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# name: (seed, V, D, C, B, k, ratio)
CASES = {
    "a": (0, 2000, 2, 16, 100, 25, 0.2),
    "b": (1, 3000, 4, 64, 160, 40, 0.2),
}


class _NS(dict):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.__dict__ = self


def main():
    sys.path.insert(0, os.path.join(REF, "subset_selection", "code"))
    import torch
    import run_greedy as ref_run_greedy  # noqa: E402  (the reference)
    from measures.batch import EfficientBatchMI  # noqa: E402

    for name, (seed, v, dd, c, B, k, ratio) in CASES.items():
        rs = np.random.RandomState(300 + seed)
        comp = rs.randint(0, c, size=v)
        cols = []
        for _ in range(dd):
            indep = rs.randint(0, c, size=v)
            share = rs.rand(v) < 0.5  # the views share the component id with probability 0.5
            cols.append(np.where(share, comp, indep))
        assignments = np.stack(cols, 1).astype(np.int64)
        assignments[0, :] = c - 1  # max() + 1 == c whatever the draw
        types = [("m%d" % i, "layer_0") for i in range(dd)]

        rec = dict(ids=[], scores=[], pick_pos=[], pick_scores=[])
        orig_operate, orig_calc_ids = EfficientBatchMI.operate_block, EfficientBatchMI.calc_ids

        def operate_block(self, batch_range=None):
            scores, samples = orig_operate(self, batch_range)
            rec["scores"].append(scores.cpu().numpy().copy())
            rec["ids"].append(samples.cpu().numpy().copy())
            return scores, samples

        def calc_ids(self, scores):
            s, ids = orig_calc_ids(self, scores)
            rec["pick_scores"].append(s.cpu().numpy().copy())
            rec["pick_pos"].append(ids.cpu().numpy().copy())
            return s, ids

        EfficientBatchMI.operate_block, EfficientBatchMI.calc_ids = operate_block, calc_ids
        args = _NS(batch=_NS(batch_size=B, selection_size=k, keep_unselected=True), computation=_NS(device="cpu"),
                   log_every=10 ** 9, log_times=None, node_rank=None, parent_pid=None)
        random.seed(seed)
        torch.manual_seed(seed)
        try:
            S, GAIN, _ = ref_run_greedy._run_greedy(args, assignments, types, None, ratio, "batch_mi", "combination", True, False)
        finally:
            EfficientBatchMI.operate_block, EfficientBatchMI.calc_ids = orig_operate, orig_calc_ids
        random.seed(seed)  # the shuffled candidate order the reference used (run_greedy.py:37-44)
        cand = list(range(v))
        random.shuffle(cand)
        out = dict(assignments=assignments, seed=seed, C=c, ratio=ratio, B=B, k=k, shuffled=np.array(cand, np.int64),
                   S=np.array(S, np.int64), GAIN=np.array(GAIN, np.float64), ids=np.stack(rec["ids"]).astype(np.int64),
                   scores=np.stack(rec["scores"]).astype(np.float32), pick_pos=np.stack(rec["pick_pos"]).astype(np.int64),
                   pick_scores=np.stack(rec["pick_scores"]).astype(np.float32))
        path = os.path.join(HERE, f"mi_wide_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"mi_wide_{name}.npz written: {len(S)} selected in {len(rec['ids'])} iterations, scores {out['scores'].shape}, "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
