"""batch_mi at wide batches: time of the whole selection and per iteration over (batch_size, selection_size).

    python tools/bench_mi_wide.py [V] [C] [subset]

One-chunk greedy selection of `subset` (default 20 %) of V (default 10^6) clips with C (default 256) centroids, at
(B, k) = (20, 4), (100, 25), (160, 40), (1024, 256) on two clusterings (one pair) and the first three on ten (45 pairs;
1024 x 45 is beyond the B x P limit).  The permutation of the candidate list costs the same per iteration whatever B, and
the number of iterations is ceil(subset / k).  One JSON line per setting."""
import itertools
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acav100m_amd
acav100m_amd.configure_runtime(quiet=True)
from acav100m_amd.subset_selection import get_measure

v = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
c = int(sys.argv[2]) if len(sys.argv) > 2 else 256
subset = int(sys.argv[3]) if len(sys.argv) > 3 else round(0.2 * v)
rs = np.random.RandomState(0)
comp = rs.randint(0, c, v)
a10 = np.stack([np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, v)) for _ in range(10)], 1).astype(np.int64)
a10[0] = c - 1
cand = [int(i) for i in rs.permutation(v)]
for dd, settings in ((2, [(20, 4), (100, 25), (160, 40), (1024, 256)]), (10, [(20, 4), (100, 25), (160, 40)])):
    a = np.ascontiguousarray(a10[:, :dd])
    pairs = list(itertools.combinations(range(dd), 2))
    for B, k in settings:
        best = None
        for rep in range(2):  # the better of two runs: the first one of a process also pays for its buffers
            acav100m_amd.manual_seed(0)
            m = get_measure("batch_mi")(a, ncentroids=c, batch_size=B, selection_size=k, device="cuda:0", keep_unselected=True)
            m.init(pairs, cand[1:])
            t0 = time.perf_counter()
            S, G, _, _ = m.run_greedy(subset, cand[:1], None)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
            del m
        iters = -(-subset // k)
        print(json.dumps({"V": v, "C": c, "P": len(pairs), "B": B, "k": k, "selected": len(S), "iters": iters,
                          "seconds": round(best, 4), "us_per_iter": round(best / iters * 1e6, 2)}), flush=True)
