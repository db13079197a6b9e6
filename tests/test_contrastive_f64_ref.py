"""CPU: oracle/contrastive_ref.py (numpy float32) against the float64 reference of tests/_contrastive_f64.py, on the
shapes and inputs of tests/test_gpu_contrastive_grads.py.

The goldens made by the reference module store losses and trained parameters, never a gradient, and AdamW divides every
element's first moment by the root of its second: a gradient scaled by a constant (per buffer, per tensor or per element)
trains nearly the same parameters (about 2e-5 relative at lr 1e-3, eps 1e-6; the parity tolerances are 1e-4).  This file pins
`Contrastive.batch_grads` and `apply` directly, and yields the oracle's own error e_oracle = max|x - x64| / max|x64| per case
and tensor, which the GPU tests compute again from the same inputs and hold the kernels to.

Bound on the oracle: 2^-18 (64 units of f32 roundoff).  The logits are cosines times 1/T = 10, so a cosine's few ulps reach
the softmax ten-fold, and the gradient passes through about six further rounded stages (two products with G, the
normalisation's backward, the weight product); the measured errors are at most 1.6e-6 on the six shapes.  A wrong factor
anywhere gives an error of order one.
"""
import numpy as np
import pytest

from tests import _contrastive_f64 as R

ORACLE_BOUND = 2.0 ** -18


def _check_grads(got, want, what):
    for name, g, g64 in zip(R.SHORT, got, want):
        e = R.err(g, g64)
        print(f"{what} {name}: e_oracle = {e:.3g}")
        assert g.dtype == np.float32 and e <= ORACLE_BOUND, (what, name, e)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_oracle_batch_grads_vs_f64(i):
    p, (v, a) = R.case_inputs(i)
    loss64, acc64, hits64, g64 = R.case_ref(i)
    loss, acc, g = R.oracle_grads(p, v, a)
    B = R.CASES[i][0]
    assert abs(acc * 2 * B / 100.0 - hits64) < 1e-3  # the same hits
    if B == 1:  # a single clip: softmax of one logit is 1, nothing to learn
        assert loss64 == 0.0 and acc64 == 100.0 and all(not x.any() for x in g64)
        assert loss == 0.0 and acc == 100.0 and all(not np.asarray(x).any() for x in g)
        return
    assert abs(loss - loss64) / abs(loss64) <= ORACLE_BOUND
    _check_grads([np.asarray(x, np.float32) for x in g], g64, R.CASE_IDS[i])


def test_oracle_duplicate_rows_vs_f64():
    p, (v, a) = R.dup_inputs()
    loss64, acc64, hits64, g64 = R.dup_ref()
    assert acc64 == 50.0  # every clip's pair holds the maxima, the first of the two wins
    loss, acc, g = R.oracle_grads(p, v, a)
    assert acc == 50.0 and abs(loss - loss64) / abs(loss64) <= ORACLE_BOUND
    _check_grads([np.asarray(x, np.float32) for x in g], g64, "dup")


def test_oracle_accumulation_vs_f64():
    from oracle import contrastive_ref as CR
    p, batches = R.accum_inputs()
    _, gsum64 = R.accum_ref()
    orc = CR.Contrastive(*p)
    for v, a in batches:
        for g, dg in zip(orc.g, orc.batch_grads(v, a)[2]):
            g += dg.astype(np.float32)
    _check_grads(orc.g, gsum64, "accum")
    assert all(np.array_equal(x, y) for x, y in zip(orc.p, p))


def test_oracle_adamw_vs_torch_f64():
    p0, grads, lrs, groups = R.adamw_case()
    assert p0.size % 256 == 194
    want = R.adamw_ref()
    got, step = R.oracle_adamw(p0, grads, lrs)
    assert step == len(lrs)
    decay = 1.0
    for k, (p, p64) in enumerate(zip(got, want)):
        decay *= 1.0 - lrs[k] * 0.01
        for name, idx in groups.items():
            e = R.err(p[idx], p64[idx])
            print(f"adamw step {k + 1} {name}: e_oracle = {e:.3g}")
            assert e <= ORACLE_BOUND, (k, name, e)
        z = groups["g_zero"]
        np.testing.assert_allclose(p64[z], p0[z].astype(np.float64) * decay, rtol=1e-14)  # the decay on its own
        assert np.abs(p[z] / p64[z] - 1.0).max() <= 2.0 ** -22 * (k + 1)  # a chain of single f32 multiplies
    # the schedule reaches the amsgrad branch: v falls by 1 - b2 = 0.1 % per shrinking step, so without the running maximum
    # the updates of steps 2, 4 and 5 grow by about 0.05 % each -- far more than the bound the GPU test can ever allow
    import torch
    t = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.AdamW([t], lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, amsgrad=False)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]['lr'] = lr
        t.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
    assert R.err(t.detach().numpy()[groups["p0_zero"]], want[-1][groups["p0_zero"]]) > 8 * R.RATIO * ORACLE_BOUND


@pytest.mark.parametrize("i", range(len(R.INFER)))
def test_oracle_infer_vs_f64(i):
    p, (v, a) = R.infer_inputs(i)
    e = float(np.abs(R.oracle_infer(p, v, a).astype(np.float64) - R.infer_ref(i)).max())
    print(f"infer {R.INFER[i]}: oracle abs error = {e:.3g}")
    assert e <= ORACLE_BOUND  # cosines in [-1, 1]


def test_f64_reference_is_what_it_says():
    """the helper against the formulas written out by hand in numpy float64 (softmax minus identity, both directions)"""
    p, (v, a) = R.case_inputs(1)
    loss64, _, _, g64 = R.case_ref(1)
    wv, bv, wa, ba = [x.astype(np.float64) for x in p]
    z1, z2 = v.astype(np.float64) @ wv.T + bv, a.astype(np.float64) @ wa.T + ba
    d1, d2 = np.linalg.norm(z1, axis=1, keepdims=True), np.linalg.norm(z2, axis=1, keepdims=True)
    o1, o2 = z1 / d1, z2 / d2
    L = o1 @ o2.T / 0.1
    B = L.shape[0]

    def softmax(x):
        ex = np.exp(x - x.max(1, keepdims=True))
        return ex / ex.sum(1, keepdims=True)
    pa, pb = softmax(L), softmax(L.T).T
    loss = -(np.log(np.diag(pa)).sum() + np.log(np.diag(pb)).sum()) / (2 * B)
    G = (pa + pb - 2 * np.eye(B)) / (2 * B)
    do1, do2 = G @ o2 / 0.1, G.T @ o1 / 0.1
    dz1 = (do1 - o1 * (o1 * do1).sum(1, keepdims=True)) / d1
    dz2 = (do2 - o2 * (o2 * do2).sum(1, keepdims=True)) / d2
    assert abs(loss - loss64) <= 1e-13 * abs(loss64)
    for got, want in zip(g64, [dz1.T @ v, dz1.sum(0), dz2.T @ a, dz2.sum(0)]):
        assert R.err(got, want) <= 1e-12
