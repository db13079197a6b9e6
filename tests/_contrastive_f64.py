"""float64 reference of the contrastive baseline, written from the formulas -- TEST INFRASTRUCTURE ONLY.

Two linear maps, F.normalize (eps 1e-12), logits = o1 o2^T / 0.1, loss = the mean of the two cross entropies (rows: visual ->
audio, columns: audio -> visual); the gradients come from torch.autograd on float64 CPU tensors, the optimizer is
torch.optim.AdamW itself.  It pins oracle/contrastive_ref.py (tests/test_contrastive_f64_ref.py) and the HIP kernels
(tests/test_gpu_contrastive_grads.py) through the gradients themselves: parameters after AdamW cannot (a gradient scaled by
any constant gives nearly the same step).

The error measure is e(x) = max|x - x64| / max|x64| per parameter tensor: an elementwise relative error is ill-conditioned at
the near-zero entries of a gradient.  The bound on the HIP kernels is e_hip <= RATIO * max(e_oracle, FLOOR): both are f32
evaluations of one formula and differ in summation order and fma contraction only; 8 is a margin over that reordering, and
the 4-ulp floor covers cases where numpy happens to round exactly.

The shapes, inputs and schedules of both test files live here, so that the CPU test pins the oracle on exactly the inputs
the GPU test feeds the kernels.
"""
import functools

import numpy as np
import torch

TEMPERATURE = 0.1
PARAM_NAMES = ('visual_linear.weight', 'visual_linear.bias', 'audio_linear.weight', 'audio_linear.bias')
SHORT = ('Wv', 'bv', 'Wa', 'ba')
RATIO = 8.0
FLOOR = 2.0 ** -22

# (B, vis, aud, out): the edges of acav_contrastive.hip's three GEMM shapes and row kernels
CASES = [
    (1, 5, 3, 2),         # loss 0, accuracy 100, every gradient exactly 0.0
    (2, 37, 3, 19),       # everything smaller than a tile
    (65, 257, 100, 65),   # one past the 64-tile in M and N; split-K S = 4 with a 17-wide last slice
    (33, 1000, 64, 2),    # split-K S = 15 with two empty slices; out < 64 lanes
    (256, 130, 17, 70),   # the batch maximum: full L / G buffers, one element per thread in k_ct_stats
    (150, 513, 257, 200),  # both projections split-K; out > 64 in the row kernels
]
CASE_IDS = ["B%d_v%d_a%d_o%d" % c for c in CASES]
DUP = (64, 24, 40, 48)              # duplicate rows: B, vis, aud, out
ACCUM = ((7, 64, 130), 130, 17, 70)  # three backward calls without a step in between
ADAMW_SIZES = (63, 1, 65)           # nparam = 4290 = 16 * 256 + 194: the last 256-thread block is partial
ADAMW_MULT = (1.0, 1e-3, 10.0, 0.0, 1e-4)   # the shrinking steps make vmax > v (the amsgrad branch); the zero step moves
ADAMW_LRS = (1e-3, 5e-4, 1e-3, 1e-3, 2e-3)  # the parameters by decay and stale momentum only
INFER = [(8195, 37, 3, 19),     # crosses the 8192-row chunk; the second chunk has three rows
         (300, 257, 100, 65)]   # more than 256 rows: no split-K (its first 200 rows alone take split-K)


def err(x, x64):
    """max|x - x64| / max|x64|"""
    x64 = np.asarray(x64, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / np.abs(x64).max())


def bound(e_oracle):
    return RATIO * max(e_oracle, FLOOR)


def nparam(vis, aud, out):
    return out * vis + out + out * aud + out


def split(flat, vis, aud, out):
    """the flat [Wv | bv | Wa | ba] buffer of the handle -> four arrays (state_dict order and shapes)"""
    cuts = np.cumsum([out * vis, out, out * aud, out])
    parts = np.split(np.asarray(flat), cuts[:-1])
    return [p.reshape(s) for p, s in zip(parts, [(out, vis), (out,), (out, aud), (out,)])]


def make_params(seed, vis, aud, out):
    """uniform in +-1/sqrt(in), float32, state_dict order"""
    rs = np.random.RandomState(seed)
    bv_, ba_ = 1.0 / np.sqrt(vis), 1.0 / np.sqrt(aud)
    return [rs.uniform(-bv_, bv_, (out, vis)).astype(np.float32), rs.uniform(-bv_, bv_, out).astype(np.float32),
            rs.uniform(-ba_, ba_, (out, aud)).astype(np.float32), rs.uniform(-ba_, ba_, out).astype(np.float32)]


def make_data(seed, n, vis, aud):
    """twelve noisy components per view, float32 (the data of tests/test_gpu_contrastive.py)"""
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, 12, n)
    cv, ca = rs.randn(12, vis).astype(np.float32), rs.randn(12, aud).astype(np.float32)
    return (cv[comp] + 0.5 * rs.randn(n, vis)).astype(np.float32), (ca[comp] + 0.5 * rs.randn(n, aud)).astype(np.float32)


def case_inputs(i):
    B, vis, aud, out = CASES[i]
    return make_params(1000 + i, vis, aud, out), make_data(2000 + i, B, vis, aud)


def dup_inputs():
    """rows 2k and 2k+1 identical in both views: their logits tie exactly.  The audio view is a linear image of the visual
    one and the audio map undoes it (up to a small perturbation), so every clip's own pair holds the row and column maxima
    and first-maximum-wins gives an accuracy of exactly 50."""
    B, vis, aud, out = DUP
    rs = np.random.RandomState(77)
    p = make_params(76, vis, aud, out)
    mix = rs.randn(aud, vis) / np.sqrt(vis)
    p[2] = (p[0] @ np.linalg.pinv(mix) + 0.02 * rs.randn(out, aud) / np.sqrt(aud)).astype(np.float32)
    p[3] = p[1].copy()
    half = rs.randn(B // 2, vis)
    visual = np.repeat(half, 2, axis=0).astype(np.float32)
    audio = (visual.astype(np.float64) @ mix.T).astype(np.float32)
    assert np.array_equal(visual[0::2], visual[1::2]) and np.array_equal(audio[0::2], audio[1::2])
    return p, (visual, audio)


def accum_inputs():
    sizes, vis, aud, out = ACCUM
    return make_params(55, vis, aud, out), [make_data(60 + k, b, vis, aud) for k, b in enumerate(sizes)]


def infer_inputs(i):
    n, vis, aud, out = INFER[i]
    return make_params(3000 + i, vis, aud, out), make_data(4000 + i, n, vis, aud)


# ---------------------------------------------------------------------------------------------- the float64 model
def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64).copy())


def _project(p, visual, audio):
    o1 = torch.nn.functional.normalize(_t(visual) @ p[0].T + p[1], dim=-1, eps=1e-12)
    o2 = torch.nn.functional.normalize(_t(audio) @ p[2].T + p[3], dim=-1, eps=1e-12)
    return o1, o2


def forward_backward(params, visual, audio):
    """-> (loss, accuracy in percent, hits out of 2 B, the four gradients), all float64"""
    p = [_t(a).requires_grad_(True) for a in params]
    o1, o2 = _project(p, visual, audio)
    L = o1 @ o2.T / TEMPERATURE
    B = L.shape[0]
    idx = torch.arange(B)
    loss = (torch.nn.functional.cross_entropy(L, idx) + torch.nn.functional.cross_entropy(L.T, idx)) / 2
    grads = torch.autograd.grad(loss, p)
    Ln = L.detach().numpy()
    hits = int(np.sum(Ln.argmax(1) == np.arange(B)) + np.sum(Ln.argmax(0) == np.arange(B)))  # np.argmax: first maximum wins
    return float(loss.detach()), hits / (2 * B) * 100.0, hits, [g.numpy() for g in grads]


def infer(params, visual, audio):
    """the cosine of every clip's aligned pair, float64"""
    with torch.no_grad():
        o1, o2 = _project([_t(a) for a in params], visual, audio)
        return (o1 * o2).sum(-1).numpy()


def adamw_f64(p, grads_per_step, lrs):
    """torch.optim.AdamW(betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, amsgrad=True) on a float64 tensor, .grad set by hand
    for each step -> the parameters after every step"""
    t = _t(p).requires_grad_(True)
    opt = torch.optim.AdamW([t], lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, amsgrad=True)
    out = []
    for g, lr in zip(grads_per_step, lrs):
        opt.param_groups[0]['lr'] = float(lr)
        t.grad = _t(g).reshape(t.shape)
        opt.step()
        out.append(t.detach().numpy().copy())
    return out


# ---------------------------------------------------------------------------------------------- cached references
@functools.lru_cache(maxsize=None)
def case_ref(i):
    p, (v, a) = case_inputs(i)
    return forward_backward(p, v, a)


@functools.lru_cache(maxsize=None)
def dup_ref():
    p, (v, a) = dup_inputs()
    return forward_backward(p, v, a)


@functools.lru_cache(maxsize=None)
def accum_ref():
    """the float64 sum of the three gradients at the unchanged parameters"""
    p, batches = accum_inputs()
    refs = [forward_backward(p, v, a) for v, a in batches]
    return refs, [sum(r[3][k] for r in refs) for k in range(4)]


@functools.lru_cache(maxsize=None)
def infer_ref(i, rows=None):
    p, (v, a) = infer_inputs(i)
    return infer(p, v[:rows], a[:rows])


def adamw_case():
    """-> (p0, gradients per step, learning rates, {group: flat indices}) on the flat buffer of ADAMW_SIZES"""
    n = nparam(*ADAMW_SIZES)
    rs = np.random.RandomState(99)
    base = (10.0 ** rs.uniform(-6, 2, n)) * rs.choice([-1.0, 1.0], n)  # log-uniform in [1e-6, 1e2], random signs
    p0 = (0.05 * rs.randn(n)).astype(np.float32)
    groups = {"p0_zero": np.arange(1000, 1300),  # p = -(the sum of the updates): nothing cancels
              "g_zero": np.arange(4200, n)}      # p = p0 * prod(1 - lr_i * 0.01): the decay on its own, up to the last element
    groups["rest"] = np.setdiff1d(np.arange(n), np.concatenate(list(groups.values())))
    p0[groups["p0_zero"]] = 0.0
    base[groups["g_zero"]] = 0.0
    assert np.all(p0[groups["g_zero"]] != 0.0)
    grads = [(base * m).astype(np.float32) for m in ADAMW_MULT]
    return p0, grads, ADAMW_LRS, groups


@functools.lru_cache(maxsize=None)
def adamw_ref():
    p0, grads, lrs, _ = adamw_case()
    return adamw_f64(p0, grads, lrs)


def oracle_adamw(p0, grads, lrs):
    """oracle.contrastive_ref.Contrastive.apply over the schedule -> the flat parameters after every step"""
    from oracle import contrastive_ref as CR
    orc = CR.Contrastive(*split(p0, *ADAMW_SIZES))
    out = []
    for g, lr in zip(grads, lrs):
        orc.g = [np.array(x, np.float32) for x in split(g, *ADAMW_SIZES)]
        orc.apply(lr)
        out.append(np.concatenate([x.ravel() for x in orc.p]))
    return out, orc.step


def oracle_grads(params, visual, audio):
    from oracle import contrastive_ref as CR
    return CR.Contrastive(*params).batch_grads(visual, audio)


def oracle_infer(params, visual, audio):
    from oracle import contrastive_ref as CR
    return CR.Contrastive(*params).infer(visual, audio)
