"""fp64 twin, per-element bounds, the fixed case list and the clamp guard for tav_soft_f_loss (csrc/loss.hip, csrc/tavhip_loss.h).
Shared by tests/test_soft_f_loss_gpu.py and tests/test_soft_f_loss_host.py; a helper module like tests/front_ref.py: no tests are collected from it.

THE TWIN (torch, float64; autograd gives the gradient), with p_b = softmax(z_b):
    tp_k = sum_b [t_b = k] p_bk      fp_k = sum_b [t_b != k] p_bk      fn_k = sum_b [t_b = k] (1 - p_bk)
    P_k = tp_k / (tp_k + fp_k + eps)                 R_k = tp_k / (tp_k + fn_k + eps)
    F_k = (1 + beta^2) P_k R_k / (beta^2 P_k + R_k + eps)   ("FBeta")          F_k = P_k   ("Precision")
    loss = 1 - sum_k w_k clamp(F_k, eps, 1 - eps)
A target outside [0, C) selects no class: its row counts towards every fp_k.

BOUNDS, u = 2^-24: the number of f32 roundings on the kernel's chain, times u, times the summed magnitudes of the terms.  The chain, from
csrc/loss.hip (the counts are read off the source, not off its output):
    p_bk     d = z - m: 1 rounding, which enters expf as |d| u relative; expf: 3 ulp = 6 u (the OpenCL full-profile limit, as
             tests/front_ref.py); r_k = (6 + |d_k|) u.  se = the C terms summed in class order: C - 1 additions of positive numbers on terms
             of relative error r_j: r_se = sum_j p_j r_j + (C - 1) u.  p = e / se: 1 division.  e_p = p (r_k + r_se + u) + (C + 1) 2^-126
             (an expf result under the smallest normal may be flushed; se >= 1 because expf(0) = 1).
    tp fp fn promoted to f64 and summed in f64: the e_p of their rows, plus (B + 8) 2^-53 of the value for the f64 additions.  1 - p is
             formed in f64 from the f32 p: fn carries the same e_p as tp.
    class    stage in f64: no f32 rounding.  Its sensitivity to the sums is first order, |dL/dtp| e_tp + |dL/dfp| e_fp + |dL/dfn| e_fn (autograd
             of the twin's class stage); the sums are positive with relative error below 2^-18, so what first order leaves out of these
             rational functions is below 2^-10 of it: every propagated term is multiplied by SECOND = 1 + 2^-10.
    loss     the propagated term, 1 rounding at the store: u |loss|, and 64 2^-53 (1 + sum |w|) for the f64 stage.
    stats    e_tp / e_fp / e_fn and 1 rounding at the store.
    g        own_k = dL/dtp_k - dL/dfn_k and other_k = dL/dfp_k: the second derivatives of the class stage (autograd twice) times the e of the
             sums, and 1 rounding each at the store to LDS.
    dlogits  s = sum_j p_j g_j: C products and C - 1 additions, a product that enters a sum one more link: (C + 1) u sum_j |p_j g_j|, and the
             e_p, e_g of its terms.  g - s: 1 rounding on |g| + sum_j |p_j g_j|.  (grad_scale p) (g - s): 2 roundings; 2^-126 for a flush.

THE GUARD (a condition on the inputs, not a tolerance): for every class the clamp branch is the same whether the probabilities are the
float64 softmax or torch's f32 softmax promoted to float64, and F_k lies at least 16 times the difference of those two F_k from either
edge.  reference() asserts it; a case that failed would be replaced in the list below, never skipped where the tests run.
"""
import functools
import itertools

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
U64 = 2.0 ** -53
SECOND = 1.0 + 2.0 ** -10
EXP_U = 6.0                  # expf: 3 ulp
EPS = 1e-7

BS = (1, 2, 3, 63, 64, 65, 257, 1000)
CS = (2, 7, 16)
BETAS = (0.5, 1.0, 2.0)
MODES = ("FBeta", "Precision")
SCALES = (1.0, 3.0)
SEEDS = (0, 1, 2)
NAMED = tuple(itertools.product(BS, CS, BETAS, MODES, SCALES, SEEDS))           # (B, C, beta, mode, scale, seed): 864
EXACT_INPUTS = ("saturated", "absent_p0", "one_class", "b1", "out_of_range")
EXACT = tuple(itertools.product(EXACT_INPUTS, BETAS, MODES))                    # (name, beta, mode)
GOLDEN_INPUTS = ((1, 2, 1.0, 0), (2, 7, 3.0, 1), (3, 16, 1.0, 2), (63, 2, 3.0, 0), (64, 2, 1.0, 1), (65, 2, 3.0, 2))     # (B, C, scale, seed), beta = 1, "FBeta"


def class_weights(C):
    """The weight vector of the weighted cases: the entry points' class weights (utils/entrypoint.common_params)."""
    return torch.linspace(0.6, 0.95, C, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def named_inputs(B, C, scale, seed):
    """(z f32 [B][C], t int64 [B]): the logits first, then the targets, from one generator seeded 1000 seed + 17 B + C."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + C)
    z = torch.randn(B, C, generator=g, dtype=torch.float32) * scale
    t = torch.randint(0, C, (B,), generator=g, dtype=torch.int64)
    return z, t


@functools.lru_cache(maxsize=None)
def exact_inputs(name):
    g = torch.Generator().manual_seed(len(name))
    if name == "saturated":              # classes 0..2: 8 rows each, predicted with a logit gap of 800 (expf and exp both give 0); class 3: no row, p = 0
        t = torch.arange(3).repeat_interleave(8)
        z = torch.full((24, 4), -400.0)
        z[torch.arange(24), t] = 400.0
    elif name == "absent_p0":            # class 2 has no row and a logit of -Inf: p = 0 exactly, the lower clamp; the other two classes are ordinary
        z = torch.randn(6, 3, generator=g)
        z[:, 2] = float("-inf")
        t = torch.tensor([0, 1, 1, 0, 1, 0])
    elif name == "one_class":
        z, t = torch.randn(5, 3, generator=g), torch.ones(5, dtype=torch.int64)
    elif name == "b1":
        z, t = torch.randn(1, 7, generator=g), torch.tensor([4])
    elif name == "out_of_range":
        z, t = torch.randn(6, 3, generator=g), torch.tensor([-1, 0, 3, 1, 2, 1])
    else:
        raise KeyError(name)
    return z.float().contiguous(), t.long()


def counts(p, t):
    """tp, fp, fn [C] of probabilities p [B][C] (any float dtype) and targets t."""
    oh = (t[:, None] == torch.arange(p.shape[1])[None, :]).to(p.dtype)
    return (oh * p).sum(0), ((1 - oh) * p).sum(0), (oh * (1 - p)).sum(0)


def f_score(tp, fp, fn, beta, mode, eps=EPS):
    P, R = tp / (tp + fp + eps), tp / (tp + fn + eps)
    if mode == "Precision":
        return P
    assert mode == "FBeta"
    b2 = beta * beta
    return (1 + b2) * P * R / (b2 * P + R + eps)


def class_loss(tp, fp, fn, w, beta, mode, eps=EPS):
    return 1 - (w * f_score(tp, fp, fn, beta, mode, eps).clamp(eps, 1 - eps)).sum()


def twin(z, t, w, beta, mode, eps=EPS, grad_scale=1.0):
    """-> (loss, dlogits, stats [3][C]) as float64 numpy; w: None or [C].  dlogits = grad_scale (as f32 holds it) dloss/dz."""
    z64 = z.double().clone().requires_grad_(True)
    w64 = torch.ones(z.shape[1], dtype=torch.float64) if w is None else w.double()
    tp, fp, fn = counts(torch.softmax(z64, 1), t)
    loss = class_loss(tp, fp, fn, w64, beta, mode, eps)
    (g,) = torch.autograd.grad(loss, z64)
    return loss.item(), (g * float(np.float32(grad_scale))).numpy(), torch.stack([tp, fp, fn]).detach().numpy()


def branch(F, eps=EPS):
    """-1 below the lower edge, +1 above the upper, 0 where the clamp passes."""
    return (F > 1 - eps).to(torch.int64) - (F < eps).to(torch.int64)


def guard(z, t, beta, mode, eps=EPS):
    """-> (holds, F64, F32, branch64): the clamp branches agree and F64 keeps 16 |F64 - F32| from both edges, for every class."""
    F64 = f_score(*counts(torch.softmax(z.double(), 1), t), beta, mode, eps)
    F32 = f_score(*counts(torch.softmax(z, 1).double(), t), beta, mode, eps)
    dist = torch.minimum((F64 - eps).abs(), (F64 - (1 - eps)).abs())
    ok = bool((branch(F64, eps) == branch(F32, eps)).all()) and bool((dist >= 16 * (F64 - F32).abs()).all())
    return ok, F64, F32, branch(F64, eps)


def _class_derivatives(tp, fp, fn, w, beta, mode, eps):
    """First and second derivatives of the class stage per class: d [3][C] = dL/d(tp, fp, fn); J [3][3][C], J[i][j] = d(d_i)/d(sum_j)."""
    x = [v.detach().clone().requires_grad_(True) for v in (tp, fp, fn)]
    d = torch.autograd.grad(class_loss(*x, w, beta, mode, eps), x, create_graph=True, allow_unused=True)         # ("Precision" does not use fn)
    d = [torch.zeros_like(tp) if di is None else di for di in d]
    J = []
    for di in d:
        row = torch.autograd.grad(di.sum(), x, retain_graph=True, allow_unused=True) if di.requires_grad else (None, None, None)
        J.append([torch.zeros_like(tp) if r is None else r for r in row])
    return torch.stack([di.detach() for di in d]).numpy(), np.array([[r.numpy() for r in row] for row in J])


def reference(z, t, w, beta, mode, eps=EPS, grad_scale=1.0, check_guard=True):
    """The twin's values and the per-element bounds of the module docstring: dict(loss, loss_b [1]; dlogits, dlogits_b [B][C]; stats,
    stats_b [3][C]; branch [C])."""
    if check_guard:
        ok, F64, F32, _ = guard(z, t, beta, mode, eps)
        assert ok, f"clamp guard fails: F64 {F64.tolist()} F32 {F32.tolist()}"
    B, C = z.shape
    loss, dl, stats = twin(z, t, w, beta, mode, eps, grad_scale)
    gs = float(np.float32(grad_scale))
    zz, tt = z.double().numpy(), t.numpy()
    w64 = torch.ones(C, dtype=torch.float64) if w is None else w.double()
    with np.errstate(invalid="ignore"):
        d = zz - zz.max(1, keepdims=True)                                              # (-inf - finite = -inf: p = 0 and r p = 0 below)
    p = torch.softmax(z.double(), 1).numpy()
    r = np.where(p > 0, (EXP_U + np.abs(np.where(np.isfinite(d), d, 0.0))) * U, 0.0)
    r_se = (p * r).sum(1, keepdims=True) + (C - 1) * U
    e_p = p * (r + r_se + U) * SECOND + (C + 1) * TINY
    oh = (tt[:, None] == np.arange(C)[None, :])
    e_tp = (oh * e_p).sum(0) + (B + 8) * U64 * stats[0]
    e_fp = (~oh * e_p).sum(0) + (B + 8) * U64 * stats[1]
    e_fn = (oh * e_p).sum(0) + (B + 8) * U64 * stats[2]
    e_sum = np.stack([e_tp, e_fp, e_fn])
    d1, J = _class_derivatives(*(torch.from_numpy(s) for s in stats), w64, beta, mode, eps)
    loss_b = (np.abs(d1) * e_sum).sum() * SECOND + U * abs(loss) + 64 * U64 * (1 + float(w64.abs().sum()))
    stats_b = e_sum + U * np.abs(stats)
    e_d = (np.abs(J) * e_sum[None, :, :]).sum(1) * SECOND                               # [3][C]: the errors of dL/dtp, dL/dfp, dL/dfn
    own, other = d1[0] - d1[2], d1[1]
    e_own, e_other = e_d[0] + e_d[2] + U * np.abs(own), e_d[1] + U * np.abs(other)
    g, e_g = np.where(oh, own[None, :], other[None, :]), np.where(oh, e_own[None, :], e_other[None, :])
    mag_s = (p * np.abs(g)).sum(1, keepdims=True)
    s = (p * g).sum(1, keepdims=True)
    e_s = (e_p * np.abs(g) + p * e_g).sum(1, keepdims=True) + (C + 1) * U * mag_s
    e_diff = e_g + e_s + U * (np.abs(g) + mag_s)
    diff = np.abs(g - s) + e_diff
    dl_b = gs * (e_p * diff + p * e_diff) * SECOND + 2 * U * gs * p * diff + TINY
    return dict(loss=np.array([loss]), loss_b=np.array([loss_b]), dlogits=dl, dlogits_b=dl_b, stats=stats, stats_b=stats_b,
                branch=branch(f_score(*(torch.from_numpy(s) for s in stats), beta, mode, eps), eps).numpy())


@functools.lru_cache(maxsize=None)
def named_reference(B, C, beta, mode, scale, seed, weighted=False, grad_scale=1.0):
    z, t = named_inputs(B, C, scale, seed)
    return reference(z, t, class_weights(C) if weighted else None, beta, mode, grad_scale=grad_scale)


@functools.lru_cache(maxsize=None)
def exact_reference(name, beta, mode, weighted=False, grad_scale=1.0):
    z, t = exact_inputs(name)
    return reference(z, t, class_weights(z.shape[1]) if weighted else None, beta, mode, grad_scale=grad_scale)


def ratio(got, want, bound):
    """The worst |got - want| / bound; inf where an element is not finite or the shapes differ.  An element whose bound is 0 has to be
    equal (ratio 0), else inf."""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if got.shape != want.shape or not np.isfinite(got).all():
        return float("inf")
    if not got.size:
        return 0.0
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max())
