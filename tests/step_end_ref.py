"""fp64 reference, per-element bounds and inputs for the step-end kernel checks (numpy only: shared by the GPU checks in kernel_checks.py and by
tests/test_step_end_reference_host.py, which tests this tester on the CPU).

AdamW as the library documents it (include/tavhip.h): decoupled decay, eps OUTSIDE the square root and AFTER the bias correction, the gradient
multiplied by the clip coefficient before it enters BOTH moments:

    gr = g * cc                      decay = 1 - lr * wd
    m' = m * b1 + (1 - b1) * gr      bc1 = 1 - b1^s
    v' = v * b2 + (1 - b2) * gr^2    bc2 = 1 - b2^s
    q  = (lr / bc1) * m' / (sqrt(v') / sqrt(bc2) + eps)
    p' = p * decay - q

The reference takes the scalars as the C ABI receives them -- betas, eps, wd and lr rounded to f32 first (1 - 0.999f differs from 0.001 by 1.3e-5
relative: not a kernel error) -- and restarts every step from the kernel's own f32 state, so every bound is the bound of ONE step.

Bounds per element, u = 2^-24 (half an f32 ulp, relative):
    p        4u |p decay| + |q| (16u + 4u / bc1 + 2u / bc2)      (the 1 / bc terms: the cancellation in 1 - b^s after powf)
    exp_avg  8u (|m| b1 + (1 - b1) |gr|)
    exp_avg_sq  8u (v b2 + (1 - b2) gr^2)

Inputs: parameters N(0, 1); gradient magnitudes log-uniform in [1e-10, 1e2] with a random sign, 5 % exact zeros (eps decides the update of the
elements whose |g| is below ~1e-8).  The SAME gradient tensor is used at every step (it is uploaded once and must come back bit-identical):
m and gr then never cancel, which the bound of p -- relative to |q| -- relies on.

Learning rate: LR = 0.1, halved before step 3.  The size is deliberate.  At step 1, bc2 = 1e-3 puts 2u / bc2 = 1.2e-4 |q| into the bound of p; a
decay applied to the UPDATED weight, (p - q) decay, is off by lr wd |q|, which that term would swallow at lr = 1e-3 (1e-5 |q|).  With lr = 0.1 and
wd = 1e-2 it is 1e-3 |q|: eight times the bound.
"""
import numpy as np

U = 2.0 ** -24
BETAS = (0.9, 0.999)
EPS = 1e-8
LR = 0.1
WD = 1e-2
CLIP_STEP2 = 0.37                                         # the clip coefficient of step 2 (step 1: no pointer, step 3: 1.0)

# loop boundaries of adamw_chunk_kernel: 256 threads x 4 floats per 16-byte access, unrolled 4 times, 16384 elements per chunk
SIZES_EDGES = [1, 3, 4, 5, 1023, 1024, 1025, 3071, 3072, 3073, 4095, 4096, 4097, 16383, 16384, 16385, 2 * 16384 + 7]


def sizes_many():
    """67 tensors of 1 .. 29 elements with two multi-chunk tensors among them: a chunk table of non-power-of-two length (67 entries, 70 chunks)
    with long runs of one-chunk tensors for chunk_owner's binary search."""
    s = [1 + (7 * i) % 29 for i in range(67)]
    s[23] = 16384 + 5
    s[50] = 2 * 16384 + 1
    return s


SIZE_LISTS = {"edges": SIZES_EDGES, "many": sizes_many(), "nt1": [16385], "nt2": [5, 2 * 16384 + 7], "nt3": [1023, 1, 4097]}


def f32(x):
    return float(np.float32(x))


def make_inputs(n, seed):
    """(params, grads) as f32 arrays of n elements."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    mag = 10.0 ** rng.uniform(-10.0, 2.0, n)
    g = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.random(n) < 0.05] = 0.0
    return p, g


def chunk_prefix(sizes, chunk=16384):
    """(chunk_prefix[t] = index of tensor t's first chunk, total chunks): the table tav_*_chunked take."""
    pre, c = [], 0
    for s in sizes:
        pre.append(c)
        c += (s + chunk - 1) // chunk
    return pre, c


def bias_corr(step, betas=BETAS):
    b1, b2 = f32(betas[0]), f32(betas[1])
    return 1.0 - b1 ** step, 1.0 - b2 ** step


def ref_step(p, g, m, v, step, lr, wd, cc, betas=BETAS, eps=EPS):
    """One fp64 AdamW step from f32 state.  lr is the f32 word the kernel reads, cc the clip coefficient (1.0 when there is none).
    -> dict with the new p / m / v and their per-element bounds."""
    b1, b2, eps, wd, lr, cc = f32(betas[0]), f32(betas[1]), f32(eps), f32(wd), f32(lr), f32(cc)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    decay = 1.0 - lr * wd
    gr = g * cc
    m1 = m * b1 + (1.0 - b1) * gr
    v1 = v * b2 + (1.0 - b2) * gr * gr
    q = (lr / bc1) * m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps)
    return dict(p=p * decay - q, m=m1, v=v1, q=q,
                p_bound=4 * U * np.abs(p * decay) + np.abs(q) * (16 * U + 4 * U / bc1 + 2 * U / bc2),
                m_bound=8 * U * (np.abs(m) * b1 + (1.0 - b1) * np.abs(gr)),
                v_bound=8 * U * (v * b2 + (1.0 - b2) * gr * gr))


def ratio(got, ref, bound):
    """Worst |got - ref| / bound over the elements; a zero bound demands equality, a non-finite result is infinitely wrong."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max())


def ratios(ref, p, m, v):
    return dict(p=ratio(p, ref["p"], ref["p_bound"]), m=ratio(m, ref["m"], ref["m_bound"]), v=ratio(v, ref["v"], ref["v_bound"]))


# ---------------------------------------------------------------------------------------------- f32 emulations (host test of the tester)
F = np.float32


def _fma32(a, b, c):
    """a * b + c rounded once (the product of two f32 is exact in f64; the f64 sum is rounded again to f32: a double rounding so rare and so
    small -- half an ulp of f64 -- that it does not matter here)."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F)


def emulate_step(p, g, m, v, step, lr, wd, cc, form="chunked", mutant=None, lr_prev=None, betas=BETAS, eps=EPS):
    """The kernels' f32 arithmetic in numpy: form "chunked" as adamw_chunk_kernel (fused multiply-adds written out, sqrt(s) * rs2), "multi" as
    adamw_multi_kernel (sqrt(s) / sqrt(bc2), no fused operations).  mutant: None or one of MUTANTS.  -> (p, m, v) f32."""
    b1, b2, eps, wd, lr, cc = F(betas[0]), F(betas[1]), F(eps), F(wd), F(lr), F(cc)
    if mutant == "lr_of_previous_step":
        lr = F(lr_prev)
    s = step + 1 if mutant == "step_off_by_one" else step
    bc1, bc2 = F(1) - np.power(b1, F(s), dtype=F), F(1) - np.power(b2, F(s), dtype=F)
    decay = F(1) if mutant == "decay_dropped" else F(1) - lr * wd
    omb1, omb2 = F(1) - b1, F(1) - b2
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    gr = g * cc
    g2 = g if mutant == "clip_missing_in_second_moment" else gr
    w = p if mutant == "decay_after_update" else p * decay
    if form == "chunked":
        a = _fma32(m, b1, omb1 * gr)
        s2 = _fma32(v, b2, (omb2 * g2) * g2)
    else:
        a = m * b1 + omb1 * gr
        s2 = v * b2 + omb2 * g2 * g2
    if mutant == "eps_inside_sqrt":
        den = np.sqrt(s2 / bc2 + eps, dtype=F)
    elif mutant == "eps_before_bias_correction":
        den = (np.sqrt(s2, dtype=F) + eps) / np.sqrt(bc2, dtype=F)
    elif form == "chunked":
        den = _fma32(np.sqrt(s2, dtype=F), F(1) / np.sqrt(bc2, dtype=F), np.full_like(s2, eps))
    else:
        den = np.sqrt(s2, dtype=F) / np.sqrt(bc2, dtype=F) + eps
    q = ((lr / bc1) * a) / den
    w = w - q
    if mutant == "decay_after_update":
        w = w * decay
    return w.astype(F), a.astype(F), s2.astype(F)


# mutant -> the step (1-based) at which the bounds must reject it
MUTANTS = {"eps_inside_sqrt": 1, "eps_before_bias_correction": 1, "decay_dropped": 1, "decay_after_update": 1, "step_off_by_one": 1,
           "clip_missing_in_second_moment": 2, "lr_of_previous_step": 3}


def step_plan(lr=LR):
    """[(step, lr word, clip coefficient, clip pointer given)]: no clip pointer, a coefficient below 1, coefficient 1 after the lr word was halved."""
    return [(1, f32(lr), 1.0, False), (2, f32(lr), CLIP_STEP2, True), (3, f32(lr) * 0.5, 1.0, True)]
