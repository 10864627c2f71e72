"""fp64 reference, per-element bounds, inputs, exact selections and an f32 emulation for the attention checks (numpy only: shared by the GPU cases
of kernel_checks.py and by tests/test_attn_reference_host.py, which tests this tester on the CPU).

What include/tavhip.h documents, per (batch entry, head), L = the entry's valid length (S without lengths), keys and rows >= L outside everything:

    t_ij = scale * log2(e) * q_i . k_j (+ mask_j * log2(e), mode 1)         the logit in the exp2 domain (q_prescaled: t_ij = q~_i . k_j)
    P_ij = 2^t_ij / sum_j 2^t_ij        lse_i = ln 2 * log2 sum_j 2^t_ij
    o_soft = P v        corr_d = sum_j mask_j v_jd (mode 2)        o = o_soft + corr
    delta_i = dO_i . o_soft_i        dS_ij = P_ij (dO_i . v_j - delta_i)
    dV_j = sum_i P_ij dO_i (+ mask_j sum_i dO_i, mode 2)        dK_j = scale sum_i dS_ij q_i        dQ_i = scale sum_j dS_ij k_j

taken from the operands as the kernel holds them (rounded to bf16 / f32 first); the gradients are with respect to the UNSCALED q.

Operands of spread magnitude (make_inputs): query row i is randn * 2^(i % 7 - 3) (its logits have a standard deviation of 1/8 .. 8: nearly
flat to nearly one-hot rows, period 7 coprime to 16 and 64), the columns of v carry 2^(d % 5 - 2), those of dO 2^(d % 7 - 3); `spike` multiplies
key S // 3 by 6 and key S - 7 by 48 (far past ATT_LAZY_THR: the lazy rescale of the pre-scaled forward runs in the last tiles); mode-1 masks
put finfo(float32).min on keys j % 5 == 3 and -65504 on j % 7 == 5 (key 0 stays: no row is fully masked); mode-2 masks are {0, -0.5, 2, 1} by
j % 4 ("small") or the reference style {0, -65504, 65505, 1} in segments.

Bounds per output element, u = 2^-24, derived from csrc/attention.hip.  A_ij = sum_d |q_id| |k_jd|.  Chains (gemm_ref.chain_len): a product
passes KM + 1 additions inside its MFMA and one per later MFMA of the reduction (f32 operands: an fma chain, chain_len below); D = chain_len(64) + 1 (the C operand the accumulator starts
from), D_L = chain_len(L) for the reductions over keys or queries; 2u per addition (nothing documents the matrix unit's internal rounding).

  logit      e_t = D 2u (c A_ij + Mb_i) + 4u (|t_ij| + M_i) + 3u |mask_j log2 e|, c = scale log2(e) (1 when pre-scaled: that rounding is in q
             and the reference shares it).  M_i bounds the running reference exponent while key j still matters: the kernels keep it between
             t_ij - ATT_LAZY_THR and the row maximum, and a key more than 160 below the maximum is flushed to zero by every later
             rescale, so M_i = max {|t_ij| : t_ij >= max_j t_ij - 160} + 12; Mb_i = M_i + log2 L + 1 also covers -lse log2(e), the start
             of the backward accumulators.  The exponent rides every addition of the chain (C operand of the fast path), so it is charged
             at every one of them.  4u: the multiply by c (or the fma), the f32 value of log2(e), the subtraction; 3u: the mask term.
  P          rho_ij = ln 2 e_t + 2u (v_exp_f32, 1 ulp) + 2^-8 (bf16 only: P~ rounded to a bf16 operand, half an ulp) + 3u per rescale
             (ceil(L / 64) + 1 of them at most) + ln 2 * u * 2 M_i (the differences of reference exponents the rescale factors are taken of).
             Keys below the 160 line have rho = 0 and an absolute allowance of 2^-120.  l is summed by the same unit from the same rounded
             P~: rl_i = sum_j P_ij rho_ij + D_L 2u.  No cancellation between numerator and denominator is assumed (the emulation of
             tests/test_attn_reference_host.py shows a common exponent error does cancel; the bound does not need it).
  o_soft     [sum_j P_ij rho_ij |v_jd| + (rl_i + D_L 2u + 3u) sum_j P_ij |v_jd|] / (1 - rl_i): the P errors, the accumulation over L keys,
             1 / l (1 ulp) and its product; then the store (below).
  corr       (n + 5) u sum_j |mask_j v_jd|, n = min(L, L // 4 + 16): a thread adds 16 keys of every 64-key tile (at L = 80 that is 32 keys: a chain
             of L / 4 + 4 would be too short), then four partial sums meet; one more u for the products.
  o          o_soft + corr: the two bounds, u (|o| + both), the store.
  store      f32: u |x|; bf16: half an ulp of bf16 at |x| + E (gemm_ref.bf16_half_ulp), so a truncating store fails.
  lse        rl / (1 - rl) + ln 2 * 3u (|lse log2 e| + 2 M_i + 2) (v_log_f32 at |log2 l| <= |lse log2 e| + M_i + 1, the sum) + 3u |lse|.
  backward   fed o_soft (o) with error e_o and lse with error e_lse per element -- ISOLATED: the reference's values rounded to the storage
             type (e_o = the store term, e_lse = u |lse|); CHAINED: the kernel's own forward, e_o and e_lse = the forward bounds above (that is
             the whole propagation: the backward reads nothing else of the forward).
             delta: sum_d |dO| e_o + 64 u sum_d |dO| (|o| + e_o) (a 64-term fma chain).
             P rebuilt: rb = ln 2 e_t + e_lse + 4u (|lse log2 e| + 1) + 2u, dP_ij = P_ij expm1(rb).
             dP' = dO . v - delta: E = D 2u (sum_d |dO||v| + |delta| + E_delta) + E_delta.   dS = P dP': dP_ij (|dP'| + E) + P E + u |dS|.
             bf16: P and dS enter the second products rounded to bf16: + 2^-8 (|x| + error).
             dV, dK, dQ: sum of the operand errors times |dO|, |q|, |k| + D_L 2u sum (|x| + error) |.| ; the final factor (scale, or ln 2 on the
             pre-scaled path) 2u; mode 2: + |mask_j| (n + 5) u sum_i |dO_id| + u |mask_j sum_i dO| + u |dV|; the store.
  probs      tav_attn_probs: a plain 64-term f32 chain, 66u c A_ij, 2u |t|, 3u |mask log2 e|, 3u |lse log2 e| + e_lse, exp2f 4u; times the
             head factor (2u), plus the mode-2 mask (u).   tav_head_scale: u |f| |b| (the factor), u |f b|, u (|a| + |f b|), the store.

Exact selections (exact_case): a live key is a unit vector e_r, a dead key all ones, a query 0 on the residues it selects and -2048 (stored
pre-scaled: -512) elsewhere.  A selected live key has logit exactly 0, every other key is below -256 in the exp2 domain where v_exp_f32
returns 0, the running maximum ends at exactly 0 on every path.  l is 1, 2 or 4; v, dO and mode-2 mask values are integers in {-7 .. 7}:
o_soft is the exact mean of the selected rows, corr an exact integer sum, o (f32) equals the fp64 value bit for bit and o (bf16) its
round-to-nearest-even, lse is exactly 0 where l = 1.  Live keys sit on both sides of every seam (0, 63, 64, 127, 128, L - 1); mode 1 adds live
DECOY keys (1, 62, L - 2) that every query selects and the mask removes (-65504 and finfo.min in turn); rows >= L of a length-aware launch are
poison: k = 0 (every query would select it), |v|, |dO| = 4096.  With single = True every query selects ONE key: fed lse = 0 and the exact o,
P is in {0, 1}, delta an exact integer, dS, dQ and dK exactly 0, dV the exact scatter-sum of dO rows (+ mask_j sum_i dO_i).  exact_ok proves
that every partial sum stays below 2^24.
"""
import math

import numpy as np

import gemm_ref as GR
from gemm_ref import F, U, bf16_half_ulp, bf16_rne, bf16_trunc, ratio, round_to  # noqa: F401

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
SCALE = 0.125
C2 = SCALE * LOG2E                                        # what a pre-scaled q carries (ops.ATTN_Q_PRESCALE)
LAZY_THR = 12.0                                           # ATT_LAZY_THR
FMIN = float(np.finfo(np.float32).min)
TINY = 2.0 ** -120
RB = 2.0 ** -8                                            # half a bf16 ulp relative to the value itself, at most
DEAD = 160.0                                              # a key this far below the row maximum (exp2 domain) is zero in f32 after any rescale
QA = 2048.0                                               # -QA on the residues a query of an exact case does not select


def _f(x):
    return np.asarray(x, dtype=np.float64).astype(F)


def chain_len(L, dtype):
    """gemm_ref.chain_len, and for f32 operands at least (L + 1) / 2: v_mfma_f32_16x16x4_f32 is a k-ordered fma chain with one rounding per
    product, so a product of a length-L reduction can pass L roundings of u each -- (L + 1) / 2 in the 2u unit the bounds count in."""
    n = GR.chain_len(L, dtype)
    return max(n, -(-(L + 1) // 2)) if dtype == "f32" else n


def sum_chain(L):
    """Longest chain of the per-thread sums of corr and of sum_q dO: 16 (8) rows of every 64 (32)-row tile, then four partial sums."""
    return min(L, L // 4 + 16) + 4


# ---------------------------------------------------------------------------------------------- inputs
def temperatures(S):
    return 2.0 ** ((np.arange(S) % 7) - 3.0)


def v_scale():
    return 2.0 ** ((np.arange(64) % 5) - 2.0)


def do_scale():
    return 2.0 ** ((np.arange(64) % 7) - 3.0)


def clamp_lens(lens, B, S):
    return [S] * B if lens is None else [min(max(int(x), 0), S) for x in lens]


def make_mask(B, S, mode, style="small"):
    if mode == 0:
        return None
    j = np.arange(S)
    m = np.zeros((B, S))
    if mode == 1:
        m[:, j % 5 == 3] = FMIN
        m[:, j % 7 == 5] = -65504.0
        m[:, 0] = 0.0
    elif style == "small":
        m[:] = np.array([0.0, -0.5, 2.0, 1.0])[j % 4]
    else:                                                 # the values the fusion encoder really runs: padded text, valid audio, padded audio
        m[:, S // 4 - min(9, S // 4): S // 4] = -65504.0
        m[:, S // 4: S // 4 + S // 2] = 65505.0
        m[0, S // 4 + S // 2 - min(20, S // 2): S // 4 + S // 2] = 1.0
    return m


def make_inputs(B, S, nh, dtype, mode, pre, seed=0, style="small", spike=False, lens=None):
    """-> dict: q, k, v, do [B][S][nh][64] float64 values the dtype holds (q pre-scaled when `pre`), mask [B][S] or None, lens [B]."""
    rng = np.random.default_rng(seed + 1000 * S + 10 * mode + int(pre))
    q = rng.standard_normal((B, S, nh, 64)) * temperatures(S)[None, :, None, None]
    k = rng.standard_normal((B, S, nh, 64))
    if spike and S >= 16:
        k[:, S // 3] *= 6.0
        k[:, S - 7] *= 48.0
    v = rng.standard_normal((B, S, nh, 64)) * v_scale()
    do = rng.standard_normal((B, S, nh, 64)) * do_scale()
    if pre:
        q = q * C2
    q, k, v, do = (round_to(t, dtype)[0] for t in (q, k, v, do))
    return dict(q=q, k=k, v=v, do=do, mask=make_mask(B, S, mode, style), lens=clamp_lens(lens, B, S), B=B, S=S, nh=nh, dtype=dtype, mode=mode,
                pre=bool(pre))


# ---------------------------------------------------------------------------------------------- reference and bounds
def _store(val, err, dtype):
    if dtype == "bf16":
        return err + bf16_half_ulp(np.abs(val) + err)
    return err + U * (np.abs(val) + err)


def _slice_ref(q, k, v, do, mask, mode, pre, dtype):
    """One (batch entry, head) at its valid length: q, k, v, do [L][64], mask [L] or None.  -> dict of values and bounds, fp64."""
    L = q.shape[0]
    D, DL = chain_len(64, dtype) + 1, chain_len(L, dtype)
    c = 1.0 if pre else C2
    A = np.abs(q) @ np.abs(k).T
    mt = np.zeros(L)
    if mode == 1:
        mt = np.maximum(mask * LOG2E, -1e300)
    t = (q @ k.T) * c + mt[None, :]
    tm = t.max(1, keepdims=True)
    live = t >= tm - DEAD
    p = np.exp2(t - tm)
    lsum = p.sum(1, keepdims=True)
    P = p / lsum
    lse2 = (tm + np.log2(lsum))[:, 0]
    lse = lse2 * LN2
    M = np.where(live, np.abs(t), 0.0).max(1) + LAZY_THR
    Mb = M + math.log2(L) + 1.0
    e_t = np.where(live, D * 2 * U * (c * A + Mb[:, None]) + 4 * U * (np.abs(t) + M[:, None]) + 3 * U * np.abs(mt)[None, :], 0.0)
    nres = -(-L // 64) + 1
    rho = np.where(live, LN2 * e_t + 2 * U + (RB if dtype == "bf16" else 0.0) + nres * 3 * U + LN2 * U * 2 * M[:, None], 0.0)
    rl = (P * rho).sum(1) + DL * 2 * U
    assert rl.max() < 0.25
    g = (1.0 + 2.0 * rho.max()) / (1.0 - rl)
    absv = np.abs(v)
    o_soft = P @ v
    E_soft = ((P * rho) @ absv + (rl + DL * 2 * U + 3 * U)[:, None] * (P @ absv)) * g[:, None] + TINY * absv.sum(0)[None, :]
    r = dict(L=L, P=P, lse=lse, o_soft=o_soft, o_soft_bound=_store(o_soft, E_soft, dtype))
    r["lse_bound"] = rl * g + LN2 * 3 * U * (np.abs(lse2) + 2 * M + 2.0) + 3 * U * np.abs(lse)
    if mode == 2:
        corr = mask @ v
        E_corr = (sum_chain(L) + 1) * U * (np.abs(mask) @ absv)
        o = o_soft + corr[None, :]
        E_o = E_soft + E_corr[None, :]
        E_o = E_o + U * (np.abs(o) + E_o)
        r.update(corr=corr, corr_bound=E_corr + U * np.abs(corr), o=o, o_bound=_store(o, E_o, dtype))
    else:
        r.update(o=o_soft, o_bound=r["o_soft_bound"])
    # ---- backward, isolated (fed the reference rounded to the storage types) and chained (fed the kernel's own forward)
    dP = do @ v.T
    Adv = np.abs(do) @ absv.T
    delta = (do * o_soft).sum(1)
    absdo = np.abs(do)
    kq = (SCALE / C2) if pre else SCALE
    for tag, e_o, e_lse in (("", _store(o_soft, 0.0, dtype), U * np.abs(lse)), ("_chained", r["o_soft_bound"], r["lse_bound"])):
        E_delta = (absdo * e_o).sum(1) + 64 * U * (absdo * (np.abs(o_soft) + e_o)).sum(1)
        rb = np.where(live, LN2 * e_t + (e_lse + 4 * U * (np.abs(lse2) + 1.0))[:, None] + 2 * U, 0.0)
        dPn = P * np.expm1(rb) + TINY
        dpp = dP - delta[:, None]
        E_dP = D * 2 * U * (Adv + (np.abs(delta) + E_delta)[:, None]) + E_delta[:, None]
        dS = P * dpp
        E_dS = dPn * (np.abs(dpp) + E_dP) + P * E_dP + U * np.abs(dS)
        eP, eS = dPn, E_dS
        if dtype == "bf16":
            eP, eS = dPn + RB * (P + dPn), E_dS + RB * (np.abs(dS) + E_dS) + TINY
        dv = P.T @ do
        E_dv = eP.T @ absdo + DL * 2 * U * ((P + eP).T @ absdo)
        if mode == 2:
            term = mask[:, None] * do.sum(0)[None, :]
            E_dv = E_dv + np.abs(mask)[:, None] * ((sum_chain(L) + 1) * U * absdo.sum(0))[None, :] + U * np.abs(term) + U * (np.abs(dv + term) + E_dv)
            dv = dv + term
        dk = kq * (dS.T @ q)
        E_dk = kq * (eS.T @ np.abs(q) + DL * 2 * U * ((np.abs(dS) + eS).T @ np.abs(q)))
        dq = SCALE * (dS @ k)
        E_dq = SCALE * (eS @ np.abs(k) + DL * 2 * U * ((np.abs(dS) + eS) @ np.abs(k)))
        E_dk, E_dq = E_dk + 2 * U * (np.abs(dk) + E_dk), E_dq + 2 * U * (np.abs(dq) + E_dq)
        r.update({"delta": delta, "dq": dq, "dk": dk, "dv": dv, "delta_bound" + tag: E_delta + U * np.abs(delta),
                  "dq_bound" + tag: _store(dq, E_dq, dtype), "dk_bound" + tag: _store(dk, E_dk, dtype), "dv_bound" + tag: _store(dv, E_dv, dtype)})
    return r


OUT4 = ("o", "o_soft", "dq", "dk", "dv")                  # [B][S][nh][64]
OUTROW = ("lse", "delta")                                 # [B][nh][S]


def attn_ref(x):
    """x = make_inputs(...) or exact_case(...).  -> dict name -> array and name_bound (and name_bound_chained for delta, dq, dk, dv) in the kernels'
    layouts: o, o_soft, dq, dk, dv [B][S][nh][64]; lse, delta [B][nh][S]; corr [B][nh][64]; probs [B][nh][S][S] (the softmax part, zero outside
    L x L).  Rows and keys >= L_b: value 0, bound 0 (delta there is not written: compare [:L_b] only)."""
    B, S, nh, mode = x["B"], x["S"], x["nh"], x["mode"]
    names = [n for n in OUT4] + [n + "_bound" for n in OUT4] + [n + "_bound_chained" for n in ("dq", "dk", "dv")]
    res = {n: np.zeros((B, S, nh, 64)) for n in names}
    for n in ("lse", "lse_bound", "delta", "delta_bound", "delta_bound_chained"):
        res[n] = np.zeros((B, nh, S))
    for n in ("corr", "corr_bound"):
        res[n] = np.zeros((B, nh, 64))
    res["probs"] = np.zeros((B, nh, S, S))
    for b in range(B):
        L = x["lens"][b]
        if L == 0:
            continue
        for h in range(nh):
            s = _slice_ref(x["q"][b, :L, h], x["k"][b, :L, h], x["v"][b, :L, h], x["do"][b, :L, h], None if mode == 0 else x["mask"][b, :L], mode,
                           x["pre"], x["dtype"])
            for n in names:
                if n in s:
                    res[n][b, :L, h] = s[n]
            for n in ("lse", "lse_bound", "delta", "delta_bound", "delta_bound_chained"):
                res[n][b, h, :L] = s[n]
            if mode == 2:
                res["corr"][b, h], res["corr_bound"][b, h] = s["corr"], s["corr_bound"]
            res["probs"][b, h, :L, :L] = s["P"]
    return res


def fed(ref, x):
    """What the isolated backward is fed: the reference's o, o_soft, lse, corr rounded to the storage types."""
    return dict(o=round_to(ref["o"], x["dtype"])[0], o_soft=round_to(ref["o_soft"], x["dtype"])[0], lse=_f(ref["lse"]).astype(np.float64),
                corr=_f(ref["corr"]).astype(np.float64))


def probs_ref(x, ref, head_scale=None):
    """tav_attn_probs fed f32(ref lse), no lengths.  head_scale: None, [nh] or [B][nh].  -> (probs, bound) [B][nh][S][S]."""
    B, S, nh, mode, dtype = x["B"], x["S"], x["nh"], x["mode"], x["dtype"]
    f = np.ones((B, nh)) if head_scale is None else np.broadcast_to(np.asarray(head_scale, dtype=np.float64).reshape(-1, nh), (B, nh))
    c = 1.0 if x["pre"] else C2
    out, bound = np.zeros((B, nh, S, S)), np.zeros((B, nh, S, S))
    for b in range(B):
        mt = np.maximum(x["mask"][b] * LOG2E, -1e300) if mode == 1 else np.zeros(S)
        for h in range(nh):
            q, k = x["q"][b, :, h], x["k"][b, :, h]
            P = ref["probs"][b, h]
            t = (q @ k.T) * c
            lse2 = ref["lse"][b, h] * LOG2E
            e = 66 * U * c * (np.abs(q) @ np.abs(k).T) + 2 * U * np.abs(t) + 3 * U * np.abs(mt)[None, :] + (4 * U * np.abs(lse2))[:, None]
            e = e + U * np.abs(t + mt[None, :] - lse2[:, None])
            dPn = np.where(P > 0, P * np.expm1(np.minimum(LN2 * e + 4 * U, 1.0)), 0.0)
            v = f[b, h] * P
            E = abs(f[b, h]) * (dPn + 2 * U * P)
            if mode == 2:
                v = v + x["mask"][b][None, :]
                E = E + U * (np.abs(v) + E)
            out[b, h], bound[b, h] = v, E + np.where(P > 0, TINY, 0.0)
    return out, bound


def head_scale_ref(a, b, f, dtype):
    """out = a + f * b (a may be None); a, b [rows][nh][64], f [rows][nh] (c0 + head factor, fp64 of f32 operands).  -> (out, bound)."""
    fb = f[:, :, None] * b
    a0 = 0.0 if a is None else a
    out = a0 + fb
    E = 2 * U * np.abs(fb) + U * (np.abs(a0) + np.abs(fb))
    return out, _store(out, E, dtype)


# ---------------------------------------------------------------------------------------------- exact selections
def exact_case(B, S, nh, dtype, mode, pre, lens=None, single=False, seed=0):
    """Operands with ONE right answer (module docstring).  -> the dict of make_inputs plus `sel` [B][S][S] bool (query i selects key j, mask
    applied).  attn_ref(case) is then exact: compare with equality (o in bf16: bf16_rne of it)."""
    rng = np.random.default_rng(seed + 7 * S + mode)
    lens = clamp_lens(lens, B, S)
    q = np.zeros((B, S, nh, 64))
    k = np.zeros((B, S, nh, 64))
    v = rng.integers(-7, 8, size=(B, S, nh, 64)).astype(np.float64)
    do = rng.integers(-7, 8, size=(B, S, nh, 64)).astype(np.float64)
    mask = None if mode == 0 else np.zeros((B, S))
    if mode == 2:
        mask = rng.integers(-7, 8, size=(B, S)).astype(np.float64)
    sel = np.zeros((B, S, S), dtype=bool)
    qa = -512.0 if pre else -QA
    for b in range(B):
        L = lens[b]
        sign = np.where(rng.integers(0, 2, size=(S - L, nh, 64)) > 0, 4096.0, -4096.0)
        v[b, L:], do[b, L:] = sign, -sign                     # poison (k = q = 0 there)
        if mode == 1:
            mask[b, L:] = 0.0
        if L == 0:
            continue
        livek = sorted({j for j in (0, 63, 64, 127, 128, L - 1) if j < L})
        decoy = sorted({j for j in (1, 62, L - 2) if 0 < j < L and j not in livek}) if mode == 1 else []
        res = {j: (17 * n + 5) % 64 for n, j in enumerate(livek + decoy)}
        k[b, :L] = 1.0
        for j, r in res.items():
            k[b, j] = 0.0
            k[b, j, :, r] = 1.0
        for n, j in enumerate(decoy):
            mask[b, j] = FMIN if n % 2 else -65504.0
        nl = len(livek)
        for i in range(L):
            want = 1 if single else (1, 1, 2, 4)[i % 4]
            while want > nl:
                want //= 2
            mine = [livek[(3 * i + 1 + c) % nl] for c in range(want)]
            q[b, i] = qa
            for j in mine + decoy:
                q[b, i, :, res[j]] = 0.0
            sel[b, i, mine] = True
    return dict(q=q, k=k, v=v, do=do, mask=mask, lens=lens, B=B, S=S, nh=nh, dtype=dtype, mode=mode, pre=bool(pre), sel=sel, single=single)


def exact_ok(x):
    """Every partial sum of an exact case is an integer (or a multiple of 1/4) below 2^24 in any order: the 64-term dot products (<= 64 * 49, the
    query's -2048 times a one: <= 64 * 2048), sums over L rows of |v|, |dO| <= 7 times |mask| <= 7 plus l <= 4 selected rows."""
    L = max(x["lens"])
    return 64 * QA < 2 ** 24 and 4 * (L * 49 + 64 * 49 + 4 * 7) < 2 ** 24 and all(
        set(np.unique(np.abs(x[n][b, :x["lens"][b]]))) <= set(range(8)) for n in ("v", "do") for b in range(x["B"]))


def exact_want(x):
    """-> dict of the exact outputs in the kernels' layouts (o, o_soft, lse where l = 1 [nan elsewhere], corr, probs; with single: delta, dq, dk, dv)."""
    B, S, nh, mode = x["B"], x["S"], x["nh"], x["mode"]
    sel = x["sel"].astype(np.float64)
    cnt = sel.sum(2)
    P = sel / np.maximum(cnt, 1.0)[:, :, None]
    valid = np.zeros((B, S))
    for b, L in enumerate(x["lens"]):
        valid[b, :L] = 1.0
    o_soft = np.einsum("bij,bjhd->bihd", P, x["v"])
    w = dict(o_soft=o_soft, o=o_soft.copy(), corr=np.zeros((B, nh, 64)), probs=np.broadcast_to(P[:, None], (B, nh, S, S)).copy())
    lse = np.where(cnt == 1, 0.0, np.nan) * np.where(valid > 0, 1.0, np.nan)
    lse = np.where(valid > 0, lse, 0.0)
    w["lse"] = np.broadcast_to(lse[:, None], (B, nh, S)).copy()
    w["lse_full"] = np.broadcast_to((np.log(np.maximum(cnt, 1.0)) * valid)[:, None], (B, nh, S)).copy()
    if mode == 2:
        w["corr"] = np.einsum("bj,bjhd->bhd", x["mask"] * valid, x["v"])
        w["o"] = (o_soft + w["corr"][:, None]) * valid[:, :, None, None]
        w["probs"] = w["probs"] + (x["mask"] * valid)[:, None, None, :] * valid[:, None, :, None]
    if x["single"]:
        w["delta"] = np.einsum("bihd,bihd->bhi", x["do"], o_soft) * valid[:, None, :]
        dv = np.einsum("bij,bihd->bjhd", P, x["do"])
        if mode == 2:
            dv = dv + (x["mask"] * valid)[:, :, None, None] * np.einsum("bi,bihd->bhd", valid, x["do"])[:, None]
        w.update(dv=dv, dq=np.zeros_like(dv), dk=np.zeros_like(dv))
    return w


# ---------------------------------------------------------------------------------------------- f32 emulation (host test of the tester)
ORDERS = ("forward", "reversed", "tileperm")
MUTANTS = {1: "one_key_dropped", 2: "first_key_of_tile_twice", 3: "key_L_included", 4: "clamped_copy_has_weight", 5: "lazy_move_without_rescale",
           6: "l_rescaled_o_not", 7: "p_truncated_to_bf16", 8: "o_store_truncates", 9: "mode1_mask_after_softmax", 10: "corr_over_padded_keys",
           11: "corr_missing_from_o", 12: "o_soft_holds_o", 13: "lse_without_log_l", 14: "lse_in_base_2", 15: "delta_from_o", 16: "delta_of_neighbour",
           17: "dk_times_scale_on_pre_path", 18: "dq_scaled_twice", 19: "dv_without_mask_term", 20: "mask_term_over_padded_rows",
           21: "padded_query_row_has_probability"}
FWD_MUTANTS = tuple(range(1, 15))
BWD_MUTANTS = tuple(range(15, 22))


def emu_acc(a, b, dtype, acc=None):
    """sum_k a[m][k] b[n][k] into an f32 accumulator, one rounding per MFMA (MFMA_K products each, exact in fp64), steps in the order given."""
    km = GR.MFMA_K[dtype]
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=F) if acc is None else acc
    for k0 in range(0, a.shape[1], km):
        acc = (acc.astype(np.float64) + a[:, k0:k0 + km] @ b[:, k0:k0 + km].T).astype(F)
    return acc


def _tiles(n, order, rng):
    tiles = [np.arange(t0, min(t0 + 64, n)) for t0 in range(0, n, 64)]
    if order == "reversed":
        return [t[::-1] for t in tiles[::-1]]
    if order == "tileperm":
        return [tiles[i] for i in rng.permutation(len(tiles))]
    return tiles


def _exp2(x):
    """v_exp_f32: f32 result, denormals flushed."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        y = np.exp2(np.asarray(x, dtype=np.float64)).astype(F)
    return np.where(y < F(2.0 ** -126), F(0.0), y)


def _seq_sum(terms):
    """f32 chain sum over axis 0."""
    if terms.shape[0] == 0:
        return np.zeros(terms.shape[1:], dtype=F)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.add.accumulate(terms.astype(F), axis=0, dtype=F)[-1]


def _kadd(mask_vals):
    with np.errstate(over="ignore"):
        return (mask_vals.astype(F) * F(LOG2E)).astype(F)


def _st(x, dtype, trunc=False):
    x = np.asarray(x, dtype=F)
    if dtype == "f32" and not trunc:
        return x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return bf16_trunc(x) if trunc else bf16_rne(x)


def emu_fwd(x, order="forward", mutant=None, drop_key=None):
    """The forward kernels' arithmetic in f32 (64-key tiles in `order`; the pre-scaled unmasked tiles but the last on the lazy path with the
    reference exponent as accumulator start; P rounded to bf16 for bf16, l summed from the rounded P).  -> dict o, o_soft, lse, corr in the
    kernels' layouts, float64 of what the storage types hold.  mutant: None or a name of MUTANTS; drop_key: the key mutant 1 drops."""
    B, S, nh, mode, pre, dtype = x["B"], x["S"], x["nh"], x["mode"], x["pre"], x["dtype"]
    rng = np.random.default_rng(5)
    out = dict(o=np.zeros((B, S, nh, 64)), o_soft=np.zeros((B, S, nh, 64)), lse=np.zeros((B, nh, S)), corr=np.zeros((B, nh, 64)))
    c2f = F(F(SCALE) * F(LOG2E))
    emode = 2 if mutant == "mode1_mask_after_softmax" else mode
    for b in range(B):
        L = x["lens"][b]
        if L == 0:
            continue
        tiles = _tiles(L, order, rng)
        for h in range(nh):
            q, kall, vall = x["q"][b, :L, h], x["k"][b, :, h], x["v"][b, :, h]
            m, l, O = np.full(L, -1e30, dtype=F), np.zeros((L, 1), dtype=F), np.zeros((L, 64), dtype=F)
            for ti, idx in enumerate(tiles):
                idx = np.asarray(idx)
                if (L - 1) in idx:
                    if mutant == "key_L_included" and L < S:
                        idx = np.append(idx, L)
                    if mutant == "clamped_copy_has_weight" and L % 64:
                        idx = np.append(idx, L - 1)
                kt, vt = kall[idx], vall[idx]
                ka = _kadd(x["mask"][b, idx]) if emode == 1 else np.zeros(len(idx), dtype=F)
                first, last = ti == 0, ti == len(tiles) - 1
                with np.errstate(over="ignore", invalid="ignore"):
                    if pre and emode != 1 and not last:
                        sacc = emu_acc(q, kt, dtype, acc=np.zeros((L, len(idx)), dtype=F) if first else np.repeat(-m[:, None], len(idx), 1))
                        mx = sacc.max(1)
                        grow = np.full(L, True) if first else mx > F(LAZY_THR)
                        shift = np.where(grow, mx if first else np.maximum(mx, F(0.0)), F(0.0)).astype(F)
                        m = np.where(grow, shift if first else (m + shift).astype(F), m).astype(F)
                        sacc = (sacc - shift[:, None]).astype(F)
                        if not first and mutant != "lazy_move_without_rescale":
                            al = _exp2(-shift)[:, None]
                            l, O = (l * al).astype(F), (O * al).astype(F)
                        p = _exp2(sacc)
                    else:
                        sacc = emu_acc(q, kt, dtype)
                        s2 = sacc if pre else (sacc * c2f).astype(F)
                        s2 = (s2 + ka[None, :]).astype(F)
                        m_new = np.maximum(m, s2.max(1)).astype(F)
                        al = _exp2(m - m_new)[:, None]
                        p = _exp2((s2 - m_new[:, None]).astype(F))
                        l = (l * al).astype(F)
                        if mutant != "l_rescaled_o_not":
                            O = (O * al).astype(F)
                        m = m_new
                if mutant == "one_key_dropped" and drop_key in idx:
                    p[:, list(idx).index(drop_key)] = 0.0
                if mutant == "first_key_of_tile_twice" and idx.min() >= 64:
                    p, vt = np.concatenate([p, p[:, :1]], 1), np.concatenate([vt, vt[:1]], 0)
                if dtype == "bf16" or mutant == "p_truncated_to_bf16":
                    pop = bf16_trunc(p) if mutant == "p_truncated_to_bf16" else bf16_rne(p)
                else:
                    pop = p.astype(np.float64)
                l = emu_acc(pop, np.ones((1, pop.shape[1])), dtype, acc=l)
                O = emu_acc(pop, vt.T, dtype, acc=O)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                inv = (F(1.0) / l).astype(F)
                osoft = (O * inv).astype(F)
                o = osoft
                if emode == 2:
                    n = S if mutant == "corr_over_padded_keys" else L
                    order_rows = np.concatenate(_tiles(n, order, rng))
                    corr = _seq_sum((x["mask"][b, order_rows, None] * vall[order_rows]))
                    if mutant != "corr_missing_from_o":
                        o = (osoft + corr[None, :]).astype(F)
                    out["corr"][b, h] = corr
                l2 = np.log2(l[:, 0].astype(np.float64)).astype(F)
                lse = ((m + l2).astype(F) * F(LN2)).astype(F)
                if mutant == "lse_without_log_l":
                    lse = (m * F(LN2)).astype(F)
                if mutant == "lse_in_base_2":
                    lse = (m + l2).astype(F)
            out["o"][b, :L, h] = _st(o, dtype, mutant == "o_store_truncates")
            out["o_soft"][b, :L, h] = _st(o if mutant == "o_soft_holds_o" else osoft, dtype) if mode == 2 else out["o"][b, :L, h]
            out["lse"][b, h, :L] = lse
    return out


def emu_bwd(x, o_fed, lse_fed, order="forward", mutant=None):
    """The two backward kernels' arithmetic in f32: delta as an fma chain, S and dP accumulators started at -lse / scale (-lse log2 e) and
    -delta, P and dS rounded to bf16 operands for bf16, reductions over queries / keys in `order`.  o_fed: what the kernel reads for delta (o_soft
    in mode 2) [B][S][nh][64]; lse_fed [B][nh][S].  -> dict delta, dq, dk, dv."""
    B, S, nh, mode, pre, dtype = x["B"], x["S"], x["nh"], x["mode"], x["pre"], x["dtype"]
    rng = np.random.default_rng(6)
    out = dict(dq=np.zeros((B, S, nh, 64)), dk=np.zeros((B, S, nh, 64)), dv=np.zeros((B, S, nh, 64)), delta=np.zeros((B, nh, S)))
    c2f = F(F(SCALE) * F(LOG2E))
    lse_mul = F(LOG2E) if pre else F(1.0 / SCALE)
    dk_mul = F(LN2) if (pre and mutant != "dk_times_scale_on_pre_path") else F(SCALE)
    for b in range(B):
        L = x["lens"][b]
        if L == 0:
            continue
        perm = np.concatenate(_tiles(L, order, rng))
        for h in range(nh):
            q, k, v, do = (x[n][b, :L, h] for n in ("q", "k", "v", "do"))
            delta = np.zeros(L, dtype=F)
            for d in range(64):
                delta = (do[:, d] * o_fed[b, :L, h, d] + delta.astype(np.float64)).astype(F)
            out["delta"][b, h, :L] = delta
            dl = np.roll(delta, -1) if mutant == "delta_of_neighbour" else delta
            start = (-(lse_fed[b, h, :L].astype(F) * lse_mul)).astype(F)
            ka = _kadd(x["mask"][b, :L]) if mode == 1 else np.zeros(L, dtype=F)
            with np.errstate(over="ignore", invalid="ignore"):
                sp = emu_acc(q, k, dtype, acc=np.repeat(start[:, None], L, 1))
                arg = (sp + ka[None, :]).astype(F) if pre else (sp.astype(np.float64) * np.float64(c2f) + ka[None, :].astype(np.float64)).astype(F)
                p = _exp2(arg)
                dpp = emu_acc(do, v, dtype, acc=np.repeat(-dl[:, None], L, 1))
                ds = (p * dpp).astype(F)
            qq, dd = q, do
            if mutant == "padded_query_row_has_probability" and L % 64:
                p, ds, qq, dd = np.vstack([p, p[-1:]]), np.vstack([ds, ds[-1:]]), np.vstack([q, q[-1:]]), np.vstack([do, do[-1:]])
            pq = np.append(perm, L) if p.shape[0] > L else perm
            pop, dsop = (bf16_rne(p), bf16_rne(ds)) if dtype == "bf16" else (p.astype(np.float64), ds.astype(np.float64))
            dv = emu_acc(pop.T[:, pq], dd.T[:, pq], dtype)
            if mode == 2 and mutant != "dv_without_mask_term":
                n = S if mutant == "mask_term_over_padded_rows" else L
                dosum = _seq_sum(x["do"][b, np.concatenate(_tiles(n, order, rng)), h])
                dv = (dosum[None, :].astype(np.float64) * x["mask"][b, :L, None] + dv).astype(F)
            dk = (emu_acc(dsop.T[:, pq], qq.T[:, pq], dtype) * dk_mul).astype(F)
            dq = (emu_acc(dsop[:L][:, perm], k.T[:, perm], dtype) * F(SCALE)).astype(F)
            if mutant == "dq_scaled_twice":
                dq = (dq * F(SCALE)).astype(F)
            out["dv"][b, :L, h], out["dk"][b, :L, h], out["dq"][b, :L, h] = _st(dv, dtype), _st(dk, dtype), _st(dq, dtype)
    return out


def emu_probs(x, lse_fed):
    """tav_attn_probs in f32 (no head factor): a 64-term chain, exp2 of the difference, the mode-2 mask added last."""
    B, S, nh, mode = x["B"], x["S"], x["nh"], x["mode"]
    out = np.zeros((B, nh, S, S))
    c = F(1.0) if x["pre"] else F(F(SCALE) * F(LOG2E))
    for b in range(B):
        for h in range(nh):
            dot = np.zeros((S, S), dtype=F)
            for d in range(64):
                dot = (np.outer(x["q"][b, :, h, d], x["k"][b, :, h, d]) + dot.astype(np.float64)).astype(F)
            s2 = (dot * c).astype(F)
            if mode == 1:
                s2 = (s2 + _kadd(x["mask"][b])[None, :]).astype(F)
            l2 = (lse_fed[b, h].astype(F) * F(LOG2E)).astype(F)
            pr = _exp2((s2 - l2[:, None]).astype(F))
            if mode == 2:
                pr = (pr + x["mask"][b].astype(F)[None, :]).astype(F)
            out[b, h] = pr
    return out


# ---------------------------------------------------------------------------------------------- the shapes the GPU cases run
BOUND_S = (1, 63, 64, 65, 128, 129, 193, 257, 321)        # 1, 2, 3 and 4+ key tiles, ragged and full; one and two 128-key workgroups and more
EXACT_S = (64, 65, 129, 257)
LEN_CASES = {65: ([0, 1, 65], [64, 65, 33]), 129: ([129, 0, 64], [65, 1, 128]), 257: ([257, 65, 200],)}      # lengths {0, 1, 64, 65, S} and two ragged
CHAINED_S = 193
FWD_OUT = ("o", "o_soft", "corr", "lse")
BWD_OUT = ("delta", "dq", "dk", "dv")


def bound_config(S, mode, pre, lens=None):
    """Keyword arguments of make_inputs for the bounded GPU case (S, mode, pre): spiked keys from two tiles on, the reference-style mode-2 mask
    where q is pre-scaled (what the fusion encoder runs), the small-valued one otherwise."""
    return dict(mode=mode, pre=pre, spike=S >= 128, style="ref" if pre else "small", lens=lens)


def fwd_ratios(x, ref, got):
    """Worst error / bound per forward output (delta and lse rows past a length hold nothing the contract promises beyond 0)."""
    return {n: ratio(got[n], ref[n], ref[n + "_bound"]) for n in FWD_OUT if n != "corr" or x["mode"] == 2}


def bwd_ratios(x, ref, got, chained=False):
    sfx = "_bound_chained" if chained else "_bound"
    r = {n: ratio(got[n], ref[n], ref[n + sfx]) for n in ("dq", "dk", "dv")}
    r["delta"] = max([0.0] + [ratio(got["delta"][b, :, :L], ref["delta"][b, :, :L], ref["delta" + sfx][b, :, :L]) for b, L in enumerate(x["lens"])])
    return r
