"""fp64 references, per-element bounds, inputs, exact cases and an f32 emulation for the audio front-end, pooling, head, loss and index checks
(numpy only: shared by the GPU cases of kernel_checks.py and by tests/test_front_reference_host.py, which tests this tester on the CPU).
Kernels: csrc/audio_frontend.hip, the pooling / head / loss / index kernels of csrc/elementwise.hip, tav_colsum (csrc/gemm.hip) and the stand-alone
tav_gelu_fwd / tav_gelu_bwd (csrc/norm.hip).

Inputs have SPREAD magnitudes: channel c is scaled by 2^(c % 7 - 3), tap j by 2^(j % 5 - 2), rows cycle through the scales 2^(r % 7 - 3) and the
offsets 0, 3 scale, 64 scale as norm_ref.ln_inputs does; everything is rounded to the storage dtype before the reference sees it.

Bounds, u = 2^-24, charged through norm_ref.V (a sum or difference: the operands' errors and u (|result| + error); a product likewise; a sum over a
chain of D additions: the summed term errors and D u / (1 - D u) times the summed MAGNITUDES).  A product that enters a sum counts as one more link
of the chain, so the bounds hold whether or not the compiler contracts the multiply-add (csrc/Makefile sets no -ffp-contract).  Division and sqrtf
are correctly rounded (hipcc's default): u.  expf, logf, tanhf: the OpenCL full-profile limits ROCm's device library is specified to meet, 3, 3 and
5 ulp, written 6u, 6u and 10u relative (the ROCm installation ships no tighter table); the error of expf's argument z - m enters
as |z - m| u relative; a result below the smallest normal f32, 2^-126, may be flushed to zero, so expf's value and the
last product of dlogits carry 2^-126 absolute.  Stores: f32 nothing more, bf16 half an ulp at |v| + E (gemm_ref).  The chains, from the source:

  conv0 forward      conv0_fwd_kernel: a = bias, then `a += x w` for the K taps in order: K + 1.
  conv0 wgrad        conv0_bwd_w_kernel: thread (cq, tg) takes the steps tg, tg + 4, ... of its chunk of C0_BT = 512: ceil(tmax / 4) + 1; the tree
                     over the four time groups is two additions deep ((a0 + a2) + (a1 + a3)), charged 3; conv0_bwd_w_final_kernel: rows k = rg,
                     rg + 4, ... of the nblocks = B ceil(T_out / 512) partial blocks, then red[0] + red[1] + red[2] + red[3]: ceil(nblocks / 4) + 3;
                     + 1 when it accumulates.
  four chains        wn_colsum_final_kernel, colsum_partial_kernel, colsum_final_kernel: s0 .. s3 take n // 4 terms each, s0 the n % 4 left over,
                     then (s0 + s1) + (s2 + s3): D4(n) = n // 4 + n % 4 + 2 (= ceil(n / 4) + 2 where 4 divides n).
  weight norm        wn_colsum_partial_kernel: rpb = ceil(rows / nb) rows in one chain, nb = min(512, ceil(H Cg / 256)): rpb + 1, then D4(nb), sqrtf;
                     w = (g v) / ||v||.  Backward: dots through the same two kernels, dv = g / n (dw - v dots / (n n)), dg = dots / n, + 1 each
                     when accumulating; ISOLATED it is fed the reference's norms rounded to f32, CHAINED the kernel's own (error = the forward bound).
  colsum             D4(rows_per_block) + D4(nparts) (+ 1 accumulating), rows_per_block = ceil(M / nparts).
  col2im             at most ceil(K / stride) terms in tap order, then the gelu' product (gemm_ref's terms, flavour of the tensor dtype).
  mean pool          mean_pool_fwd_kernel: ceil(S / 16) rows per row group, 15 additions over the groups, then a (1.f / S): an f32 reciprocal (u unless
                     S is a power of two) that is then multiplied.  Length-aware: L_b = clamp(lens[b], 0, S) in place of S; L_b = 0 gives exactly 0.
  head               head_fwd_kernel: ceil(K / 64) + 1 per lane, 6 for wave_sum, then the bias.  head_bwd_kernel: chains of N + 1 (dx) and of B + 1
                     (dW, db; + 1 accumulating).
  tanh               y = tanhf(x); dx = dy (1 - y y) from the STORED y.
  cross entropy      per row m = max z (exact), se = sum_c expf(z_c - m) over C, logf, w (m + log se - z_t); each of 256 threads chains its
                     ceil(B / 256) rows, a tree of 8 levels joins them, loss = num / den; dlogits = (w grad_scale / den) (expf(z_c - m) / se - [c = t]).

Exact cases (exact=True of the input builders): data integers in {-7 .. 7}, weights / g / scales powers of two, previous contents integers times 64;
every sum in any order is an integer below 2^24 (exact_ok), so the reference IS the one right answer and is compared bit for bit (a bf16 output with
its round-to-nearest-even).  Weight norm: one non-zero power of two per tap, so ||v|| = 2^k exactly.  The mean pools at S and L_b powers of two.
The copies (group_pad, gather_rows, patchify, embed_add_fwd, text_embed's pre and pos_ids) are exact for any data.
"""
import functools
import math

import numpy as np

import gemm_ref as GR
import norm_ref as NR
from gemm_ref import F, U, bf16_half_ulp, bf16_rne, bf16_trunc, ratio  # noqa: F401
from norm_ref import V, _g, fed, gsum, inv, lp_bound, rnd, vgelu, vgelu_d  # noqa: F401

EXP_REL, LOG_REL, TANH_REL = 6 * U, 6 * U, 10 * U          # 3, 3 and 5 ulp (OpenCL full profile)
TINY = 2.0 ** -126                                          # the smallest normal f32: a result below it may be flushed to zero
C0_BT = 512
WN_MAX_BLOCKS = 512

MUTANTS = {1: "conv0_reads_x_plus_1", 2: "last_tap_dropped", 3: "bias_once_per_tap", 4: "bf16_store_truncates", 5: "wgrad_skips_last_step",
           6: "wgrad_t0_of_previous_chunk", 7: "time_group_missing", 8: "final_drops_k_mod_4_eq_3", 9: "dbias_from_column_k_minus_1",
           10: "accumulate_overwrites", 11: "second_pass_overwrites_first", 12: "norms_over_co_k", 13: "norm_without_sqrt", 14: "w_flip_unreversed",
           15: "w_transposed_in_group", 16: "dv_without_projection", 17: "dg_not_divided", 18: "blocks_past_first_dropped",
           19: "group_pad_left_frame_off_by_one", 20: "group_pad_frame_unwritten", 21: "col2im_ignores_phase", 22: "col2im_gelu_at_sum",
           23: "colsum_drops_ragged_rows", 24: "colsum_n_for_ld", 25: "pool_divides_by_padded_s", 26: "len_pool_divides_by_s",
           27: "len_pool_bwd_past_len", 28: "head_idle_lanes_left_out", 29: "head_dw_from_w", 30: "head_db_over_n", 31: "ce_without_max",
           32: "ce_mean_over_b", 33: "ce_grad_scale_on_loss", 34: "ce_rows_ge_256_missing", 35: "ce_onehot_before_normalising", 36: "tanh_grad_from_x",
           37: "pos_ids_count_pads", 38: "pos_ids_scan_stops_at_64", 39: "embed_add_bwd_drops_row_7", 40: "scatter_second_match_twice",
           41: "gelu_tanh_flavour"}


def _f(a):
    return np.asarray(a, dtype=np.float64).astype(F)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(F).astype(np.float64)


def ch_scale(n):
    return 2.0 ** (np.arange(n) % 7 - 3.0)


def tap_scale(n):
    return 2.0 ** (np.arange(n) % 5 - 2.0)


def row_affine(n):
    """(scale, offset) per row, the cycles of norm_ref.ln_inputs."""
    r = np.arange(n)
    sc = 2.0 ** (r % 7 - 3.0)
    return sc, np.array([0.0, 3.0, 64.0])[r % 3] * sc


def ints(rng, shape, lo=-7, hi=7):
    return NR._ints(rng, shape, lo, hi)


def pow2(rng, shape, kmax=2, signed=True):
    a = 2.0 ** rng.integers(0, kmax + 1, size=shape)
    return a * rng.choice([1.0, -1.0], size=shape) if signed else a


def d4(n):
    return n // 4 + n % 4 + 2


def vdiv(a, b):
    a, b = V.of(a), V.of(b)
    v = a.v / b.v
    e = (a.e + np.abs(v) * b.e) / (np.abs(b.v) - b.e)
    return V(v, e + U * (np.abs(v) + e))


def vsqrt(a):
    v = np.sqrt(a.v)
    e = np.maximum(v - np.sqrt(np.maximum(a.v - a.e, 0.0)), np.sqrt(a.v + a.e) - v)
    return V(v, e + U * (v + e))


def store_b(y, dt):
    """The bound of y as a tensor of dtype dt holds it."""
    return lp_bound(y) if dt == "bf16" else y.e + 0 * y.v


def held(v, dt):
    """An exact value as the dtype holds it (the one right answer of an exact case)."""
    return bf16_rne(v) if dt == "bf16" else f32(v)


def _st(v, dt, mut=None):
    if dt == "bf16":
        return (bf16_trunc if mut == "bf16_store_truncates" else bf16_rne)(v)
    return np.asarray(v, dtype=F).astype(np.float64)


def exact_ok():
    """The bit budget of the largest exact case of each family: every sum of the integer constructions, in any order, stays below 2^24."""
    return (5 * 2050 * 49 + 7 * 64 < 2 ** 24                # conv0 dw: B T_out products of two values <= 7, onto 64 * 7
            and 16 * 7 * 4 + 7 < 2 ** 24                     # conv0 forward: K taps, weights <= 4
            and 4097 * 7 + 7 * 64 < 2 ** 24                  # colsum
            and 128 * 7 < 2 ** 24                            # mean pool, S <= 128 (a power of two: the factor 1 / S is exact)
            and 3072 * 7 * 4 + 7 < 2 ** 24 and 256 * 28 < 2 ** 24          # head forward, head dx
            and (65536 + 300) * 7 + 7 * 64 < 2 ** 24         # embed_add_bwd
            and 4096 * 7 + 7 * 64 < 2 ** 24)                 # scatter_add_rows


def _four_chain(P, rev=False, drop_ragged=False):
    """colsum_partial_kernel / colsum_final_kernel / wn_colsum_final_kernel over axis 0 of the f32 array P."""
    n = P.shape[0]
    s = np.zeros((4,) + P.shape[1:], dtype=F)
    full = n - n % 4
    groups = range(0, full, 4)
    tail = () if drop_ragged else range(full, n)
    if rev:
        for i in reversed(tail):
            s[0] = s[0] + P[i]
    for i in (reversed(groups) if rev else groups):
        s = s + P[i:i + 4]
    if not rev:
        for i in tail:
            s[0] = s[0] + P[i]
    return (s[0] + s[1]) + (s[2] + s[3])


def _seq(P, rev=False):
    s = np.zeros(P.shape[1:], dtype=F)
    for i in (range(P.shape[0] - 1, -1, -1) if rev else range(P.shape[0])):
        s = s + P[i]
    return s


# ---------------------------------------------------------------------------------------------- conv0
@functools.lru_cache(maxsize=8)
def conv0_inputs(B, T_out, C, K, stride, extra=0, dydt="f32", seed=0, exact=False):
    """wave [B][T_in], w [C][K], bias [C], dy [B][T_out][C] (rounded to dydt), prev_w / prev_b what dw / dbias hold before an accumulating call.
    T_in = (T_out - 1) stride + K + extra."""
    rng = np.random.default_rng(seed + 31 * T_out + 7 * C + K + B)
    T_in = (T_out - 1) * stride + K + extra
    if exact:
        wave, w, bias, dy = ints(rng, (B, T_in)), pow2(rng, (C, K)), ints(rng, (C,)), ints(rng, (B, T_out, C))
        prev_w, prev_b = ints(rng, (C, K)) * 64, ints(rng, (C,)) * 64
    else:
        sc, off = row_affine(B)
        ch, tp = ch_scale(C), tap_scale(K)
        wave = f32(rng.standard_normal((B, T_in)) * sc[:, None] + off[:, None])
        w = f32(0.3 * rng.standard_normal((C, K)) * ch[:, None] * tp[None, :])
        bias = f32(rng.standard_normal(C) * ch)
        dy = rnd(rng.standard_normal((B, T_out, C)) * ch, dydt)
        prev_w = f32(rng.standard_normal((C, K)) * ch[:, None] * math.sqrt(B * T_out))
        prev_b = f32(rng.standard_normal(C) * ch * math.sqrt(B * T_out))
    return dict(B=B, T_in=T_in, T_out=T_out, C=C, K=K, stride=stride, dydt=dydt, wave=wave, w=w, bias=bias, dy=dy, prev_w=prev_w, prev_b=prev_b)


def _windows(p, wave=None, shift=0):
    """X[b][t][j] = wave[b][stride t + j (+ shift)], zero past the end."""
    wave = p["wave"] if wave is None else wave
    idx = p["stride"] * np.arange(p["T_out"])[:, None] + np.arange(p["K"])[None, :] + shift
    wz = np.concatenate([wave, np.zeros((wave.shape[0], 1 + shift), dtype=wave.dtype)], 1)
    return wz[:, np.minimum(idx, wave.shape[1])]


def conv0_ref_fwd(p, bias, dt):
    X = _windows(p)
    val = np.einsum("btj,cj->btc", X, p["w"])
    mag = np.einsum("btj,cj->btc", np.abs(X), np.abs(p["w"]))
    b = p["bias"] if bias else 0.0
    y = V(val + b, _g(p["K"] + 1) * (mag + np.abs(b)))
    return dict(y=y.v, y_b=store_b(y, dt))


def conv0_chain_w(p, accumulate):
    nblocks = p["B"] * -(-p["T_out"] // C0_BT)
    return -(-min(p["T_out"], C0_BT) // 4) + 1 + 3 + -(-nblocks // 4) + 3 + (1 if accumulate else 0)


def conv0_ref_bwd_w(p, accumulate):
    X = _windows(p)
    D = conv0_chain_w(p, accumulate)
    pw, pb = (p["prev_w"], p["prev_b"]) if accumulate else (0.0, 0.0)
    dw = np.einsum("btc,btj->cj", p["dy"], X) + pw
    db = p["dy"].sum((0, 1)) + pb
    return dict(dw=dw, dw_b=_g(D) * (np.einsum("btc,btj->cj", np.abs(p["dy"]), np.abs(X)) + np.abs(pw)),
                dbias=db, dbias_b=_g(D) * (np.abs(p["dy"]).sum((0, 1)) + np.abs(pb)))


def emu_conv0_fwd(p, bias, dt, rev=False, mut=None):
    X, w, K = _f(_windows(p, shift=1 if mut == "conv0_reads_x_plus_1" else 0)), _f(p["w"]), p["K"]
    bv = _f(p["bias"]) if bias else F(0.0)
    a = np.zeros((p["B"], p["T_out"], p["C"]), dtype=F) + bv
    for n, j in enumerate(range(K - 1, -1, -1) if rev else range(K)):
        if mut == "last_tap_dropped" and j == K - 1:
            continue
        a = a + X[:, :, j, None] * w[None, None, :, j]
        if mut == "bias_once_per_tap" and n > 0:
            a = a + bv
    return dict(y=_st(a, dt, mut))


def emu_conv0_bwd_w(p, accumulate, rev=False, mut=None):
    """The weight gradient with its real structure: chunks of 512 steps, four time groups per chunk, their tree, the final kernel's four row
    groups over the partial blocks."""
    B, T_out, C, K = p["B"], p["T_out"], p["C"], p["K"]
    X, dy = _f(_windows(p)), _f(p["dy"])
    nch = -(-T_out // C0_BT)
    parts = np.zeros((B * nch, C, K + 1), dtype=F)
    for b in range(B):
        for ch in range(nch):
            t0 = ch * C0_BT
            tmax = min(C0_BT, T_out - t0)
            tx = t0 - C0_BT if mut == "wgrad_t0_of_previous_chunk" and ch > 0 else t0
            Xe = np.concatenate([X[b, tx:tx + tmax], np.ones((tmax, 1), dtype=F)], 1)
            D = dy[b, t0:t0 + tmax]
            last = tmax - 1 if mut == "wgrad_skips_last_step" else tmax
            acc = np.zeros((4, C, K + 1), dtype=F)
            steps = range(-(-tmax // 4))
            for i in (reversed(steps) if rev else steps):
                n = max(0, min(4, last - 4 * i))
                acc[:n] = acc[:n] + D[4 * i:4 * i + n, :, None] * Xe[4 * i:4 * i + n, None, :]
            if mut == "time_group_missing":
                acc[3] = 0
            parts[b * nch + ch] = (acc[0] + acc[2]) + (acc[1] + acc[3])
    s4 = np.zeros((4, C, K + 1), dtype=F)
    ks = range(B * nch)
    for k in (reversed(ks) if rev else ks):
        if mut == "final_drops_k_mod_4_eq_3" and k % 4 == 3:
            continue
        s4[k % 4] = s4[k % 4] + parts[k]
    s = ((s4[0] + s4[1]) + s4[2]) + s4[3]
    if mut == "second_pass_overwrites_first" and C > 512:
        t = np.full_like(s, np.nan)
        t[:512] = s[:512]
        t[:C - 512] = s[512:]
        s = t
    dw, db = s[:, :K], (s[:, K - 1] if mut == "dbias_from_column_k_minus_1" else s[:, K])
    if accumulate and mut != "accumulate_overwrites":
        dw, db = _f(p["prev_w"]) + dw, _f(p["prev_b"]) + db
    return dict(dw=dw.astype(np.float64), dbias=db.astype(np.float64))


# ---------------------------------------------------------------------------------------------- weight norm
def wn_blocks(H, Cg):
    nb = min(WN_MAX_BLOCKS, (H * Cg + 255) // 256)
    return nb, -(-(H * Cg) // nb)


def wn_bwd_workspace_floats(H, Cg, K):
    return H * Cg * K + wn_blocks(H, Cg)[0] * K + K


@functools.lru_cache(maxsize=8)
def wn_inputs(H, Cg, K, seed=0, exact=False):
    """v [H][Cg][K], g [K], dw (the GEMM layout [G][Cg_out][K][Cg_in]), prev_v / prev_g.  exact: ONE non-zero +-2^e per tap, g = 2^k."""
    rng = np.random.default_rng(seed + H + 3 * Cg + K)
    G = H // Cg
    if exact:
        v = np.zeros((H * Cg, K))
        v[rng.integers(0, H * Cg, size=K), np.arange(K)] = pow2(rng, (K,), 3)
        v = v.reshape(H, Cg, K)
        g, dw = pow2(rng, (K,), 3, signed=False), ints(rng, (G, Cg, K, Cg))
        prev_v, prev_g = ints(rng, (H, Cg, K)) * 64, ints(rng, (K,)) * 64
    else:
        v = f32(0.05 * rng.standard_normal((H, Cg, K)) * ch_scale(H)[:, None, None] * tap_scale(K))
        g = f32(np.abs(1.0 + 0.1 * rng.standard_normal(K)) * 2.0 ** (np.arange(K) % 3 - 1.0))
        dw = f32(rng.standard_normal((G, Cg, K, Cg)) * tap_scale(K)[None, None, :, None])
        prev_v, prev_g = f32(rng.standard_normal((H, Cg, K)) * 8.0), f32(rng.standard_normal(K) * 8.0)
    return dict(H=H, Cg=Cg, K=K, G=G, v=v, g=g, dw=dw, prev_v=prev_v, prev_g=prev_g, key=(H, Cg, K, seed, exact))


def wn_layouts(val, H, Cg, K):
    """val [H][Cg][K] -> (w [G][Cg_out][K][Cg_in], w_flip [G][Cg_in][K reversed][Cg_out])."""
    t = val.reshape(H // Cg, Cg, Cg, K)
    return np.ascontiguousarray(t.transpose(0, 1, 3, 2)), np.ascontiguousarray(t[..., ::-1].transpose(0, 2, 3, 1))


def wn_dw_nat(p):
    return np.ascontiguousarray(p["dw"].transpose(0, 1, 3, 2)).reshape(p["H"], p["Cg"], p["K"])


@functools.lru_cache(maxsize=2)
def _wn_fwd_v(key):
    p = wn_inputs(*key)
    nb, rpb = wn_blocks(p["H"], p["Cg"])
    ss = (p["v"] ** 2).sum((0, 1))
    norms = vsqrt(V(ss, _g(rpb + 1 + d4(nb)) * ss))
    return norms, vdiv(V(p["g"]) * V(p["v"]), norms)


def wn_ref_fwd(p, dt):
    H, Cg, K = p["H"], p["Cg"], p["K"]
    norms, w = _wn_fwd_v(p["key"])
    wv, wf = wn_layouts(w.v, H, Cg, K)
    wb, wfb = wn_layouts(store_b(w, dt), H, Cg, K)
    return dict(norms=norms.v, norms_b=norms.e, w=wv, w_b=wb, w_flip=wf, w_flip_b=wfb, _norms=norms)


def wn_ref_bwd(p, norms, accumulate):
    """norms: the V pair of what the kernel is fed."""
    nb, rpb = wn_blocks(p["H"], p["Cg"])
    dw, v = V(wn_dw_nat(p)), V(p["v"])
    dots = gsum(dw * v, (0, 1), rpb + d4(nb))
    dv = vdiv(V(p["g"]), norms) * (dw - vdiv(v * dots, norms * norms))
    dg = vdiv(dots, norms)
    if accumulate:
        dv, dg = V(p["prev_v"]) + dv, V(p["prev_g"]) + dg
    return dict(dv=dv.v, dv_b=dv.e, dg=dg.v, dg_b=dg.e)


def _wn_colsum(t, H, Cg, K, rev, mut):
    """wn_colsum_partial_kernel + wn_colsum_final_kernel on the f32 term array t [H Cg][K]."""
    nb, rpb = wn_blocks(H, Cg)
    pad = np.zeros((nb * rpb, K), dtype=F)
    pad[:H * Cg] = t
    pad = pad.reshape(nb, rpb, K)
    part = np.zeros((nb, K), dtype=F)
    for r in (range(rpb - 1, -1, -1) if rev else range(rpb)):
        part = part + pad[:, r]
    if mut == "blocks_past_first_dropped":
        part = part[:1]
    return _four_chain(part, rev)


def emu_wn_fwd(p, dt, rev=False, mut=None):
    H, Cg, K = p["H"], p["Cg"], p["K"]
    v, g = _f(p["v"]), _f(p["g"])
    s = _wn_colsum((v * v).reshape(H * Cg, K), H, Cg, K, rev, mut)
    norms = s if mut == "norm_without_sqrt" else np.sqrt(s)
    den = norms
    if mut == "norms_over_co_k":
        den = np.sqrt((v.astype(np.float64) ** 2).sum((0, 2))).astype(F)[None, :, None]
        norms = np.resize(den, K)
    with np.errstate(divide="ignore", invalid="ignore"):                          # (a mutant's norm may be zero)
        val = _st(g * v / den, dt, mut)
    w, wf = wn_layouts(val, H, Cg, K)
    if mut == "w_flip_unreversed":
        wf = np.ascontiguousarray(wf[:, :, ::-1])
    if mut == "w_transposed_in_group":
        w = np.ascontiguousarray(val.reshape(H // Cg, Cg, Cg, K).transpose(0, 2, 3, 1))
    return dict(norms=norms.astype(np.float64), w=w, w_flip=wf)


def emu_wn_bwd(p, norms, accumulate, rev=False, mut=None):
    H, Cg, K = p["H"], p["Cg"], p["K"]
    v, g, nr, dw = _f(p["v"]), _f(p["g"]), _f(norms), _f(wn_dw_nat(p))
    dots = _wn_colsum((dw * v).reshape(H * Cg, K), H, Cg, K, rev, mut)
    val = g / nr * (dw if mut == "dv_without_projection" else dw - v * dots / (nr * nr))
    dg = dots if mut == "dg_not_divided" else dots / nr
    if accumulate and mut != "accumulate_overwrites":
        val, dg = _f(p["prev_v"]) + val, _f(p["prev_g"]) + dg
    return dict(dv=val.astype(np.float64), dg=dg.astype(np.float64))


# ---------------------------------------------------------------------------------------------- group_pad
@functools.lru_cache(maxsize=8)
def gp_inputs(B, T, H, sdt, seed=0):
    rng = np.random.default_rng(seed + B + T + H)
    sc, off = row_affine(B * T)
    return rnd((rng.standard_normal((B * T, H)) * ch_scale(H) * sc[:, None] + off[:, None]).reshape(B, T, H), sdt)


def gp_ref(x, G, pad_l, pad_r, ddt):
    B, T, H = x.shape
    t = x.reshape(B, T, G, H // G).transpose(0, 2, 1, 3)
    return held(np.pad(t, ((0, 0), (0, 0), (pad_l, pad_r), (0, 0))), ddt)


def emu_group_pad(x, G, pad_l, pad_r, ddt, mut=None):
    """group_pad_kernel's own index arithmetic, element by element."""
    B, T, H = x.shape
    Cg, TP = H // G, pad_l + T + pad_r
    e = np.arange(B * G * TP * Cg)
    cg, r = e % Cg, e // Cg
    pp, r = r % TP, r // TP
    g, b = r % G, r // G
    t = pp - pad_l + (1 if mut == "group_pad_left_frame_off_by_one" and pad_l > 0 else 0)
    ok = (t >= 0) & (t < T)
    out = np.where(ok, x.reshape(-1)[(b * T + np.clip(t, 0, T - 1)) * H + g * Cg + cg], 0.0)
    if mut == "group_pad_frame_unwritten":
        out = np.where(t >= T, np.nan, out)
    return held(out, ddt).reshape(B, G, TP, Cg)


# ---------------------------------------------------------------------------------------------- col2im
@functools.lru_cache(maxsize=8)
def c2i_inputs(B, T_out, C, K, stride, extra, dt, seed=0, exact=False):
    """dcol [B][T_out][K C], pre [B][T_in][C]; exact: integers, pre in [16, 48] where gelu' is exactly 1 (norm_ref.gelu_saturates)."""
    rng = np.random.default_rng(seed + T_out + C + 5 * K + stride)
    T_in = (T_out - 1) * stride + K + extra
    if exact:
        dcol, pre = ints(rng, (B, T_out, K * C)), ints(rng, (B, T_in, C), 16, 48)
    else:
        cs = (tap_scale(K)[:, None] * ch_scale(C)[None, :]).reshape(-1)
        dcol, pre = rnd(rng.standard_normal((B, T_out, K * C)) * cs, dt), rnd(1.5 * rng.standard_normal((B, T_in, C)), dt)
    return dict(B=B, T_in=T_in, T_out=T_out, C=C, K=K, stride=stride, dt=dt, dcol=dcol, pre=pre)


def c2i_ref(p, with_pre):
    B, T_in, T_out, C, K, s = p["B"], p["T_in"], p["T_out"], p["C"], p["K"], p["stride"]
    val, mag = np.zeros((B, T_in, C)), np.zeros((B, T_in, C))
    for j in range(K):
        tau = s * np.arange(T_out) + j
        val[:, tau] += p["dcol"][:, :, j * C:(j + 1) * C]
        mag[:, tau] += np.abs(p["dcol"][:, :, j * C:(j + 1) * C])
    dx = V(val, _g(-(-K // s)) * mag)
    if with_pre:
        dx = dx * vgelu_d(V(p["pre"]), GR.DCDF[p["dt"]])
    return dict(dx=dx.v, dx_b=store_b(dx, p["dt"]))


def emu_col2im(p, with_pre, rev=False, mut=None):
    B, T_in, T_out, C, K, s = p["B"], p["T_in"], p["T_out"], p["C"], p["K"], p["stride"]
    dcol, a = _f(p["dcol"]), np.zeros((B, T_in, C), dtype=F)
    tau = np.arange(T_in)
    for j in (range(K - 1, -1, -1) if rev else range(K)):
        d = tau - j
        ok = (d >= 0) & (d // s < T_out)
        if mut != "col2im_ignores_phase":
            ok &= d % s == 0
        a[:, ok] = a[:, ok] + dcol[:, d[ok] // s, j * C:(j + 1) * C]
    if with_pre:
        a = a * GR._emu_gelu_both(a if mut == "col2im_gelu_at_sum" else _f(p["pre"]), p["dt"])[1]
    return dict(dx=_st(a, p["dt"], mut))


# ---------------------------------------------------------------------------------------------- stand-alone GELU, tanh
@functools.lru_cache(maxsize=8)
def gelu_inputs(n, dt, seed=0):
    """x: +-0, +-40 and n - 4 points over [-12, 12]; dy columns 2^(i % 11 - 5)."""
    rng = np.random.default_rng(seed + n)
    x = np.concatenate([np.linspace(-12.0, 12.0, n - 4), [0.0, -0.0, 40.0, -40.0]])
    return dict(n=n, dt=dt, x=rnd(x, dt), dy=rnd(rng.standard_normal(n) * 2.0 ** (np.arange(n) % 11 - 5.0), dt))


def gelu_ref(p):
    dc = GR.DCDF[p["dt"]]
    y, dx = vgelu(V(p["x"]), dc), V(p["dy"]) * vgelu_d(V(p["x"]), dc)
    return dict(y=y.v, y_b=store_b(y, p["dt"]), dx=dx.v, dx_b=store_b(dx, p["dt"]))


def emu_gelu(p, mut=None):
    y, d = GR._emu_gelu_both(_f(p["x"]), p["dt"], tanh=mut == "gelu_tanh_flavour")
    return dict(y=_st(y, p["dt"], mut), dx=_st(_f(p["dy"]) * d, p["dt"], mut))


@functools.lru_cache(maxsize=8)
def tanh_inputs(n, seed=0):
    rng = np.random.default_rng(seed + n)
    x = f32(np.concatenate([np.linspace(-10.0, 10.0, n - 4), [0.0, -0.0, 90.0, -90.0]]))
    return dict(n=n, x=x, y=f32(np.tanh(x)), dy=f32(rng.standard_normal(n) * 2.0 ** (np.arange(n) % 11 - 5.0)))


def tanh_ref(p):
    y = np.tanh(p["x"])
    yv = V(p["y"])
    dx = V(p["dy"]) * (V(1.0) - yv * yv)
    return dict(y=y, y_b=TANH_REL * np.abs(y), dx=dx.v, dx_b=dx.e)


def emu_tanh(p, mut=None):
    x, y, dy = _f(p["x"]), _f(p["y"]), _f(p["dy"])
    t = x if mut == "tanh_grad_from_x" else y
    return dict(y=np.tanh(x.astype(np.float64)).astype(F).astype(np.float64), dx=(dy * (F(1.0) - t * t)).astype(np.float64))


# ---------------------------------------------------------------------------------------------- colsum
def colsum_nparts(M):
    return max(1, min(256, (M + 15) // 16))


@functools.lru_cache(maxsize=8)
def colsum_inputs(M, N, dt, seed=0, exact=False):
    rng = np.random.default_rng(seed + 3 * M + N)
    if exact:
        return dict(M=M, N=N, dt=dt, x=ints(rng, (M, N)), prev=ints(rng, (N,)) * 64)
    sc, off = row_affine(M)
    x = rnd(rng.standard_normal((M, N)) * ch_scale(N) * sc[:, None] + off[:, None], dt)
    return dict(M=M, N=N, dt=dt, x=x, prev=f32(rng.standard_normal(N) * ch_scale(N) * math.sqrt(M)))


def colsum_ref(p, nparts, accumulate):
    D = d4(-(-p["M"] // nparts)) + d4(nparts) + (1 if accumulate else 0)
    pv = p["prev"] if accumulate else 0.0
    return dict(out=p["x"].sum(0) + pv, out_b=_g(D) * (np.abs(p["x"]).sum(0) + np.abs(pv)))


def emu_colsum(p, nparts, accumulate, rev=False, mut=None, ld=None):
    M, N = p["M"], p["N"]
    x = _f(p["x"])
    if mut == "colsum_n_for_ld" and ld and ld > N:
        wide = np.full((M, ld), np.nan, dtype=F)
        wide[:, :N] = x
        x = wide.reshape(-1)[:M * N].reshape(M, N)
    rpb = -(-M // nparts)
    part = np.zeros((nparts, N), dtype=F)
    for k in range(nparts):
        part[k] = _four_chain(x[min(k * rpb, M):min(k * rpb + rpb, M)], rev, mut == "colsum_drops_ragged_rows")
    s = _four_chain(part, rev)
    if accumulate and mut != "accumulate_overwrites":
        s = _f(p["prev"]) + s
    return dict(out=s.astype(np.float64))


# ---------------------------------------------------------------------------------------------- mean pools
@functools.lru_cache(maxsize=8)
def pool_inputs(B, S, W, seed=0, exact=False):
    rng = np.random.default_rng(seed + B + 5 * S + W)
    if exact:
        return dict(B=B, S=S, W=W, x=ints(rng, (B, S, W)), dy=ints(rng, (B, W)))
    sc, off = row_affine(B * S)
    x = f32((rng.standard_normal((B * S, W)) * ch_scale(W) * sc[:, None] + off[:, None]).reshape(B, S, W))
    return dict(B=B, S=S, W=W, x=x, dy=f32(rng.standard_normal((B, W)) * ch_scale(W)))


def pool_lens(p, lens):
    return [p["S"]] * p["B"] if lens is None else [max(0, min(int(L), p["S"])) for L in lens]


def pool_ref(p, lens=None):
    """-> y [B][W], dx_f32 / dx_lp [B][S][W] and their bounds."""
    B, S, W = p["B"], p["S"], p["W"]
    y, yb, dx, dxb, dlb = np.zeros((B, W)), np.zeros((B, W)), np.zeros((B, S, W)), np.zeros((B, S, W)), np.zeros((B, S, W))
    for b, L in enumerate(pool_lens(p, lens)):
        if L == 0:
            continue
        m = gsum(V(p["x"][b, :L]), 0, -(-L // 16) + 15) * inv(L)
        d = V(p["dy"][b]) * inv(L)
        y[b], yb[b], dx[b, :L], dxb[b, :L], dlb[b, :L] = m.v, m.e, d.v, d.e, lp_bound(d)
    return dict(y=y, y_b=yb, dx_f32=dx, dx_f32_b=dxb, dx_lp=dx, dx_lp_b=dlb)


def emu_pool(p, lens=None, rev=False, mut=None):
    B, S, W = p["B"], p["S"], p["W"]
    x, dy = _f(p["x"]), _f(p["dy"])
    y, dx = np.zeros((B, W), dtype=F), np.zeros((B, S, W), dtype=F)
    for b, L in enumerate(pool_lens(p, lens)):
        if L == 0:
            continue
        acc = np.zeros((16, W), dtype=F)
        it = range(-(-L // 16))
        for i in (reversed(it) if rev else it):
            n = min(16, L - 16 * i)
            acc[:n] = acc[:n] + x[b, 16 * i:16 * i + n]
        a = acc[0]
        for k in (range(15, 0, -1) if rev else range(1, 16)):
            a = a + acc[k]
        den = L
        if mut == "pool_divides_by_padded_s":
            den = 16 * -(-L // 16)
        if mut == "len_pool_divides_by_s" and lens is not None:
            den = S
        r = F(1.0) / F(den)
        y[b] = a * r
        dx[b, :S if mut == "len_pool_bwd_past_len" and lens is not None else L] = dy[b] * r
    return dict(y=y.astype(np.float64), dx_f32=dx.astype(np.float64), dx_lp=_st(dx, "bf16", mut))


# ---------------------------------------------------------------------------------------------- head
@functools.lru_cache(maxsize=8)
def head_inputs(B, K, N, seed=0, exact=False):
    rng = np.random.default_rng(seed + B + K + 3 * N)
    if exact:
        return dict(B=B, K=K, N=N, x=ints(rng, (B, K)), W=pow2(rng, (N, K)), bias=ints(rng, (N,)), dy=ints(rng, (B, N)),
                    prev_W=ints(rng, (N, K)) * 64, prev_b=ints(rng, (N,)) * 64)
    sc, off = row_affine(B)
    x = f32(rng.standard_normal((B, K)) * ch_scale(K) * sc[:, None] + off[:, None])
    W = f32(0.1 * rng.standard_normal((N, K)) * tap_scale(N)[:, None])
    return dict(B=B, K=K, N=N, x=x, W=W, bias=f32(rng.standard_normal(N) * tap_scale(N)), dy=f32(rng.standard_normal((B, N)) * tap_scale(N)),
                prev_W=f32(rng.standard_normal((N, K)) * ch_scale(K)), prev_b=f32(rng.standard_normal(N)))


def head_ref(p, bias=True, accumulate=False):
    B, K, N = p["B"], p["K"], p["N"]
    x, W, dy = p["x"], p["W"], p["dy"]
    y = V(x @ W.T, _g(-(-K // 64) + 1 + 6) * (np.abs(x) @ np.abs(W).T))
    if bias:
        y = y + V(p["bias"])
    a = 1 if accumulate else 0
    pW, pb = (p["prev_W"], p["prev_b"]) if accumulate else (0.0, 0.0)
    return dict(y=y.v, y_b=y.e + 0 * y.v, dx=dy @ W, dx_b=_g(N + 1) * (np.abs(dy) @ np.abs(W)),
                dW=dy.T @ x + pW, dW_b=_g(B + 1 + a) * (np.abs(dy).T @ np.abs(x) + np.abs(pW)),
                db=dy.sum(0) + pb, db_b=_g(B + a) * (np.abs(dy).sum(0) + np.abs(pb)))


def emu_head(p, bias=True, accumulate=False, rev=False, mut=None):
    B, K, N = p["B"], p["K"], p["N"]
    x, W, dy = _f(p["x"]), _f(p["W"]), _f(p["dy"])
    passes = -(-K // 64)
    xp, Wp = np.zeros((B, passes * 64), dtype=F), np.zeros((N, passes * 64), dtype=F)
    xp[:, :K], Wp[:, :K] = x, W
    lanes = np.zeros((B * N, 64), dtype=F)
    for i in (range(passes - 1, -1, -1) if rev else range(passes)):
        lanes = lanes + (xp[:, None, 64 * i:64 * i + 64] * Wp[None, :, 64 * i:64 * i + 64]).reshape(B * N, 64)
    if mut == "head_idle_lanes_left_out" and K % 64:
        lanes[:, K % 64:] = 0
    y = NR._wave_sum(lanes, rev).reshape(B, N) + (_f(p["bias"]) if bias else F(0.0))
    dx = _seq(dy.T[:, :, None] * W[:, None, :], rev)
    dW = _seq(dy[:, :, None] * (W[None] if mut == "head_dw_from_w" else x[:, None, :]), rev)
    db = _seq(dy, rev)
    if mut == "head_db_over_n":
        db = np.resize(dy.sum(1), N).astype(F)
    if accumulate and mut != "accumulate_overwrites":
        dW, db = _f(p["prev_W"]) + dW, _f(p["prev_b"]) + db
    return dict(y=y.astype(np.float64), dx=dx.astype(np.float64), dW=dW.astype(np.float64), db=db.astype(np.float64))


# ---------------------------------------------------------------------------------------------- cross entropy
@functools.lru_cache(maxsize=8)
def ce_inputs(B, C, seed=0):
    """Row r = randn 2^(r % 5); rows r % 7 = 1, 2, 3, 4 offset by +80, -80, +3e4, -3e4; rows r % 11 = 5 (C > 1) flat but for ONE logit 60 above
    the rest, which is the target: their loss is ~ (C - 1) e^-60.  cw[c] = 2^(c % 7 - 3); targets in range."""
    rng = np.random.default_rng(seed + 17 * B + C)
    r = np.arange(B)
    z = rng.standard_normal((B, C)) * (2.0 ** (r % 5))[:, None]
    t = rng.integers(0, C, size=B)
    peak = (r % 11 == 5) & (C > 1)
    z[peak] = 0.01 * rng.standard_normal((int(peak.sum()), C))
    z[peak, t[peak]] += 60.0
    z += np.array([0.0, 80.0, -80.0, 3e4, -3e4, 0.0, 0.0])[r % 7][:, None]
    return dict(B=B, C=C, z=f32(z), t=t.astype(np.int64), cw=ch_scale(C), peak=peak)


def ce_ref(p, weighted, grad_scale):
    B, C, z, t = p["B"], p["C"], p["z"], p["t"]
    rows = np.arange(B)
    w = V(p["cw"][t] if weighted else np.ones(B))
    m = z.max(1, keepdims=True)
    d = V(z) - V(m)
    ex = np.exp(d.v)
    e = V(ex, ex * (EXP_REL + np.expm1(np.abs(d.v) * U) * (1 + EXP_REL)) + TINY)
    se = gsum(e, 1, C)
    rest = ex.copy()
    rest[rows, z.argmax(1)] = 0.0                                                  # log se = log1p(se - 1): fp64 keeps a loss of ~ e^-60
    lse = np.log1p(rest.sum(1))
    lg = V(lse, se.e / (se.v - se.e) + LOG_REL * np.abs(lse))
    row = (V(m[:, 0]) + lg) - V(z[rows, t])
    row = w * V((m[:, 0] - z[rows, t]) + lse, row.e)
    D = -(-B // 256) + 8
    num, den = gsum(row, 0, D), gsum(w, 0, D)
    loss = vdiv(num, den)
    onehot = np.zeros((B, C))
    onehot[rows, t] = 1.0
    dl = vdiv(w * V(f32(grad_scale)), den)[:, None] * (vdiv(e, se[:, None]) - V(onehot))
    return dict(loss=loss.v.reshape(1), loss_b=loss.e.reshape(1), dlogits=dl.v, dlogits_b=dl.e + TINY)


def emu_ce(p, weighted, grad_scale, rev=False, mut=None):
    B, C, t = p["B"], p["C"], p["t"]
    z = _f(p["z"])
    rows = np.arange(B)
    w = _f(p["cw"])[t] if weighted else np.ones(B, dtype=F)
    m = np.zeros((B, 1), dtype=F) if mut == "ce_without_max" else z.max(1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ex = np.exp((z - m).astype(np.float64)).astype(F)
        se = _seq(ex.T, rev)
        row = w * ((m[:, 0] + np.log(se.astype(np.float64)).astype(F)) - z[rows, t])
        nrow = min(B, 256) if mut == "ce_rows_ge_256_missing" else B
        pad = np.zeros((2, -(-B // 256) * 256), dtype=F)
        pad[0, :nrow], pad[1, :nrow] = row[:nrow], w[:nrow]
        th = _seq(pad.reshape(2, -1, 256).transpose(1, 0, 2), rev)                 # [2][256]: each thread's chain over its rows
        off = 128
        while off:
            th = th[:, :off] + th[:, off:2 * off]
            off //= 2
        num, den = th[0, 0], th[1, 0]
        if mut == "ce_mean_over_b":
            den = F(B)
        gs = F(grad_scale)
        loss = num / den * (gs if mut == "ce_grad_scale_on_loss" else F(1.0))
        onehot = np.zeros((B, C), dtype=F)
        onehot[rows, t] = 1.0
        wi = (w * gs / den)[:, None]
        dl = wi * ((ex - onehot) / se[:, None] if mut == "ce_onehot_before_normalising" else ex / se[:, None] - onehot)
        if mut == "ce_rows_ge_256_missing":
            dl[256:] = np.nan
    return dict(loss=np.array([loss], dtype=np.float64), dlogits=dl.astype(np.float64))


# ---------------------------------------------------------------------------------------------- index kernels (exact)
@functools.lru_cache(maxsize=8)
def text_inputs(B, S, pad_id, W=8, vocab=50, seed=0):
    """ids [B][S]: row 0 padded at the front, row 1 in the interior, row 2 as a suffix, row 3 (B >= 4) all pads, row 4 none; integer tables."""
    rng = np.random.default_rng(seed + S + B)
    pid = pad_id if pad_id >= 0 else 1
    ids = rng.integers(2, vocab, size=(B, S))
    n = max(1, S // 3)
    ids[0, :n] = pid
    if B > 1:
        ids[1, S // 2:S // 2 + n] = pid
        ids[1, ::7] = pid
    if B > 2:
        ids[2, S - n:] = pid
    if B > 3:
        ids[3] = pid
    return dict(B=B, S=S, W=W, pad_id=pad_id, ids=ids.astype(np.int64), word=ints(rng, (vocab, W)), pos=ints(rng, (S + vocab + 2, W)) * 16,
                type=ints(rng, (W,)) * 256)


def text_ref(p):
    ids, pad = p["ids"], p["pad_id"]
    if pad >= 0:
        nonpad = (ids != pad).astype(np.int64)
        pos_ids = np.cumsum(nonpad, 1) * nonpad + pad
    else:
        pos_ids = np.broadcast_to(np.arange(p["S"], dtype=np.int64), ids.shape).copy()
    return dict(pos_ids=pos_ids, pre=(p["word"][ids] + p["pos"][pos_ids] + p["type"]).reshape(-1, p["W"]))


def emu_text(p, mut=None):
    """text_pos_ids_kernel's Hillis-Steele scan over 64 * 2^k >= S threads, then the three-table sum."""
    ids, pad, S = p["ids"], p["pad_id"], p["S"]
    threads = 64
    while threads < S:
        threads *= 2
    idp = np.full((p["B"], threads), pad, dtype=np.int64)
    idp[:, :S] = ids
    nonpad = (idp != pad).astype(np.int64) if pad >= 0 else np.ones_like(idp)
    scan = np.where(np.arange(threads) < S, np.ones_like(nonpad) if mut == "pos_ids_count_pads" else nonpad, 0)
    off = 1
    while off < (64 if mut == "pos_ids_scan_stops_at_64" else threads):
        scan = scan + np.concatenate([np.zeros((p["B"], off), dtype=np.int64), scan[:, :-off]], 1)
        off *= 2
    pos_ids = (scan * nonpad + pad if pad >= 0 else np.broadcast_to(np.arange(threads), scan.shape))[:, :S].astype(np.int64)
    pre = (_f(p["word"])[ids] + _f(p["pos"])[np.clip(pos_ids, 0, len(p["pos"]) - 1)]) + _f(p["type"])
    return dict(pos_ids=pos_ids, pre=pre.astype(np.float64).reshape(-1, p["W"]))


def embed_parts(rows):
    return min(256, (rows + 255) // 256)


@functools.lru_cache(maxsize=8)
def embed_inputs(rows, W, ntable, seed=0):
    rng = np.random.default_rng(seed + rows + ntable)
    ids = rng.integers(0, ntable, size=rows).astype(np.int64)
    ids[-1] = ntable - 1
    return dict(rows=rows, W=W, ntable=ntable, ids=ids, x=ints(rng, (rows, W)), table=ints(rng, (ntable, W)) * 8, dy=ints(rng, (rows, W)),
                prev=ints(rng, (ntable, W)) * 64)


def embed_ref(p, accumulate):
    d = np.zeros((p["ntable"], p["W"]))
    np.add.at(d, p["ids"], p["dy"])
    return dict(out=p["x"] + p["table"][p["ids"]], dtable=d + (p["prev"] if accumulate else 0.0))


def emu_embed(p, accumulate, rev=False, mut=None):
    rows, W, nt = p["rows"], p["W"], p["ntable"]
    nparts = embed_parts(rows)
    rpb = -(-rows // nparts)
    dy = np.zeros((nparts * rpb, W), dtype=F)
    dy[:rows] = _f(p["dy"])
    ids = np.full(nparts * rpb, -1)
    ids[:rows] = p["ids"]
    hit = (ids[:, None] == np.arange(nt)[None, :]).reshape(nparts, rpb, nt)
    if mut == "embed_add_bwd_drops_row_7":
        hit[:, :, 7:] = False
    dy = dy.reshape(nparts, rpb, W)
    part = np.zeros((nparts, nt, W), dtype=F)
    for r in (range(rpb - 1, -1, -1) if rev else range(rpb)):
        part = part + np.where(hit[:, r, :, None], dy[:, r, None, :], F(0.0))
    s = _seq(part, rev)
    if accumulate and mut != "accumulate_overwrites":
        s = _f(p["prev"]) + s
    return dict(out=(_f(p["x"]) + _f(p["table"])[p["ids"]]).astype(np.float64), dtable=s.astype(np.float64))


@functools.lru_cache(maxsize=8)
def scatter_inputs(rows, W, ntable=64, seed=0):
    """One index carried by 1, 16, 17 rows and by a quarter of the rows (as far as rows allows), the rest distinct or random."""
    rng = np.random.default_rng(seed + rows + W)
    idx = rng.integers(4, ntable, size=rows).astype(np.int64)
    perm = rng.permutation(rows)
    at = 0
    for k, cnt in enumerate((rows // 4, 17, 16, 1)):
        cnt = min(cnt, rows - at)
        idx[perm[at:at + cnt]] = k
        at += cnt
    return dict(rows=rows, W=W, ntable=ntable, idx=idx, d=ints(rng, (rows, W)), prev=ints(rng, (ntable, W)) * 64)


def scatter_ref(p):
    out = p["prev"].copy()
    np.add.at(out, p["idx"], p["d"])
    return dict(dtable=out)


def emu_scatter(p, rev=False, mut=None):
    """scatter_add_rows_kernel: per index the matching rows in ascending order, wave w sums matches w, w + 16, ..., the partial rows join in wave order."""
    d, out = _f(p["d"]), _f(p["prev"]).copy()
    for ident in np.unique(p["idx"]):
        match = np.flatnonzero(p["idx"] == ident)
        if mut == "scatter_second_match_twice" and len(match) > 1:
            match = np.concatenate([match[:2], match[1:]])
        n = len(match)
        pad = np.zeros((-(-n // 16) * 16, p["W"]), dtype=F)
        pad[:n] = d[match]
        waves = _seq(pad.reshape(-1, 16, p["W"]), rev)
        out[ident] = out[ident] + _seq(waves[:min(n, 16)], rev)
    return dict(dtable=out.astype(np.float64))


def gather_ref(table, idx):
    return table[np.clip(idx, 0, len(table) - 1)]


def patchify_ref(video, keep_idx):
    """video [B][F][3][H][W] -> [B nkeep][1536], element order (c, dt, dh, dw) of the 2 x 16 x 16 patch of token (tt, hh, ww)."""
    B, Fr, _, H, W = video.shape
    gh, gw = H // 16, W // 16
    t = video.reshape(B, Fr // 2, 2, 3, gh, 16, gw, 16).transpose(0, 1, 4, 6, 3, 2, 5, 7).reshape(B, (Fr // 2) * gh * gw, 1536)
    tok = np.clip(keep_idx, 0, t.shape[1] - 1)
    return np.take_along_axis(t, tok[:, :, None].astype(np.int64), 1).reshape(-1, 1536)


def mask_to_index_ref(mask, keep_value, nkeep):
    """-> (keep_idx [B][nkeep] int32: the kept positions ascending, short rows repeat their last kept index (0 if none); counts [B])."""
    B, n = mask.shape
    out, counts = np.zeros((B, nkeep), dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        kept = np.flatnonzero((mask[b] != 0) == bool(keep_value))
        counts[b] = len(kept)
        out[b] = kept[-1] if len(kept) else 0
        out[b, :min(nkeep, len(kept))] = kept[:nkeep]
    return out, counts


def ratios(got, ref, names):
    return {n: ratio(got[n], ref[n], ref[n + "_b"]) for n in names if got.get(n) is not None}


def equal(got, want):
    """Bit-for-bit as values: same shape, every element equal, no NaN."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.array_equal(got, want))
