"""Tensor-level wrappers over the C ABI: allocate outputs with torch, pass raw pointers + the current HIP stream.

No arithmetic happens here; torch is used for device memory and streams only.  Scratch buffers are cached per
(name, stream) so that concurrent branches on different HIP streams never share a workspace.
"""
import collections
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib as L
from ._lib import check, dt, lib, ptr, stream

_ws = {}


def workspace(name, nfloats, device):
    key = (name, torch.cuda.current_stream().cuda_stream, str(device))
    t = _ws.get(key)
    if t is None or t.numel() < nfloats:
        t = torch.empty(max(int(nfloats), 1), dtype=torch.float32, device=device)
        _ws[key] = t
    return t


def clear_workspaces():
    _ws.clear()


# Optional live timing of one kernel family with HIP events on the launch stream (bench.py's roofline pass only).
_prof = None


def profile_start(kinds):
    """kinds: one family name or several of "gemm_nt", "gemm_tn", "attn", "ln" (every launch of those families gets a HIP event pair)."""
    global _prof
    _prof = {"kinds": {kinds} if isinstance(kinds, str) else set(kinds), "ev": []}


def _prof_launch(family, select, work, nbytes, launch, work_exec=None):
    """Run `launch()`; while a profile of `family` is active, bracket it with a HIP event pair on the launch stream and record its
    algorithmic work (FLOPs for the MFMA-bound families, 0 for the HBM-bound one) and algorithmic bytes.  work_exec: the FLOPs the kernels
    really execute where that differs from the algorithmic count (the atomic-free attention backward recomputes two products)."""
    if _prof is not None and family in _prof["kinds"]:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        _prof["ev"].append((e0, e1, float(work), select, float(nbytes), family, float(work if work_exec is None else work_exec)))
    else:
        launch()


def profile_stop(select="bf16"):
    """-> (algorithmic FLOPs, seconds inside the kernels, launches) of the gemm_nt launches with `select` operands ("bf16" / "fp8") since
    profile_start(); profile_stop.families = {family: {"work", "bytes", "secs", "launches"}} for every profiled family (all operand types)."""
    global _prof
    torch.cuda.synchronize()
    allev, _prof = _prof["ev"], None
    fam = {}
    for e0, e1, work, sel, nbytes, family, work_exec in allev:
        d = fam.setdefault(family, {"work": 0.0, "work_exec": 0.0, "bytes": 0.0, "secs": 0.0, "launches": 0})
        d["work"] += work
        d["work_exec"] += work_exec
        d["bytes"] += nbytes
        d["secs"] += e0.elapsed_time(e1) * 1e-3
        d["launches"] += 1
    profile_stop.families = fam
    ev = [e for e in allev if e[5] == "gemm_nt" and e[3] == select]
    secs = sum(e[0].elapsed_time(e[1]) for e in ev) * 1e-3
    profile_stop.algorithmic_bytes = sum(e[4] for e in ev)          # operands + output once each (the minimum the launches could move)
    return sum(e[2] for e in ev), secs, len(ev)


# ---------------------------------------------------------------------------------------------- GEMM
def gemm_nt(a, b, *, bias=None, act=0, resid=None, gelu_in=None, out_dtype=None, want_pre=False, out=None,
            accumulate=False, alpha=1.0, M=None, N=None, K=None, lda=None, ldb=None, ldc=None,
            nzb=1, nzg=1, a_zb=0, a_zg=0, b_zb=0, b_zg=0, c_zb=0, c_zg=0, bias_zg=0, out_shape=None, tile_m=0, a_dequant=None, b_dequant=None,
            ld_gelu=None, gelu_zb=0):
    """C = epi(alpha * A @ B^T).  Plain use: a [M,K], b [N,K] contiguous.  Strided/batched use: pass sizes/strides.
    fp8 operands (torch.float8_e4m3fn): pass their dequantisation scalars (Fp8.dequant) and an explicit out_dtype."""
    if M is None:
        M, K = a.shape[-2], a.shape[-1]
        N = b.shape[-2]
        lda, ldb = a.stride(-2), b.stride(-2)
    out_dtype = out_dtype or (torch.bfloat16 if a.dtype == torch.float8_e4m3fn else a.dtype)
    if out is None:
        out = torch.empty(out_shape or (M, N), dtype=out_dtype, device=a.device)
    if ldc is None:
        ldc = out.stride(-2)
    pre = torch.empty_strided(out.shape, out.stride(), dtype=out.dtype, device=out.device) if want_pre else None   # (same row stride as out: ld_pre = ldc)
    g = L.GemmNTArgs()
    g.A, g.B, g.C, g.C_pre = ptr(a), ptr(b), ptr(out), ptr(pre)
    g.bias, g.gelu_in, g.resid = ptr(bias), ptr(gelu_in), ptr(resid)
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc, g.ld_pre = lda, ldb, ldc, ldc
    g.ld_gelu_in = (ld_gelu if ld_gelu is not None else gelu_in.stride(-2)) if gelu_in is not None else 0
    g.gelu_zb = gelu_zb
    g.ld_resid = resid.stride(-2) if resid is not None else 0
    g.nzb, g.nzg = nzb, nzg
    g.a_zb, g.a_zg, g.b_zb, g.b_zg, g.c_zb, g.c_zg, g.bias_zg = a_zb, a_zg, b_zb, b_zg, c_zb, c_zg, bias_zg
    g.in_dtype, g.out_dtype, g.act, g.accumulate, g.alpha = dt(a), dt(out), act, int(accumulate), alpha
    g.tile_m_hint = tile_m
    g.a_dequant, g.b_dequant = ptr(a_dequant), ptr(b_dequant)
    if bias is not None:
        assert bias.dtype == torch.float32
    if resid is not None:
        assert resid.dtype == torch.float32
    if gelu_in is not None:
        assert gelu_in.dtype == (torch.bfloat16 if a.dtype == torch.float8_e4m3fn else a.dtype)
    nz = max(nzb, 1) * max(nzg, 1)
    osz = 4 if out_dtype == torch.float32 else 2
    # operands, output and every epilogue side tensor once each: the minimum the launch could move
    nbytes = nz * ((M * K + N * K) * a.element_size() + M * N * (osz * (2 if want_pre else 1) + (4 if resid is not None else 0)
                                                                 + (2 if gelu_in is not None else 0) + (osz if accumulate else 0)))
    sel = "bf16" if a.dtype == torch.bfloat16 else ("fp8" if a.dtype == torch.float8_e4m3fn else "f32")
    _prof_launch("gemm_nt", sel, 2.0 * M * N * K * nz, nbytes, lambda: check(lib().tav_gemm_nt(C.byref(g), stream()), "gemm_nt"))
    return (out, pre) if want_pre else out


def gemm_tn(a, b, *, out=None, accumulate=False, N1=None, N2=None, lda=None, ldb=None, rows_per_batch=None, nbatch=1,
            a_zb=0, b_zb=0, perm_inner=0, perm_outer=0, scale=1.0, out_shape=None, want_bias=False):
    """out[n1][perm(n2)] (+)= sum_tokens A[t][n1] * B[t][n2]  (weight gradient).  want_bias: also return
    dbias[n1] = sum_tokens A[t][n1] computed inside the same kernel."""
    if N1 is None:
        N1, N2 = a.shape[-1], b.shape[-1]
        rows_per_batch = a.shape[-2]
        lda, ldb = a.stride(-2), b.stride(-2)
    cr, ns = C.c_int32(), C.c_int32()
    check(lib().tav_gemm_tn_splits(N1, N2, rows_per_batch, nbatch, C.byref(cr), C.byref(ns)), "gemm_tn_splits")
    slabs = workspace("tn_slabs", ns.value * N1 * N2, a.device)
    if out is None:
        out = torch.empty(out_shape or (N1, N2), dtype=torch.float32, device=a.device)
    g = L.GemmTNArgs()
    g.A, g.B, g.slabs, g.out = ptr(a), ptr(b), ptr(slabs), ptr(out)
    g.N1, g.N2, g.lda, g.ldb = N1, N2, lda, ldb
    g.rows_per_batch, g.nbatch, g.a_zb, g.b_zb = rows_per_batch, nbatch, a_zb, b_zb
    g.chunk_rows, g.nsplit, g.perm_inner, g.perm_outer = cr.value, ns.value, perm_inner, perm_outer
    g.dtype, g.accumulate, g.scale = dt(a), int(accumulate), scale
    dbias = None
    if want_bias:
        dbias = torch.empty(N1, dtype=torch.float32, device=a.device)
        bpart = workspace("tn_bias", ns.value * N1, a.device)
        g.dbias, g.bias_partials = ptr(dbias), ptr(bpart)
    assert a.dtype == b.dtype
    tokens = rows_per_batch * nbatch
    _prof_launch("gemm_tn", "bf16" if a.dtype == torch.bfloat16 else "f32", 2.0 * tokens * N1 * N2, tokens * (N1 + N2) * a.element_size() + 4 * N1 * N2,
                 lambda: check(lib().tav_gemm_tn(C.byref(g), stream()), "gemm_tn"))
    return (out, dbias) if want_bias else out


def gemm_tn_grouped(pairs, want_bias=True, flags=0, into=None):
    """[(A_k [rows, N1_k], B_k [rows, N2_k]), ...] (<= 4, same rows and dtype) -> [(dW_k [N1_k, N2_k] f32, db_k [N1_k] f32 | None), ...]
    in ONE launch (the weight gradients of one transformer layer): 128-wide tiles that each sum over all rows, or -- bf16, large problems --
    256-wide tiles with the rows split over workgroups into f32 slabs plus a fixed-order reduce (the library decides; `flags` as in tavhip.h).
    into: optional [(dW_buffer | None, db_buffer | None), ...] -- contiguous f32 destinations (the data-parallel gradient arena: the kernels
    write the bucket directly, ddp.GraphedStep); missing entries are allocated."""
    n = len(pairs)
    rows, dtype = pairs[0][0].shape[0], pairs[0][0].dtype
    probs = (L.GemmTNProblem * n)()
    outs = []
    for k, (a, b) in enumerate(pairs):
        assert a.shape[0] == rows and b.shape[0] == rows and a.dtype == dtype and b.dtype == dtype
        N1, N2 = a.shape[1], b.shape[1]
        dW_to, db_to = into[k] if into is not None else (None, None)
        dW = dW_to if dW_to is not None else torch.empty(N1, N2, dtype=torch.float32, device=a.device)
        db = (db_to if db_to is not None else torch.empty(N1, dtype=torch.float32, device=a.device)) if want_bias else None
        assert dW.shape == (N1, N2) and dW.is_contiguous() and dW.dtype == torch.float32 and (db is None or (db.shape == (N1,) and db.is_contiguous()))
        pr = probs[k]
        pr.A, pr.B, pr.out, pr.dbias = ptr(a), ptr(b), ptr(dW), ptr(db)
        pr.N1, pr.N2, pr.lda, pr.ldb = N1, N2, a.stride(0), b.stride(0)
        outs.append((dW, db))
    nbytes = lib().tav_gemm_tn_grouped_ws_bytes(probs, n, rows, dt(pairs[0][0]), flags)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pairs[0][0].device) if nbytes > 0 else None
    es = pairs[0][0].element_size()
    _prof_launch("gemm_tn", "bf16" if dtype == torch.bfloat16 else "f32", sum(2.0 * rows * a.shape[1] * b.shape[1] for a, b in pairs),
                 sum(rows * (a.shape[1] + b.shape[1]) * es + 4 * a.shape[1] * b.shape[1] for a, b in pairs),
                 lambda: check(lib().tav_gemm_tn_grouped_ws(probs, n, rows, dt(pairs[0][0]), ptr(ws), nbytes, flags, stream()), "gemm_tn_grouped"))
    return outs


# ---------------------------------------------------------------------------------------------- fp8 operands (BASELINE config 5)
FP8 = torch.float8_e4m3fn
FP8_KPAD = 1024        # the token axis of a transposed copy is padded to a multiple of this (8 K-splits of whole 128-byte K-tiles)


class Fp8:
    """A per-tensor-scaled e4m3 copy of a 2-D activation / gradient / weight: q [rows, cols] (the NT GEMM's A or B operand), optionally
    qt [cols, rows_pad] (the same values transposed, token axis zero padded: the operand of the weight-gradient GEMM), and the device
    scalars (scales[0] = 448/amax, scales[1] = amax/448 = `dequant`)."""
    __slots__ = ("q", "qt", "scales", "rows", "cols")

    def __init__(self, q, qt, scales, rows, cols):
        self.q, self.qt, self.scales, self.rows, self.cols = q, qt, scales, rows, cols

    @property
    def dequant(self):
        return self.scales[1:2]


# Delayed scaling (round 4): a tensor that is quantised every step at the same place of the graph keeps a 4-float STATE on the device
# (tav_fp8_quantize_delayed).  Its first quantisation calibrates (current scaling: amax passes + quantiser, what rounds 2-3 did every time);
# from then on ONE launch quantises with the scale the previous step left and gathers the new maximum on the way; fp8_roll_all() -- called by the
# optimizer step, inside the captured graph -- turns the gathered maxima into the next step's scales.
_fp8_state_sets = []


class Fp8States:
    """`n` states of 4 floats in one device tensor; slot(key) hands out (and remembers) the state of one quantisation site."""

    def __init__(self, device, n=8192):
        import weakref
        self.dev = torch.zeros(n, 4, dtype=torch.float32, device=device)
        self.index, self.calibrated = {}, set()
        _fp8_state_sets.append(weakref.ref(self))

    def slot(self, key):
        i = self.index.get(key)
        if i is None:
            i = len(self.index)
            if i >= self.dev.shape[0]:
                raise RuntimeError("Fp8States: out of slots")
            self.index[key] = i
        return i

    def roll(self):
        if self.index:
            check(lib().tav_fp8_roll_states(ptr(self.dev), len(self.index), stream()), "fp8_roll_states")


def fp8_roll_all():
    """End of a training step: every quantisation site's gathered maximum becomes its next scale (one tiny launch per state set)."""
    live = []
    for r in _fp8_state_sets:
        st = r()
        if st is not None:
            st.roll()
            live.append(r)
    _fp8_state_sets[:] = live


def fp8_quantize(x, *, want_q=True, want_t=False, state=None):
    """x [rows, cols] f32 / bf16 (row stride arbitrary) -> Fp8.  Without `state`: current scaling (two launches for the absolute maximum, one for
    the copies).  state = (Fp8States, key): delayed scaling once the site is calibrated (see above).  The scale stays on the device either way."""
    rows, cols = x.shape
    q = torch.empty(rows, cols, dtype=FP8, device=x.device) if want_q else None
    rows_pad = (rows + FP8_KPAD - 1) // FP8_KPAD * FP8_KPAD
    qt = torch.empty(cols, rows_pad, dtype=FP8, device=x.device) if want_t else None
    if state is not None:
        sts, key = state
        i = sts.slot(key)
        scales = sts.dev[i]
        if i in sts.calibrated:
            check(lib().tav_fp8_quantize_delayed(ptr(x), dt(x), rows, cols, x.stride(0), ptr(scales), ptr(q), cols, ptr(qt), rows_pad, rows_pad, stream()),
                  "fp8_quantize_delayed")
            return Fp8(q, qt, scales, rows, cols)
        sts.calibrated.add(i)
    else:
        scales = torch.empty(3, dtype=torch.float32, device=x.device)
    part = workspace("fp8_amax", lib().tav_fp8_amax_partials(rows, cols), x.device)
    check(lib().tav_fp8_amax(ptr(x), dt(x), rows, cols, x.stride(0), ptr(part), ptr(scales), stream()), "fp8_amax")
    check(lib().tav_fp8_quantize(ptr(x), dt(x), rows, cols, x.stride(0), ptr(scales), ptr(q), cols, ptr(qt), rows_pad, rows_pad, stream()), "fp8_quantize")
    return Fp8(q, qt, scales, rows, cols)


def gemm_nt_fp8(a8, b8, **kw):
    """epi(A @ B^T) on two Fp8 operands (their .q copies)."""
    return gemm_nt(a8.q, b8.q, a_dequant=a8.dequant, b_dequant=b8.dequant, **kw)


def wgrad_fp8(dy8, x8, nsplit=8):
    """dW [N1, N2] f32 = dY^T X for two Fp8 tensors over the same token axis, as the NT GEMM of their transposed copies: M = N1, N = N2,
    K = padded tokens split into `nsplit` z-slices that write f32 slabs, summed in a fixed order by tav_splitk_reduce."""
    at, bt = dy8.qt, x8.qt
    N1, Kp = at.shape
    N2 = bt.shape[0]
    assert bt.shape[1] == Kp and Kp % (128 * nsplit) == 0
    kc = Kp // nsplit
    slabs = workspace("fp8_wgrad_slabs", nsplit * N1 * N2, at.device)
    gemm_nt(at, bt, out=slabs.view(-1)[:nsplit * N1 * N2].view(nsplit * N1, N2), out_dtype=torch.float32, M=N1, N=N2, K=kc, lda=Kp, ldb=Kp, ldc=N2,
            nzb=nsplit, a_zb=kc, b_zb=kc, c_zb=N1 * N2, a_dequant=dy8.dequant, b_dequant=x8.dequant)
    out = torch.empty(N1, N2, dtype=torch.float32, device=at.device)
    check(lib().tav_splitk_reduce(ptr(slabs), ptr(out), nsplit, N1 * N2, 0, stream()), "splitk_reduce")
    return out


def colsum(x, *, out=None, accumulate=False, M=None, N=None, ld=None):
    if M is None:
        M, N, ld = x.shape[-2], x.shape[-1], x.stride(-2)
    nparts = max(1, min(256, (M + 15) // 16))        # a workgroup column-sums >= 16 rows (hundreds of rows per workgroup at small M was latency bound)
    part = workspace("colsum", nparts * N, x.device)
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x.device)
    check(lib().tav_colsum(ptr(x), dt(x), M, N, ld, ptr(part), nparts, ptr(out), int(accumulate), stream()), "colsum")
    return out


# ---------------------------------------------------------------------------------------------- attention
def _attn_args(q, k, v, o, B, S, nheads, key_mask, lse, corr, mask_mode, scale, o_soft=None, q_prescaled=False):
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o = ptr(q), ptr(k), ptr(v), ptr(o)
    a.key_mask, a.lse, a.corr, a.o_soft = ptr(key_mask), ptr(lse), ptr(corr), ptr(o_soft)
    a.B, a.S, a.nheads = B, S, nheads
    a.ld_q, a.ld_k, a.ld_v, a.ld_o = q.stride(-2), k.stride(-2), v.stride(-2), o.stride(-2)
    a.dtype, a.mask_mode, a.scale, a.q_prescaled = dt(q), mask_mode, scale, int(bool(q_prescaled))
    return a


ATTN_Q_PRESCALE = 0.125 * 1.4426950408889634      # what a prescaled q carries: softmax scale (head dim 64) x log2(e)


def _seq_lens(seq_lens, B, device):
    """Per-row valid lengths of a length-aware launch: an int32 [B] tensor on the attention's device (a bad one is an error, not a copy)."""
    if not (isinstance(seq_lens, torch.Tensor) and seq_lens.dtype == torch.int32 and seq_lens.device == device and seq_lens.numel() == B
            and seq_lens.is_contiguous()):
        raise ValueError(f"seq_lens must be a contiguous int32 tensor of {B} entries on {device}, got {seq_lens!r}")
    return seq_lens


def attn_fwd(q, k, v, B, S, nheads, *, key_mask=None, mask_mode=0, scale=0.125, q_prescaled=False, seq_lens=None):
    """q,k,v: [B*S, >=nheads*64] views (row stride arbitrary).  Returns o [B*S, nheads*64], lse, corr.
    q_prescaled: q already holds q * scale * log2(e) (tav_attn_args.q_prescaled).
    seq_lens: None, or int32 [B] on the device: row b holds L_b valid tokens of its S (tav_attn_fwd_len; rows past L_b come out zero)."""
    H = nheads * 64
    o = torch.empty(B * S, H, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, nheads, S, dtype=torch.float32, device=q.device)
    corr = torch.empty(B, nheads, 64, dtype=torch.float32, device=q.device) if mask_mode == 2 else None
    o_soft = torch.empty_like(o) if mask_mode == 2 else None
    a = _attn_args(q, k, v, o, B, S, nheads, key_mask, lse, corr, mask_mode, scale, o_soft, q_prescaled)
    es = q.element_size()
    if seq_lens is None:
        run = lambda: check(lib().tav_attn_fwd(C.byref(a), stream()), "attn_fwd")      # noqa: E731
    else:
        sl = _seq_lens(seq_lens, B, q.device)
        run = lambda: check(lib().tav_attn_fwd_len(C.byref(a), ptr(sl), stream()), "attn_fwd_len")      # noqa: E731
    _prof_launch("attn", "bf16" if q.dtype == torch.bfloat16 else "f32", 4.0 * B * nheads * S * S * 64, 4 * B * S * H * es,      # Q, K, V, O once
                 run)
    return o, lse, (corr, o_soft)


def attn_bwd(q, k, v, o, dout, lse, corr, B, S, nheads, *, key_mask=None, mask_mode=0, scale=0.125, dqkv=None, q_prescaled=False, seq_lens=None):
    """Returns dqkv [B*S, 3H] (dq | dk | dv), the layout the fused QKV projection's backward consumes.
    seq_lens: as in attn_fwd (tav_attn_bwd_len; dq / dk / dv rows past L_b come out zero)."""
    H = nheads * 64
    if dqkv is None:
        dqkv = torch.empty(B * S, 3 * H, dtype=q.dtype, device=q.device)
    dq, dk, dv = dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:]
    delta = workspace("attn_delta", B * nheads * S, q.device)
    corr, o_soft = corr if corr is not None else (None, None)
    a = _attn_args(q, k, v, o, B, S, nheads, key_mask, lse, corr, mask_mode, scale, o_soft, q_prescaled)
    a.dout, a.dq, a.dk, a.dv, a.delta = ptr(dout), ptr(dq), ptr(dk), ptr(dv), ptr(delta)
    a.ld_do, a.ld_dq, a.ld_dk, a.ld_dv = dout.stride(-2), dq.stride(-2), dk.stride(-2), dv.stride(-2)
    es = q.element_size()
    # algorithmic work by the contract (BASELINE.md section 2 / SURVEY.md section 8d: fwd + bwd = 3 x fwd, so the backward is 2 x 4 B h S^2 d); the two
    # atomic-free kernels EXECUTE 14 B h S^2 d (S and dP are recomputed in both), reported beside it as `frac_executed`
    if seq_lens is None:
        run = lambda: check(lib().tav_attn_bwd(C.byref(a), stream()), "attn_bwd")      # noqa: E731
    else:
        sl = _seq_lens(seq_lens, B, q.device)
        run = lambda: check(lib().tav_attn_bwd_len(C.byref(a), ptr(sl), stream()), "attn_bwd_len")      # noqa: E731
    _prof_launch("attn", "bf16" if q.dtype == torch.bfloat16 else "f32", 8.0 * B * nheads * S * S * 64, 8 * B * S * H * es,     # Q, K, V, O, dO in; dQ, dK, dV out
                 run, work_exec=14.0 * B * nheads * S * S * 64)
    return dqkv


def attn_probs(q, k, lse, B, S, nheads, *, key_mask=None, mask_mode=0, scale=0.125, q_prescaled=False, head_scale=None):
    """Attention probabilities as a tensor, f32 [B, nheads, S, S] (slow path: VideoMAEEncoder(output_attentions=True), reference
    utils/TAVFormer.py:362-375, :389), from q, k and the lse of attn_fwd.  head_scale: f32 [nheads] or [B, nheads] (head_mask) or None."""
    probs = torch.empty(B, nheads, S, S, dtype=torch.float32, device=q.device)
    a = _attn_args(q, k, q, q, B, S, nheads, key_mask, lse, None, mask_mode, scale, None, q_prescaled)
    bstride = 0 if head_scale is None or head_scale.numel() == nheads else nheads
    check(lib().tav_attn_probs(C.byref(a), ptr(probs), ptr(head_scale), bstride, stream()), "attn_probs")
    return probs


def head_scale(a, b, hs, c0, B, S, nheads, out=None):
    """out[r, h*64+d] = (a or 0) + (c0 + hs[b, h]) * b[r, h*64+d] for token-major [B*S, nheads*64] tensors (row stride arbitrary); hs f32
    [nheads] / [B, nheads] or None.  The head_mask arithmetic of the fusion encoder's slow path (reference utils/TAVFormer.py:368-370)."""
    if out is None:
        out = torch.empty(B * S, nheads * 64, dtype=b.dtype, device=b.device)
    bstride = 0 if hs is None or hs.numel() == nheads else nheads
    check(lib().tav_head_scale(ptr(a), ptr(b), ptr(out), dt(b), ptr(hs), bstride, float(c0), B, S, nheads,
                               a.stride(-2) if a is not None else 0, b.stride(-2), out.stride(-2), stream()), "head_scale")
    return out


# ---------------------------------------------------------------------------------------------- layer norm
def ln_fwd(x, gamma, beta, eps, *, want_f32=True, lp_dtype=None, act=0):
    """x [rows, W] f32 or bf16.  Returns (y_f32 | None, y_lp | None, mean, rstd)."""
    rows, W = x.shape
    y32 = torch.empty(rows, W, dtype=torch.float32, device=x.device) if want_f32 else None
    ylp = torch.empty(rows, W, dtype=lp_dtype, device=x.device) if lp_dtype is not None else None
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    a = L.LnArgs()
    a.x, a.x_dtype, a.gamma, a.beta = ptr(x), dt(x), ptr(gamma), ptr(beta)
    a.y_f32, a.y_lp, a.lp_dtype = ptr(y32), ptr(ylp), dt(lp_dtype) if lp_dtype is not None else 0
    a.mean, a.rstd = ptr(mean), ptr(rstd)
    a.rows, a.W, a.ld_x, a.ld_y, a.eps, a.act = rows, W, x.stride(0), W, eps, act
    nb = rows * W * (x.element_size() + (4 if want_f32 else 0) + (ylp.element_size() if ylp is not None else 0)) + rows * 8
    _prof_launch("ln", "hbm", 0.0, nb, lambda: check(lib().tav_ln_fwd(C.byref(a), stream()), "ln_fwd"))
    return y32, ylp, mean, rstd


# Deferred second stage of the LayerNorm backward.  Inside an autograd backward pass nobody reads dgamma / dbeta before the pass ends (they
# flow straight into AccumulateGrad), so every LayerNorm keeps its own partial slab and ONE launch per 64 of them reduces the lot from a
# callback the engine runs when the pass is over -- on the caller's stream, after it has been synchronised with every stream a gradient was
# produced on (torch/csrc/autograd/engine.cpp, GraphTask::exec_post_processing), hence also under multi-stream capture.  ~210 launches per step
# become 4.  Off (immediate reduce) outside a backward pass and while a hook-mode reducer is active (ddp.BucketedAllReduce reads gradients
# from post-accumulate hooks, i.e. before the pass ends).
# What autograd does with a returned gradient decides the rest (torch/csrc/autograd/functions/accumulate_grad.h):
#   * a parameter WITHOUT a gradient takes it over -- `grad = new_grad.detach()`, same storage -- provided nobody else holds the tensor: the
#     pending list therefore keeps the STORAGES of dgamma / dbeta alive, never the tensors (a second reference would make AccumulateGrad
#     clone the still unwritten buffer);
#   * a parameter that already HAS a gradient is accumulated in place, at once: it reads the buffer -- so a LayerNorm whose gamma / beta
#     carry a gradient (accumulation over several backwards, zero-filled gradients) is reduced immediately, not deferred.
# Two facts, kept apart: whether this torch can run the flush when the pass ends (cleared for good by the queue_callback fallback below), and
# whether a hook-mode reducer is live (ln_hook_mode, owned by ddp.BucketedAllReduce).
_ln_state = {"supported": True, "hook_mode": False}
_ln_pending = {"task": -1, "items": []}


def ln_hook_mode(live):
    """A hook-mode gradient reducer went live / away: while one is, LayerNorm parameter gradients are reduced at once."""
    _ln_state["hook_mode"] = bool(live)


def ln_deferring():
    """Whether a LayerNorm backward inside an autograd pass defers its parameter reduce to the end of the pass."""
    return _ln_state["supported"] and not _ln_state["hook_mode"]


def _graph_task_id():
    try:
        return torch._C._current_graph_task_id()
    except Exception:
        return -1


def ln_flush():
    """Reduce every pending LayerNorm's partial slab into its dgamma / dbeta (current stream)."""
    items, _ln_pending["items"] = _ln_pending["items"], []
    _ln_pending["task"] = -1
    cur = torch.cuda.current_stream() if items and items[0][0].is_cuda else None
    for i in range(0, len(items), L.LN_REDUCE_MAX):
        chunk = items[i:i + L.LN_REDUCE_MAX]
        arr = (L.LnReduceItem * len(chunk))()
        for j, (part, dg_st, db_st, dg_ptr, db_ptr, nblk, W) in enumerate(chunk):
            if cur is not None:              # allocated under a branch stream, used here: the allocator must not recycle them before this launch ran
                part.record_stream(cur)
                for st in (dg_st, db_st):
                    torch.empty(0, dtype=torch.float32, device=part.device).set_(st).record_stream(cur)
            arr[j].partials, arr[j].dgamma, arr[j].dbeta, arr[j].nblocks, arr[j].W, arr[j].accumulate = ptr(part), dg_ptr, db_ptr, nblk, W, 0
        check(lib().tav_ln_param_reduce_multi(arr, len(chunk), stream()), "ln_param_reduce_multi")


def _ln_defer_register(part, dgamma, dbeta, nblk, W):
    tid = _graph_task_id()
    item = (part, dgamma.untyped_storage(), dbeta.untyped_storage(), dgamma.data_ptr(), dbeta.data_ptr(), nblk, W)
    if _ln_pending["task"] != tid:
        # a new backward pass (whatever an aborted earlier one left behind is dropped: its gradients were never consumed)
        _ln_pending["task"], _ln_pending["items"] = tid, []
        try:
            torch.autograd.Variable._execution_engine.queue_callback(ln_flush)
        except Exception:                       # (a torch without this private hook: reduce at once and stop deferring)
            _ln_state["supported"] = False
            _ln_pending["items"] = [item]
            ln_flush()
            return
    _ln_pending["items"].append(item)


def _grad_free_leaf(p):
    return bool(getattr(p, "is_leaf", False)) and p.grad is None


def ln_bwd(dy, x, gamma, beta, mean, rstd, *, dx_add=None, want_f32=True, lp_dtype=None, act=0, param_grads=True):
    """Returns (dx_f32 | None, dx_lp | None, dgamma, dbeta)."""
    rows, W = x.shape
    dx32 = torch.empty(rows, W, dtype=torch.float32, device=x.device) if want_f32 else None
    dxlp = torch.empty(rows, W, dtype=lp_dtype, device=x.device) if lp_dtype is not None else None
    dgamma = dbeta = part = None
    defer = False
    if param_grads:
        dgamma = torch.empty(W, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(W, dtype=torch.float32, device=x.device)
        nblk = lib().tav_ln_bwd_partials(rows)
        defer = ln_deferring() and _graph_task_id() >= 0 and _grad_free_leaf(gamma) and _grad_free_leaf(beta)
        if defer:
            part = torch.empty(nblk * 2 * W, dtype=torch.float32, device=x.device)      # its own slab: alive until ln_flush()
        else:
            part = workspace("ln_part", nblk * 2 * W, x.device)
    a = L.LnArgs()
    a.x, a.x_dtype, a.gamma, a.beta = ptr(x), dt(x), ptr(gamma), ptr(beta)
    a.mean, a.rstd = ptr(mean), ptr(rstd)
    a.dy, a.dy_dtype, a.dx_add = ptr(dy), dt(dy), ptr(dx_add)
    a.dx_f32, a.dx_lp, a.lp_dtype = ptr(dx32), ptr(dxlp), dt(lp_dtype) if lp_dtype is not None else 0
    a.dgamma, a.dbeta, a.partials, a.accumulate_params = ptr(dgamma), ptr(dbeta), ptr(part), 0
    a.defer_param_reduce = int(defer)
    a.rows, a.W, a.ld_x, a.ld_dy, a.ld_dx, a.act = rows, W, x.stride(0), dy.stride(0), W, act
    nb = rows * W * (x.element_size() + dy.element_size() + (4 if dx_add is not None else 0) + (4 if want_f32 else 0)
                     + (dxlp.element_size() if dxlp is not None else 0)) + rows * 8
    _prof_launch("ln", "hbm", 0.0, nb, lambda: check(lib().tav_ln_bwd(C.byref(a), stream()), "ln_bwd"))
    if defer:
        _ln_defer_register(part, dgamma, dbeta, nblk, W)
    return dx32, dxlp, dgamma, dbeta


# ---------------------------------------------------------------------------------------------- casts & small ops
def cast_weight(w, dtype, *, want_t=True, want_n=True, out_n=None, out_t=None):
    """f32 [R,C] parameter -> (copy in dtype [R,C], transposed copy [C,R]).  out_n / out_t may be (strided) views of a
    larger fused operand (row stride taken from the view)."""
    R, Cc = w.shape
    n = out_n if out_n is not None else (torch.empty(R, Cc, dtype=dtype, device=w.device) if want_n else None)
    t = out_t if out_t is not None else (torch.empty(Cc, R, dtype=dtype, device=w.device) if want_t else None)
    check(lib().tav_cast_weight(ptr(w), R, Cc, ptr(n), n.stride(0) if n is not None else 0, ptr(t), t.stride(0) if t is not None else 0,
                                dt(dtype), stream()), "cast_weight")
    return n, t


def make_cast_descs(entries, device):
    """entries: list of (src f32 [R,C], dst|None, dst_t|None[, scale_n]).  scale_n multiplies the values written to dst only (the transposed
    copy stays unscaled): the attention pre-scale of the q rows.  Returns a device uint8 tensor holding the C descriptor table."""
    import struct
    buf = bytearray()
    for ent in entries:
        src, dst, dst_t = ent[:3]
        scale_n = float(ent[3]) if len(ent) > 3 and ent[3] is not None else 1.0
        R, Cc = src.shape
        ref = dst if dst is not None else dst_t
        buf += struct.pack("<QQQqqiiif", src.data_ptr(), dst.data_ptr() if dst is not None else 0, dst_t.data_ptr() if dst_t is not None else 0,
                           dst.stride(0) if dst is not None else Cc, dst_t.stride(0) if dst_t is not None else R, R, Cc, dt(ref), scale_n)
    tiles = max(((e[0].shape[0] + 31) // 32) * ((e[0].shape[1] + 31) // 32) for e in entries)
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).clone().to(device), tiles


def cast_weights_multi(descs, n, blocks_per_tensor=96):
    check(lib().tav_cast_weights_multi(ptr(descs), n, blocks_per_tensor, stream()), "cast_weights_multi")


def cast_conv_weight(w, dtype, conv_stride=0):
    """-> (forward operand [co, k*ci], column-buffer dgrad operand [k*ci, co], per-phase dgrad operands flat [co*ci*k] or None).
    conv_stride > 0 asks for the phase operands (tav_cast_conv_weight, include/tavhip.h)."""
    co, ci, k = w.shape
    n = torch.empty(co, k * ci, dtype=dtype, device=w.device)
    t = torch.empty(k * ci, co, dtype=dtype, device=w.device)
    ph = torch.empty(co * ci * k, dtype=dtype, device=w.device) if conv_stride and conv_stride <= k else None
    check(lib().tav_cast_conv_weight(ptr(w), co, ci, k, ptr(n), ptr(t), ptr(ph), conv_stride if ph is not None else 0, dt(dtype), stream()), "cast_conv_weight")
    return n, t, ph


def zero_pad_rows(buf, B, T, Cc, pad):
    """Zero the `pad` leading and trailing rows of each of the B entries of a [B, T + 2*pad, Cc] buffer."""
    check(lib().tav_zero_pad_rows(ptr(buf), dt(buf), B, T, Cc, pad, stream()), "zero_pad_rows")
    return buf


def cast2d(x, dtype, out=None):
    R, Cc = x.shape
    if out is None:
        out = torch.empty(R, Cc, dtype=dtype, device=x.device)
    check(lib().tav_cast2d(ptr(x), dt(x), x.stride(0), ptr(out), dt(out), out.stride(0), R, Cc, stream()), "cast2d")
    return out


def transpose2d(x, R, Cc, nbatch):
    """x: [nbatch*R, Cc] -> per batch transposed [nbatch*Cc, R] (returned with the same 2-D shape as x: the reference re-views it)."""
    out = torch.empty_like(x)
    check(lib().tav_transpose2d(ptr(x), ptr(out), dt(x), R, Cc, nbatch, stream()), "transpose2d")
    return out


def add_f32(a, b, *, want_f32=True, lp_dtype=None):
    y = torch.empty_like(a) if want_f32 else None
    ylp = torch.empty(a.shape, dtype=lp_dtype, device=a.device) if lp_dtype is not None else None
    check(lib().tav_add_f32(ptr(a), ptr(b), ptr(y), ptr(ylp), dt(lp_dtype) if lp_dtype is not None else 0, a.numel(), stream()), "add_f32")
    return y, ylp


def zeros_f32(shape, device):
    t = torch.empty(shape, dtype=torch.float32, device=device)
    check(lib().tav_fill_f32(ptr(t), 0.0, t.numel(), stream()), "fill")
    return t


def embed_add_fwd(x, ids, table):
    rows, W = x.shape
    out = torch.empty_like(x)
    check(lib().tav_embed_add_fwd(ptr(x), ptr(ids), ptr(table), ptr(out), rows, W, table.shape[0], stream()), "embed_add_fwd")
    return out


def embed_add_bwd(dy, ids, ntable):
    rows, W = dy.shape
    parts = lib().tav_embed_add_bwd_parts(rows)
    part = workspace("embed_part", parts * ntable * W, dy.device)
    d = torch.empty(ntable, W, dtype=torch.float32, device=dy.device)
    check(lib().tav_embed_add_bwd(ptr(dy), ptr(ids), ptr(d), ptr(part), rows, W, ntable, 0, stream()), "embed_add_bwd")
    return d


def text_embed_fwd(ids, word, pos, type_, gamma, beta, eps, pad_id, *, want_f32=True, lp_dtype=None):
    B, S = ids.shape
    W = word.shape[1]
    dev = ids.device
    pre = torch.empty(B * S, W, dtype=torch.float32, device=dev)
    pos_ids = torch.empty(B, S, dtype=torch.int64, device=dev)
    y32 = torch.empty(B * S, W, dtype=torch.float32, device=dev) if want_f32 else None
    ylp = torch.empty(B * S, W, dtype=lp_dtype, device=dev) if lp_dtype is not None else None
    mean = torch.empty(B * S, dtype=torch.float32, device=dev)
    rstd = torch.empty(B * S, dtype=torch.float32, device=dev)
    a = L.TextEmbedArgs()
    a.ids, a.word, a.pos, a.type, a.gamma, a.beta = ptr(ids), ptr(word), ptr(pos), ptr(type_), ptr(gamma), ptr(beta)
    a.pre, a.pos_ids, a.y_f32, a.y_lp = ptr(pre), ptr(pos_ids), ptr(y32), ptr(ylp)
    a.lp_dtype = dt(lp_dtype) if lp_dtype is not None else 0
    a.mean, a.rstd = ptr(mean), ptr(rstd)
    a.B, a.S, a.W, a.vocab, a.max_pos, a.pad_id, a.eps = B, S, W, word.shape[0], pos.shape[0], pad_id, eps
    check(lib().tav_text_embed_fwd(C.byref(a), stream()), "text_embed_fwd")
    return y32, ylp, pre, pos_ids, mean, rstd


def scatter_add_rows(d, idx, ntable):
    rows, W = d.shape
    out = zeros_f32((ntable, W), d.device)
    check(lib().tav_scatter_add_rows(ptr(d), ptr(idx), ptr(out), rows, W, ntable, stream()), "scatter_add_rows")
    return out


def gather_rows(table, idx):
    rows, W = idx.numel(), table.shape[1]
    out = torch.empty(rows, W, dtype=torch.float32, device=table.device)
    check(lib().tav_gather_rows(ptr(table), ptr(idx), ptr(out), rows, W, table.shape[0], stream()), "gather_rows")
    return out


def mask_to_index(mask_bool, keep_value, nkeep):
    B, n = mask_bool.shape
    m8 = mask_bool.view(torch.uint8) if mask_bool.dtype == torch.bool else mask_bool
    idx = torch.empty(B, nkeep, dtype=torch.int32, device=mask_bool.device)
    counts = torch.empty(B, dtype=torch.int32, device=mask_bool.device)
    check(lib().tav_mask_to_index(ptr(m8), int(keep_value), ptr(idx), ptr(counts), B, n, nkeep, stream()), "mask_to_index")
    return idx, counts


RAGGED_OVER_TRUE, RAGGED_OVER_KEEP = 1, 2        # bits of the status word (include/tavhip.h)


def ragged_lens(mask_bool, cap_true, cap_keep, base):
    """Per-row lengths of a ragged batch at fixed capacities, from the video mask [B, ntok] as it is on the device when the kernel runs:
    -> (true_cnt, vid_lens = min(ntok - true_cnt, cap_keep), av_lens = base + min(true_cnt, cap_true), status), int32 [B] x 3 and int32 [1].
    status is zeroed here and gets RAGGED_OVER_TRUE / RAGGED_OVER_KEEP OR-ed in by rows that do not fit (tav_ragged_lens)."""
    B, n = mask_bool.shape
    m8 = mask_bool.view(torch.uint8) if mask_bool.dtype == torch.bool else mask_bool
    if not m8.is_contiguous():
        raise ValueError("ragged_lens: the mask must be contiguous")
    dev = mask_bool.device
    true_cnt, vid_lens, av_lens = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().tav_ragged_lens(ptr(m8), ptr(true_cnt), ptr(vid_lens), ptr(av_lens), ptr(status), B, n, int(cap_true), int(cap_keep), int(base),
                                stream()), "ragged_lens")
    return true_cnt, vid_lens, av_lens, status


def patchify(video, keep_idx, dtype):
    B, F, Cc, H, W = video.shape
    assert Cc == 3 and video.dtype == torch.float32 and video.is_contiguous()
    nkeep = keep_idx.shape[1]
    out = torch.empty(B * nkeep, 1536, dtype=dtype, device=video.device)
    check(lib().tav_patchify(ptr(video), ptr(keep_idx), ptr(out), dt(dtype), B, F, H, W, nkeep, stream()), "patchify")
    return out


# ---------------------------------------------------------------------------------------------- video clip transform
CLIP_MEAN, CLIP_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # reference models/tav.py:67-68


def clip_layout(src, layout=None):
    """Layout of decoded frames: "THWC" (uint8 [T, H, W, 3], a decoder's output) or "CTHW" ([3, T, H, W], pytorchvideo's get_clip).  f32 frames are CTHW; uint8 frames
    are THWC unless only the first axis is 3.  `layout` overrides."""
    if layout is None:
        layout = "CTHW" if src.dtype != torch.uint8 or (src.shape[0] == 3 and src.shape[-1] != 3) else "THWC"
    if layout not in ("THWC", "CTHW") or src.dim() != 4 or src.shape[3 if layout == "THWC" else 0] != 3:
        raise ValueError(f"video frames: need uint8 [T, H, W, 3] or uint8 / float32 [3, T, H, W], got {tuple(src.shape)} {src.dtype} as {layout}")
    return layout


def clip_xform(src, frames, *, layout=None, crop=None, mid=None, out_hw=(224, 224), hflip=False, vflip=False, mean=CLIP_MEAN, std=CLIP_STD):
    """The tav_clip_xform of one clip: src's sizes and strides, the source frame of every output frame, crop (top, left, h, w) or None, the
    size after the first resize (mid_h, mid_w) or None, the output size, the flips, and y = v * scale[c] - shift[c] with
    scale = 1 / (255 std) and shift = mean / std rounded to f32 (mean = 0, std = 1 / 255 leaves the raw value)."""
    layout = clip_layout(src, layout)
    if src.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"video frames must be uint8 or float32, got {src.dtype}")
    x = L.ClipXform()
    x.src_dtype = L.TAV_U8 if src.dtype == torch.uint8 else L.TAV_F32
    st = src.stride()
    if layout == "THWC":
        (x.T, x.H, x.W), (x.sT, x.sH, x.sW, x.sC) = src.shape[:3], st
    else:
        (x.T, x.H, x.W), (x.sC, x.sT, x.sH, x.sW) = src.shape[1:], st
    frames = [int(f) for f in frames]
    if not 1 <= len(frames) <= 32:
        raise ValueError(f"a clip has 1..32 frames, got {len(frames)}")
    x.nf = len(frames)
    for i, f in enumerate(frames):
        x.frame[i] = f
    x.crop_top, x.crop_left, x.crop_h, x.crop_w = (0, 0, x.H, x.W) if crop is None else [int(v) for v in crop]
    x.mid_h, x.mid_w = (0, 0) if mid is None else [int(v) for v in mid]
    x.out_h, x.out_w = [int(v) for v in out_hw]
    x.hflip, x.vflip = int(bool(hflip)), int(bool(vflip))
    for c in range(3):
        x.scale[c] = 1.0 / (255.0 * std[c])
        x.shift[c] = mean[c] / std[c]
    return x


def video_clip_transform(src, out, xform):
    """tav_video_clip_transform: src (device, uint8 or f32, any strides; xform from clip_xform(src, ...)) -> out f32 [nf, 3, out_h, out_w],
    contiguous -- a slab of the batch tensor or, with out=None, a new tensor.  One launch, nothing staged on the host."""
    if not src.is_cuda:
        raise ValueError("video_clip_transform runs on the GPU only (libtavhip has no host form): move the frames to the device, or use "
                         "models.tav.video_features_device, which ships the selected frames once")
    shape = (xform.nf, 3, xform.out_h, xform.out_w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    if tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != src.device:
        raise ValueError(f"video_clip_transform: out must be a contiguous float32 {shape} tensor on {src.device}, "
                         f"got {tuple(out.shape)} {out.dtype} on {out.device}")
    last = (xform.T - 1) * xform.sT + (xform.H - 1) * xform.sH + (xform.W - 1) * xform.sW + 2 * xform.sC
    if src.storage_offset() + last >= src.untyped_storage().nbytes() // src.element_size():
        raise ValueError("video_clip_transform: the transform's sizes and strides reach past the source tensor's storage")
    check(lib().tav_video_clip_transform(ptr(src), ptr(out), C.byref(xform), stream()), "video_clip_transform")
    return out


# ---------------------------------------------------------------------------------------------- audio waveform transform
_resample_tables = {}


def resample_ratio(sr, target=16000):
    """(o, n) = (sr / g, target / g), g = gcd(sr, target)."""
    sr, target = int(sr), int(target)
    if sr < 1 or target < 1:
        raise ValueError(f"sampling rates must be positive, got {sr} -> {target}")
    g = math.gcd(sr, target)
    return sr // g, target // g


def resampled_length(L, sr, target=16000):
    """Samples torchaudio's Resample(sr, target) returns for L: ceil(target * L / sr), in integers."""
    o, n = resample_ratio(sr, target)
    return (n * int(L) + o - 1) // o


def sinc_resample_coefficients(sr, target=16000):
    """torchaudio's _get_sinc_resample_kernel at Resample's defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99, dtype None):
    fp64 arithmetic, rounded once to f32.  -> (h f32 [n][2 width + o], o, n, width), numpy."""
    o, n = resample_ratio(sr, target)
    base = min(o, n) * 0.99
    width = math.ceil(6 * o / base)
    k = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    p = np.arange(0, -n, -1, dtype=np.float64)[:, None] / n
    t = np.clip((p + k) * base, -6.0, 6.0)
    win = np.cos(t * math.pi / 6 / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.where(t == 0, 1.0, np.sin(t) / t) * win * (base / o)
    return h.astype(np.float32), o, n, width


class ResampleTable:
    """The compact filter of one (sr, target) pair on one device: table f32 [n, ntap] and first int32 [n] there (row p holds taps first[p] ..
    first[p] + ntap - 1 of phase p, zero-filled past its own live taps), their host copies (h, first_host) and o, n, width, ntap, tile."""

    def __init__(self, sr, target, device):
        self.sr, self.target = int(sr), int(target)
        if self.sr == self.target:                                      # Resample.forward returns its input: one phase, the one tap 1.0
            self.o, self.n, self.width = 1, 1, 0
            self.h, self.first_host = np.ones((1, 1), np.float32), np.zeros(1, np.int32)
        else:
            full, self.o, self.n, self.width = sinc_resample_coefficients(sr, target)
            K = full.shape[1]
            nz = full != 0
            lo, hi = nz.argmax(1), K - 1 - nz[:, ::-1].argmax(1)
            ntap = int((hi - lo + 1).max())
            self.first_host = np.minimum(lo, K - ntap).astype(np.int32)
            cols = self.first_host[:, None] + np.arange(ntap)[None, :]
            self.h = np.ascontiguousarray(np.take_along_axis(full, cols, 1))
            kept = np.zeros_like(nz)
            np.put_along_axis(kept, cols, True, 1)
            assert np.all(full[~kept] == 0.0), "a tap outside the compact table is not 0.0f"
        self.ntap = self.h.shape[1]
        self.first_max = int(self.first_host.max())
        assert self.first_host.min() >= 0 and self.first_max + self.ntap <= 2 * self.width + self.o
        self.tile = int(lib().tav_audio_resample_tile(self.o, self.n, self.width))
        if self.tile == 0:
            raise ValueError(f"audio_resample_table: {self.sr} -> {self.target} Hz (o / n = {self.o} / {self.n}) needs a longer input span per "
                             "workgroup than the kernel keeps in LDS")
        self.device = torch.device(device)
        self.table = torch.from_numpy(self.h).to(self.device)
        self.first = torch.from_numpy(self.first_host).to(self.device)


def audio_resample_table(sr, target=16000, device="cuda"):
    """The ResampleTable of (sr, target) on `device`: computed in fp64 numpy, rounded to f32, compacted (every dropped tap is asserted to be
    0.0f), uploaded once and cached."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(sr), int(target), str(device))
    if key not in _resample_tables:
        _resample_tables[key] = ResampleTable(sr, target, device)
    return _resample_tables[key]


def pcm_layout(src, layout=None):
    """Layout of decoded PCM: "L" (mono [L]), "CL" (planar [C, L], torchaudio.load) or "LC" (interleaved [L, C], a decoder's frames).  A 2-D
    tensor's shorter axis is taken as the channels (planar when equal); `layout` overrides."""
    if layout is None:
        layout = "L" if src.dim() == 1 else ("CL" if src.dim() == 2 and src.shape[0] <= src.shape[1] else "LC")
    if layout not in ("L", "CL", "LC") or src.dim() != (1 if layout == "L" else 2):
        raise ValueError(f"PCM: need [L], [C, L] or [L, C], got {tuple(src.shape)} as {layout}")
    return layout


def resample_args(src, table, T_row=None, layout=None):
    """The tav_resample_args of one utterance: src's channel count, length and element strides, the table's rate pair, the row length
    (L_out when None)."""
    layout = pcm_layout(src, layout)
    if src.dtype not in (torch.int16, torch.float32):
        raise TypeError(f"PCM must be int16 or float32, got {src.dtype}")
    a = L.ResampleArgs()
    a.src_dtype = L.TAV_I16 if src.dtype == torch.int16 else L.TAV_F32
    if layout == "L":
        a.C, a.L, a.sC, a.sL = 1, src.shape[0], 0, src.stride(0)
    elif layout == "CL":
        (a.C, a.L), (a.sC, a.sL) = src.shape, src.stride()
    else:
        (a.L, a.C), (a.sL, a.sC) = src.shape, src.stride()
    a.o, a.n, a.width, a.ntap, a.first_max = table.o, table.n, table.width, table.ntap, table.first_max
    L_out = (a.n * a.L + a.o - 1) // a.o
    a.T_row = L_out if T_row is None else int(T_row)
    return a


def audio_resample(src, table, out=None, mask=None, layout=None):
    """tav_audio_resample: src (device, int16 or f32; [L], [C, L] or [L, C], any strides) through `table` (audio_resample_table) -> out, a 1-D
    f32 row of at least L_out elements with unit stride -- a row of the batch tensor or, with out=None, a new tensor of L_out.  The row is
    written in full: the samples, then 0.0; so is `mask` (same length): 1.0 for the samples, then 0.0.  One launch."""
    if not src.is_cuda:
        raise ValueError("audio_resample runs on the GPU only (libtavhip has no host form): move the PCM to the device, or use "
                         "models.tav.speech_features_device, which ships it once")
    a = resample_args(src, table, None if out is None else out.numel(), layout)
    if a.C < 1 or a.L < 1:
        raise ValueError(f"audio_resample: empty waveform {tuple(src.shape)}")
    if a.T_row < resampled_length(a.L, table.sr, table.target):
        raise ValueError(f"audio_resample: out holds {a.T_row} elements, the resampled waveform has {resampled_length(a.L, table.sr, table.target)}")
    if out is None:
        out = torch.empty(a.T_row, dtype=torch.float32, device=src.device)
    for name, t in (("out", out), ("mask", mask)):
        if t is not None and (t.dim() != 1 or t.numel() != a.T_row or t.dtype != torch.float32 or (t.numel() > 1 and t.stride(0) != 1) or
                              t.device != src.device):
            raise ValueError(f"audio_resample: {name} must be a 1-D float32 row of {a.T_row} elements with unit stride on {src.device}, "
                             f"got {tuple(t.shape)} {t.dtype} on {t.device}")
    if table.table.device != src.device:
        raise ValueError(f"audio_resample: the table lives on {table.table.device}, the PCM on {src.device}")
    if src.storage_offset() + (a.C - 1) * a.sC + (a.L - 1) * a.sL >= src.untyped_storage().nbytes() // src.element_size():
        raise ValueError("audio_resample: the sizes and strides reach past the source tensor's storage")
    check(lib().tav_audio_resample(ptr(src), ptr(table.table), ptr(table.first), ptr(out), ptr(mask), C.byref(a), stream()), "audio_resample")
    return out


def mean_pool_fwd(x, B, S, *, seq_lens=None):
    """y[b] = mean over the S rows of batch entry b, or over its first seq_lens[b] (int32 [B] on the device; tav_mean_pool_fwd_len)."""
    W = x.shape[-1]
    y = torch.empty(B, W, dtype=torch.float32, device=x.device)
    if seq_lens is None:
        check(lib().tav_mean_pool_fwd(ptr(x), ptr(y), B, S, W, stream()), "mean_pool_fwd")
    else:
        check(lib().tav_mean_pool_fwd_len(ptr(x), ptr(y), ptr(_seq_lens(seq_lens, B, x.device)), B, S, W, stream()), "mean_pool_fwd_len")
    return y


def mean_pool_bwd(dy, B, S, *, want_f32=True, lp_dtype=None, seq_lens=None):
    W = dy.shape[-1]
    dx = torch.empty(B * S, W, dtype=torch.float32, device=dy.device) if want_f32 else None
    dxlp = torch.empty(B * S, W, dtype=lp_dtype, device=dy.device) if lp_dtype is not None else None
    lp = dt(lp_dtype) if lp_dtype is not None else 0
    if seq_lens is None:
        check(lib().tav_mean_pool_bwd(ptr(dy), ptr(dx), ptr(dxlp), lp, B, S, W, stream()), "mean_pool_bwd")
    else:
        check(lib().tav_mean_pool_bwd_len(ptr(dy), ptr(dx), ptr(dxlp), lp, ptr(_seq_lens(seq_lens, B, dy.device)), B, S, W, stream()),
              "mean_pool_bwd_len")
    return dx, dxlp


def head_fwd(x, W, b):
    B, K = x.shape
    N = W.shape[0]
    y = torch.empty(B, N, dtype=torch.float32, device=x.device)
    check(lib().tav_head_fwd(ptr(x), ptr(W), ptr(b), ptr(y), B, K, N, stream()), "head_fwd")
    return y


def head_bwd(x, W, dy, need_dx=True, need_db=True):
    B, K = x.shape
    N = W.shape[0]
    dx = torch.empty(B, K, dtype=torch.float32, device=x.device) if need_dx else None
    dW = torch.empty(N, K, dtype=torch.float32, device=x.device)
    db = torch.empty(N, dtype=torch.float32, device=x.device) if need_db else None
    check(lib().tav_head_bwd(ptr(x), ptr(W), ptr(dy), ptr(dx), ptr(dW), ptr(db), B, K, N, 0, stream()), "head_bwd")
    return dx, dW, db


def tanh_fwd(x):
    y = torch.empty_like(x)
    check(lib().tav_tanh_fwd(ptr(x), ptr(y), x.numel(), stream()), "tanh_fwd")
    return y


def tanh_bwd(y, dy):
    dx = torch.empty_like(y)
    check(lib().tav_tanh_bwd(ptr(y), ptr(dy), ptr(dx), y.numel(), stream()), "tanh_bwd")
    return dx


def cross_entropy(logits, target, class_weight=None, grad_scale=1.0, want_grad=True):
    B, Cn = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlog = torch.empty_like(logits) if want_grad else None
    check(lib().tav_cross_entropy(ptr(logits), ptr(target), ptr(class_weight), ptr(loss), ptr(dlog), B, Cn, grad_scale, stream()), "cross_entropy")
    return loss, dlog


SOFT_F_MODES = {"FBeta": L.SOFT_F_FBETA, "Precision": L.SOFT_F_PRECISION}
_DEBUG_CHECKS = os.environ.get("TAV_DEBUG_CHECKS", "0") == "1"      # host-synchronising input checks on the sync-free paths


def soft_f_loss(logits, target, weight, beta, mode, eps=1e-7, grad_scale=1.0, want_grad=True, want_loss=True, stats=None):
    """One launch of tav_soft_f_loss on the current stream -> (loss [1], dlogits [B, C]); either is None when not wanted.  logits f32
    [B, C] with unit column stride (any row pitch >= C), target int64 [B], weight f32 [C] or None, mode "FBeta" / "Precision"; stats, if
    given, is a contiguous f32 [3, C] tensor that receives tp, fp, fn.  A target outside [0, C) belongs to no class (its row counts as a
    false positive of every class); with TAV_DEBUG_CHECKS=1 it raises instead, as F.one_hot would -- that check reads the targets back."""
    if mode not in SOFT_F_MODES:
        raise ValueError(f"soft_f_loss: mode must be one of {sorted(SOFT_F_MODES)}, got {mode!r}")
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1 or target.dtype != torch.int64 or not target.is_contiguous():
        raise ValueError(f"soft_f_loss: logits must be f32 [B, C] with unit column stride and target contiguous int64, got {logits.dtype} "
                         f"{tuple(logits.shape)} strides {tuple(logits.stride())}, {target.dtype}")
    B, Cn = logits.shape
    if target.numel() != B or (weight is not None and (weight.dtype != torch.float32 or weight.numel() != Cn or not weight.is_contiguous())):
        raise ValueError(f"soft_f_loss: {B} rows of {Cn} classes need {B} targets and a contiguous f32 weight of {Cn} elements")
    if stats is not None and (stats.dtype != torch.float32 or stats.numel() != 3 * Cn or not stats.is_contiguous()):
        raise ValueError(f"soft_f_loss: stats must be a contiguous f32 tensor of 3 x {Cn} elements")
    if _DEBUG_CHECKS and bool(((target < 0) | (target >= Cn)).any()):
        raise ValueError(f"soft_f_loss: a target lies outside [0, {Cn})")
    loss = torch.empty(1, dtype=torch.float32, device=logits.device) if want_loss else None
    dlog = torch.empty(B, Cn, dtype=torch.float32, device=logits.device) if want_grad else None
    a = L.SoftFArgs(ptr(logits), ptr(target), ptr(weight), ptr(loss), ptr(dlog), ptr(stats), B, Cn, logits.stride(0) if B > 1 else Cn,
                    float(beta), float(eps), float(grad_scale), SOFT_F_MODES[mode])
    check(lib().tav_soft_f_loss(C.byref(a), stream()), "soft_f_loss")
    return loss, dlog


LOOP_ACC_WORDS = 8                               # tav_loop_acc as int64 words
_ACC_UNSET = -(1 << 32)                          # word 5 = (status = 0, first_bad_step = -1), little endian


def _stats_arg(name, t, dtype, numel=None):
    if t is None:
        return None
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"step_stats: {name} must be a tensor on the GPU (the kernel has no host form)")
    if t.dtype != dtype or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise ValueError(f"step_stats: {name} must be contiguous {dtype}" + (f" with {numel} element(s)" if numel is not None else "")
                         + f", got {t.dtype} {tuple(t.shape)}")
    return t


def step_stats(logits=None, preds=None, target=None, cm=None, loss=None, status=None, acc=None, num_classes=None):
    """One launch of tav_step_stats on the current stream; nothing is read back.  Exactly one of logits (f32 [B, C]) / preds (int64 [B]);
    target int64 [B].  cm (int64, C * C elements) gets cm[target, pred] += 1 for the rows inside [0, C); acc (loop_acc_new) gets the loss
    scalar, the status word, the row and out-of-range counts.  The number of classes comes from logits, else from cm, else num_classes."""
    if target is None:
        raise ValueError("step_stats: target is required")
    _stats_arg("target", target, torch.int64)
    B = target.numel()
    if logits is not None:
        _stats_arg("logits", logits, torch.float32)
        if logits.dim() != 2 or logits.shape[0] != B:
            raise ValueError(f"step_stats: logits {tuple(logits.shape)} do not match {B} targets")
        Cn = logits.shape[1]
    else:
        Cn = num_classes if num_classes is not None else (int(round(cm.numel() ** 0.5)) if cm is not None else 0)
    if preds is not None:
        _stats_arg("preds", preds, torch.int64, B)
    _stats_arg("cm", cm, torch.int64, Cn * Cn)
    _stats_arg("loss", loss, torch.float32, 1)
    _stats_arg("status", status, torch.int32, 1)
    _stats_arg("acc", acc, torch.int64, LOOP_ACC_WORDS)
    check(lib().tav_step_stats(ptr(logits), ptr(preds), ptr(target), ptr(cm), ptr(loss), ptr(status), ptr(acc), B, Cn, stream()), "step_stats")


def loop_acc_new(device):
    """A zeroed tav_loop_acc (first_bad_step = -1) on `device`, as 8 int64 words."""
    acc = torch.zeros(LOOP_ACC_WORDS, dtype=torch.int64, device=device)
    acc[5:6].fill_(_ACC_UNSET)
    return acc


def loop_acc_reset(acc):
    """Back to loop_acc_new's state: two fills on the current stream, no host read."""
    acc.zero_()
    acc[5:6].fill_(_ACC_UNSET)


def loop_acc_read(acc):
    """-> dict of the accumulator's fields.  The single device-to-host copy of the sync-free loop, and the only place that synchronises."""
    words = acc.cpu().numpy()
    i32 = words.view("int32")
    return dict(loss_sum=float(words.view("float64")[0]), steps=int(words[1]), rows=int(words[2]), nonfinite=int(words[3]), bad_rows=int(words[4]),
                status=int(i32[10]), first_bad_step=int(i32[11]))


def dropout_fwd(x, p, seed, offset):
    """seed: an int (passed by value), or a one-word int64 device tensor that the kernel reads when it runs (runtime.dropout_seeds under a
    hipGraph capture: the host rewrites the word before every replay)."""
    y = torch.empty_like(x)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if isinstance(seed, torch.Tensor):
        if not seed.is_cuda or seed.dtype != torch.int64 or seed.numel() != 1:
            raise ValueError(f"dropout_fwd: a device seed is one int64 word on the GPU, got {seed.dtype} x {seed.numel()} on {seed.device}")
        check(lib().tav_dropout_fwd_dev(ptr(x), ptr(y), ptr(mask), x.numel(), p, ptr(seed), offset, stream()), "dropout_fwd_dev")
    else:
        check(lib().tav_dropout_fwd(ptr(x), ptr(y), ptr(mask), x.numel(), p, seed, offset, stream()), "dropout_fwd")
    return y, mask


def dropout_bwd(dy, mask, p):
    dx = torch.empty_like(dy)
    check(lib().tav_dropout_bwd(ptr(dy), ptr(mask), ptr(dx), dy.numel(), p, stream()), "dropout_bwd")
    return dx


# ---------------------------------------------------------------------------------------------- SpecAugment
SPECAUG_TAG_TIME = 0x5350010000000000          # include/tavhip.h TAV_SPECAUG_TAG_*
SPECAUG_TAG_FEATURE = 0x5350030000000000


def _mask_bytes(m, shape, what):
    """A bool / uint8 mask as the uint8 tensor the kernels read (a bool tensor is one byte per element: a view, no copy)."""
    if m is None:
        return None
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    if m.dtype != torch.uint8 or m.numel() != shape[0] * shape[1]:
        raise ValueError(f"{what}: expected a bool / uint8 mask of {shape[0]} x {shape[1]} elements, got {m.dtype} {tuple(m.shape)}")
    return m.contiguous()


def specaug_draw(valid, B, L, prob, length, min_masks, seed, tag, *, device=None, want_nspans=False):
    """uint8 [B, L] span mask (tav_specaug_draw).  valid: bool / uint8 [B, L] or None; seed: an int (by value) or a one-word int64 device
    tensor read when the kernel runs (runtime.dropout_seeds under a capture), as in dropout_fwd."""
    valid = _mask_bytes(valid, (B, L), "specaug_draw")
    dev = valid.device if valid is not None else (seed.device if isinstance(seed, torch.Tensor) else device)
    mask = torch.empty(B, L, dtype=torch.uint8, device=dev)
    nspans = torch.empty(B, dtype=torch.int32, device=dev) if want_nspans else None
    if isinstance(seed, torch.Tensor):
        if not seed.is_cuda or seed.dtype != torch.int64 or seed.numel() != 1:
            raise ValueError(f"specaug_draw: a device seed is one int64 word on the GPU, got {seed.dtype} x {seed.numel()} on {seed.device}")
        check(lib().tav_specaug_draw_dev(ptr(valid), ptr(mask), ptr(nspans), B, L, prob, length, min_masks, ptr(seed), tag, stream()), "specaug_draw_dev")
    else:
        check(lib().tav_specaug_draw(ptr(valid), ptr(mask), ptr(nspans), B, L, prob, length, min_masks, seed, tag, stream()), "specaug_draw")
    return (mask, nspans) if want_nspans else mask


def specaug_fwd(x, tmask, fmask, embed, B, T):
    """y = fmask ? 0 : (tmask ? embed : x) for x f32 [B*T, H]; tmask [B, T] / fmask [B, H] bool or uint8, either may be None."""
    H = x.shape[-1]
    tmask, fmask = _mask_bytes(tmask, (B, T), "specaug_fwd"), _mask_bytes(fmask, (B, H), "specaug_fwd")
    y = torch.empty_like(x)
    check(lib().tav_specaug_fwd(ptr(x), ptr(tmask), ptr(fmask), ptr(embed), ptr(y), B, T, H, stream()), "specaug_fwd")
    return y


def specaug_bwd(dy, tmask, fmask, B, T, want_dembed=True):
    """-> (dx, dembed or None): dx = (tmask | fmask) ? 0 : dy, dembed = column sums of the unmasked channels of dy over the time-masked rows."""
    H = dy.shape[-1]
    tmask, fmask = _mask_bytes(tmask, (B, T), "specaug_bwd"), _mask_bytes(fmask, (B, H), "specaug_bwd")
    dx = torch.empty_like(dy)
    dembed = part = None
    nbytes = 0
    if want_dembed:
        dembed = torch.empty(H, dtype=torch.float32, device=dy.device)
        nbytes = lib().tav_specaug_bwd_ws_bytes(B * T, H)
        part = workspace("specaug_part", nbytes // 4, dy.device)
    check(lib().tav_specaug_bwd(ptr(dy), ptr(tmask), ptr(fmask), ptr(dx), ptr(dembed), ptr(part), nbytes, B, T, H, stream()), "specaug_bwd")
    return dx, dembed


# ---------------------------------------------------------------------------------------------- audio front-end
def conv0_fwd(wave, w, bias, T_out, stride, dtype):
    B, T_in = wave.shape
    Cc, K = w.shape[0], w.shape[-1]
    y = torch.empty(B, T_out, Cc, dtype=dtype, device=wave.device)
    check(lib().tav_conv0_fwd(ptr(wave), ptr(w), ptr(bias), ptr(y), dt(dtype), B, T_in, T_out, Cc, K, stride, stream()), "conv0_fwd")
    return y


def conv0_bwd_w(wave, dy, K, stride, want_bias):
    B, T_in = wave.shape
    _, T_out, Cc = dy.shape
    part = workspace("conv0_part", lib().tav_conv0_bwd_partials(B, T_out, Cc, K), wave.device)
    dw = torch.empty(Cc, 1, K, dtype=torch.float32, device=wave.device)
    db = torch.empty(Cc, dtype=torch.float32, device=wave.device) if want_bias else None
    check(lib().tav_conv0_bwd_w(ptr(wave), ptr(dy), dt(dy), ptr(dw), ptr(db), ptr(part), B, T_in, T_out, Cc, K, stride, 0, stream()), "conv0_bwd_w")
    return dw, db


def gn_gelu_fwd(x, gamma, beta, eps):
    B, T, Cc = x.shape
    y = torch.empty_like(x)
    stats = torch.empty(B, Cc, 2, dtype=torch.float32, device=x.device)
    wsb = workspace("gn_ws", lib().tav_gn_workspace_floats(B, Cc), x.device)
    check(lib().tav_gn_gelu_fwd(ptr(x), ptr(y), dt(x), ptr(gamma), ptr(beta), ptr(stats), ptr(wsb), B, T, Cc, eps, stream()), "gn_gelu_fwd")
    return y, stats


def gn_gelu_bwd(x, dy, gamma, beta, stats):
    B, T, Cc = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(Cc, dtype=torch.float32, device=x.device)
    db = torch.empty(Cc, dtype=torch.float32, device=x.device)
    wsb = workspace("gn_ws", lib().tav_gn_workspace_floats(B, Cc), x.device)
    check(lib().tav_gn_gelu_bwd(ptr(x), ptr(dy), ptr(dx), dt(x), ptr(gamma), ptr(beta), ptr(stats), ptr(wsb), ptr(dg), ptr(db), B, T, Cc, 0, stream()), "gn_gelu_bwd")
    return dx, dg, db


def gelu_bwd(x, dy):
    dx = torch.empty_like(x)
    check(lib().tav_gelu_bwd(ptr(x), ptr(dy), ptr(dx), dt(x), x.numel(), stream()), "gelu_bwd")
    return dx


def col2im_1d(dcol, B, T_in, T_out, Cc, K, stride, pre_act=None):
    dx = torch.empty(B, T_in, Cc, dtype=dcol.dtype, device=dcol.device)
    check(lib().tav_col2im_1d(ptr(dcol), ptr(dx), ptr(pre_act), dt(dcol), B, T_in, T_out, Cc, K, stride, stream()), "col2im_1d")
    return dx


def group_pad(x, B, T, H, G, pad_l, pad_r, dtype):
    xg = torch.empty(B, G, pad_l + T + pad_r, H // G, dtype=dtype, device=x.device)
    check(lib().tav_group_pad(ptr(x), dt(x), ptr(xg), dt(dtype), B, T, H, G, pad_l, pad_r, stream()), "group_pad")
    return xg


def weight_norm_fwd(v, g, dtype):
    H, Cg, K = v.shape
    norms = torch.empty(K, dtype=torch.float32, device=v.device)
    part = workspace("wn_part", lib().tav_weight_norm_partials(H, Cg) * K, v.device)
    G = H // Cg
    w = torch.empty(G, Cg, K * Cg, dtype=dtype, device=v.device)
    wf = torch.empty(G, Cg, K * Cg, dtype=dtype, device=v.device)
    check(lib().tav_weight_norm_fwd(ptr(v), ptr(g), ptr(norms), ptr(part), ptr(w), ptr(wf), dt(dtype), H, Cg, K, stream()), "weight_norm_fwd")
    return w, wf, norms


def weight_norm_bwd(v, g, norms, dw_gemm):
    H, Cg, K = v.shape
    wsb = workspace("wn_bwd", H * Cg * K + lib().tav_weight_norm_partials(H, Cg) * K + K, v.device)
    dv = torch.empty_like(v)
    dg = torch.empty(K, dtype=torch.float32, device=v.device)
    check(lib().tav_weight_norm_bwd(ptr(v), ptr(g), ptr(norms), ptr(dw_gemm), ptr(wsb), ptr(dv), ptr(dg), H, Cg, K, 0, stream()), "weight_norm_bwd")
    return dv, dg


# ---------------------------------------------------------------------------------------------- forced alignment (include/tavhip_align.h)
CtcAlignment = collections.namedtuple("CtcAlignment", "path_token path_prob seg seg_score span trellis")


def ctc_align_plan(T, N, V):
    """tav_ctc_align_plan as a dict: block, tokens_per_thread, frames_per_stage, bits_frames, lds_bytes, ws_bytes_per_row."""
    p = L.AlignPlan()
    check(lib().tav_ctc_align_plan(int(T), int(N), int(V), C.byref(p)), "ctc_align_plan")
    return {name: int(getattr(p, name)) for name, _ in L.AlignPlan._fields_}


def _rows_2d(x, what):
    """(rows, row stride) of a tensor whose last dimension is dense and whose leading dimensions lie at one pitch."""
    if x.dim() < 2 or x.stride(-1) != 1 or x.dtype != torch.float32:
        raise ValueError(f"{what}: a float32 tensor [..., W] with a dense last dimension is needed, got {tuple(x.shape)} {x.dtype} strides {x.stride()}")
    ld, rows = x.stride(-2), 1
    for d in range(x.dim() - 2, -1, -1):
        if x.shape[d] != 1 and x.stride(d) != ld * rows:
            raise ValueError(f"{what}: the rows of {tuple(x.shape)} (strides {x.stride()}) do not lie at one pitch")
        rows *= x.shape[d]
    return rows, ld


def ctc_log_softmax(logits, V=None, out=None):
    """tav_ctc_log_softmax: the row log-softmax over the first V columns of logits [..., W] (V = W by default).  Columns [V, W) are neither
    read nor written (a new `out` keeps whatever its allocation held there)."""
    W = logits.shape[-1]
    V = W if V is None else int(V)
    R, ld_in = _rows_2d(logits, "ctc_log_softmax")
    if out is None:
        out = torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
    if out.shape != logits.shape or out.device != logits.device:
        raise ValueError(f"ctc_log_softmax: out {tuple(out.shape)} on {out.device} for logits {tuple(logits.shape)} on {logits.device}")
    _, ld_out = _rows_2d(out, "ctc_log_softmax (out)")
    if not logits.is_cuda:
        raise ValueError("ctc_log_softmax runs on the GPU only (libtavhip has no host form)")
    check(lib().tav_ctc_log_softmax(ptr(logits), ptr(out), R, V, ld_in, ld_out, stream()), "ctc_log_softmax")
    return out


def ctc_align(emission, tokens, n_frames, n_tokens, *, V=None, blank_id=0, want_trellis=False, out=None, _enqueue=None):
    """tav_ctc_align, one launch for the batch: emission f32 [B, Tmax, W] log-probabilities (V valid columns, V = W by default), tokens int32
    [B, Nmax], n_frames / n_tokens int32 [B] (all on the device) -> CtcAlignment(path_token [B, Tmax] i32, path_prob [B, Tmax] f32,
    seg [B, Nmax, 2] i32, seg_score [B, Nmax] f32, span [B, 4] i32, trellis [B, Tmax + 1, Nmax + 1] f32 or None); include/tavhip_align.h
    says what they hold.  `out`: a CtcAlignment of contiguous tensors to fill instead of new ones.  Nothing is read back: a row that
    failed to align says so in span[:, 3] bit 0.  `_enqueue`: a list that receives the argument struct and everything it points to."""
    if not emission.is_cuda:
        raise ValueError("ctc_align runs on the GPU only (libtavhip has no host form)")
    if emission.dim() != 3 or tokens.dim() != 2 or tokens.dtype != torch.int32 or n_frames.dtype != torch.int32 or n_tokens.dtype != torch.int32:
        raise ValueError("ctc_align: emission [B, Tmax, W] float32, tokens [B, Nmax] int32, n_frames and n_tokens [B] int32")
    B, Tmax, W = emission.shape
    Nmax = tokens.shape[1]
    V = W if V is None else int(V)
    rows, ld = _rows_2d(emission, "ctc_align")
    if tokens.shape[0] != B or n_frames.numel() != B or n_tokens.numel() != B or not (tokens.is_contiguous() and n_frames.is_contiguous() and n_tokens.is_contiguous()):
        raise ValueError("ctc_align: tokens, n_frames and n_tokens must be contiguous and have one row per utterance")
    dev = emission.device
    if out is None:
        out = CtcAlignment(torch.empty(B, Tmax, dtype=torch.int32, device=dev), torch.empty(B, Tmax, dtype=torch.float32, device=dev),
                           torch.empty(B, Nmax, 2, dtype=torch.int32, device=dev), torch.empty(B, Nmax, dtype=torch.float32, device=dev),
                           torch.empty(B, 4, dtype=torch.int32, device=dev),
                           torch.empty(B, Tmax + 1, Nmax + 1, dtype=torch.float32, device=dev) if want_trellis else None)
    shapes = ((B, Tmax), (B, Tmax), (B, Nmax, 2), (B, Nmax), (B, 4), (B, Tmax + 1, Nmax + 1))
    for name, t, shape in zip(CtcAlignment._fields, out, shapes):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"ctc_align: out.{name} must be a contiguous {shape} tensor on {dev}, got {tuple(t.shape)} strides {t.stride()}")
    nbytes = lib().tav_ctc_align_ws_bytes(B, Tmax, Nmax, V)
    if nbytes < 0:
        check(int(nbytes), "ctc_align")
    ws = workspace("ctc_align", (nbytes + 3) // 4, dev) if nbytes else None
    a = L.CtcAlignArgs()
    a.emission, a.tokens, a.n_frames, a.n_tokens = ptr(emission), ptr(tokens), ptr(n_frames), ptr(n_tokens)
    a.trellis, a.path_token, a.path_prob, a.seg, a.seg_score, a.span = ptr(out.trellis), ptr(out.path_token), ptr(out.path_prob), ptr(out.seg), ptr(out.seg_score), ptr(out.span)
    a.workspace, a.workspace_bytes = ptr(ws), (ws.numel() * 4 if ws is not None else 0)
    a.B, a.Tmax, a.Nmax, a.V, a.ld, a.blank_id = B, Tmax, Nmax, V, ld, int(blank_id)
    if _enqueue is not None:                   # (tools/gpu_align_speed.py times the entry point without this wrapper's host work)
        _enqueue.append((a, ws, emission, tokens, n_frames, n_tokens, out))
    check(lib().tav_ctc_align(C.byref(a), stream()), "ctc_align")
    return out


# ---------------------------------------------------------------------------------------------- LSTM recurrence, log-sigmoid (include/tavhip_rnn.h)
LstmSaved = collections.namedtuple("LstmSaved", "y workspace B T H Hp dtype")


def lstm_plan(B, T, H, dtype):
    """tav_lstm_get_plan as a dict: block, rows_per_wg, Hp, tiles_per_wave, lds_bytes, ws_gates_off, ws_cell_off, ws_bytes."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"lstm: the recurrence runs in float32 or bfloat16 operands, got {dtype}")
    p = L.LstmPlan()
    check(lib().tav_lstm_get_plan(int(B), int(T), int(H), dt(dtype), C.byref(p)), "lstm_plan")
    return {name: int(getattr(p, name)) for name, _ in L.LstmPlan._fields_}


def _bt_strides(x, B, T, W, what, time_major):
    """(stride_b, stride_t) in elements of a [B, T, W] (or, time-major, [T, B, W]) tensor with a dense last dimension."""
    want = (T, B, W) if time_major else (B, T, W)
    if x.dim() != 3 or tuple(x.shape) != want or x.stride(-1) != 1:
        raise ValueError(f"{what}: a {want} tensor with a dense last dimension is needed, got {tuple(x.shape)} strides {x.stride()}")
    return (x.stride(1), x.stride(0)) if time_major else (x.stride(0), x.stride(1))


def _state(x, B, Hp, what):
    if x is not None and (tuple(x.shape) != (B, Hp) or x.dtype != torch.float32 or not x.is_contiguous()):
        raise ValueError(f"{what}: a contiguous float32 [{B}, {Hp}] tensor is needed, got {tuple(x.shape)} {x.dtype}")
    return x


def lstm_fwd(xproj, w_hh, b_hh=None, h0=None, c0=None, *, H=None, time_major=False):
    """tav_lstm_fwd, one launch: xproj [B, T, 4 Hp] (time_major: [T, B, 4 Hp]) and w_hh [4 Hp, Hp] in one operand dtype (float32 / bfloat16),
    gate blocks padded to Hp = ceil(H / 64) 64 with zero pads; b_hh f32 [4 Hp], h0 / c0 f32 [B, Hp], all optional.  -> LstmSaved: y
    [T + 1, B, Hp] (slot 0 = h0, slot t + 1 = h_t) and the workspace (f32 words) the backward reads; lstm_cells() / lstm_gates() view it."""
    if not xproj.is_cuda:
        raise ValueError("lstm_fwd runs on the GPU only (libtavhip has no host form)")
    Hp = w_hh.shape[1]
    H = Hp if H is None else int(H)
    B, T = (xproj.shape[1], xproj.shape[0]) if time_major else (xproj.shape[0], xproj.shape[1])
    plan = lstm_plan(B, T, H, xproj.dtype)
    if plan["Hp"] != Hp or tuple(w_hh.shape) != (4 * Hp, Hp) or w_hh.dtype != xproj.dtype or not w_hh.is_contiguous():
        raise ValueError(f"lstm_fwd: w_hh must be a contiguous {xproj.dtype} [{4 * plan['Hp']}, {plan['Hp']}] tensor for H = {H}, got {tuple(w_hh.shape)} {w_hh.dtype}")
    sb, st = _bt_strides(xproj, B, T, 4 * Hp, "lstm_fwd: xproj", time_major)
    if b_hh is not None and (b_hh.dtype != torch.float32 or b_hh.numel() != 4 * Hp or not b_hh.is_contiguous()):
        raise ValueError(f"lstm_fwd: b_hh must be a contiguous float32 [{4 * Hp}] tensor")
    y = torch.empty(T + 1, B, Hp, dtype=xproj.dtype, device=xproj.device)
    ws = torch.empty(plan["ws_bytes"] // 4, dtype=torch.float32, device=xproj.device)
    a = L.LstmFwdArgs()
    a.xproj, a.w_hh, a.b_hh, a.h0, a.c0 = ptr(xproj), ptr(w_hh), ptr(b_hh), ptr(_state(h0, B, Hp, "lstm_fwd: h0")), ptr(_state(c0, B, Hp, "lstm_fwd: c0"))
    a.y, a.workspace, a.workspace_bytes = ptr(y), ptr(ws), ws.numel() * 4
    a.B, a.T, a.H, a.xp_stride_b, a.xp_stride_t, a.dtype = B, T, H, sb, st, dt(xproj)
    check(lib().tav_lstm_fwd(C.byref(a), stream()), "lstm_fwd")
    return LstmSaved(y, ws, B, T, H, Hp, xproj.dtype)


def lstm_gates(s):
    """The saved gate activations of a forward, f32 [T, B, 4, Hp] (i, f, g, o): a view of the workspace."""
    p = lstm_plan(s.B, s.T, s.H, s.dtype)
    return s.workspace[p["ws_gates_off"] // 4:p["ws_gates_off"] // 4 + s.T * s.B * 4 * s.Hp].view(s.T, s.B, 4, s.Hp)


def lstm_cells(s):
    """The saved cell states of a forward, f32 [T + 1, B, Hp] (slot 0 = c0, slot T = c_T): a view of the workspace."""
    p = lstm_plan(s.B, s.T, s.H, s.dtype)
    return s.workspace[p["ws_cell_off"] // 4:p["ws_cell_off"] // 4 + (s.T + 1) * s.B * s.Hp].view(s.T + 1, s.B, s.Hp)


def lstm_bwd(saved, dy, w_hh_t, dh_T=None, dc_T=None, *, time_major=False, dz_time_major=True, want_state_grads=True, want_trace=False):
    """tav_lstm_bwd, one launch: dy [B, T, Hp] (time_major: [T, B, Hp]) in the forward's dtype, w_hh_t [Hp, 4 Hp] the transposed operand.
    -> (dZ [T, B, 4 Hp] (or [B, T, 4 Hp]) in that dtype, dh0, dc0 f32 [B, Hp] or None, dc_trace f32 [T, B, Hp] or None)."""
    B, T, H, Hp = saved.B, saved.T, saved.H, saved.Hp
    if tuple(w_hh_t.shape) != (Hp, 4 * Hp) or w_hh_t.dtype != saved.dtype or not w_hh_t.is_contiguous() or dy.dtype != saved.dtype:
        raise ValueError(f"lstm_bwd: w_hh_t must be a contiguous {saved.dtype} [{Hp}, {4 * Hp}] tensor and dy of that dtype, got {tuple(w_hh_t.shape)} {w_hh_t.dtype}, {dy.dtype}")
    ysb, yst = _bt_strides(dy, B, T, Hp, "lstm_bwd: dy", time_major)
    dev = dy.device
    dz = torch.empty((T, B, 4 * Hp) if dz_time_major else (B, T, 4 * Hp), dtype=saved.dtype, device=dev)
    zsb, zst = _bt_strides(dz, B, T, 4 * Hp, "lstm_bwd: dz", dz_time_major)
    dh0 = torch.empty(B, Hp, dtype=torch.float32, device=dev) if want_state_grads else None
    dc0 = torch.empty(B, Hp, dtype=torch.float32, device=dev) if want_state_grads else None
    trace = torch.empty(T, B, Hp, dtype=torch.float32, device=dev) if want_trace else None
    a = L.LstmBwdArgs()
    a.dy, a.dh_T, a.dc_T, a.w_hh_t = ptr(dy), ptr(_state(dh_T, B, Hp, "lstm_bwd: dh_T")), ptr(_state(dc_T, B, Hp, "lstm_bwd: dc_T")), ptr(w_hh_t)
    a.workspace, a.workspace_bytes, a.dz, a.dh0, a.dc0, a.dc_trace = ptr(saved.workspace), saved.workspace.numel() * 4, ptr(dz), ptr(dh0), ptr(dc0), ptr(trace)
    a.B, a.T, a.H, a.dy_stride_b, a.dy_stride_t, a.dz_stride_b, a.dz_stride_t, a.dtype = B, T, H, ysb, yst, zsb, zst, dt(saved.dtype)
    check(lib().tav_lstm_bwd(C.byref(a), stream()), "lstm_bwd")
    return dz, dh0, dc0, trace


def logsigmoid_fwd(x):
    if x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"logsigmoid_fwd: a contiguous float32 tensor on the GPU is needed, got {x.dtype} on {x.device}")
    y = torch.empty_like(x)
    check(lib().tav_logsigmoid_fwd(ptr(x), ptr(y), x.numel(), stream()), "logsigmoid_fwd")
    return y


def logsigmoid_bwd(x, dy):
    if x.dtype != torch.float32 or dy.dtype != torch.float32 or not x.is_contiguous() or not dy.is_contiguous() or dy.shape != x.shape or not x.is_cuda:
        raise ValueError("logsigmoid_bwd: x and dy must be contiguous float32 tensors of one shape on the GPU")
    dx = torch.empty_like(x)
    check(lib().tav_logsigmoid_bwd(ptr(x), ptr(dy), ptr(dx), x.numel(), stream()), "logsigmoid_bwd")
    return dx


# ---------------------------------------------------------------------------------------------- dense 3-D convolution, flatten + Linear, sigmoid (include/tavhip_conv.h)
def _conv_dtype(dtype, what):
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{what}: the convolution runs in float32 or bfloat16 operands, got {dtype}")
    return dt(dtype)


def conv3d_plan(B, D, H, W, Cin, Cout, dtype, pad=0):
    """tav_conv3d_get_plan as a dict (every field of tav_conv3d_plan): the padded widths, the patch tw x th, block, LDS bytes, grid (= patches),
    and for pad = 0 the weight gradient's channel block, slab count and slab size."""
    p = L.Conv3dPlan()
    check(lib().tav_conv3d_get_plan(int(B), int(D), int(H), int(W), int(Cin), int(Cout), int(pad), _conv_dtype(dtype, "conv3d_plan"), C.byref(p)), "conv3d_plan")
    return {name: int(getattr(p, name)) for name, _ in L.Conv3dPlan._fields_ if name != "reserved"}


def conv3d_cp(Cn):
    """The padded channel count of the channels-last activations: ceil(C / 16) 16."""
    return (int(Cn) + 15) // 16 * 16


def _cl(x, what, C=None):
    """(B, D, H, W, Cp) of a contiguous channels-last activation on the GPU."""
    if not x.is_cuda or x.dim() != 5 or not x.is_contiguous() or x.shape[4] % 16 or (C is not None and x.shape[4] != conv3d_cp(C)):
        raise ValueError(f"{what}: a contiguous channels-last [B, D, H, W, Cp] GPU tensor with Cp = ceil(C / 16) 16 is needed, got {tuple(x.shape)} on {x.device}")
    return tuple(x.shape)


def conv3d_pack_input(x, dtype):
    """NCDHW float32 [B, C, D, H, W] -> channels-last [B, D, H, W, Cp] in `dtype`, pad channels zero."""
    if not x.is_cuda or x.dim() != 5 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"conv3d_pack_input: a contiguous float32 [B, C, D, H, W] GPU tensor is needed, got {tuple(x.shape)} {x.dtype} on {x.device}")
    B, Cn, D, H, W = x.shape
    out = torch.empty(B, D, H, W, conv3d_cp(Cn), dtype=dtype, device=x.device)
    check(lib().tav_conv3d_pack_input(ptr(x), ptr(out), B, Cn, D, H, W, _conv_dtype(dtype, "conv3d_pack_input"), stream()), "conv3d_pack_input")
    return out


def conv3d_pack_weight(w, dtype, flip_transpose=False):
    """torch's Conv3d weight f32 [Cout, Cin, 3, 3, 3] -> the forward's operand [cout_p, kp(Cin)] or (flip_transpose) the input gradient's
    [cin_p, kp(Cout)], in `dtype`, pads zero."""
    if not w.is_cuda or w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3) or w.dtype != torch.float32 or not w.is_contiguous():
        raise ValueError(f"conv3d_pack_weight: a contiguous float32 [Cout, Cin, 3, 3, 3] GPU tensor is needed, got {tuple(w.shape)} {w.dtype}")
    Cout, Cin = w.shape[:2]
    rows, inner = (Cin, Cout) if flip_transpose else (Cout, Cin)
    kstep = 32 if dtype == torch.bfloat16 else 16
    kp = (27 * conv3d_cp(inner) + kstep - 1) // kstep * kstep
    out = torch.empty(conv3d_cp(rows), kp, dtype=dtype, device=w.device)
    check(lib().tav_conv3d_pack_weight(ptr(w), ptr(out), Cout, Cin, int(bool(flip_transpose)), _conv_dtype(dtype, "conv3d_pack_weight"), stream()), "conv3d_pack_weight")
    return out


def _conv3d_launch(x, w_op, bias, Cin, Cout, pad, gelu, want_g, what):
    B, D, H, W, cin_p = _cl(x, what, Cin)
    plan = conv3d_plan(B, D, H, W, Cin, Cout, x.dtype, pad)
    if tuple(w_op.shape) != (plan["cout_p"], plan["kp"]) or w_op.dtype != x.dtype or not w_op.is_contiguous():
        raise ValueError(f"{what}: the weight operand must be a contiguous {x.dtype} [{plan['cout_p']}, {plan['kp']}] tensor, got {tuple(w_op.shape)} {w_op.dtype}")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != plan["cout_p"] or not bias.is_contiguous()):
        raise ValueError(f"{what}: bias must be a contiguous float32 [{plan['cout_p']}] tensor (pads zero)")
    y = torch.empty(B, plan["od"], plan["oh"], plan["ow"], plan["cout_p"], dtype=x.dtype, device=x.device)
    g = torch.empty_like(y) if (gelu and want_g) else None
    a = L.Conv3dFwdArgs()
    a.x, a.w, a.bias, a.y, a.g = ptr(x), ptr(w_op), ptr(bias), ptr(y), ptr(g)
    a.B, a.D, a.H, a.W, a.Cin, a.Cout, a.pad, a.gelu, a.dtype = B, D, H, W, Cin, Cout, pad, int(bool(gelu)), dt(x)
    check(lib().tav_conv3d_fwd(C.byref(a), stream()), what)
    return y, g


def conv3d_fwd(x, w_op, bias, Cin, Cout, *, gelu=True, want_g=True):
    """tav_conv3d_fwd with pad 0: x channels-last [B, D, H, W, cin_p], w_op from conv3d_pack_weight, bias f32 [cout_p] or None ->
    (y [B, D-2, H-2, W-2, cout_p] = gelu(z) (or z), g = gelu'(z) or None), in x's dtype."""
    return _conv3d_launch(x, w_op, bias, Cin, Cout, 0, gelu, want_g, "conv3d_fwd")


def conv3d_dgrad(dz, w_flip, Cin, Cout):
    """The input gradient of a Cin -> Cout layer: tav_conv3d_fwd with pad 2 on dz [B, D', H', W', cout_p] and the flip_transpose operand
    [cin_p, kp(Cout)] -> dx [B, D'+2, H'+2, W'+2, cin_p]."""
    return _conv3d_launch(dz, w_flip, None, Cout, Cin, 2, False, False, "conv3d_dgrad")[0]


def conv3d_dz(dy, g=None):
    """dz = dy * g (a copy without g), rounded once to the operand dtype: what both conv3d_dgrad and conv3d_wgrad read."""
    if not dy.is_cuda or not dy.is_contiguous() or dy.numel() % 4 or (g is not None and (g.shape != dy.shape or g.dtype != dy.dtype or not g.is_contiguous())):
        raise ValueError("conv3d_dz: dy and g must be contiguous GPU tensors of one shape and dtype")
    dz = torch.empty_like(dy)
    check(lib().tav_conv3d_dz(ptr(dy), ptr(g), ptr(dz), dy.numel(), _conv_dtype(dy.dtype, "conv3d_dz"), stream()), "conv3d_dz")
    return dz


def conv3d_wgrad(x, dz, Cin, Cout, *, nslabs=0, want_bias=True):
    """tav_conv3d_wgrad: x [B, D, H, W, cin_p], dz [B, D-2, H-2, W-2, cout_p] -> (dw f32 [Cout, Cin, 3, 3, 3], db f32 [Cout] or None).
    nslabs = 0: the plan's slab count."""
    B, D, H, W, _ = _cl(x, "conv3d_wgrad: x", Cin)
    if _cl(dz, "conv3d_wgrad: dz", Cout) != (B, D - 2, H - 2, W - 2, conv3d_cp(Cout)) or dz.dtype != x.dtype:
        raise ValueError(f"conv3d_wgrad: dz must be [{B}, {D - 2}, {H - 2}, {W - 2}, {conv3d_cp(Cout)}] in {x.dtype}, got {tuple(dz.shape)} {dz.dtype}")
    code = _conv_dtype(x.dtype, "conv3d_wgrad")
    nbytes = lib().tav_conv3d_wgrad_ws_bytes(B, D, H, W, Cin, Cout, code, int(nslabs))
    if nbytes < 0:
        check(int(nbytes), "conv3d_wgrad_ws_bytes")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    dw = torch.empty(Cout, Cin, 3, 3, 3, dtype=torch.float32, device=x.device)
    db = torch.empty(Cout, dtype=torch.float32, device=x.device) if want_bias else None
    a = L.Conv3dWgradArgs()
    a.x, a.dz, a.workspace, a.workspace_bytes, a.dw, a.db = ptr(x), ptr(dz), ptr(ws), nbytes, ptr(dw), ptr(db)
    a.B, a.D, a.H, a.W, a.Cin, a.Cout, a.nslabs, a.dtype = B, D, H, W, Cin, Cout, int(nslabs), code
    check(lib().tav_conv3d_wgrad(C.byref(a), stream()), "conv3d_wgrad")
    return dw, db


def _flat_args(x, w, Cn, what):
    B, D, H, W, cp = _cl(x, what, Cn)
    S = D * H * W
    if not w.is_cuda or w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] != Cn * S or not w.is_contiguous():
        raise ValueError(f"{what}: the weight must be a contiguous float32 [O, {Cn * S}] GPU tensor (torch's flatten order c S + s), got {tuple(w.shape)} {w.dtype}")
    return B, S, w.shape[0]


def flat_linear_fwd(x, w, bias, Cn, *, nparts=0):
    """out[b, o] = bias[o] + sum_f x[b, f] w[o, f] with x channels-last [B, D, H, W, cp] and w f32 [O, C D H W] in torch's flatten order -> f32 [B, O]."""
    B, S, O = _flat_args(x, w, Cn, "flat_linear_fwd")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != O or not bias.is_contiguous()):
        raise ValueError(f"flat_linear_fwd: bias must be a contiguous float32 [{O}] tensor")
    nbytes = lib().tav_flat_linear_ws_bytes(B, S, O, int(nparts))
    if nbytes < 0:
        check(int(nbytes), "flat_linear_ws_bytes")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    out = torch.empty(B, O, dtype=torch.float32, device=x.device)
    a = L.FlatLinearFwdArgs()
    a.x, a.w, a.bias, a.out, a.workspace, a.workspace_bytes = ptr(x), ptr(w), ptr(bias), ptr(out), ptr(ws), nbytes
    a.B, a.S, a.C, a.O, a.nparts, a.dtype = B, S, Cn, O, int(nparts), _conv_dtype(x.dtype, "flat_linear_fwd")
    check(lib().tav_flat_linear_fwd(C.byref(a), stream()), "flat_linear_fwd")
    return out


def flat_linear_bwd(x, w, dy, Cn, *, need_dx=True, need_db=True):
    """-> (dx like x or None, dw f32 like w, db f32 [O] or None) from dy f32 [B, O], in one pass over x and w."""
    B, S, O = _flat_args(x, w, Cn, "flat_linear_bwd")
    if dy.dtype != torch.float32 or tuple(dy.shape) != (B, O) or not dy.is_contiguous():
        raise ValueError(f"flat_linear_bwd: dy must be a contiguous float32 [{B}, {O}] tensor, got {tuple(dy.shape)} {dy.dtype}")
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w)
    db = torch.empty(O, dtype=torch.float32, device=x.device) if need_db else None
    a = L.FlatLinearBwdArgs()
    a.x, a.w, a.dy, a.dx, a.dw, a.db = ptr(x), ptr(w), ptr(dy), ptr(dx), ptr(dw), ptr(db)
    a.B, a.S, a.C, a.O, a.dtype = B, S, Cn, O, _conv_dtype(x.dtype, "flat_linear_bwd")
    check(lib().tav_flat_linear_bwd(C.byref(a), stream()), "flat_linear_bwd")
    return dx, dw, db


def sigmoid_fwd(x):
    if x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"sigmoid_fwd: a contiguous float32 tensor on the GPU is needed, got {x.dtype} on {x.device}")
    y = torch.empty_like(x)
    check(lib().tav_sigmoid_fwd(ptr(x), ptr(y), x.numel(), stream()), "sigmoid_fwd")
    return y


def sigmoid_bwd(y, dy):
    if y.dtype != torch.float32 or dy.dtype != torch.float32 or not y.is_contiguous() or not dy.is_contiguous() or dy.shape != y.shape or not y.is_cuda:
        raise ValueError("sigmoid_bwd: y and dy must be contiguous float32 tensors of one shape on the GPU")
    dx = torch.empty_like(y)
    check(lib().tav_sigmoid_bwd(ptr(y), ptr(dy), ptr(dx), y.numel(), stream()), "sigmoid_bwd")
    return dx
