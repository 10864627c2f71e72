"""Per-kernel numerical checks of libtavhip against plain PyTorch references of the same op (run on the GPU).

Each check returns (name, max_abs_err, tolerance, ok).  Used by tests/test_kernels_gpu.py (asserts) and by
tools/gpu_kernel_check.py (prints a table without stopping at the first failure).
"""
import contextlib
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import attn_ref as AR
import front_ref as FR
import gemm_ref as GR
import guarded
import nonfinite_ref as NF
import norm_ref as NR
import step_end_ref as SR
import tav_amd.ops as ops

DEV = "cuda"


def _in(t, pitch_extra=0):
    """Input hook: the identity without a guard; inside guarded.active() the tensor moves into a 0xFF-filled buffer (tests/guarded.py), with
    pitch_extra > 0 as a strided view whose rows are pitch_extra elements further apart than they are long."""
    g = guarded.current()
    if g is not None:
        return g.input(t, pitch_extra)
    if not pitch_extra:
        return t
    wide = _blank(tuple(t.shape[:-1]) + (t.shape[-1] + pitch_extra,), t.dtype)
    wide[..., :t.shape[-1]] = t
    return wide[..., :t.shape[-1]]


def _blank(shape, dtype):
    """A tensor whose every byte is 0xFF (NaN / -1), under guard when one is active: for outputs the checks hand to the library themselves."""
    g = guarded.current()
    if g is not None:
        return g.empty(shape, dtype=dtype, device=DEV)
    n = 1
    for s_ in shape:
        n *= s_
    return torch.full((n * dtype.itemsize,), 0xFF, dtype=torch.uint8, device=DEV).view(dtype).view(shape)


def _all_ff(name, *tensors):
    """Result tuple: every byte of these (possibly strided) tensors is still 0xFF -- nothing stored into them."""
    bad = sum(int(t.contiguous().view(torch.uint8).ne(0xFF).sum().item()) for t in tensors if t.numel())
    return (name, float(bad), 0.0, bad == 0)


_REF = [torch.float32]


def _r(t):
    """A tensor in the precision the references are computed in: f32 as the checks were written, fp64 inside ref64()."""
    return t.to(_REF[0])


@contextlib.contextmanager
def ref64():
    """Inside: every check that builds its reference through _r() computes it in fp64 (the edge cases do)."""
    old, _REF[0] = _REF[0], torch.float64
    try:
        yield
    finally:
        _REF[0] = old


def _in64(fn):
    def run():
        with ref64():
            return fn()
    return run


def _rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return _in((torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype))


def _res(name, got, ref, tol):
    got = got.float()
    ref = ref.float()
    err = (got - ref).abs().max().item()
    den = ref.abs().max().item() + 1e-12
    ok = bool(err <= tol * max(den, 1.0)) and bool(torch.isfinite(got).all())
    return (name, err / max(den, 1.0), tol, ok)


def tol_for(dtype):
    return 2e-2 if dtype == torch.bfloat16 else 2e-5


# ------------------------------------------------------------------------------------------------ GEMM
def check_gemm_nt(dtype, M=300, N=256, K=128, bias=True, act=0, resid=True, pre=False, out_f32=False, tile_m=0):
    a = _rnd(M, K, dtype=dtype, seed=1)
    b = _rnd(N, K, dtype=dtype, scale=0.1, seed=2)
    bi = _rnd(N, seed=3) if bias else None
    r = _rnd(M, N, seed=4) if resid else None
    out_dtype = torch.float32 if (out_f32 or dtype == torch.float32) else dtype
    res = ops.gemm_nt(a, b, bias=bi, act=act, resid=r, want_pre=pre, out_dtype=out_dtype, tile_m=tile_m)
    out, p = res if pre else (res, None)
    ref = a.float() @ b.float().t()
    if bias:
        ref = ref + bi
    ref_pre = ref
    if act == 1:
        ref = F.gelu(ref)
    if resid:
        ref = ref + r
    tol = tol_for(dtype if out_dtype != torch.float32 else torch.float32) if dtype == torch.float32 else (1e-2 if out_dtype == torch.bfloat16 else 2e-3)
    rs = [_res(f"gemm_nt[{dtype},M{M},N{N},K{K},b{int(bias)},a{act},r{int(resid)},f32out{int(out_f32)},tm{tile_m}]", out, ref, tol)]
    if pre:
        rs.append(_res("gemm_nt.pre", p, ref_pre, tol))
    return rs


def check_gemm_nt_mixed_schedule(M=46848 + 37, N=768, K=768):
    """The library may cover a launch's rows with whole rounds of 256 x 256 tiles plus 128-wide tiles over the rest (tav_gemm_nt_schedule).
    Every output element sums over K in the same order whatever the tile, so the mixed schedule must reproduce the single-tile launch
    (hint 17) BIT FOR BIT, for each epilogue flavour and every side tensor (bias, residual, second output, gelu' input)."""
    import ctypes as C
    dtype = torch.bfloat16
    a = _rnd(M, K, dtype=dtype, seed=41)
    b = _rnd(N, K, dtype=dtype, scale=0.1, seed=42)
    bi = _rnd(N, seed=43)
    r = _rnd(M, N, seed=44)
    u = _rnd(M, N, dtype=dtype, seed=45)
    g = ops.L.GemmNTArgs()
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.in_dtype, g.out_dtype, g.nzb, g.nzg = M, N, K, K, K, N, 1, 1, 1, 1
    t, rf, tr = C.c_int32(), C.c_int32(), C.c_int32()
    assert ops.lib().tav_gemm_nt_schedule(C.byref(g), C.byref(t), C.byref(rf), C.byref(tr)) == 0
    split = 0 < rf.value < M and tr.value > 0
    rs = [(f"gemm_nt.mixed.plan[M{M},N{N},K{K}] is two launches", 0.0 if split else 1.0, 0.0, bool(split))]
    flavours = [("bias->bf16", dict(bias=bi)), ("bias+resid->f32", dict(bias=bi, resid=r, out_dtype=torch.float32)),
                ("gelu+pre", dict(bias=bi, act=3, want_pre=True)), ("*gelu'", dict(gelu_in=u, act=4)), ("->f32", dict(out_dtype=torch.float32))]
    for name, kw in flavours:
        mixed = ops.gemm_nt(a, b, tile_m=0, **kw)
        single = ops.gemm_nt(a, b, tile_m=17, **kw)
        mixed, single = (mixed if isinstance(mixed, tuple) else (mixed,)), (single if isinstance(single, tuple) else (single,))
        same = all(torch.equal(x, y) for x, y in zip(mixed, single))
        rs.append((f"gemm_nt.mixed[{name}] bitwise == single tile", 0.0 if same else 1.0, 0.0, bool(same)))
    ref = a.float() @ b.float().t() + bi
    rs.append(_res("gemm_nt.mixed[bias->bf16] vs torch", ops.gemm_nt(a, b, bias=bi), ref, 1e-2))
    return rs


def check_gemm_nt_gelu_bwd(dtype, M=200, N=384, K=256):
    a = _rnd(M, K, dtype=dtype, seed=5)
    b = _rnd(N, K, dtype=dtype, scale=0.1, seed=6)
    u = _rnd(M, N, dtype=dtype, seed=7)
    out = ops.gemm_nt(a, b, gelu_in=u)
    uu = u.float().requires_grad_(True)
    (gr,) = torch.autograd.grad(F.gelu(uu).sum(), uu)
    ref = (a.float() @ b.float().t()) * gr
    return [_res(f"gemm_nt.gelu_bwd[{dtype}]", out, ref, 1e-2 if dtype == torch.bfloat16 else 2e-5)]


def check_gemm_nt_gelu_derivative_pair(dtype, M=300, N=384, K=256, tile_m=0):
    """act 3 (forward FFN1: GELU out + gelu' stored in C_pre) and act 4 (dgrad: multiply by the stored derivative) against autograd."""
    a = _rnd(M, K, dtype=dtype, seed=11)
    b = _rnd(N, K, dtype=dtype, scale=0.1, seed=12)
    bi = _rnd(N, seed=13)
    h, gp = ops.gemm_nt(a, b, bias=bi, act=3, want_pre=True, tile_m=tile_m)
    pre = (a.float() @ b.float().t() + bi).requires_grad_(True)
    y = F.gelu(pre)
    (gr,) = torch.autograd.grad(y.sum(), pre)
    tol = 1e-2 if dtype == torch.bfloat16 else 2e-5
    rs = [_res(f"gemm_nt.act3.gelu[{dtype},tm{tile_m}]", h, y.detach(), tol), _res(f"gemm_nt.act3.gelu'[{dtype},tm{tile_m}]", gp, gr, tol)]
    dy = _rnd(M, K, dtype=dtype, seed=14)
    w_t = _rnd(N, K, dtype=dtype, scale=0.1, seed=15)
    du = ops.gemm_nt(dy, w_t, gelu_in=gp, act=4, tile_m=tile_m)
    rs.append(_res(f"gemm_nt.act4[{dtype},tm{tile_m}]", du, (dy.float() @ w_t.float().t()) * gp.float(), tol))
    return rs


def check_fp8(M=700, N=384, K=1024, tile_m=0):
    """fp8 path (BASELINE config 5): per-tensor amax scaling, e4m3 quantisation (+ zero-padded transposed copy), the block-scaled MFMA GEMM with
    every epilogue flavour, and the weight gradient as the NT GEMM of the transposed copies.  References are computed from the DEQUANTISED
    operands, so the GEMM comparison is exact up to f32 summation order; the quantiser is compared with torch's own e4m3 conversion."""
    x = _rnd(M, K, dtype=torch.bfloat16, seed=21)
    w = _rnd(N, K, seed=22, scale=0.05)
    x8 = ops.fp8_quantize(x, want_t=True)
    w8 = ops.fp8_quantize(w)
    amax = x.float().abs().max()
    rs = [_res("fp8.amax", x8.scales[2:3], amax.reshape(1), 0.0), _res("fp8.scale", x8.scales[0:1], (448.0 / amax).reshape(1), 1e-6)]
    ref_q = (x.float() * x8.scales[0]).to(torch.float8_e4m3fn).float()
    rs.append(_res("fp8.quantize_vs_torch", x8.q.float(), ref_q, 0.0))
    # the row-major-only form takes the streaming kernel (16-B loads, no transposing tiles): same bytes; and so does its delayed-scaling form
    x8s = ops.fp8_quantize(x)
    rs.append(_res("fp8.quantize_stream == tiled", x8s.q.float(), x8.q.float(), 0.0))
    sts = ops.Fp8States(x.device, n=4)
    xa = ops.fp8_quantize(x, state=(sts, "x"))             # calibrates
    xb = ops.fp8_quantize(x, state=(sts, "x"))             # delayed: same scale, gathers the maximum
    rs.append(_res("fp8.quantize_stream delayed == calibrated", xb.q.float(), xa.q.float(), 0.0))
    rs.append(_res("fp8.delayed gathered amax", sts.dev[0, 3:4], amax.reshape(1), 0.0))
    xv = x[:, : K // 2]                                     # a strided view (row stride K, 16-B aligned): still the streaming kernel
    rs.append(_res("fp8.quantize_stream strided", ops.fp8_quantize(xv).q.float(), (xv.float() * (448.0 / xv.float().abs().max())).to(torch.float8_e4m3fn).float(), 0.0))
    kp = x8.qt.shape[1]
    rs.append(_res("fp8.quantize_t", x8.qt.float()[:, :M], x8.q.float().t(), 0.0))
    rs.append(_res("fp8.quantize_t_pad", x8.qt.float()[:, M:].abs().sum().reshape(1), torch.zeros(1, device=DEV), 0.0))
    xd, wd = x8.q.float() * x8.scales[1], w8.q.float() * w8.scales[1]
    bias = _rnd(N, seed=23)
    res = _rnd(M, N, seed=24)
    y = ops.gemm_nt_fp8(x8, w8, bias=bias, tile_m=tile_m)
    rs.append(_res(f"fp8.gemm_nt[bf16 out,tm{tile_m}]", y, xd @ wd.t() + bias, 1e-2))
    y32 = ops.gemm_nt_fp8(x8, w8, bias=bias, resid=res, out_dtype=torch.float32, tile_m=tile_m)
    rs.append(_res(f"fp8.gemm_nt[f32 out + resid,tm{tile_m}]", y32, xd @ wd.t() + bias + res, 2e-5))
    h, gp = ops.gemm_nt_fp8(x8, w8, bias=bias, act=3, want_pre=True, tile_m=tile_m)
    pre = (xd @ wd.t() + bias).requires_grad_(True)
    (gr,) = torch.autograd.grad(F.gelu(pre).sum(), pre)
    rs += [_res("fp8.gemm_nt.gelu", h, F.gelu(pre.detach()), 1e-2), _res("fp8.gemm_nt.gelu'", gp, gr, 1e-2)]
    # rough quantisation error of the whole product against the unquantised one (per-tensor e4m3, K = 1024): a sanity bound, not a parity claim
    rs.append(_res("fp8.gemm_nt.vs_unquantised", y32, x.float() @ w.t() + bias + res, 3e-2))
    dy = _rnd(M, N, dtype=torch.bfloat16, seed=25)
    dy8 = ops.fp8_quantize(dy, want_q=False, want_t=True)
    dw = ops.wgrad_fp8(dy8, x8)
    dyd, xdt = dy8.qt.float()[:, :M] * dy8.scales[1], x8.qt.float()[:, :M] * x8.scales[1]
    rs.append(_res("fp8.wgrad", dw, dyd @ xdt.t(), 1e-4))
    return rs


def check_gemm_tn(dtype, M=1000, N1=256, N2=384, nbatch=1):
    a = _rnd(nbatch * M, N1, dtype=dtype, seed=8)
    b = _rnd(nbatch * M, N2, dtype=dtype, seed=9)
    out, dbias = ops.gemm_tn(a, b, N1=N1, N2=N2, lda=N1, ldb=N2, rows_per_batch=M, nbatch=nbatch, a_zb=M * N1, b_zb=M * N2, want_bias=True)
    ref = a.float().t() @ b.float()
    return [_res(f"gemm_tn[{dtype},M{M},N1{N1},N2{N2},nb{nbatch}]", out, ref, 2e-3 if dtype == torch.bfloat16 else 2e-5),
            _res("gemm_tn.dbias", dbias, a.float().sum(0), 1e-5)]


def check_gemm_tn_grouped(dtype, M=777):
    """Four weight gradients over the same (ragged) token axis in one launch; operands are column slices of wider buffers."""
    shapes = [(384, 128), (128, 136), (256, 128), (128, 264)]
    wide_a = _rnd(M, 640, dtype=dtype, seed=21)
    pairs, refs = [], []
    for k, (n1, n2) in enumerate(shapes):
        a = wide_a[:, 64:64 + n1] if k == 0 else _rnd(M, n1, dtype=dtype, seed=22 + k)
        b = _rnd(M, n2, dtype=dtype, seed=30 + k)
        pairs.append((a, b))
        refs.append((a.float().t() @ b.float(), a.float().sum(0)))
    outs = ops.gemm_tn_grouped(pairs, want_bias=True)
    rs = []
    for k, ((dW, db), (rW, rb)) in enumerate(zip(outs, refs)):
        rs.append(_res(f"gemm_tn_grouped[{dtype},M{M}].dW{k}", dW, rW, 2e-3 if dtype == torch.bfloat16 else 2e-5))
        rs.append(_res(f"gemm_tn_grouped[{dtype},M{M}].db{k}", db, rb, 1e-5))
    return rs


def check_gemm_tn_grouped_big(M=5000, flags=1):
    """The 256-wide weight-gradient tile (bf16): ragged N1 / N2 (not multiples of 256), a ragged last K-tile, operands that are column slices
    of wider buffers, one to three token splits with the fixed-order slab reduce -- against f32 matmuls; and twice for bitwise reproducibility."""
    dtype = torch.bfloat16
    shapes = [(384, 136), (136, 264), (256, 512), (520, 128)]
    wide_a = _rnd(M, 640, dtype=dtype, seed=51)
    pairs, refs = [], []
    for k, (n1, n2) in enumerate(shapes):
        a = wide_a[:, 64:64 + n1] if k == 0 else _rnd(M, n1, dtype=dtype, seed=52 + k)
        b = _rnd(M, n2, dtype=dtype, seed=60 + k)
        pairs.append((a, b))
        refs.append((a.float().t() @ b.float(), a.float().sum(0)))
    rs = []
    for nsplit in (1, 2, 3):
        if (nsplit - 1) * (((M + nsplit - 1) // nsplit + 63) // 64 * 64) >= M:       # (the library refuses a split that would be empty)
            continue
        outs = ops.gemm_tn_grouped(pairs, want_bias=True, flags=flags | (nsplit << 8))
        again = ops.gemm_tn_grouped(pairs, want_bias=True, flags=flags | (nsplit << 8))
        for k, ((dW, db), (rW, rb)) in enumerate(zip(outs, refs)):
            rs.append(_res(f"gemm_tn_grouped.big[M{M},splits{nsplit}].dW{k}", dW, rW, 2e-3))
            rs.append(_res(f"gemm_tn_grouped.big[M{M},splits{nsplit}].db{k}", db, rb, 1e-5))
        same = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(outs, again))
        rs.append((f"gemm_tn_grouped.big[splits{nsplit}] bitwise repeatable", 0.0 if same else 1.0, 0.0, bool(same)))
    small = ops.gemm_tn_grouped(pairs, want_bias=True, flags=2)
    for k, ((dW, db), (rW, rb)) in enumerate(zip(small, refs)):
        rs.append(_res(f"gemm_tn_grouped.small(flag)[M{M}].dW{k}", dW, rW, 2e-3))
    return rs


def check_conv_as_gemm(dtype, B=2, T_in=203, Cc=64, k=3, s=2):
    """Conv1d(C,C,k,stride s) on channels-last activations as an NT GEMM over overlapping rows + its gradients."""
    T_out = (T_in - k) // s + 1
    x = _rnd(B, T_in, Cc, dtype=dtype, seed=10)
    w = _rnd(Cc, Cc, k, scale=0.1, seed=11)              # nn.Conv1d layout [co][ci][k], f32 parameter
    wn, wt, _ = ops.cast_conv_weight(w, dtype)
    y, pre = ops.gemm_nt(x, wn, act=1, want_pre=True, M=T_out, N=Cc, K=k * Cc, lda=s * Cc, ldb=k * Cc, ldc=Cc,
                         nzb=B, a_zb=T_in * Cc, c_zb=T_out * Cc, out_shape=(B, T_out, Cc))
    xr = _r(x).permute(0, 2, 1).requires_grad_(True)
    wr = _r(w).clone().requires_grad_(True)
    pre_ref = F.conv1d(xr, wr if dtype == torch.float32 else _r(wr.to(dtype)), stride=s)
    y_ref = F.gelu(pre_ref)
    tol = 1e-2 if dtype == torch.bfloat16 else 2e-5
    rs = [_res(f"conv_gemm.fwd[{dtype}]", y, y_ref.permute(0, 2, 1), tol)]
    dy = _rnd(B, T_out, Cc, dtype=dtype, seed=12)
    y_ref.backward(_r(dy).permute(0, 2, 1))
    du = ops.gelu_bwd(pre, dy)
    dcol = ops.gemm_nt(du.view(B * T_out, Cc), wt, out_shape=(B * T_out, k * Cc))
    dx = ops.col2im_1d(dcol, B, T_in, T_out, Cc, k, s)
    rs.append(_res(f"conv_gemm.dx[{dtype}]", dx, xr.grad.permute(0, 2, 1), tol))
    dw = ops.gemm_tn(du, x, N1=Cc, N2=k * Cc, lda=Cc, ldb=s * Cc, rows_per_batch=T_out, nbatch=B, a_zb=T_out * Cc,
                     b_zb=T_in * Cc, perm_inner=Cc, perm_outer=k, out_shape=(Cc, Cc, k))
    rs.append(_res(f"conv_gemm.dw[{dtype}]", dw, wr.grad, 1e-2 if dtype == torch.bfloat16 else 2e-5))
    return rs


def check_conv_chain(dtype, B=3, T=407, Cc=64):
    """engine.ConvGemmFn as the wav2vec2 feature extractor chains it (HF wav2vec2:382-419, preset B: conv -> GELU, k = 3, 3, 2 at stride 2): the
    round-4 input gradient -- one NT GEMM per output phase over a zero-framed dy, gelu' in the epilogue, no column buffer / col2im -- against
    torch's conv1d autograd, and against the column-buffer path of rounds 1-3 (same products: bf16 differs only by where it rounds)."""
    from tav_amd import engine as E
    from tav_amd import runtime
    ectx = E.Ctx("fp32" if dtype == torch.float32 else "bf16")
    ks = [(3, 2), (3, 2), (2, 2)]
    ws = [torch.nn.Parameter(_rnd(Cc, Cc, k, scale=0.12, seed=300 + i)) for i, (k, _) in enumerate(ks)]
    bs = [torch.nn.Parameter(_rnd(Cc, scale=0.1, seed=310 + i)) for i in range(3)]
    x0 = _rnd(B, T, Cc, dtype=dtype, seed=320)

    def run(phase):
        E.CONV_PHASE_DGRAD[0] = phase
        for p_ in ws + bs:
            p_.grad = None
        x = x0.clone().requires_grad_(True)
        h, u = x, None
        for (k, st), w, b in zip(ks, ws, bs):
            h, u = E.ConvGemmFn.apply(h, u, w, b, st, True, ectx)
        (h.float() * h.float()).sum().backward()
        return h.detach(), x.grad.detach(), [w.grad.detach().clone() for w in ws], [b.grad.detach().clone() for b in bs]
    try:
        y1, dx1, dw1, db1 = run(True)
        y0, dx0, dw0, db0 = run(False)
    finally:
        E.CONV_PHASE_DGRAD[0] = True
    xr = x0.float().permute(0, 2, 1).requires_grad_(True)
    wr = [w.detach().clone().requires_grad_(True) for w in ws]
    br = [b.detach().clone().requires_grad_(True) for b in bs]
    h = xr
    for (k, st), w, b in zip(ks, wr, br):
        h = F.gelu(F.conv1d(h, w if dtype == torch.float32 else w.to(dtype).float(), b, stride=st))
    (h * h).sum().backward()
    tol = 3e-2 if dtype == torch.bfloat16 else 5e-5
    rs = [_res(f"conv_chain.y[{dtype}]", y1, h.permute(0, 2, 1), tol), _res(f"conv_chain.dx phase[{dtype}]", dx1, xr.grad.permute(0, 2, 1), tol),
          _res(f"conv_chain.dx col2im[{dtype}]", dx0, xr.grad.permute(0, 2, 1), tol)]
    for i in range(3):
        rs.append(_res(f"conv_chain.dw{i} phase[{dtype}]", dw1[i], wr[i].grad, tol))
        rs.append(_res(f"conv_chain.db{i} phase[{dtype}]", db1[i], br[i].grad, tol))
        rs.append(_res(f"conv_chain.dw{i} phase vs col2im[{dtype}]", dw1[i], dw0[i], tol))
    return rs


# ------------------------------------------------------------------------------------------------ attention
def _attn_ref(q, k, v, mask, mode, scale):
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if mode == 1:
        s = s + mask[:, None, None, :]
    p = torch.softmax(s, dim=-1)
    if mode == 2:
        p = p + mask[:, None, None, :]
    return torch.einsum("bhqk,bhkd->bhqd", p, v)


def check_attention(dtype, mode, B=2, S=200, nh=3, bwd=True, ref_style_mask=False, pre=False, spike=0.0):
    """ref_style_mask: the values PreFormer really produces (models/tav.py:383-397): {0,-65504} text, {65505,1} audio,
    {0} video.  The rank-1 term then dwarfs softmax(s)v, so the check is against an fp64 reference.
    pre: the q_prescaled convention of tav_attn_args (q holds q * scale * log2(e)); the reference sees the SAME rounded values divided
    by the factor, and dq is still the gradient w.r.t. the unscaled q.
    spike: scale factor on a few late (and one early) key rows, so a tile's maximum jumps past the running reference exponent by far
    more than the lazy-rescale threshold of the forward kernel -- the rare branch gets its own test (and an fp64 reference)."""
    H = nh * 64
    qkv = _rnd(B * S, 3 * H, dtype=dtype, seed=20 + mode)
    if spike:
        qkv = qkv.float().clone()
        for row in {min(S - 1, 3), S // 2, max(0, S - 40), S - 1}:
            qkv.view(B, S, 3 * H)[:, row, H:2 * H] *= spike
        qkv = qkv.to(dtype)
    c2 = ops.ATTN_Q_PRESCALE
    if pre:
        qkv = qkv.clone()
        qkv[:, :H] = (qkv[:, :H].float() * c2).to(dtype)
    mask = None
    if mode == 1:
        mask = torch.zeros(B, S, device=DEV)
        mask[:, S - 37:] = torch.finfo(torch.float32).min
    if mode == 2:
        mask = torch.zeros(B, S, device=DEV)
        mask[:, : S // 3] = -0.5
        mask[:, S // 3: S // 2] = 2.0
        mask[0, S // 2:] = 1.0
        if ref_style_mask:
            mask = torch.zeros(B, S, device=DEV)
            mask[:, S // 4 - 9: S // 4] = -65504.0          # padded text tokens
            mask[:, S // 4: S // 4 + S // 2] = 65505.0      # valid audio frames
            mask[0, S // 4 + S // 2 - 20: S // 4 + S // 2] = 1.0   # padded audio frames of row 0
    if spike or pre:
        qkv = _in(qkv)
    if mask is not None:
        mask = _in(mask)
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    o, lse, corr = ops.attn_fwd(q, k, v, B, S, nh, key_mask=mask, mask_mode=mode, q_prescaled=pre)

    rdt = torch.float64 if (ref_style_mask or spike) else torch.float32

    def heads(t, div=1.0):
        return (t.to(rdt) / div).reshape(B, S, nh, 64).permute(0, 2, 1, 3).contiguous().requires_grad_(True)

    qr, kr, vr = heads(q, c2 if pre else 1.0), heads(k), heads(v)
    o_ref = _attn_ref(qr, kr, vr, mask.to(rdt) if mask is not None else None, mode, 0.125)
    tol = 2e-2 if dtype == torch.bfloat16 else 5e-5
    tag = f"{dtype},mode{mode},S{S},ref{int(ref_style_mask)},pre{int(pre)},spike{spike:g}"
    rs = [_res(f"attn.fwd[{tag}]", o, o_ref.permute(0, 2, 1, 3).reshape(B * S, H), tol)]
    lse_ref = torch.logsumexp(torch.einsum("bhqd,bhkd->bhqk", qr.detach(), kr.detach()) * 0.125 + (mask.to(rdt)[:, None, None, :] if mode == 1 else 0.0), dim=-1)
    rs.append(_res(f"attn.lse[{tag}]", lse, lse_ref, 2e-2 if dtype == torch.bfloat16 else 1e-5))
    if bwd:
        do = _rnd(B * S, H, dtype=dtype, seed=30 + mode)
        o_ref.backward(do.to(rdt).reshape(B, S, nh, 64).permute(0, 2, 1, 3))
        dqkv = ops.attn_bwd(q, k, v, o, do, lse, corr, B, S, nh, key_mask=mask, mask_mode=mode, q_prescaled=pre)

        def flat(t):
            return t.permute(0, 2, 1, 3).reshape(B * S, H)

        tolb = (6e-2 if mode == 2 else 3e-2) if dtype == torch.bfloat16 else 1e-4
        rs.append(_res(f"attn.dq[{tag}]", dqkv[:, :H], flat(qr.grad), tolb))
        rs.append(_res(f"attn.dk[{tag}]", dqkv[:, H:2 * H], flat(kr.grad), tolb))
        rs.append(_res(f"attn.dv[{tag}]", dqkv[:, 2 * H:], flat(vr.grad), tolb))
    return rs


# ------------------------------------------------------------------------------------------------ layer norm
def check_layernorm(x_dtype, W=768, rows=333, act=0):
    x = _rnd(rows, W, dtype=x_dtype, seed=40)
    gamma = 1.0 + 0.1 * _rnd(W, seed=41)
    beta = 0.1 * _rnd(W, seed=42)
    y32, ylp, mean, rstd = ops.ln_fwd(x, gamma, beta, 1e-5, want_f32=True, lp_dtype=torch.bfloat16, act=act)
    xr = _r(x).requires_grad_(True)
    gr, br = _r(gamma).clone().requires_grad_(True), _r(beta).clone().requires_grad_(True)
    ref = F.layer_norm(xr, (W,), gr, br, 1e-5)
    if act:
        ref = F.gelu(ref)
    rs = [_res(f"ln.fwd[{x_dtype},W{W},act{act}]", y32, ref, 2e-5), _res("ln.fwd.lp", ylp, ref, 1e-2)]
    dy = _rnd(rows, W, seed=43)
    add = _rnd(rows, W, seed=44)
    ref.backward(_r(dy))
    dx32, dxlp, dg, db = ops.ln_bwd(dy, x, gamma, beta, mean, rstd, dx_add=add, want_f32=True, lp_dtype=torch.bfloat16, act=act)
    rs += [_res("ln.dx", dx32, xr.grad + _r(add), 5e-5), _res("ln.dx.lp", dxlp, xr.grad + _r(add), 1e-2),
           _res("ln.dgamma", dg, gr.grad, 1e-4), _res("ln.dbeta", db, br.grad, 1e-4)]
    return rs


def check_layernorm_deferred_param_reduce(n_ln=70):
    """ABI v5: inside an autograd backward pass ops.ln_bwd keeps the per-workgroup column sums and ONE tav_ln_param_reduce_multi launch per 64
    LayerNorms reduces them when the pass ends (ops.ln_flush, queued on the engine).  70 LayerNorms of three widths and ragged row counts
    (two launches): dgamma / dbeta must equal the immediate two-stage form bit for bit, and nothing may be pending afterwards."""
    cases = []
    for i in range(n_ln):
        W = (768, 512, 1024)[i % 3]
        rows = 37 + 61 * i
        x = _rnd(rows, W, seed=400 + i)
        gamma, beta = _rnd(W, seed=401 + i) * 0.1 + 1.0, _rnd(W, seed=402 + i) * 0.1
        _, _, mean, rstd = ops.ln_fwd(x, gamma, beta, 1e-5, want_f32=True, lp_dtype=None)
        dy = _rnd(rows, W, seed=403 + i)
        cases.append((x, gamma, beta, mean, rstd, dy))
    assert ops._graph_task_id() < 0
    want = [ops.ln_bwd(dy, x, g, b, m, r, want_f32=True)[2:] for (x, g, b, m, r, dy) in cases]       # outside a pass: immediate

    class Ln(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, g, b, i):
            ctx.i = i
            return x.clone()

        @staticmethod
        def backward(ctx, dy):
            x, g, b, m, r, _ = cases[ctx.i]
            dx, _, dg, db = ops.ln_bwd(dy.contiguous(), x, g, b, m, r, want_f32=True)
            return dx, dg, db, None

    leaves, total = [], None
    for i, (x, g, b, m, r, dy) in enumerate(cases):
        gp, bp = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
        leaves.append((gp, bp))
        t = (Ln.apply(x.clone().requires_grad_(True), gp, bp, i) * dy).sum()
        total = t if total is None else total + t
    total.backward()
    torch.cuda.synchronize()
    assert not ops._ln_pending["items"]
    worst_g = max(float((gp.grad - w[0]).abs().max()) for (gp, _), w in zip(leaves, want))
    worst_b = max(float((bp.grad - w[1]).abs().max()) for (_, bp), w in zip(leaves, want))
    ok_g, ok_b = worst_g == 0.0, worst_b == 0.0
    return [(f"ln.deferred dgamma bitwise x{n_ln}", worst_g, 0.0, ok_g), (f"ln.deferred dbeta bitwise x{n_ln}", worst_b, 0.0, ok_b)]


# ------------------------------------------------------------------------------------------------ misc
def check_cast_weight():
    w = _rnd(300, 200, seed=50)
    n, t = ops.cast_weight(w, torch.bfloat16)
    return [_res("cast_weight.n", n, w.bfloat16(), 0.0), _res("cast_weight.t", t, w.bfloat16().t(), 0.0)]


def check_colsum():
    x = _rnd(1000, 768, dtype=torch.bfloat16, seed=51)
    return [_res("colsum", ops.colsum(x), x.float().sum(0), 1e-5)]


def check_text_embed(pad_id=1, B=3, S=50):
    W, V = 768, 1000
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(3, V, (B, S), generator=g)
    ids[:, S - min(9, S // 2):] = 1
    ids = _in(ids.to(DEV))
    word, pos, typ = _rnd(V, W, seed=52), _rnd(S + 10, W, seed=53), _rnd(1, W, seed=54)
    gamma, beta = 1 + 0.1 * _rnd(W, seed=55), 0.1 * _rnd(W, seed=56)
    y32, _, pre, pos_ids, _, _ = ops.text_embed_fwd(ids, word, pos, typ, gamma, beta, 1e-5, pad_id)
    if pad_id >= 0:
        m = ids.ne(pad_id).int()
        pid = (torch.cumsum(m, 1) * m).long() + pad_id
    else:
        pid = torch.arange(S, device=DEV)[None].expand(B, S)
    ref = F.layer_norm(_r(word)[ids] + _r(pos)[pid] + _r(typ)[0], (W,), _r(gamma), _r(beta), 1e-5).reshape(B * S, W)
    return [_res(f"text_embed[pad{pad_id}]", y32, ref, 2e-5), _res("text_embed.pos_ids", pos_ids.float(), pid.float(), 0.0)]


def check_patchify(dtype=torch.float32, B=2, nkeep=5):
    Fr, H, W = 4, 32, 48
    video = _rnd(B, Fr, 3, H, W, seed=57)
    ntok = (Fr // 2) * (H // 16) * (W // 16)
    mask = torch.zeros(B, ntok, dtype=torch.bool)
    if (B, nkeep) == (2, 5):
        mask[0, [0, 3, 4, 7, 11]] = True
        mask[1, [1, 2, 5, 9, 10]] = True
    else:
        g = torch.Generator().manual_seed(59)
        for b_ in range(B):
            mask[b_, torch.randperm(ntok, generator=g)[:nkeep]] = True
    mask = _in(mask.to(DEV))
    idx, counts = ops.mask_to_index(mask, True, nkeep)
    patches = ops.patchify(video, idx, dtype)
    wconv = _rnd(8, 3, 2, 16, 16, scale=0.05, seed=58)
    emb = F.conv3d(_r(video).permute(0, 2, 1, 3, 4), _r(wconv), stride=(2, 16, 16)).flatten(2).transpose(1, 2)   # [B, ntok, 8]
    ref = emb[mask].reshape(B * nkeep, 8)
    got = _r(patches) @ _r(wconv).reshape(8, -1).t()
    return [_res("patchify+gemm", got, ref, 1e-4), _res("mask_to_index.counts", counts.float(), torch.full((B,), float(nkeep), device=DEV), 0.0)]


def check_pool_head_ce(B=3, S=77):
    W = 768
    x = _rnd(B * S, W, seed=60)
    rs = [_res("mean_pool", ops.mean_pool_fwd(x, B, S), _r(x).reshape(B, S, W).mean(1), 1e-5)]
    dy = _rnd(B, W, seed=61)
    dx, _ = ops.mean_pool_bwd(dy, B, S)
    rs.append(_res("mean_pool.bwd", dx, (_r(dy) / S)[:, None, :].expand(B, S, W).reshape(B * S, W), 1e-6))
    xh = _rnd(B, 3072, seed=62)
    Wh, bh = _rnd(7, 3072, scale=0.05, seed=63), _rnd(7, seed=64)
    y = ops.head_fwd(xh, Wh, bh)
    xr, Wr, br = _r(xh).clone().requires_grad_(True), _r(Wh).clone().requires_grad_(True), _r(bh).clone().requires_grad_(True)
    yr = F.linear(xr, Wr, br)
    rs.append(_res("head.fwd", y, yr, 1e-5))
    tgt = _in(torch.tensor([1, 6, 3, 0, 5, 2, 4][:B], device=DEV))
    cw = _in(torch.rand(7, device=DEV) + 0.5)
    for weights in (None, cw):
        loss, dlog = ops.cross_entropy(y, tgt, weights)
        yl = _r(y).clone().requires_grad_(True)
        lr = F.cross_entropy(yl, tgt, weight=None if weights is None else _r(weights))
        lr.backward()
        rs.append(_res(f"ce.loss[w{weights is not None}]", loss, lr.reshape(1), 1e-5))
        rs.append(_res(f"ce.dlogits[w{weights is not None}]", dlog, yl.grad, 1e-5))
    dyh = _rnd(B, 7, seed=65)
    yr.backward(_r(dyh))
    dxh, dWh, dbh = ops.head_bwd(xh, Wh, dyh)
    rs += [_res("head.dx", dxh, xr.grad, 1e-5), _res("head.dW", dWh, Wr.grad, 1e-5), _res("head.db", dbh, br.grad, 1e-5)]
    t = _rnd(5, 768, seed=66)
    ty = ops.tanh_fwd(t)
    rs += [_res("tanh", ty, torch.tanh(_r(t)), 1e-6), _res("tanh.bwd", ops.tanh_bwd(ty, t), _r(t) * (1 - torch.tanh(_r(t)) ** 2), 1e-5)]
    return rs


def check_embed_add(rows=500):
    W = 768
    x = _rnd(rows, W, seed=67)
    ids = _in(torch.randint(0, 3, (rows,), generator=torch.Generator().manual_seed(1)).to(DEV))
    table = _rnd(3, W, seed=68)
    rs = [_res("embed_add.fwd", ops.embed_add_fwd(x, ids, table), _r(x) + _r(table)[ids], 1e-6)]
    dy = _rnd(rows, W, seed=69)
    ref = torch.zeros(3, W, device=DEV, dtype=_REF[0]).index_add_(0, ids, _r(dy))
    rs.append(_res("embed_add.bwd", ops.embed_add_bwd(dy, ids, 3), ref, 1e-5))
    rs.append(_res("scatter_add_rows", ops.scatter_add_rows(dy, ids, 3), ref, 1e-5))
    return rs


def check_scatter_deterministic():
    """The embedding-table gradient at the size of a real text batch: 4096 token rows, a padding id shared by a quarter of them, ids outside
    the table skipped; equal to index_add_ and bitwise identical from run to run (no atomics)."""
    rows, W, ntab = 4096, 768, 1000
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(3, ntab, (rows,), generator=g)
    ids[torch.rand(rows, generator=g) < 0.25] = 0
    ids[7] = 2
    ids = ids.to(DEV)
    dy = _rnd(rows, W, seed=91)
    ref = torch.zeros(ntab, W, device=DEV, dtype=torch.float64).index_add_(0, ids, dy.double()).float()
    a = ops.scatter_add_rows(dy, ids, ntab)
    b = ops.scatter_add_rows(dy, ids, ntab)
    bad = ids.clone()
    bad[5] = ntab + 3                                  # out-of-table index: skipped, never written out of bounds
    c = ops.scatter_add_rows(dy, bad, ntab)
    ref_c = torch.zeros(ntab, W, device=DEV, dtype=torch.float64).index_add_(0, ids[torch.arange(rows, device=DEV) != 5],
                                                                           dy.double()[torch.arange(rows, device=DEV) != 5]).float()
    return [_res("scatter_add_rows.large", a, ref, 2e-6), _res("scatter_add_rows.bitwise_repeat", (a != b).float().sum().reshape(1), torch.zeros(1, device=DEV), 0.0),
            _res("scatter_add_rows.bad_index_skipped", c, ref_c, 2e-6)]


def check_index_safety():
    """Rows of the video mask that keep FEWER tokens than nkeep (what the reference's collate can produce at batch > 1): keep_idx is still fully
    written with in-range indices, counts report the truth, and out-of-range indices handed to the gathers are clamped instead of faulting."""
    B, n, nkeep = 3, 96, 10
    mask = torch.zeros(B, n, dtype=torch.bool)
    mask[0, torch.arange(0, 40, 4)] = True              # exactly nkeep
    mask[1, [3, 50, 95]] = True                         # short row
    # row 2 keeps nothing
    idx, counts = ops.mask_to_index(mask.to(DEV), True, nkeep)
    exp = torch.zeros(B, nkeep)
    exp[0] = torch.arange(0, 40, 4).float()
    exp[1] = torch.tensor([3., 50., 95.] + [95.] * 7)
    rs = [_res("mask_to_index.padded", idx.float(), exp.to(DEV), 0.0), _res("mask_to_index.counts_short", counts.float(), torch.tensor([10., 3., 0.], device=DEV), 0.0)]
    table = _rnd(20, 64, seed=92)
    wild = torch.tensor([0, 19, -5, 20, 1 << 30], dtype=torch.int32, device=DEV)
    rs.append(_res("gather_rows.clamped", ops.gather_rows(table, wild), table[torch.tensor([0, 19, 0, 19, 19], device=DEV)], 0.0))
    video = _rnd(1, 2, 3, 32, 32, seed=93)
    ok = ops.patchify(video, torch.tensor([[3]], dtype=torch.int32, device=DEV), torch.float32)
    hi = ops.patchify(video, torch.tensor([[1 << 20]], dtype=torch.int32, device=DEV), torch.float32)
    rs.append(_res("patchify.clamped", hi, ok, 0.0))
    return rs


def check_conv0_gn(dtype, B=2, T_in=1605, ref64=False):
    """ref64: every reference in fp64, the group norm written out by hand (mean and biased variance over time, per entry and channel) -- torch's
    own group_norm refuses one value per channel, which is exactly the smallest launch (B = 1, one output step: y = gelu(beta), dx = 0)."""
    Cc, K, s = 512, 10, 5
    rd = torch.float64 if ref64 else torch.float32
    T_out = (T_in - K) // s + 1
    wave = _rnd(B, T_in, scale=0.5, seed=70)
    w = _rnd(Cc, 1, K, scale=0.3, seed=71)
    gamma, beta = 1 + 0.1 * _rnd(Cc, seed=72), 0.1 * _rnd(Cc, seed=73)
    y0 = ops.conv0_fwd(wave, w, None, T_out, s, dtype)
    wr = w.to(rd).clone().requires_grad_(True)
    gr, br = gamma.to(rd).clone().requires_grad_(True), beta.to(rd).clone().requires_grad_(True)
    c_ref = F.conv1d(wave.to(rd)[:, None], wr, stride=s)     # [B, C, T_out]
    tol = 1e-2 if dtype == torch.bfloat16 else 3e-5
    rs = [_res(f"conv0.fwd[{dtype}]", y0, c_ref.permute(0, 2, 1), tol)]
    y1, stats = ops.gn_gelu_fwd(y0, gamma, beta, 1e-5)
    c_in = y0.to(rd).permute(0, 2, 1).detach().requires_grad_(True)
    if ref64:
        mu, var = c_in.mean(2, keepdim=True), c_in.var(2, unbiased=False, keepdim=True)
        g_ref = F.gelu((c_in - mu) / torch.sqrt(var + 1e-5) * gr[None, :, None] + br[None, :, None])
    else:
        g_ref = F.gelu(F.group_norm(c_in, Cc, gr, br, 1e-5))
    rs.append(_res(f"gn_gelu.fwd[{dtype}]", y1, g_ref.permute(0, 2, 1), tol))
    dy = _rnd(B, T_out, Cc, dtype=dtype, seed=74)
    g_ref.backward(dy.to(rd).permute(0, 2, 1))
    dx, dg, db = ops.gn_gelu_bwd(y0, dy, gamma, beta, stats)
    tolb = 3e-2 if dtype == torch.bfloat16 else 2e-4
    rs += [_res(f"gn_gelu.dx[{dtype}]", dx, c_in.grad.permute(0, 2, 1), tolb), _res("gn_gelu.dgamma", dg, gr.grad, tolb),
           _res("gn_gelu.dbeta", db, br.grad, tolb)]
    c_ref.backward(dx.to(rd).permute(0, 2, 1))
    dw, _ = ops.conv0_bwd_w(wave, dx, K, s, False)
    rs.append(_res(f"conv0.dw[{dtype}]", dw, wr.grad, 1e-4))
    return rs


def check_posconv(dtype, B=2, T=49):
    """grouped conv k=128, pad 64, drop last, GELU, + residual: forward and all gradients vs torch."""
    H, G, K = 256, 4, 128
    Cg = H // G
    x = _rnd(B, T, H, seed=80)                                   # f32 residual stream
    v = _rnd(H, Cg, K, scale=0.05, seed=81)
    g = (1.0 + 0.1 * _rnd(K, seed=82)).abs()
    bias = 0.1 * _rnd(H, seed=83)
    w, wf, norms = ops.weight_norm_fwd(v, g, dtype)
    xg = ops.group_pad(x.view(B * T, H), B, T, H, G, 64, 64, dtype)
    TP = T + 128
    y, pre = ops.gemm_nt(xg, w, bias=bias, act=1, resid=x.view(B * T, H), want_pre=True, out_dtype=torch.float32,
                         M=T, N=Cg, K=K * Cg, lda=Cg, ldb=K * Cg, ldc=H, nzb=B, nzg=G, a_zb=G * TP * Cg, a_zg=TP * Cg,
                         b_zg=Cg * K * Cg, c_zb=T * H, c_zg=Cg, bias_zg=Cg, out_shape=(B * T, H))
    xr = _r(x).clone().requires_grad_(True)
    vr, gr_, br = _r(v).clone().requires_grad_(True), _r(g).clone().requires_grad_(True), _r(bias).clone().requires_grad_(True)
    wr = gr_[None, None, :] * vr / vr.pow(2).sum((0, 1), keepdim=True).sqrt()
    conv = F.conv1d(xr.permute(0, 2, 1), wr, br, padding=64, groups=G)[:, :, :-1]
    ref = xr + F.gelu(conv).permute(0, 2, 1)
    tol = 2e-2 if dtype == torch.bfloat16 else 5e-5
    rs = [_res(f"posconv.fwd[{dtype}]", y, ref.reshape(B * T, H), tol)]
    gout = _rnd(B * T, H, seed=84)
    ref.backward(_r(gout).view(B, T, H))
    du = ops.gelu_bwd(pre, gout)                                  # f32 [B*T, H]
    dug = ops.group_pad(du, B, T, H, G, 63, 64, dtype)
    TPd = T + 127
    dx = ops.gemm_nt(dug, wf, resid=gout, out_dtype=torch.float32, M=T, N=Cg, K=K * Cg, lda=Cg, ldb=K * Cg, ldc=H, nzb=B, nzg=G,
                     a_zb=G * TPd * Cg, a_zg=TPd * Cg, b_zg=Cg * K * Cg, c_zb=T * H, c_zg=Cg, out_shape=(B * T, H))
    rs.append(_res(f"posconv.dx[{dtype}]", dx, xr.grad.reshape(B * T, H), tol))
    du_lp = ops.cast2d(du, dtype)
    dw = _blank((G, Cg, K * Cg), torch.float32)
    for gi in range(G):
        ops.gemm_tn(du_lp[:, gi * Cg:], xg[:, gi], out=dw[gi], N1=Cg, N2=K * Cg, lda=H, ldb=Cg, rows_per_batch=T, nbatch=B,
                    a_zb=T * H, b_zb=G * TP * Cg)
    dv, dg = ops.weight_norm_bwd(v, g, norms, dw)
    tolw = 3e-2 if dtype == torch.bfloat16 else 2e-4
    rs += [_res(f"posconv.dv[{dtype}]", dv, vr.grad, tolw), _res(f"posconv.dg[{dtype}]", dg, gr_.grad, tolw),
           _res(f"posconv.dbias[{dtype}]", ops.colsum(du), br.grad, tolw)]
    return rs


# ------------------------------------------------------------------------------------------------ edges that only make sense under guard
# Every case below hands the library 0xFF-filled outputs (NaN until written) and, inside guarded.active(), operands with 0xFF all around
# them: an element left unwritten, a store outside the logical tensor and an outside read that reaches the result all fail.  References are
# fp64; tolerances are the constants of the family's existing check.
def _gelu_d(x):
    xx = x.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(F.gelu(xx).sum(), xx)
    return g


def check_gemm_nt_edges(dtype, hint):
    """M in {1, tile-1, tile, tile+1} of the hint's tile height (128 for the library's own choice, hints 0 and 17), N in {4, 132, 260}, K = one
    and three K-tiles (128 bytes of operand), every epilogue flavour in turn; each once into a contiguous output and once with out / C_pre /
    resid / gelu_in as column slices of wider buffers (ldc > N).  The columns outside the slice must still be 0xFF."""
    bm = {2: 64, 3: 96, 4: 128, 8: 256, 16: 256}.get(hint, 128)
    kt = 128 // dtype.itemsize
    lp = dtype == torch.bfloat16
    rs, n = [], 0
    for M in (1, bm - 1, bm, bm + 1):
        for N in (4, 132, 260):
            for K in (kt, 3 * kt):
                flavour = n % 5
                n += 1
                a = _rnd(M, K, dtype=dtype, seed=500 + n)
                b = _rnd(N, K, dtype=dtype, scale=0.1, seed=600 + n)
                bias = _rnd(N, seed=700 + n)
                prod = a.double() @ b.double().t()
                for strided in (False, True):
                    ex = 16 if strided else 0

                    def side(t):
                        return _in(t, ex) if strided else t
                    kw, want_pre = {}, None
                    if flavour == 0:                                  # plain: bias only
                        kw = dict(bias=bias)
                        want = prod + bias
                    elif flavour == 1:                                # f32 out + f32 residual
                        r = _rnd(M, N, seed=800 + n)
                        kw = dict(bias=bias, resid=side(r), out_dtype=torch.float32)
                        want = prod + bias + r.double()
                    elif flavour == 2:                                # GELU out + gelu' in C_pre
                        kw = dict(bias=bias, act=3, want_pre=True)
                        want, want_pre = F.gelu(prod + bias), _gelu_d(prod + bias)
                    elif flavour == 3:                                # multiply by a stored derivative
                        u = _rnd(M, N, dtype=dtype, seed=810 + n)
                        kw = dict(gelu_in=side(u), act=4)
                        want = prod * u.double()
                    else:                                             # the generic epilogue with every side tensor at once
                        r, u = _rnd(M, N, seed=820 + n), _rnd(M, N, dtype=dtype, seed=830 + n)
                        kw = dict(bias=bias, want_pre=True, gelu_in=side(u), act=4, resid=side(r))
                        want, want_pre = (prod + bias) * u.double() + r.double(), prod + bias
                    odt = kw.get("out_dtype", dtype)
                    wide = None
                    if strided:
                        wide = _blank((M, N + 16), odt)
                        kw["out"] = wide[:, 8:8 + N]
                    res = ops.gemm_nt(a, b, tile_m=hint, **kw)
                    out, pre = res if isinstance(res, tuple) else (res, None)
                    tol = 2e-5 if not lp else (1e-2 if odt == torch.bfloat16 else 2e-3)
                    tag = f"gemm_nt.edge[{dtype},tm{hint},M{M},N{N},K{K},f{flavour},{'strided' if strided else 'dense'}]"
                    rs.append(_res(tag, out, want, tol))
                    if pre is not None:
                        rs.append(_res(tag + ".pre", pre, want_pre, tol))
                    if strided:
                        assert out.data_ptr() == wide[:, 8:].data_ptr() and (pre is None or pre.stride(0) == N + 16)
                        rs.append(_all_ff(tag + ".gap", wide[:, :8], wide[:, 8 + N:]))
    return rs


def check_fp8_quantize_edges():
    """rows not a multiple of the transposing tile (1, 33, 1025: one past the padding unit too), the smallest legal cols (4) and a ragged 132:
    q against torch's own e4m3 conversion, qt its transpose, qt's padding columns exactly zero; nothing past rows_pad (the guard).  Then ties,
    e4m3 subnormals and an all-zero tensor (check_fp8_quantize_ties)."""
    rs = []
    for rows, cols in ((1, 4), (33, 4), (33, 132), (1025, 132), (1, 1024)):
        for dtype in (torch.float32, torch.bfloat16):
            ops.clear_workspaces()                                    # scratch at exactly this shape's size, not the running maximum
            x = _rnd(rows, cols, dtype=dtype, seed=900)
            f = ops.fp8_quantize(x, want_t=True)
            ref_q = (x.float() * f.scales[0]).to(torch.float8_e4m3fn).float()
            tag = f"fp8.edge[{dtype},{rows}x{cols}]"
            rs.append(_res(tag + ".q", f.q.float(), ref_q, 0.0))
            rs.append(_res(tag + ".qt", f.qt.float()[:, :rows], ref_q.t(), 0.0))
            pad = f.qt[:, rows:].contiguous().view(torch.uint8)
            rs.append((tag + ".qt_pad bytes zero", float(pad.ne(0).sum().item()), 0.0, not bool(pad.ne(0).any())))
            rs.append(_res(tag + ".amax", f.scales[2:3], x.float().abs().max().reshape(1), 0.0))
    return rs + check_fp8_quantize_ties()


def check_gemm_tn_edges(dtype):
    """rows in {1, 63, 64, 65} (around the 64-row chunk), one batch and three (rows_per_batch not a multiple of the chunk), N1 / N2 ragged against
    the 128-wide tile, `out=` a slice of a gradient arena with unused floats on both sides."""
    rs = []
    for rows in (1, 63, 64, 65):
        for nb in (1, 3):
            N1, N2 = 136, 264
            ops.clear_workspaces()                                    # slabs / bias partials at exactly tav_gemm_tn_splits' size for this shape
            a = _rnd(nb * rows, N1, dtype=dtype, seed=910 + rows)
            b = _rnd(nb * rows, N2, dtype=dtype, seed=920 + rows)
            arena = _blank((64 + N1 * N2 + 64,), torch.float32)
            out, dbias = ops.gemm_tn(a, b, out=arena[64:64 + N1 * N2].view(N1, N2), N1=N1, N2=N2, lda=N1, ldb=N2, rows_per_batch=rows, nbatch=nb,
                                     a_zb=rows * N1, b_zb=rows * N2, want_bias=True)
            tag = f"gemm_tn.edge[{dtype},rows{rows},nb{nb}]"
            rs.append(_res(tag, out, a.double().t() @ b.double(), 2e-3 if dtype == torch.bfloat16 else 2e-5))
            rs.append(_res(tag + ".dbias", dbias, a.double().sum(0), 1e-5))
            rs.append(_all_ff(tag + ".arena gaps", arena[:64], arena[64 + N1 * N2:]))
    return rs


def check_gemm_tn_grouped_edges(dtype):
    """Four weight gradients in one launch written straight into four slices of ONE arena buffer (`into=`) with unused floats between them,
    rows in {1, 63, 64, 65}, every form and split count the library accepts for that size (`flags` as in check_gemm_tn_grouped_big)."""
    shapes = [(384, 136), (136, 264), (256, 512), (520, 128)]
    rs = []
    for rows in (1, 63, 64, 65):
        wide_a = _rnd(rows, 640, dtype=dtype, seed=930 + rows)
        pairs, refs = [], []
        for k, (n1, n2) in enumerate(shapes):
            a = wide_a[:, 64:64 + n1] if k == 0 else _rnd(rows, n1, dtype=dtype, seed=940 + k + rows)
            b = _rnd(rows, n2, dtype=dtype, seed=950 + k + rows)
            pairs.append((a, b))
            refs.append((a.double().t() @ b.double(), a.double().sum(0)))
        forms = [0, 2] + ([1] if dtype == torch.bfloat16 else [])
        for form in forms:
            for nsplit in ((0,) if form != 1 else (0, 1, 2, 3)):
                if nsplit and (nsplit - 1) * (((rows + nsplit - 1) // nsplit + 63) // 64 * 64) >= rows:     # (the library refuses an empty split)
                    continue
                total = sum(n1 * n2 + n1 + 2 * 36 for n1, n2 in shapes)
                arena = _blank((total,), torch.float32)
                into, gaps, off = [], [], 0
                for n1, n2 in shapes:
                    gaps.append(arena[off:off + 36])
                    dW = arena[off + 36:off + 36 + n1 * n2].view(n1, n2)
                    off += 36 + n1 * n2
                    gaps.append(arena[off:off + 36])
                    db = arena[off + 36:off + 36 + n1]
                    off += 36 + n1
                    into.append((dW, db))
                assert off == total
                outs = ops.gemm_tn_grouped(pairs, want_bias=True, flags=form | (nsplit << 8), into=into)
                tag = f"gemm_tn_grouped.edge[{dtype},rows{rows},form{form},splits{nsplit}]"
                for k, ((dW, db), (rW, rb)) in enumerate(zip(outs, refs)):
                    assert dW.data_ptr() == into[k][0].data_ptr() and db.data_ptr() == into[k][1].data_ptr()
                    rs.append(_res(f"{tag}.dW{k}", dW, rW, 2e-3 if dtype == torch.bfloat16 else 2e-5))
                    rs.append(_res(f"{tag}.db{k}", db, rb, 1e-5))
                rs.append(_all_ff(tag + ".arena gaps", *gaps))
    return rs


def check_attention_edges(dtype, mode, S, B=3, nh=3, pre=False, lens=None):
    """q / k / v as slices of a qkv buffer whose row pitch is wider than 3H, dq / dk / dv into a column slice of a wider buffer, S around the
    64- and 128-row tiles, B * nheads * tiles not a multiple of 8 -- against an fp64 reference.  lens: the length-aware entry points with these
    per-row lengths (0 and S included): rows past a length come out zero, the others equal attention over the first L keys."""
    H = nh * 64
    g = torch.Generator(device="cpu").manual_seed(1000 + S + mode)
    qkv0 = torch.randn(B * S, 3 * H, generator=g).to(DEV).to(dtype)
    c2 = ops.ATTN_Q_PRESCALE
    if pre:
        qkv0[:, :H] = (qkv0[:, :H].float() * c2).to(dtype)
    qkv = _in(qkv0, 24)                                               # row pitch 3H + 24 elements (16-B aligned rows in both dtypes)
    do = _in(torch.randn(B * S, H, generator=g).to(DEV).to(dtype), 8)
    mask = None
    if mode == 1:
        mask = torch.zeros(B, S)
        mask[:, S - S // 3:] = torch.finfo(torch.float32).min
    if mode == 2:
        mask = torch.where(torch.rand(B, S, generator=g) < 0.3, -0.5, 0.0) + torch.where(torch.rand(B, S, generator=g) < 0.2, 2.0, 0.0)
    if mask is not None:
        mask = _in(mask.float().to(DEV))
    sl = None if lens is None else _in(torch.tensor(lens, dtype=torch.int32, device=DEV))
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    o, lse, corr = ops.attn_fwd(q, k, v, B, S, nh, key_mask=mask, mask_mode=mode, q_prescaled=pre, seq_lens=sl)
    wide = _blank((B * S, 3 * H + 16), dtype)
    dqkv = ops.attn_bwd(q, k, v, o, do, lse, corr, B, S, nh, key_mask=mask, mask_mode=mode, q_prescaled=pre, seq_lens=sl, dqkv=wide[:, 8:8 + 3 * H])

    o_ref = torch.zeros(B, S, H, dtype=torch.float64, device=DEV)
    lse_ref = torch.zeros(B, nh, S, dtype=torch.float64, device=DEV)
    d_ref = torch.zeros(B, S, 3 * H, dtype=torch.float64, device=DEV)
    for b_ in range(B):
        L = S if lens is None else min(max(lens[b_], 0), S)
        if L == 0:
            continue
        rows = slice(b_ * S, b_ * S + L)

        def heads(t, div=1.0):
            return (t[rows].double() / div).reshape(1, L, nh, 64).permute(0, 2, 1, 3).contiguous().requires_grad_(True)
        qr, kr, vr = heads(q, c2 if pre else 1.0), heads(k), heads(v)
        mb = None if mask is None else mask[b_:b_ + 1, :L].double()
        ob = _attn_ref(qr, kr, vr, mb, mode, 0.125)
        ob.backward(do[rows].double().reshape(1, L, nh, 64).permute(0, 2, 1, 3))
        o_ref[b_, :L] = ob.detach().permute(0, 2, 1, 3).reshape(L, H)
        sc = torch.einsum("bhqd,bhkd->bhqk", qr.detach(), kr.detach()) * 0.125 + (mb[:, None, None, :] if mode == 1 else 0.0)
        lse_ref[b_, :, :L] = torch.logsumexp(sc, dim=-1)[0]
        for j, t in enumerate((qr, kr, vr)):
            d_ref[b_, :L, j * H:(j + 1) * H] = t.grad.permute(0, 2, 1, 3).reshape(L, H)
    lp = dtype == torch.bfloat16
    tolb = (6e-2 if mode == 2 else 3e-2) if lp else 1e-4
    tag = f"attn.edge[{dtype},mode{mode},S{S},B{B},nh{nh},pre{int(pre)},lens{lens}]"
    d_ref = d_ref.reshape(B * S, 3 * H)
    rs = [_res(tag + ".fwd", o, o_ref.reshape(B * S, H), 2e-2 if lp else 5e-5), _res(tag + ".lse", lse, lse_ref, 2e-2 if lp else 1e-5),
          _res(tag + ".dq", dqkv[:, :H], d_ref[:, :H], tolb), _res(tag + ".dk", dqkv[:, H:2 * H], d_ref[:, H:2 * H], tolb),
          _res(tag + ".dv", dqkv[:, 2 * H:], d_ref[:, 2 * H:], tolb), _all_ff(tag + ".dqkv gap", wide[:, :8], wide[:, 8 + 3 * H:])]
    if lens is not None:
        for b_, L in enumerate(lens):
            L = min(max(L, 0), S)
            pad = slice(b_ * S + L, (b_ + 1) * S)
            z = o[pad].float().abs().sum() + dqkv[pad].float().abs().sum() + lse[b_, :, L:].abs().sum()
            rs.append((f"{tag}.row{b_} padding exactly zero", float(z.item()), 0.0, float(z.item()) == 0.0))
    return rs


def check_elementwise_tails():
    """Element counts around the 4-wide vector and the 256-thread block (x 4 elements): n in {1, 3, 4k+1, 4k+3, 1024 +- 1} where the kernel takes
    any n (tanh, dropout, fill); add_f32 and gelu_bwd require n % 4 == 0 (TAV_ERR_SHAPE otherwise), so they run at the nearest multiples of 4
    (4, 1020, 1024, 1028); cast2d at C % 4 == 0 with both sides strided with gaps."""
    rs = []
    for n in (1, 3, 41, 43, 1023, 1025):
        x = _rnd(n, seed=960)
        dy = _rnd(n, seed=961)
        y = ops.tanh_fwd(x)
        rs.append(_res(f"tanh[n{n}]", y, torch.tanh(x.double()), 1e-6))
        rs.append(_res(f"tanh.bwd[n{n}]", ops.tanh_bwd(y, dy), dy.double() * (1 - y.double() ** 2), 1e-5))
        z = ops.zeros_f32((n,), DEV)
        rs.append((f"zeros_f32[n{n}]", float(z.abs().sum().item()), 0.0, bool((z == 0).all())))
        for p in (0.0, 0.3):
            yd, m = ops.dropout_fwd(x, p, 1234, 7)
            keep = m.ne(0)
            # element i's draw depends on (seed, offset + i) alone: the n-element mask is the prefix of a longer launch's, and the launch
            # at offset + 1 is that mask shifted by one -- a tail lane that always kept / always dropped would break both; p = 0 keeps all
            xl = _rnd(n + 2049, seed=967)
            _, ml = ops.dropout_fwd(xl, p, 1234, 7)
            _, ms = ops.dropout_fwd(x, p, 1234, 8)
            same = torch.equal(m, ml[:n]) and torch.equal(ms, ml[1:n + 1]) and (p > 0 or bool(keep.all()))
            rs.append((f"dropout.mask == prefix of a longer launch[n{n},p{p}]", 0.0 if same else 1.0, 0.0, bool(same)))
            if p > 0:
                frac = float(ml.float().mean().item())                # 2k draws: 5 sigma of a fair p = 0.3 coin is 0.05
                rs.append((f"dropout.keep fraction[p{p}]", abs(frac - (1 - p)), 0.05, abs(frac - (1 - p)) <= 0.05))
            ok_m = bool(((m == 0) | (m == 1)).all())
            rs.append((f"dropout.mask is 0/1[n{n},p{p}]", 0.0 if ok_m else 1.0, 0.0, ok_m))
            rs.append(_res(f"dropout.fwd[n{n},p{p}]", yd, torch.where(keep, x.double() / (1 - p), torch.zeros_like(x, dtype=torch.float64)), 1e-6))
            rs.append(_res(f"dropout.bwd[n{n},p{p}]", ops.dropout_bwd(dy, m, p), torch.where(keep, dy.double() / (1 - p), torch.zeros_like(dy, dtype=torch.float64)), 1e-6))
    for n in (4, 1020, 1024, 1028):
        a, b = _rnd(n, seed=962), _rnd(n, seed=963)
        for lpd in (None, torch.bfloat16, torch.float32):
            y, ylp = ops.add_f32(a, b, want_f32=True, lp_dtype=lpd)
            same = torch.equal(y, a + b) and (ylp is None or torch.equal(ylp, (a + b).to(lpd)))
            rs.append((f"add_f32[n{n},lp{lpd}] exact", 0.0 if same else 1.0, 0.0, bool(same)))
        _, only_lp = ops.add_f32(a, b, want_f32=False, lp_dtype=torch.bfloat16)
        same = torch.equal(only_lp, (a + b).bfloat16())
        rs.append((f"add_f32[n{n}] bf16 only exact", 0.0 if same else 1.0, 0.0, bool(same)))
        for dtype in (torch.float32, torch.bfloat16):
            x, dy = _rnd(n, dtype=dtype, seed=964), _rnd(n, dtype=dtype, seed=965)
            rs.append(_res(f"gelu_bwd[{dtype},n{n}]", ops.gelu_bwd(x, dy), dy.double() * _gelu_d(x.double()), 1e-2 if dtype == torch.bfloat16 else 2e-5))
    for R, Cc in ((1, 4), (3, 132), (65, 1028)):
        for sd in (torch.float32, torch.bfloat16):
            for dd in (torch.float32, torch.bfloat16):
                x = _in(_rnd(R, Cc, dtype=sd, seed=966), 8)
                wide = _blank((R, Cc + 16), dd)
                out = ops.cast2d(x, dd, out=wide[:, 8:8 + Cc])
                same = torch.equal(out, x.to(dd))
                rs.append((f"cast2d[{sd}->{dd},{R}x{Cc}] strided exact", 0.0 if same else 1.0, 0.0, bool(same)))
                rs.append(_all_ff(f"cast2d[{sd}->{dd},{R}x{Cc}].gap", wide[:, :8], wide[:, 8 + Cc:]))
    return rs


def check_layernorm_edges():
    """rows in {1, 2} and one less / one more than the rows a workgroup handles (4 in the forward: one wave per row, 4 waves; 16 in the backward's
    column-sum blocks), all three widths; mean, rstd and the partial slabs sit under guard."""
    rs = []
    for W in (512, 768, 1024):
        for rows in (1, 2, 3, 5, 15, 17):
            for xd in (torch.float32, torch.bfloat16):
                ops.clear_workspaces()                                # the partial slab at exactly tav_ln_bwd_partials(rows) * 2 W
                rs += [(f"{n}[rows{rows},W{W},{xd}]", e, t, ok) for n, e, t, ok in check_layernorm(xd, W=W, rows=rows, act=rows % 2)]
    return rs


def check_attn_probs(dtype, S, B=2, nh=3):
    """tav_attn_probs against fp64 softmax(q k^T * scale [+ mask]) (+ post-softmax mask in mode 2, as _attn_ref does), the softmax part times
    head_scale in its [nheads] and [B, nheads] layouts and None; raw and q_prescaled.  Tolerance: the attn.fwd constants of check_attention."""
    H = nh * 64
    rs = []
    tol = 2e-2 if dtype == torch.bfloat16 else 5e-5
    for mode in (0, 1, 2):
        for pre in (False, True):
            g = torch.Generator(device="cpu").manual_seed(1100 + S + mode)
            qkv0 = torch.randn(B * S, 3 * H, generator=g).to(DEV).to(dtype)
            if pre:
                qkv0[:, :H] = (qkv0[:, :H].float() * ops.ATTN_Q_PRESCALE).to(dtype)
            qkv = _in(qkv0, 8)
            mask = None
            if mode == 1:
                mask = torch.zeros(B, S)
                mask[:, S - S // 3:] = torch.finfo(torch.float32).min
            if mode == 2:
                mask = torch.where(torch.rand(B, S, generator=g) < 0.3, -0.5, 0.0)
            if mask is not None:
                mask = _in(mask.float().to(DEV))
            q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
            _, lse, _ = ops.attn_fwd(q, k, v, B, S, nh, key_mask=mask, mask_mode=mode, q_prescaled=pre)

            def heads(t, div=1.0):
                return (t.double() / div).reshape(B, S, nh, 64).permute(0, 2, 1, 3)
            sc = torch.einsum("bhqd,bhkd->bhqk", heads(q, ops.ATTN_Q_PRESCALE if pre else 1.0), heads(k)) * 0.125
            if mode == 1:
                sc = sc + mask.double()[:, None, None, :]
            soft = torch.softmax(sc, dim=-1)
            for name, hs in (("none", None), ("[nh]", _rnd(nh, seed=1101)), ("[B,nh]", _rnd(B, nh, seed=1102))):
                got = ops.attn_probs(q, k, lse, B, S, nh, key_mask=mask, mask_mode=mode, q_prescaled=pre, head_scale=hs)
                f = 1.0 if hs is None else (hs.double().reshape(1, nh, 1, 1) if hs.dim() == 1 else hs.double().reshape(B, nh, 1, 1))
                want = soft * f + (mask.double()[:, None, None, :] if mode == 2 else 0.0)
                rs.append(_res(f"attn_probs[{dtype},S{S},mode{mode},pre{int(pre)},hs{name}]", got, want, tol))
    return rs


def check_head_scale(dtype, B=2, S=37, nh=3):
    """out = (a or 0) + (c0 + hs[b, h]) * b: `a` present / absent, hs [nheads] / [B, nheads] / None, in place (out = a, as the engine's head-mask
    path calls it) and into a fresh tensor, every operand a strided slice.  The kernel does one multiply-add in f32: f32 results within
    tol_for(f32) of the fp64 value; a bf16 result within ONE bf16 rounding of it, |err| <= 2^-8 |ref|.  That bound is applied as it stands
    wherever the two terms do not cancel (|ref| >= (|a| + |f b|) / 2: a half ulp is below 2^-8 (1 - 2^-8) |ref|, the f32 roundings of f, f b
    and the sum below 2^-21 |ref|).  Where they cancel further no f32 multiply-add can meet a bound relative to the result alone, and the
    f32 rounding of the terms, 2^-22 (|a| + |f b|), is added."""
    H = nh * 64
    rs = []
    for use_a in (False, True):
        for name, hs in (("none", None), ("[nh]", _rnd(nh, seed=1201)), ("[B,nh]", _rnd(B, nh, seed=1202))):
            for inplace in ((False, True) if use_a else (False,)):
                for c0 in (-1.0, 1.0):
                    a_vals = _rnd(B * S, H, dtype=dtype, seed=1203) if use_a else None
                    a, awide = (_in(a_vals, 8) if use_a else None), None
                    if inplace:                                       # (a destination, so not a watched input: a slice of a 0xFF buffer)
                        awide = _blank((B * S, H + 16), dtype)
                        a = awide[:, 8:8 + H]
                        a.copy_(a_vals)
                    b = _in(_rnd(B * S, H, dtype=dtype, seed=1204), 16)
                    a0 = a_vals.double() if use_a else torch.zeros(B * S, H, dtype=torch.float64, device=DEV)
                    f = torch.full((B, nh), c0, dtype=torch.float64, device=DEV)
                    if hs is not None:
                        f = f + (hs.double()[None, :] if hs.dim() == 1 else hs.double())
                    fb = (f[:, None, :, None] * b.double().reshape(B, S, nh, 64)).reshape(B * S, H)
                    want = a0 + fb
                    wide = None
                    if inplace:
                        out = ops.head_scale(a, b, hs, c0, B, S, nh, out=a)
                    else:
                        wide = _blank((B * S, H + 16), dtype)
                        out = ops.head_scale(a, b, hs, c0, B, S, nh, out=wide[:, 8:8 + H])
                    tag = f"head_scale[{dtype},a{int(use_a)},hs{name},inplace{int(inplace)},c0{c0:g}]"
                    if dtype == torch.float32:
                        rs.append(_res(tag, out, want, tol_for(torch.float32)))
                    else:
                        mag = a0.abs() + fb.abs()
                        bound = torch.where(2 * want.abs() >= mag, 2.0 ** -8 * want.abs(), 2.0 ** -8 * want.abs() + 2.0 ** -22 * mag)
                        err = (out.double() - want).abs()
                        ok = bool((err <= bound).all()) and bool(torch.isfinite(out.float()).all())
                        rs.append((tag, float((err / bound.clamp_min(1e-300)).max().item()), 1.0, ok))
                    for w_ in (wide, awide):
                        if w_ is not None:
                            rs.append(_all_ff(tag + ".gap", w_[:, :8], w_[:, 8 + H:]))
    return rs


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.dtype.itemsize])


def check_transpose2d():
    """Bitwise against x.view(nb, R, C).transpose(1, 2): R and C not multiples of the 32 x 32 tile, one batch and three, both dtypes."""
    rs = []
    for dtype in (torch.float32, torch.bfloat16):
        for nb in (1, 3):
            for R, Cc in ((1, 1), (33, 31), (70, 130), (37, 64)):
                x = _rnd(nb * R, Cc, dtype=dtype, seed=1300)
                got = ops.transpose2d(x, R, Cc, nb)
                same = got.shape == x.shape and torch.equal(_bits(got).view(nb, Cc, R), _bits(x).view(nb, R, Cc).transpose(1, 2))
                rs.append((f"transpose2d[{dtype},nb{nb},{R}x{Cc}] bitwise", 0.0 if same else 1.0, 0.0, bool(same)))
    return rs


def check_zero_pad_rows():
    """The `pad` leading and trailing rows of each batch entry become zero; the T interior rows keep 0xFF in every byte (never touched)."""
    rs = []
    for dtype in (torch.float32, torch.bfloat16):
        for B, T, Cc, pad in ((1, 1, 4, 1), (3, 5, 132, 2), (2, 70, 64, 3)):
            buf = _blank((B, T + 2 * pad, Cc), dtype)
            ops.zero_pad_rows(buf, B, T, Cc, pad)
            frame = torch.cat([buf[:, :pad], buf[:, pad + T:]], 1).contiguous().view(torch.uint8)
            tag = f"zero_pad_rows[{dtype},B{B},T{T},C{Cc},pad{pad}]"
            rs.append((tag + ".frame bytes zero", float(frame.ne(0).sum().item()), 0.0, not bool(frame.ne(0).any())))
            rs.append(_all_ff(tag + ".interior untouched", buf[:, pad:pad + T]))
    return rs


def check_small_counts():
    """Index / pooling / head kernels and the audio front-end at one row / one batch entry and at odd counts, the front-end also at the
    smallest length its host validation accepts (T_in = K = 10: one output step) and one output step past its 512-step chunk."""
    rs = []
    for B, S in ((1, 1), (1, 77), (5, 3)):
        rs += [(f"{n}[B{B},S{S}]", e, t, ok) for n, e, t, ok in check_pool_head_ce(B=B, S=S)]
    for rows in (1, 257):
        ops.clear_workspaces()                                        # the partial slab at exactly tav_embed_add_bwd_parts(rows) * ntable * W
        rs += [(f"{n}[rows{rows}]", e, t, ok) for n, e, t, ok in check_embed_add(rows=rows)]
    for pad_id in (1, -1):
        for B, S in ((1, 1), (1, 65), (3, 7)):
            rs += [(f"{n}[pad{pad_id},B{B},S{S}]", e, t, ok) for n, e, t, ok in check_text_embed(pad_id, B=B, S=S)]
    for B, nkeep in ((1, 1), (1, 5), (3, 7), (5, 12)):               # (12 = every token of the 4 x 32 x 48 clip kept)
        rs += [(f"{n}[B{B},nkeep{nkeep}]", e, t, ok) for n, e, t, ok in check_patchify(B=B, nkeep=nkeep)]
    table = _rnd(7, 132, seed=1400)
    for idx in ([3], [6, 0, 6, 2, 5]):
        it = _in(torch.tensor(idx, dtype=torch.int32, device=DEV))
        rs.append(_res(f"gather_rows[{len(idx)}]", ops.gather_rows(table, it), table[it.long()], 0.0))
        i64 = _in(torch.tensor(idx, dtype=torch.int64, device=DEV))
        d = _rnd(len(idx), 132, seed=1401)
        rs.append(_res(f"scatter_add_rows[{len(idx)}]", ops.scatter_add_rows(d, i64, 7), torch.zeros(7, 132, dtype=torch.float64, device=DEV).index_add_(0, i64, d.double()), 1e-6))
    m = torch.zeros(1, 5, dtype=torch.bool)
    m[0, [1, 4]] = True
    idx, counts = ops.mask_to_index(_in(m.to(DEV)), True, 2)
    rs.append(_res("mask_to_index[B1,n5]", idx.float(), torch.tensor([[1., 4.]], device=DEV), 0.0))
    rs.append(_res("mask_to_index.counts[B1,n5]", counts.float(), torch.tensor([2.], device=DEV), 0.0))
    m = torch.zeros(3, 7, dtype=torch.bool)
    m[0, [0, 6]] = True
    m[1, [2, 3, 5]] = True                                            # more than nkeep: truncated
    m[2, [4]] = True                                                  # fewer: the last kept index repeats
    idx, counts = ops.mask_to_index(_in(m.to(DEV)), True, 2)
    rs.append(_res("mask_to_index[B3,n7]", idx.float(), torch.tensor([[0., 6.], [2., 3.], [4., 4.]], device=DEV), 0.0))
    rs.append(_res("mask_to_index.counts[B3,n7]", counts.float(), torch.tensor([2., 3., 1.], device=DEV), 0.0))
    return rs


def check_fp8_edges(M, N, K, tile_m):
    """The fp8 GEMM's epilogue like check_gemm_nt_edges: every flavour once into a contiguous output and once with out / C_pre / resid /
    gelu_in as column slices of wider buffers (ldc > N), the columns outside the slice still 0xFF afterwards.  References in fp64 from the
    DEQUANTISED operands (as check_fp8: exact up to summation order); tolerances are check_fp8's."""
    ops.clear_workspaces()
    x = _rnd(M, K, dtype=torch.bfloat16, seed=970)
    w = _rnd(N, K, seed=971, scale=0.05)
    x8, w8 = ops.fp8_quantize(x), ops.fp8_quantize(w)
    prod = (x8.q.double() * x8.scales[1].double()) @ (w8.q.double() * w8.scales[1].double()).t()
    bias = _rnd(N, seed=972)
    r, u = _rnd(M, N, seed=973), _rnd(M, N, dtype=torch.bfloat16, seed=974)
    rs = []
    for strided in (False, True):
        def side(t):
            return _in(t, 16) if strided else t
        for flavour in range(5):
            want_pre = None
            if flavour == 0:
                kw, want = dict(bias=bias), prod + bias
            elif flavour == 1:
                kw, want = dict(bias=bias, resid=side(r), out_dtype=torch.float32), prod + bias + r.double()
            elif flavour == 2:
                kw, want, want_pre = dict(bias=bias, act=3, want_pre=True), F.gelu(prod + bias), _gelu_d(prod + bias)
            elif flavour == 3:
                kw, want = dict(gelu_in=side(u), act=4), prod * u.double()
            else:
                kw = dict(bias=bias, want_pre=True, gelu_in=side(u), act=4, resid=side(r))
                want, want_pre = (prod + bias) * u.double() + r.double(), prod + bias
            odt = kw.get("out_dtype", torch.bfloat16)
            wide = None
            if strided:
                wide = _blank((M, N + 16), odt)
                kw["out"] = wide[:, 8:8 + N]
            res = ops.gemm_nt_fp8(x8, w8, tile_m=tile_m, **kw)
            out, pre = res if isinstance(res, tuple) else (res, None)
            tol = 1e-2 if odt == torch.bfloat16 else 2e-5
            tag = f"fp8.edge[M{M},N{N},K{K},tm{tile_m},f{flavour},{'strided' if strided else 'dense'}]"
            rs.append(_res(tag, out, want, tol))
            if pre is not None:
                rs.append(_res(tag + ".pre", pre, want_pre, tol))
            if strided:
                assert out.data_ptr() == wide[:, 8:].data_ptr() and (pre is None or pre.stride(0) == N + 16)
                rs.append(_all_ff(tag + ".gap", wide[:, :8], wide[:, 8 + N:]))
    return rs



# ------------------------------------------------------------------------------------------------ step-end kernels ("Step-end checks")
# Between one backward pass and the next forward pass: gradient norm, clip coefficient, AdamW, operand casts, fp8 state roll.  The optimizer
# checks call the C ABI with pointer / size / chunk tables built here; reference and bounds are tests/step_end_ref.py (fp64, per element).
_GAP = 36                    # floats of 0xFF between two slices of an arena (a multiple of 4: alignment is decided by `mis` alone)


def _exact(name, got, ref):
    """Result tuple of a comparison that has ONE right answer: same shape, same dtype, every element equal (no tolerance)."""
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return (name + f" shape/dtype {tuple(got.shape)} {got.dtype} vs {tuple(ref.shape)} {ref.dtype}", float("inf"), 0.0, False)
    bad = int(got.ne(ref).sum().item()) + int(got.ne(got).sum().item())           # (a NaN -- an unwritten 0xFF element -- never counts as equal)
    return (name, float(bad), 0.0, bad == 0)


def _refill(t):
    """Every byte of a contiguous buffer back to 0xFF (an output reused by the next launch must not keep the previous launch's values)."""
    assert t.is_contiguous()
    t.view(torch.uint8).fill_(0xFF)


class _Arena:
    """The tensors of one role as slices of one 0xFF buffer with 0xFF gaps between them (a 1 MiB flat guard per tensor would cost gigabytes);
    mis = True starts every slice 4 bytes past a 16-byte boundary."""

    def __init__(self, sizes, mis):
        self.sizes, self.starts, c = list(sizes), [], _GAP
        for n in sizes:
            self.starts.append(c + (1 if mis else 0))
            c = (self.starts[-1] + n + 3) // 4 * 4 + _GAP
        self.buf = _blank((c,), torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        idx = torch.cat([torch.arange(s, s + n) for s, n in zip(self.starts, sizes)])
        self.idx = idx.to(DEV)
        gap = torch.ones(c, dtype=torch.bool)
        gap[idx] = False
        self.gap_idx = gap.nonzero().flatten().to(DEV)
        self.ptrs = [self.buf.data_ptr() + 4 * s for s in self.starts]
        assert all((p_ % 16 == 4) == bool(mis) and p_ % 16 in (0, 4) for p_ in self.ptrs)

    def put(self, flat):
        self.buf[self.idx] = torch.as_tensor(flat, dtype=torch.float32).to(DEV)

    def get(self):
        return self.buf[self.idx].cpu().numpy()

    def gaps(self):
        return self.buf[self.gap_idx]

    def table(self):
        return _in(torch.tensor(self.ptrs, dtype=torch.int64).to(DEV))


_LAYOUTS = {"aligned": (False, False), "all+4B": (True, True), "grads+4B": (False, True)}        # name -> (params / moments misaligned, gradients misaligned)


def _i32(vals):
    return _in(torch.tensor(vals, dtype=torch.int32).to(DEV))


def _i64(vals):
    return _in(torch.tensor(vals, dtype=torch.int64).to(DEV))


def check_optimizer_step(list_name, layout, wd):
    """tav_adamw_chunked and tav_adamw_multi, three steps from zero moments (SR.step_plan: no clip pointer / coefficient < 1 / coefficient 1 after
    the device lr word was halved), each step against the fp64 reference restarted from the kernel's own previous state, per-element bounds of
    step_end_ref.py, err = worst |got - ref| / bound.  The chunked form walks its own trajectory; the multi form takes every step from the
    chunked form's previous state, so the two can also be compared with each other (within the sum of their bounds; they are not bitwise
    equal).  After every step: the step word counts the calls, bias_corr = 1 - b^s to 4u, arena gaps still 0xFF, gradients bit-identical."""
    L = ops.lib()
    sizes = SR.SIZE_LISTS[list_name]
    mis_p, mis_g = _LAYOUTS[layout]
    n_all, nt = sum(sizes), len(sizes)
    p0, g0 = SR.make_inputs(n_all, seed=len(sizes) + 1000 * list(_LAYOUTS).index(layout))
    G = _Arena(sizes, mis_g)
    G.put(g0)
    g_snapshot = G.buf.clone().view(torch.int32)
    forms = {}
    for form in ("chunked", "multi"):
        A = dict(p=_Arena(sizes, mis_p), m=_Arena(sizes, mis_p), v=_Arena(sizes, mis_p))
        A["p"].put(p0)
        A["m"].put(np.zeros(n_all))
        A["v"].put(np.zeros(n_all))
        scal = _blank((8,), torch.float32)                            # [1] clip coefficient, [4] lr, [5:7] bias_corr (as optim.FusedAdamW lays them out)
        step = _blank((1,), torch.int32)
        step.zero_()
        scal[4] = SR.LR
        forms[form] = dict(A=A, scal=scal, step=step, t=[A[k].table() for k in "pmv"])
    t_g, t_s = G.table(), _i64(sizes)
    pre, nchunks = SR.chunk_prefix(sizes, int(L.tav_optim_chunk_elems()))
    t_c = _i32(pre)
    b1, b2 = SR.BETAS
    tag0 = f"adamw[{list_name},{layout},wd{wd:g}]"
    rs = []
    for (s, lr, cc, with_ptr) in SR.step_plan():
        C_, M_ = forms["chunked"], forms["multi"]
        for k in "pmv":                                               # the multi form starts from the chunked form's state (bitwise, gaps included)
            M_["A"][k].buf.copy_(C_["A"][k].buf)
        before = {k: C_["A"][k].get() for k in "pmv"}
        got = {}
        for form, f in forms.items():
            if s == 3:
                f["scal"][4:5].mul_(0.5)                              # halve the device learning-rate word, change nothing else
            f["scal"][1] = cc
            coef = ops.ptr(f["scal"][1:2]) if with_ptr else None
            tp, tm, tv = (ops.ptr(t) for t in f["t"])
            if form == "chunked":
                ops.check(L.tav_adamw_chunked(tp, ops.ptr(t_g), tm, tv, ops.ptr(t_s), ops.ptr(t_c), nt, nchunks, coef, ops.ptr(f["scal"][4:5]), b1, b2,
                                              SR.EPS, wd, ops.ptr(f["step"]), ops.ptr(f["scal"][5:7]), ops.stream()), "adamw_chunked")
            else:
                ops.check(L.tav_adamw_multi(tp, ops.ptr(t_g), tm, tv, ops.ptr(t_s), nt, coef, ops.ptr(f["scal"][4:5]), b1, b2, SR.EPS, wd,
                                            ops.ptr(f["step"]), ops.ptr(f["scal"][5:7]), ops.stream()), "adamw_multi")
            got[form] = {k: f["A"][k].get() for k in "pmv"}
        lr_dev = float(C_["scal"][4].item())
        ref = SR.ref_step(before["p"], g0, before["m"], before["v"], s, lr_dev, wd, cc)
        for form, f in forms.items():
            tag = f"{tag0}.step{s}.{form}"
            for k, r in SR.ratios(ref, got[form]["p"], got[form]["m"], got[form]["v"]).items():
                rs.append((f"{tag}.{k} ratio to bound", r, 1.0, r <= 1.0))
            sw = int(f["step"].item())
            rs.append((tag + ".step word", float(abs(sw - s)), 0.0, sw == s))
            bc = f["scal"][5:7].cpu().numpy().astype(np.float64)
            e_bc = float(np.abs(bc - np.array(SR.bias_corr(s))).max() / (4 * SR.U))
            rs.append((tag + ".bias_corr / 4u", e_bc, 1.0, e_bc <= 1.0))
            e_lr = abs(float(f["scal"][4].item()) - lr)
            rs.append((tag + ".lr word", e_lr, 0.0, e_lr == 0.0))
            rs.append(_all_ff(tag + ".gap", *[f["A"][k].gaps() for k in "pmv"], f["scal"][0:1], f["scal"][2:4], f["scal"][7:8]))
        for k in "pmv":                                               # chunked against multi, from the same state: the sum of their two bounds
            r = SR.ratio(got["chunked"][k], got["multi"][k].astype(np.float64), 2 * ref[k + "_bound"])
            rs.append((f"{tag0}.step{s}.chunked vs multi.{k}", r, 1.0, r <= 1.0))
        same = torch.equal(G.buf.view(torch.int32), g_snapshot)
        rs.append((f"{tag0}.step{s}.gradients bit-identical", 0.0 if same else 1.0, 0.0, bool(same)))
    return rs


def _d_final(n):
    """Longest chain of additions through sum_final_kernel for n partials: accumulator a0 takes one addition per pass of the 4-way loop
    (n // 1024 passes at most) and up to three in the 256-stride tail loop; (a0 + a1) + (a2 + a3) is two more; the 256-wide LDS tree eight."""
    return n // 1024 + 3 + 2 + 8


def check_grad_norm():
    """tav_sumsq_chunked, tav_sumsq_multi and tav_sum_partials against the fp64 sum of squares.  Every term is positive, so a relative bound
    holds: (D + 3) u with D the longest chain of f32 additions any element goes through (each rounds by at most u relative to a partial sum
    that never exceeds the total); the + 3 covers the square, the subnormal-free tail and the final rounding.
      sumsq_chunk_kernel   misaligned chunk: a thread adds 16384 / 256 = 64 squares one by one (the 16-byte form: 16 passes of 4 additions);
                           wave_sum is 6 butterfly steps, red[0] + .. + red[3] three more: D1 = 64 + 6 + 3 = 73
      sumsq_multi_kernel   96 x 256 threads stride over a tensor: ceil(n / 24576) additions per thread, then the 256-wide tree, 8: D1 = that + 8
      sum_final_kernel     _d_final(number of partials)
    With at most 70 chunks / 67 x 96 partials here D stays below 100, (D + 3) u below 2^-16 (asserted)."""
    L = ops.lib()
    rs = []
    for list_name, sizes in SR.SIZE_LISTS.items():
        for mis in (False, True):
            nt = len(sizes)
            _, g0 = SR.make_inputs(sum(sizes), seed=77 + nt)
            G = _Arena(sizes, mis)
            G.put(g0)
            snap = G.buf.clone().view(torch.int32)
            want = float((g0.astype(np.float64) ** 2).sum())
            t_g, t_s = G.table(), _i64(sizes)
            pre, nchunks = SR.chunk_prefix(sizes, int(L.tav_optim_chunk_elems()))
            outs = _blank((4,), torch.float32)
            part_c = _blank((nchunks,), torch.float32)
            ops.check(L.tav_sumsq_chunked(ops.ptr(t_g), ops.ptr(t_s), ops.ptr(_i32(pre)), nt, nchunks, ops.ptr(part_c), ops.ptr(outs[0:1]), ops.stream()), "sumsq_chunked")
            n_part = int(L.tav_sumsq_partials(nt))
            part_m = _blank((n_part,), torch.float32)
            ops.check(L.tav_sumsq_multi(ops.ptr(t_g), ops.ptr(t_s), nt, ops.ptr(part_m), ops.ptr(outs[1:2]), ops.stream()), "sumsq_multi")
            ops.check(L.tav_sum_partials(ops.ptr(part_c), nchunks, ops.ptr(outs[2:3]), ops.stream()), "sum_partials")
            d_c = 1 + 73 + _d_final(nchunks)
            d_m = 1 + -(-max(sizes) // (96 * 256)) + 8 + _d_final(n_part)
            tag = f"sumsq[{list_name},{'+4B' if mis else 'aligned'}]"
            for form, d, k in (("chunked", d_c, 0), ("multi", d_m, 1)):
                bound = (d + 3) * SR.U
                assert bound <= 2.0 ** -16, (form, d)
                r = abs(float(outs[k].item()) - want) / want / bound
                rs.append((f"{tag}.{form} rel err / ((D={d}) + 3)u", r, 1.0, r <= 1.0))
            same = torch.equal(outs[2:3], outs[0:1])
            rs.append((tag + ".sum_partials == second stage bitwise", 0.0 if same else 1.0, 0.0, bool(same)))
            rs.append(_all_ff(tag + ".gap", G.gaps(), outs[3:4]))
            same = torch.equal(G.buf.view(torch.int32), snap)
            rs.append((tag + ".gradients bit-identical", 0.0 if same else 1.0, 0.0, bool(same)))
    # the boundaries of sum_final_kernel's 4-way loop (i + 768 < n, 256 threads): n one-element tensors make n chunks, whose partials are the
    # squares themselves (a wave sum of one value and zeros is exact)
    for n in (1, 255, 256, 257, 1023, 1024, 1025, 1279):
        sizes = [1] * n
        _, g0 = SR.make_inputs(n, seed=500 + n)
        g0[g0 == 0] = 3.0
        G = _Arena(sizes, bool(n % 2))
        G.put(g0)
        outs = _blank((3,), torch.float32)
        part = _blank((n,), torch.float32)
        ops.check(L.tav_sumsq_chunked(ops.ptr(G.table()), ops.ptr(_i64(sizes)), ops.ptr(_i32(list(range(n)))), n, n, ops.ptr(part), ops.ptr(outs[0:1]), ops.stream()),
                  "sumsq_chunked")
        ops.check(L.tav_sum_partials(ops.ptr(part), n, ops.ptr(outs[1:2]), ops.stream()), "sum_partials")
        sq = torch.as_tensor(g0).to(DEV)
        sq = sq * sq
        tag = f"sum_partials[n{n}]"
        rs.append(_exact(tag + ".partials are the squares", part, sq))
        want = float(sq.double().sum().item())
        bound = (_d_final(n) + 3) * SR.U
        r = abs(float(outs[1].item()) - want) / want / bound
        rs.append((f"{tag} rel err / ((D={_d_final(n)}) + 3)u", r, 1.0, r <= 1.0))
        same = torch.equal(outs[0:1], outs[1:2])
        rs.append((tag + " == second stage of sumsq_chunked bitwise", 0.0 if same else 1.0, 0.0, bool(same)))
        rs.append(_all_ff(tag + ".gap", G.gaps(), outs[2:3]))
    return rs


def check_clip_coef():
    """clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)) at sumsq = 0, finite above / below max_norm, +inf and NaN: a NaN norm gives a
    NaN coefficient (every parameter goes NaN, loudly), an infinite one 0.  norm within 2u of sqrt(sumsq) (one f32 ulp), a clipping coefficient
    within 4u relative, a non-clipping one exactly 1.  norm_out = NULL is accepted."""
    L = ops.lib()
    inf, nan = float("inf"), float("nan")
    rs = []
    for max_norm in (1.0, 0.25):
        for sumsq in (0.0, 1e-30, 0.5 * max_norm ** 2, max_norm ** 2, 1.0000002 * max_norm ** 2, 4.0, 3.7e9, 3.0e38, inf, nan):
            for with_norm in (True, False):
                scal = _blank((4,), torch.float32)
                scal[0] = sumsq
                ops.check(L.tav_clip_coef(ops.ptr(scal[0:1]), max_norm, ops.ptr(scal[1:2]), ops.ptr(scal[2:3]) if with_norm else None, ops.stream()), "clip_coef")
                s32 = float(scal[0].item())
                coef, norm = float(scal[1].item()), float(scal[2].item())
                tag = f"clip_coef[max{max_norm:g},sumsq{sumsq:g},{'norm' if with_norm else 'norm NULL'}]"
                if math.isnan(s32):
                    ok_n, ok_c, e = math.isnan(norm), math.isnan(coef), 0.0
                elif math.isinf(s32):
                    ok_n, ok_c, e = norm == inf, coef == 0.0, 0.0
                else:
                    want_n = math.sqrt(s32)
                    want_c = max_norm / (want_n + float(np.float32(1e-6)))
                    ok_n = abs(norm - want_n) <= 2 * SR.U * want_n
                    if want_c > 1.0 + 8 * SR.U:
                        e, ok_c = abs(coef - 1.0), coef == 1.0
                    elif want_c >= 1.0 - 8 * SR.U:                       # within rounding of the clamp: either side of it is right
                        e = abs(coef - min(want_c, 1.0)) / (4 * SR.U)
                        ok_c = e <= 1.0 and coef <= 1.0
                    else:
                        e = abs(coef - want_c) / want_c / (4 * SR.U)
                        ok_c = e <= 1.0
                if with_norm:
                    rs.append((tag + ".norm", 0.0 if ok_n else 1.0, 0.0, bool(ok_n)))
                    rs.append(_all_ff(tag + ".gap", scal[3:4]))
                else:
                    rs.append(_all_ff(tag + ".gap", scal[2:4]))
                rs.append((tag + ".coef", e if ok_c else max(e, 2.0), 1.0, bool(ok_c)))
    return rs


# ------------------------------------------------------------------------------------------------ operand casts (exact: a cast has one right answer)
def _sliced(shape, dtype, pad=8):
    """(wide 0xFF buffer, its column slice [:, pad:pad + cols], the columns either side of the slice)."""
    wide = _blank((shape[0], shape[1] + 2 * pad), dtype)
    return wide, wide[:, pad:pad + shape[1]], (wide[:, :pad], wide[:, pad + shape[1]:])


def check_cast_weight_edges():
    """tav_cast_weight around its 32 x 32 tile: one row, one past / one short of a tile in either direction, whole tiles; bf16 and f32; dst only,
    dst_t only, both; into dense outputs and into column slices of wider 0xFF buffers whose other columns stay 0xFF."""
    rs = []
    for R, Cc in ((1, 4), (31, 33), (32, 32), (33, 31), (64, 64), (65, 127)):
        w = _rnd(R, Cc, seed=1500)
        for dtype in (torch.bfloat16, torch.float32):
            ref_n, ref_t = w.to(dtype), w.to(dtype).t().contiguous()
            for want_n, want_t in ((True, False), (False, True), (True, True)):
                for sliced in (False, True):
                    tag = f"cast_weight[{R}x{Cc},{dtype},{'n' if want_n else ''}{'t' if want_t else ''},{'sliced' if sliced else 'dense'}]"
                    if sliced:
                        wn, on, gn = _sliced((R, Cc), dtype) if want_n else (None, None, ())
                        wt, ot, gt = _sliced((Cc, R), dtype) if want_t else (None, None, ())
                        n, t = ops.cast_weight(w, dtype, want_n=want_n, want_t=want_t, out_n=on, out_t=ot)
                        rs.append(_all_ff(tag + ".gap", *gn, *gt))
                    else:
                        n, t = ops.cast_weight(w, dtype, want_n=want_n, want_t=want_t)
                    assert (n is not None) == want_n and (t is not None) == want_t
                    if want_n:
                        rs.append(_exact(tag + ".n", n.contiguous(), ref_n))
                    if want_t:
                        rs.append(_exact(tag + ".t", t.contiguous(), ref_t))
    return rs


def check_cast_weights_multi():
    """tav_cast_weights_multi, one launch over a mixed descriptor table (ops.make_cast_descs): the layer layout at H = 64, K = 128 (q / k / v into
    row blocks of one [3H, K] and column blocks of one [K, 3H] buffer, q scaled by ATTN_Q_PRESCALE in dst and NOT in dst_t; the three [1, H] f32
    bias rows into one [3H] vector), a 128 x 192 entry with both copies (the 64 x 64 fast path), the same shape with dst only and with an ld_t
    that is no multiple of 4 (both must take the 32 x 32 path), a ragged 65 x 100 and an f32 -> f32 entry.  blocks_per_tensor 1 (one block
    walks every tile: the LDS tile is reused between iterations), 3, the tile count and 5 more.  Then the same through
    engine.WeightCache.layer: first build, refresh in place after a weight changed, and no launch at all when nothing did."""
    import tav_amd.engine as engine
    H, K = 64, 128
    bf = torch.bfloat16
    qs = ops.ATTN_Q_PRESCALE
    wq, wk, wv = (_rnd(H, K, seed=1600 + j) for j in range(3))
    bq, bk, bv = (_rnd(1, H, seed=1610 + j) for j in range(3))
    big, rag, w32 = _rnd(128, 192, seed=1620), _rnd(65, 100, seed=1621), _rnd(40, 72, seed=1622)
    n_qkv, t_qkv, bias = _blank((3 * H, K), bf), _blank((K, 3 * H), bf), _blank((3 * H,), torch.float32)
    bufs = [n_qkv, t_qkv, bias]

    def new(shape, dtype):
        bufs.append(_blank(shape, dtype))
        return bufs[-1]

    ents, want = [], []                                               # want: (name, tensor the launch wrote, expected)
    for j, (w, b) in enumerate(((wq, bq), (wk, bk), (wv, bv))):
        sc = qs if j == 0 else None
        f = qs if j == 0 else 1.0
        ents.append((w, n_qkv[j * H:(j + 1) * H], t_qkv[:, j * H:(j + 1) * H], sc))
        want.append((f"qkv{j}.n", ents[-1][1], (w * f).to(bf)))
        want.append((f"qkv{j}.t", ents[-1][2], w.to(bf).t()))
        ents.append((b, bias[j * H:(j + 1) * H].view(1, H), None, sc))
        want.append((f"bias{j}", ents[-1][1], b * f))
    ents.append((big, new((128, 192), bf), new((192, 128), bf)))                                   # fast path
    want += [("fast.n", ents[-1][1], big.to(bf)), ("fast.t", ents[-1][2], big.to(bf).t())]
    ents.append((big, new((128, 192), bf), None))                                                  # dst only: slow path
    want.append(("dst_only.n", ents[-1][1], big.to(bf)))
    wide_t = new((192, 128 + 6), bf)                                                               # ld_t = 134: slow path
    ents.append((big, new((128, 192), bf), wide_t[:, :128]))
    assert ents[-1][2].stride(0) % 4 != 0
    want += [("odd_ld_t.n", ents[-1][1], big.to(bf)), ("odd_ld_t.t", ents[-1][2], big.to(bf).t())]
    ents.append((rag, new((65, 100), bf), new((100, 65), bf)))
    want += [("ragged.n", ents[-1][1], rag.to(bf)), ("ragged.t", ents[-1][2], rag.to(bf).t())]
    ents.append((w32, new((40, 72), torch.float32), new((72, 40), torch.float32)))
    want += [("f32.n", ents[-1][1], w32), ("f32.t", ents[-1][2], w32.t())]
    descs, tiles = ops.make_cast_descs(ents, DEV)
    descs = _in(descs)
    assert tiles == 4 * 6
    rs = []
    for bpt in (1, 3, tiles, tiles + 5):
        for b_ in bufs:
            _refill(b_)
        ops.cast_weights_multi(descs, len(ents), bpt)
        for name, got, ref in want:
            rs.append(_exact(f"cast_multi[bpt{bpt}].{name}", got.contiguous(), ref.contiguous()))
        rs.append(_all_ff(f"cast_multi[bpt{bpt}].gap", wide_t[:, 128:]))
    # ---- engine.WeightCache.layer at the same sizes (weights that change in place are plain tensors: guarded operands must stay what they were)
    g = torch.Generator(device="cpu").manual_seed(1630)
    wo, w1, w2 = (torch.randn(s, generator=g).to(DEV) for s in ((128, 64), (128, 192), (65, 100)))
    cache = engine.WeightCache(engine.Policy("bf16"))
    args = (wq, wk, wv, bq.view(H), bk.view(H), bv.view(H), wo, w1, w2)

    def refs():
        r_n = torch.cat([(wq * qs).to(bf), wk.to(bf), wv.to(bf)])
        r_t = torch.cat([wq.to(bf).t(), wk.to(bf).t(), wv.to(bf).t()], 1)
        r_b = torch.cat([bq.view(H) * qs, bk.view(H), bv.view(H)])
        out = [r_n, r_t, r_b]
        for w in (wo, w1, w2):
            out += [w.to(bf), w.to(bf).t().contiguous()]
        return out

    names = ("Wqkv", "Wqkv_t", "bias_qkv", "Wo", "Wo_t", "W1", "W1_t", "W2", "W2_t")
    val = cache.layer(*args, q_scale=qs)
    assert len(val) == 9
    for name, got, ref in zip(names, val, refs()):
        rs.append(_exact(f"weight_cache.layer.{name}", got, ref))
    ptrs = [t.data_ptr() for t in val]
    w1.mul_(-1.5)
    engine.bump_weight_epoch()
    val2 = cache.layer(*args, q_scale=qs)
    same = [t.data_ptr() for t in val2] == ptrs
    rs.append(("weight_cache.layer refresh keeps its buffers", 0.0 if same else 1.0, 0.0, bool(same)))
    for name, got, ref in zip(names, val2, refs()):
        rs.append(_exact(f"weight_cache.layer.refreshed.{name}", got, ref))
    val2[5].fill_(7.0)                                                # a sentinel in W1: a call with nothing changed must not launch the refresh
    val3 = cache.layer(*args, q_scale=qs)
    same = [t.data_ptr() for t in val3] == ptrs
    rs.append(("weight_cache.layer unchanged call keeps its buffers", 0.0 if same else 1.0, 0.0, bool(same)))
    expect = refs()
    expect[5] = torch.full_like(expect[5], 7.0)
    for name, got, ref in zip(names, val3, expect):
        rs.append(_exact(f"weight_cache.layer.unchanged.{name}", got, ref))
    return rs


def check_cast_conv_weight():
    """tav_cast_conv_weight: dst [co][k][ci], dst_t [k * ci][co] and every per-phase block, each built here element by element from the formula
    in include/tavhip.h (ph_r[ci][q' co + c] = W[c][ci][r + (Q_r - 1 - q') s], Q_r = ceil((k - r) / s), blocks back to back); every output is
    co ci k elements inside a longer 0xFF buffer whose tail stays 0xFF (so the phase buffer is fully written and nothing lands past it)."""
    L = ops.lib()
    rs = []
    for co, ci, k, s in ((8, 4, 3, 2), (8, 4, 2, 2), (5, 3, 3, 1), (6, 2, 5, 3), (4, 4, 1, 1), (8, 4, 10, 5)):
        g = torch.Generator(device="cpu").manual_seed(1700 + co * ci * k + s)
        W = torch.randn(co, ci, k, generator=g)
        n = co * ci * k
        e_n, e_t, e_ph = [0.0] * n, [0.0] * n, []
        for c in range(co):
            for i in range(ci):
                for j in range(k):
                    e_n[(c * k + j) * ci + i] = W[c, i, j].item()
                    e_t[(j * ci + i) * co + c] = W[c, i, j].item()
        for r in range(s):
            Q = (k - r + s - 1) // s
            for i in range(ci):
                for q_ in range(Q):
                    for c in range(co):
                        e_ph.append(W[c, i, r + (Q - 1 - q_) * s].item())
        assert len(e_ph) == n
        w_dev = _in(W.to(DEV))
        for dtype in (torch.bfloat16, torch.float32):
            outs = [_blank((n + 64,), dtype) for _ in range(3)]
            ops.check(L.tav_cast_conv_weight(ops.ptr(w_dev), co, ci, k, ops.ptr(outs[0]), ops.ptr(outs[1]), ops.ptr(outs[2]), s, ops.dt(dtype), ops.stream()),
                      "cast_conv_weight")
            tag = f"cast_conv_weight[co{co},ci{ci},k{k},s{s},{dtype}]"
            for name, got, e in zip(("dst", "dst_t", "dst_phase"), outs, (e_n, e_t, e_ph)):
                rs.append(_exact(f"{tag}.{name}", got[:n], torch.tensor(e, dtype=torch.float32).to(DEV).to(dtype)))
            rs.append(_all_ff(tag + ".tail", *[o[n:] for o in outs]))
            only = _blank((n + 64,), dtype)                           # the phase operand alone (dst = dst_t = NULL)
            ops.check(L.tav_cast_conv_weight(ops.ptr(w_dev), co, ci, k, None, None, ops.ptr(only), s, ops.dt(dtype), ops.stream()), "cast_conv_weight")
            rs.append(_exact(tag + ".dst_phase alone", only[:n], outs[2][:n]))
            rs.append(_all_ff(tag + ".dst_phase alone.tail", only[n:]))
    return rs


# ------------------------------------------------------------------------------------------------ fp8 states
def _e4m3_bytes(x_f32):
    return x_f32.to(torch.float8_e4m3fn).view(torch.uint8)


def _fp8_state(a0):
    """{448 / a0, a0 / 448, a0, 0} divided in f32, in a 0xFF buffer of 6 floats (the two after the state must stay 0xFF)."""
    buf = _blank((6,), torch.float32)
    a = torch.tensor(float(a0), dtype=torch.float32)
    buf[:4] = torch.stack([torch.tensor(448.0) / a, a / torch.tensor(448.0), a, torch.tensor(0.0)]).to(DEV)
    return buf


def _quantize_delayed(x, state, want_q, want_t):
    rows, cols = x.shape
    rows_pad = (rows + ops.FP8_KPAD - 1) // ops.FP8_KPAD * ops.FP8_KPAD
    q = _blank((rows, cols), torch.uint8) if want_q else None
    qt = _blank((cols, rows_pad), torch.uint8) if want_t else None
    ops.check(ops.lib().tav_fp8_quantize_delayed(ops.ptr(x), ops.dt(x), rows, cols, x.stride(0), ops.ptr(state), ops.ptr(q), cols, ops.ptr(qt), rows_pad, rows_pad,
                                                 ops.stream()), "fp8_quantize_delayed")
    return q, qt


def _tie_values(dtype):
    """(inputs, the e4m3 values round-to-nearest-even gives them), both f32: the midpoints 17 (16 | 18), 19 (18 | 20), 2^-10 (0 | 2^-9, the smallest
    subnormal), 3 * 2^-10 (2^-9 | 2^-8), 432 (416 | 448), both signs, and for f32 inputs their neighbours one f32 ulp either side (those are no
    bf16 values); padded with zeros to a multiple of 8 (32 values for f32, 16 for bf16)."""
    xs, es = [], []
    for mid, lo, hi, even in ((17.0, 16.0, 18.0, 16.0), (19.0, 18.0, 20.0, 20.0), (2.0 ** -10, 0.0, 2.0 ** -9, 0.0),
                              (3 * 2.0 ** -10, 2.0 ** -9, 2.0 ** -8, 2.0 ** -8), (432.0, 416.0, 448.0, 448.0)):
        m32 = np.float32(mid)
        for sign in (1.0, -1.0):
            if dtype == torch.float32:
                xs += [sign * float(np.nextafter(m32, np.float32(0))), sign * mid, sign * float(np.nextafter(m32, np.float32(1e9)))]
                es += [sign * lo, sign * even, sign * hi]
            else:
                xs.append(sign * mid)
                es.append(sign * even)
    pad = -len(xs) % 8
    return torch.tensor(xs + [0.0] * pad, dtype=torch.float32), torch.tensor(es + [0.0] * pad, dtype=torch.float32)


def check_fp8_delayed(dtype):
    """tav_fp8_quantize_delayed on a hand-made state {448 / a0, a0 / 448, a0, 0} with a0 = 2 amax(x) and a0 = amax(x) / 2 (half the range
    saturates): q == clamp(x state[0], +-448) in e4m3 as bytes, qt its transpose zero padded to rows_pad, state[0..2] untouched, state[3] ==
    amax(x) bit for bit, unchanged by a second tensor of smaller magnitude, 0 for an all-zero tensor.  q only takes the streaming kernel
    where cols % 8 == 0 and the tiled one otherwise, q + qt the tiled one; x dense and with a wider row pitch.  Then ties and e4m3 subnormals
    at a scale of exactly 1."""
    rs = []
    for rows, cols in ((1, 4), (1, 8), (33, 136), (129, 1032), (1025, 132)):
        for pitch in (0, 16):
            gen = torch.Generator(device="cpu").manual_seed(1800 + rows + cols)
            x = _in(torch.randn(rows, cols, generator=gen).to(DEV).to(dtype), pitch)
            amax = x.float().abs().max()
            for fac in (2.0, 0.5):
                for want_t in (False, True):
                    state = _fp8_state(float(amax.item()) * fac)
                    s0 = state.clone()
                    q, qt = _quantize_delayed(x, state, True, want_t)
                    ref = _e4m3_bytes((x.float() * state[0]).clamp(-448.0, 448.0))
                    tag = f"fp8.delayed[{dtype},{rows}x{cols},pitch+{pitch},a0={fac:g}amax,{'q+qt' if want_t else 'q'}]"
                    rs.append(_exact(tag + ".q", q, ref))
                    if fac < 1.0:                                   # (the largest element itself lands at twice the range)
                        sat = int((ref & 0x7F).eq(0x7E).sum().item())   # 0x7e = 448: the clip really is exercised
                        rs.append((tag + ".saturated elements present", float(sat), 0.0, sat > 0))
                    if want_t:
                        rs.append(_exact(tag + ".qt", qt[:, :rows].contiguous(), ref.t().contiguous()))
                        pad = int(qt[:, rows:].ne(0).sum().item())
                        rs.append((tag + ".qt_pad bytes zero", float(pad), 0.0, pad == 0))
                    rs.append(_exact(tag + ".state[0:3] unchanged", _bits(state[:3]), _bits(s0[:3])))
                    rs.append(_exact(tag + ".state[3] == amax", _bits(state[3:4]), _bits(amax.reshape(1))))
                    rs.append(_all_ff(tag + ".gap", state[4:]))
                    if want_t:
                        continue
                    small = _in((x.float() * 0.5).to(dtype), pitch)
                    _quantize_delayed(small, state, True, False)
                    rs.append(_exact(tag + ".state[3] kept by a smaller tensor", _bits(state[3:4]), _bits(amax.reshape(1))))
        zero = _in(torch.zeros(rows, cols, dtype=dtype, device=DEV))
        for want_t in (False, True):
            state = _fp8_state(1.0)
            q, qt = _quantize_delayed(zero, state, True, want_t)
            tag = f"fp8.delayed[{dtype},{rows}x{cols},zeros,{'q+qt' if want_t else 'q'}]"
            z = int(q.ne(0).sum().item()) + (int(qt.ne(0).sum().item()) if want_t else 0)
            rs.append((tag + ".bytes zero", float(z), 0.0, z == 0))
            rs.append(_exact(tag + ".state[3] stays 0", _bits(state[3:4]), _bits(torch.zeros(1, device=DEV))))
    xs, es = _tie_values(dtype)
    for shape, want_t in (((1, xs.numel()), False), ((xs.numel() // 4, 4), False), ((xs.numel() // 4, 4), True)):
        x = _in(xs.view(shape).to(DEV).to(dtype))
        assert torch.equal(x.float().cpu(), xs.view(shape))
        state = _fp8_state(448.0)
        assert float(state[0].item()) == 1.0
        q, qt = _quantize_delayed(x, state, True, want_t)
        tag = f"fp8.delayed.ties[{dtype},{shape[0]}x{shape[1]},{'q+qt' if want_t else 'q'}]"
        rs.append(_exact(tag + ".q", q, _e4m3_bytes(es.view(shape).to(DEV))))
        if want_t:
            rs.append(_exact(tag + ".qt", qt[:, :shape[0]].contiguous(), _e4m3_bytes(es.view(shape).to(DEV)).t().contiguous()))
    return rs


def check_fp8_quantize_ties():
    """The plain quantiser (tav_fp8_quantize) at a scale of exactly 1 on the same midpoints, neighbours and subnormals, streaming and tiled kernel;
    ops.fp8_quantize of an all-zero tensor: scales (1, 1, 0), every byte zero."""
    L = ops.lib()
    rs = []
    for dtype in (torch.float32, torch.bfloat16):
        xd, ed = _tie_values(dtype)
        for shape, want_t in (((1, xd.numel()), False), ((xd.numel() // 4, 4), False), ((xd.numel() // 4, 4), True)):
            x = _in(xd.view(shape).to(DEV).to(dtype))
            rows, cols = shape
            rows_pad = ops.FP8_KPAD
            scales = _in(torch.tensor([1.0, 1.0, 448.0], device=DEV))
            q = _blank(shape, torch.uint8)
            qt = _blank((cols, rows_pad), torch.uint8) if want_t else None
            ops.check(L.tav_fp8_quantize(ops.ptr(x), ops.dt(x), rows, cols, x.stride(0), ops.ptr(scales), ops.ptr(q), cols, ops.ptr(qt), rows_pad, rows_pad,
                                         ops.stream()), "fp8_quantize")
            tag = f"fp8.ties[{dtype},{rows}x{cols},{'q+qt' if want_t else 'q'}]"
            ref = _e4m3_bytes(ed.view(shape).to(DEV))
            rs.append(_exact(tag + ".q", q, ref))
            rs.append(_exact(tag + ".torch's own conversion agrees", _e4m3_bytes(x.float()), ref))
            if want_t:
                rs.append(_exact(tag + ".qt", qt[:, :rows].contiguous(), ref.t().contiguous()))
        f = ops.fp8_quantize(_in(torch.zeros(33, 132, dtype=dtype, device=DEV)), want_t=True)
        tag = f"fp8.zeros[{dtype}]"
        rs.append(_exact(tag + ".scales (1, 1, 0)", f.scales[:3], torch.tensor([1.0, 1.0, 0.0], device=DEV)))
        z = int(f.q.view(torch.uint8).ne(0).sum().item()) + int(f.qt.view(torch.uint8).ne(0).sum().item())
        rs.append((tag + ".bytes zero", float(z), 0.0, z == 0))
    return rs


def check_fp8_roll_states():
    """tav_fp8_roll_states over n in {1, 255, 257} states: a state whose running maximum m = state[3] moved (0 < m < 3e38) becomes
    {448 / m, m / 448, m, 0}, divided in f32; one at 0, +inf or NaN keeps its first three words; every state[3] is 0 afterwards; the 0xFF
    bytes after the last state are untouched."""
    L = ops.lib()
    inf, nan = float("inf"), float("nan")
    rs = []
    for n, kinds in ((1, "m"), (1, "0"), (1, "i"), (1, "n"), (255, None), (257, None)):
        g = torch.Generator(device="cpu").manual_seed(1900 + n)
        st = torch.rand(n, 4, generator=g) * 10 + 0.01
        m = 10.0 ** (torch.rand(n, generator=g) * 12 - 6)
        kind = list(kinds) if kinds else ["0" if i % 3 == 0 else "m" for i in range(n)]
        if kinds is None:
            kind[7], kind[n - 1], kind[n - 2] = "i", "n", "m"
        for i, k_ in enumerate(kind):
            st[i, 3] = {"m": float(m[i]), "0": 0.0, "i": inf, "n": nan}[k_]
        buf = _blank((n + 2, 4), torch.float32)
        buf[:n] = st.to(DEV)
        ops.check(L.tav_fp8_roll_states(ops.ptr(buf), n, ops.stream()), "fp8_roll_states")
        want = st.clone()
        moved = torch.tensor([k_ == "m" for k_ in kind])
        mm = st[:, 3]
        want[moved, 0] = torch.tensor(448.0) / mm[moved]
        want[moved, 1] = mm[moved] / torch.tensor(448.0)
        want[moved, 2] = mm[moved]
        want[:, 3] = 0.0
        tag = f"fp8.roll_states[n{n}{',' + kinds if kinds else ''}]"
        rs.append(_exact(tag, _bits(buf[:n]), _bits(want.to(DEV))))
        rs.append(_all_ff(tag + ".tail", buf[n:]))
    return rs


def step_end_checks():
    """The step-end cases, in the order all_checks() appends them."""
    out = []
    for list_name in SR.SIZE_LISTS:
        for layout in _LAYOUTS:
            for wd in (SR.WD, 0.0):
                out.append(lambda a=(list_name, layout, wd): check_optimizer_step(*a))
    out += [check_grad_norm, check_clip_coef, check_cast_weight_edges, check_cast_weights_multi, check_cast_conv_weight,
            lambda: check_fp8_delayed(torch.float32), lambda: check_fp8_delayed(torch.bfloat16), check_fp8_roll_states]
    return out


# ------------------------------------------------------------------------------------------------ GEMM family against fp64 ("GEMM checks")
# Two instruments on top of the _res cases above, which stay as they are.  (1) Per-element bounds: operands with spread magnitudes, the fp64
# reference of the documented epilogue and a bound per output element from tests/gemm_ref.py; err = worst |got - ref| / bound, tol = 1.  (2) Exact
# integers: operands in {-7 .. 7}, every partial sum an integer below 2^24 in any order, so the result has ONE right answer (_exact).
_GDT = {torch.bfloat16: "bf16", torch.float32: "f32"}
_TDT = {"bf16": torch.bfloat16, "f32": torch.float32}


def _up(x, dtype):
    """A numpy array of values the dtype holds exactly -> a (guarded) device tensor of that dtype."""
    return _in(torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dtype))


def _bounded(name, got, ref, bound):
    r = GR.ratio(got.detach().double().cpu().numpy(), ref, bound)
    return (name, r, 1.0, bool(r <= 1.0))


@functools.lru_cache(maxsize=None)
def _nt_problem(dname, M, N, K, seed=0):
    return GR.nt_inputs(M, N, K, dname, seed=seed + 7 * M + 3 * N + K)


@functools.lru_cache(maxsize=None)
def _nt_reference(dname, M, N, K, flavour):
    return GR.nt_ref(_nt_problem(dname, M, N, K), **GR.FLAVOURS[flavour])


_NT_FEW = ("bias", "bias+resid->f32", "act3", "gelu_in.act4", "accumulate->f32", "act1+pre->f32")


def _nt_flavours(dtype, names):
    """f32 operands store f32 only: their "->f32" twins would be the same launch twice."""
    return [n for n in names if dtype != torch.float32 or not n.endswith("->f32")]


def check_gemm_nt_bounded(dtype, hint, M=333, N=384, K=256, flavours=None):
    """tav_gemm_nt, every epilogue flavour of gemm_ref.FLAVOURS, each output element (C and C_pre) within its own bound."""
    dname = _GDT[dtype]
    x = _nt_problem(dname, M, N, K)
    a, b = _up(x["a"], dtype), _up(x["b"], dtype)
    rs = []
    for name in _nt_flavours(dtype, flavours or tuple(GR.FLAVOURS)):
        kw = GR.FLAVOURS[name]
        ref = _nt_reference(dname, M, N, K, name)
        odt = torch.float32 if (dtype == torch.float32 or kw.get("out_dtype") == "f32") else torch.bfloat16
        args = dict(tile_m=hint, out_dtype=odt, act=kw.get("act", 0), want_pre=kw.get("want_pre", False), alpha=kw.get("alpha", 1.0))
        if kw.get("bias"):
            args["bias"] = _up(x["bias"], torch.float32)
        if kw.get("resid"):
            args["resid"] = _up(x["resid"], torch.float32)
        if kw.get("gelu_in"):
            args["gelu_in"] = _up(x[kw["gelu_in"]], dtype)
        if kw.get("accumulate"):
            out = _blank((M, N), odt)
            out.copy_(torch.from_numpy(x["cprev_" + ("f32" if odt == torch.float32 else "bf16")]).to(DEV).to(odt))
            args.update(out=out, accumulate=True)
        res = ops.gemm_nt(a, b, **args)
        out, pre = res if isinstance(res, tuple) else (res, None)
        tag = f"gemm_nt.bound[{dname},tm{hint},M{M},N{N},K{K},{name}]"
        rs.append(_bounded(tag, out, ref["out"], ref["out_bound"]))
        if pre is not None:
            rs.append(_bounded(tag + ".pre", pre, ref["pre"], ref["pre_bound"]))
    return rs


def check_gemm_nt_bounded_shapes(dtype):
    """The shapes around the main loop and the tile edges: every prologue / tail length of the 256 x 256 tile's 3 + 2 image ring (1, 2, 3 and 5
    K-tiles), the longest K of the per-element cases, and M = 1, tile - 1, tile + 1 (bf16: hints 8 and 16; f32 has the 128-wide tiles only)."""
    rs = []
    if dtype == torch.bfloat16:
        for K in (64, 128, 192, 320):
            rs += check_gemm_nt_bounded(dtype, 16, M=300, N=260, K=K, flavours=_NT_FEW)
        for hint in (8, 16):
            rs += check_gemm_nt_bounded(dtype, hint, M=513, N=132, K=1536, flavours=_NT_FEW)
        for M in (1, 255, 257):
            rs += check_gemm_nt_bounded(dtype, 16, M=M, N=260, K=128, flavours=_NT_FEW)
    else:
        rs += check_gemm_nt_bounded(dtype, 0, M=513, N=132, K=1536, flavours=_NT_FEW)
        for M in (1, 127, 129):
            rs += check_gemm_nt_bounded(dtype, 4, M=M, N=260, K=128, flavours=_NT_FEW)
    return rs


def check_gemm_nt_bounded_batched(dtype, nzb=2, nzg=3, M=70, N=132, K=128):
    """One call with nzb x nzg slices: A and C stride over both, B and the bias over the group only."""
    dname = _GDT[dtype]
    probs = [[_nt_problem(dname, M, N, K, seed=100 + 10 * zb + zg) for zg in range(nzg)] for zb in range(nzb)]
    a = _up(np.stack([np.stack([probs[zb][zg]["a"] for zg in range(nzg)]) for zb in range(nzb)]), dtype)
    b = _up(np.stack([probs[0][zg]["b"] for zg in range(nzg)]), dtype)
    bias = _up(np.stack([probs[0][zg]["bias"] for zg in range(nzg)]), torch.float32)
    out = ops.gemm_nt(a, b, bias=bias, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, nzb=nzb, nzg=nzg, a_zb=nzg * M * K, a_zg=M * K, b_zg=N * K,
                      c_zb=nzg * M * N, c_zg=M * N, bias_zg=N, out_shape=(nzb, nzg, M, N))
    rs = []
    for zb in range(nzb):
        for zg in range(nzg):
            x = dict(probs[zb][zg], b=probs[0][zg]["b"], bias=probs[0][zg]["bias"])
            ref = GR.nt_ref(x, bias=True)
            rs.append(_bounded(f"gemm_nt.bound.batched[{dname},zb{zb},zg{zg}]", out[zb, zg], ref["out"], ref["out_bound"]))
    return rs


def _int_dev(shape, seed, dtype=torch.float32):
    return _in(torch.from_numpy(GR.int_tensor(shape, seed)).to(DEV).to(dtype))


def _exact_both(tag, run, want):
    """run(out_dtype) against the exact integer result `want` (fp64): f32 bit for bit, bf16 its round-to-nearest-even."""
    return [_exact(tag + "->f32", run(torch.float32), want.float()), _exact(tag + "->bf16", run(torch.bfloat16), want.float().to(torch.bfloat16))]


def check_gemm_nt_int(dtype, hint, M=333, N=384, K=256):
    """Exact integer operands (bf16 / f32) with an integer bias: no tolerance."""
    assert GR.int_exact_ok(K)
    a, b, bias = _int_dev((M, K), 1000 + K, dtype), _int_dev((N, K), 2000 + K, dtype), _int_dev((N,), 3000 + K)
    want = a.double() @ b.double().t() + bias.double()
    tag = f"gemm_nt.int[{_GDT[dtype]},tm{hint},M{M},N{N},K{K}]"
    if dtype == torch.float32:
        return [_exact(tag, ops.gemm_nt(a, b, bias=bias, tile_m=hint), want.float())]
    return _exact_both(tag, lambda odt: ops.gemm_nt(a, b, bias=bias, tile_m=hint, out_dtype=odt), want)


def check_gemm_nt_int_all(dtype):
    """Every tile hint at the shape of the per-element cases, the ring and edge shapes of the 256 x 256 tile, and one case at K = 3072."""
    rs = []
    for hint in (0, 2, 3, 4, 17) + ((8, 16) if dtype == torch.bfloat16 else ()):
        rs += check_gemm_nt_int(dtype, hint)
    if dtype == torch.bfloat16:
        for K in (64, 128, 192, 320):
            rs += check_gemm_nt_int(dtype, 16, M=300, N=260, K=K)
        for hint in (8, 16):
            rs += check_gemm_nt_int(dtype, hint, M=513, N=132, K=3072)
    else:
        rs += check_gemm_nt_int(dtype, 0, M=513, N=132, K=3072)
    return rs


def check_gemm_nt_int_mixed_schedule(M=46848 + 37, N=768, K=768):
    """The two-launch schedule of check_gemm_nt_mixed_schedule against the TRUTH, not only against the single-tile launch."""
    assert GR.int_exact_ok(K)
    a, b, bias = _int_dev((M, K), 41, torch.bfloat16), _int_dev((N, K), 42, torch.bfloat16), _int_dev((N,), 43)
    want = a.double() @ b.double().t() + bias.double()
    return _exact_both(f"gemm_nt.int.mixed[M{M},N{N},K{K}]", lambda odt: ops.gemm_nt(a, b, bias=bias, out_dtype=odt), want)


def check_fp8_int(M, N, K, tile_m):
    """fp8 operands from integers with amax = 7: the quantisation scale is 64 and the dequantisation factor 2^-6, both exact, so q = 64 x and the
    GEMM with its dequantisation scales has one right answer."""
    assert GR.int_exact_ok(K)
    ops.clear_workspaces()
    x, w, bias = _int_dev((M, K), 5000 + K, torch.bfloat16), _int_dev((N, K), 6000 + K), _int_dev((N,), 7000 + K)
    x8, w8 = ops.fp8_quantize(x), ops.fp8_quantize(w)
    tag = f"fp8.int[M{M},N{N},K{K},tm{tile_m}]"
    rs = [_exact(tag + ".scales", torch.stack([x8.scales[:3], w8.scales[:3]]), torch.tensor([[64.0, 2.0 ** -6, 7.0]] * 2, device=DEV)),
          _exact(tag + ".q", x8.q.float(), x.float() * 64.0)]
    want = x.double() @ w.double().t() + bias.double()
    return rs + _exact_both(tag, lambda odt: ops.gemm_nt_fp8(x8, w8, bias=bias, out_dtype=odt, tile_m=tile_m), want)


def check_wgrad_fp8_int(T=333, N1=132, N2=256):
    """ops.wgrad_fp8 (the NT GEMM of the zero-padded transposed copies in eight K-slices plus tav_splitk_reduce) on integer operands: exact."""
    ops.clear_workspaces()
    rows_pad = (T + ops.FP8_KPAD - 1) // ops.FP8_KPAD * ops.FP8_KPAD
    assert GR.int_exact_ok(rows_pad)
    dy, x = _int_dev((T, N1), 8001, torch.bfloat16), _int_dev((T, N2), 8002, torch.bfloat16)
    dy8, x8 = ops.fp8_quantize(dy, want_q=False, want_t=True), ops.fp8_quantize(x, want_t=True)
    return [_exact(f"fp8.int.wgrad[T{T},N1{N1},N2{N2}]", ops.wgrad_fp8(dy8, x8), (dy.double().t() @ x.double()).float())]


# ---- weight gradients
def _tn_call(a, b, N1, N2, rows, nbatch, *, chunk_rows=0, scale=1.0, accumulate=False, perm=(0, 0), out=None, dbias=None):
    """tav_gemm_tn through the C ABI (ops.gemm_tn chooses the split and allocates dbias itself: here the caller may force chunk_rows and hand in
    the tensors an accumulating call adds to).  -> (out, dbias, nsplit)."""
    import ctypes as C
    cr, ns = C.c_int32(), C.c_int32()
    ops.check(ops.lib().tav_gemm_tn_splits(N1, N2, rows, nbatch, C.byref(cr), C.byref(ns)), "gemm_tn_splits")
    if chunk_rows:
        cr.value, ns.value = chunk_rows, nbatch * ((rows + chunk_rows - 1) // chunk_rows)
    g = ops.L.GemmTNArgs()
    out = out if out is not None else _blank((N1, N2), torch.float32)
    dbias = dbias if dbias is not None else _blank((N1,), torch.float32)
    slabs, bpart = ops.workspace("tn_slabs", ns.value * N1 * N2, a.device), ops.workspace("tn_bias", ns.value * N1, a.device)
    g.A, g.B, g.slabs, g.out, g.dbias, g.bias_partials = ops.ptr(a), ops.ptr(b), ops.ptr(slabs), ops.ptr(out), ops.ptr(dbias), ops.ptr(bpart)
    g.N1, g.N2, g.lda, g.ldb, g.rows_per_batch, g.nbatch, g.a_zb, g.b_zb = N1, N2, N1, N2, rows, nbatch, rows * N1, rows * N2
    g.chunk_rows, g.nsplit, g.perm_inner, g.perm_outer = cr.value, ns.value, perm[0], perm[1]
    g.dtype, g.accumulate, g.scale = ops.dt(a), int(accumulate), scale
    ops.check(ops.lib().tav_gemm_tn(C.byref(g), ops.stream()), "gemm_tn")
    return out, dbias, ns.value


@functools.lru_cache(maxsize=None)
def _tn_problem(dname, T, N1, N2, seed=0):
    return GR.tn_inputs(T, N1, N2, dname, seed=seed + T + 3 * N1 + 5 * N2)


_TN_VARIANTS = [("plain", dict(), 0), ("chunk64,scale", dict(scale=0.37), 64), ("accumulate,scale", dict(scale=-1.7, accumulate=True), 0),
                ("conv perm", dict(perm=(88, 3)), 0), ("conv perm,chunk64,accumulate", dict(perm=(88, 3), accumulate=True), 64)]


def check_gemm_tn_bounded(dtype, rows, nbatch=1, N1=136, N2=264):
    """tav_gemm_tn: the library's own split and one chunk per 64 rows, scale != 1, accumulate into out AND dbias, the conv-style column
    permutation (N2 = 3 taps x 88 channels); out and dbias per element."""
    dname = _GDT[dtype]
    x = _tn_problem(dname, rows * nbatch, N1, N2)
    a, b = _up(x["a"], dtype), _up(x["b"], dtype)
    rs = []
    for name, kw, chunk in _TN_VARIANTS:
        ops.clear_workspaces()
        out = dbias = None
        if kw.get("accumulate"):
            out, dbias = _blank((N1, N2), torch.float32), _blank((N1,), torch.float32)
            out.copy_(torch.from_numpy(x["prev"]).to(DEV))
            dbias.copy_(torch.from_numpy(x["prev_b"]).to(DEV))
        out, dbias, ns = _tn_call(a, b, N1, N2, rows, nbatch, chunk_rows=chunk, out=out, dbias=dbias, **kw)
        ref = GR.tn_ref(x, nsplit=ns, **kw)
        tag = f"gemm_tn.bound[{dname},rows{rows},nb{nbatch},{name},splits{ns}]"
        rs += [_bounded(tag, out, ref["out"], ref["out_bound"]), _bounded(tag + ".dbias", dbias, ref["dbias"], ref["dbias_bound"])]
    return rs


def check_gemm_tn_int(dtype, rows, nbatch=1, N1=136, N2=264):
    assert GR.int_exact_ok(rows * nbatch)
    a, b = _int_dev((rows * nbatch, N1), 9001 + rows, dtype), _int_dev((rows * nbatch, N2), 9002 + rows, dtype)
    want, want_b = (a.double().t() @ b.double()).float(), a.double().sum(0).float()
    rs = []
    for name, perm, chunk in (("plain", (0, 0), 0), ("chunk64", (0, 0), 64), ("conv perm", (88, 3), 0)):
        ops.clear_workspaces()
        out, dbias, ns = _tn_call(a, b, N1, N2, rows, nbatch, chunk_rows=chunk, perm=perm)
        p = torch.from_numpy(GR.tn_perm(N2, *perm)).to(DEV)
        tag = f"gemm_tn.int[{_GDT[dtype]},rows{rows},nb{nbatch},{name},splits{ns}]"
        rs += [_exact(tag, out[:, p], want), _exact(tag + ".dbias", dbias, want_b)]
    return rs


_GROUP_SHAPES = [(384, 136), (136, 264), (256, 512), (520, 128)]


def _grouped_forms(dtype, rows):
    """(name, flags | None = the workspace-free tav_gemm_tn_grouped, upper limit of slab additions) of every form the library accepts here."""
    forms = [("plain", None, 1), ("ws", 0, 1), ("ws.flag2", 2, 1)]
    if dtype == torch.bfloat16:
        for nsplit in (1, 2, 3):
            if (nsplit - 1) * (((rows + nsplit - 1) // nsplit + 63) // 64 * 64) < rows:           # (the library refuses an empty split)
                forms.append((f"ws.flag1.splits{nsplit}", 1 | (nsplit << 8), nsplit))
    return forms


def _grouped_run(pairs, flags):
    if flags is not None:
        return ops.gemm_tn_grouped(pairs, want_bias=True, flags=flags)
    n = len(pairs)
    probs, outs = (ops.L.GemmTNProblem * n)(), []
    for k, (a, b) in enumerate(pairs):
        dW, db = _blank((a.shape[1], b.shape[1]), torch.float32), _blank((a.shape[1],), torch.float32)
        pr = probs[k]
        pr.A, pr.B, pr.out, pr.dbias = ops.ptr(a), ops.ptr(b), ops.ptr(dW), ops.ptr(db)
        pr.N1, pr.N2, pr.lda, pr.ldb = a.shape[1], b.shape[1], a.stride(0), b.stride(0)
        outs.append((dW, db))
    ops.check(ops.lib().tav_gemm_tn_grouped(probs, n, pairs[0][0].shape[0], ops.dt(pairs[0][0]), ops.stream()), "gemm_tn_grouped")
    return outs


def check_gemm_tn_grouped_bounded(dtype, rows):
    """tav_gemm_tn_grouped and tav_gemm_tn_grouped_ws (flags 0, 1 with one to three splits, 2): four problems of ragged widths, dW and db of each
    per element.  The bias of a bias-spread launch is summed from splits x tiles_2 partials: that count enters its chain."""
    dname = _GDT[dtype]
    xs = [_tn_problem(dname, rows, n1, n2, seed=50 + k) for k, (n1, n2) in enumerate(_GROUP_SHAPES)]
    pairs = [(_up(x["a"], dtype), _up(x["b"], dtype)) for x in xs]
    rs = []
    for name, flags, nsplit in _grouped_forms(dtype, rows):
        outs = _grouped_run(pairs, flags)
        for k, (x, (dW, db)) in enumerate(zip(xs, outs)):
            ref = GR.tn_ref(x, nsplit=nsplit)
            tag = f"gemm_tn_grouped.bound[{dname},rows{rows},{name}]"
            rs += [_bounded(f"{tag}.dW{k}", dW, ref["out"], ref["out_bound"]), _bounded(f"{tag}.db{k}", db, ref["dbias"], ref["dbias_bound"])]
    return rs


def check_gemm_tn_grouped_fallback(dtype, rows, flags=0):
    """tav_gemm_tn_grouped_ws with a workspace that is too small -- NULL with 0 bytes, and the planned size less 4 bytes -- is
    tav_gemm_tn_grouped: dW and db of four problems of ragged widths, bit for bit against the direct call."""
    import ctypes as C
    pairs = [(_rnd(rows, n1, dtype=dtype, seed=70 + k), _rnd(rows, n2, dtype=dtype, seed=80 + k)) for k, (n1, n2) in enumerate(_GROUP_SHAPES)]
    want = _grouped_run(pairs, None)
    n = len(pairs)
    rs = []
    for form in ("NULL", "4 bytes short"):
        probs, outs = (ops.L.GemmTNProblem * n)(), []
        for k, (a, b) in enumerate(pairs):
            dW, db = _blank((a.shape[1], b.shape[1]), torch.float32), _blank((a.shape[1],), torch.float32)
            pr = probs[k]
            pr.A, pr.B, pr.out, pr.dbias = ops.ptr(a), ops.ptr(b), ops.ptr(dW), ops.ptr(db)
            pr.N1, pr.N2, pr.lda, pr.ldb = a.shape[1], b.shape[1], a.stride(0), b.stride(0)
            outs.append((dW, db))
        nbytes = ops.lib().tav_gemm_tn_grouped_ws_bytes(probs, n, rows, ops.dt(pairs[0][0]), flags)
        assert nbytes > 4, "the plan needs no workspace: nothing to fall back from"
        ws = _blank((nbytes,), torch.uint8) if form != "NULL" else None
        ops.check(ops.lib().tav_gemm_tn_grouped_ws(probs, n, rows, ops.dt(pairs[0][0]), ops.ptr(ws), nbytes - 4 if ws is not None else 0, flags,
                                                   ops.stream()), "gemm_tn_grouped_ws")
        tag = f"gemm_tn_grouped.fallback[{_GDT[dtype]},rows{rows},flags{flags:#x},workspace {form}]"
        for k, ((dW, db), (wW, wb)) in enumerate(zip(outs, want)):
            rs += [_exact(f"{tag}.dW{k}", dW, wW), _exact(f"{tag}.db{k}", db, wb)]
        if ws is not None:                                              # ... and the workspace it was offered stays untouched
            rs.append(_all_ff(f"{tag}.workspace untouched", ws))
    return rs


def check_gemm_tn_grouped_int(dtype, rows):
    assert GR.int_exact_ok(rows)
    pairs = [(_int_dev((rows, n1), 9100 + k, dtype), _int_dev((rows, n2), 9200 + k, dtype)) for k, (n1, n2) in enumerate(_GROUP_SHAPES)]
    wants = [((a.double().t() @ b.double()).float(), a.double().sum(0).float()) for a, b in pairs]
    rs = []
    for name, flags, _ in _grouped_forms(dtype, rows):
        for k, ((dW, db), (wW, wb)) in enumerate(zip(_grouped_run(pairs, flags), wants)):
            tag = f"gemm_tn_grouped.int[{_GDT[dtype]},rows{rows},{name}]"
            rs += [_exact(f"{tag}.dW{k}", dW, wW), _exact(f"{tag}.db{k}", db, wb)]
    return rs


def gemm_fp64_checks():
    """The GEMM cases against fp64, in the order all_checks() appends them."""
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        for hint in (0, 2, 3, 4, 17) + ((8, 16) if dtype == torch.bfloat16 else ()):
            out.append(lambda d=dtype, h=hint: check_gemm_nt_bounded(d, h))
        out.append(lambda d=dtype: check_gemm_nt_bounded_shapes(d))
        out.append(lambda d=dtype: check_gemm_nt_bounded_batched(d))
        out.append(lambda d=dtype: check_gemm_nt_int_all(d))
        for rows, nb in ((64, 1), (130, 1), (777, 1), (249, 3)):
            out.append(lambda d=dtype, r=rows, n=nb: check_gemm_tn_bounded(d, r, n))
            out.append(lambda d=dtype, r=rows, n=nb: check_gemm_tn_int(d, r, n))
        out.append(lambda d=dtype: check_gemm_tn_int(d, 5000))
        for rows in (64, 130, 777):
            out.append(lambda d=dtype, r=rows: check_gemm_tn_grouped_bounded(d, r))
            out.append(lambda d=dtype, r=rows: check_gemm_tn_grouped_int(d, r))
        out.append(lambda d=dtype: check_gemm_tn_grouped_int(d, 5000))
    out.append(check_gemm_nt_int_mixed_schedule)
    # a workspace too small for the plan: tav_gemm_tn_grouped_ws answers with tav_gemm_tn_grouped's bits (at 5000 rows the forced 256-wide
    # form, with bias partials alone and with two slabs per gradient, is what it falls back from)
    for dtype in (torch.float32, torch.bfloat16):
        out.append(lambda d=dtype: check_gemm_tn_grouped_fallback(d, 777))
    for flags in (1, 1 | (2 << 8)):
        out.append(lambda f=flags: check_gemm_tn_grouped_fallback(torch.bfloat16, 5000, f))
    for M, N, K, tm in ((333, 384, 256, 0), (333, 384, 256, 16), (130, 132, 128, 4), (257, 260, 3072, 16)):
        out.append(lambda a=(M, N, K, tm): check_fp8_int(*a))
    out.append(check_wgrad_fp8_int)
    return out


# ================================================================================================= attention against fp64
# tests/attn_ref.py: per-element bounds at operands of spread magnitude, and selections with ONE right answer.
_ALENS_EXACT = {64: [64, 1, 33], 65: [0, 65, 64], 129: [65, 1, 128], 257: [257, 65, 200]}


def _attn_operands(x, dtype):
    """The operands of an attn_ref problem on the device: q / k / v as slices of one qkv buffer with a widened pitch, dO widened too."""
    B, S, nh = x["B"], x["S"], x["nh"]
    H = nh * 64
    qkv = _in(torch.from_numpy(np.concatenate([x[n].reshape(B * S, H) for n in ("q", "k", "v")], 1)).to(DEV).to(dtype), 24)
    do = _in(torch.from_numpy(x["do"].reshape(B * S, H)).to(DEV).to(dtype), 8)
    mask = None if x["mask"] is None else _in(torch.from_numpy(x["mask"]).to(DEV).float())
    return qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], do, mask


def _attn_fwd(x, ops_in, sl):
    q, k, v, _, mask = ops_in
    o, lse, (corr, o_soft) = ops.attn_fwd(q, k, v, x["B"], x["S"], x["nh"], key_mask=mask, mask_mode=x["mode"], q_prescaled=x["pre"], seq_lens=sl)
    return dict(o=o, lse=lse, corr=corr, o_soft=o_soft if o_soft is not None else o)


def _attn_bwd(x, ops_in, sl, o, o_soft, lse, corr, tag):
    """-> (dict dq, dk, dv [B][S][nh][64] views and delta [B][nh][S] with the rows past each length zeroed (not written by contract), gap check)."""
    q, k, v, do, mask = ops_in
    B, S, nh = x["B"], x["S"], x["nh"]
    H = nh * 64
    wide = _blank((B * S, 3 * H + 16), q.dtype)
    dqkv = ops.attn_bwd(q, k, v, o, do, lse, (corr, o_soft) if x["mode"] == 2 else None, B, S, nh, key_mask=mask, mask_mode=x["mode"],
                        q_prescaled=x["pre"], seq_lens=sl, dqkv=wide[:, 8:8 + 3 * H])
    delta = ops.workspace("attn_delta", B * nh * S, q.device)[:B * nh * S].view(B, nh, S).clone()
    for b, L in enumerate(x["lens"]):
        delta[b, :, L:] = 0.0
    got = {n: dqkv[:, j * H:(j + 1) * H].reshape(B, S, nh, 64) for j, n in enumerate(("dq", "dk", "dv"))}
    got["delta"] = delta
    return got, _all_ff(tag + ".dqkv gap", wide[:, :8], wide[:, 8 + 3 * H:])


def _attn_fed(x, fd, dtype):
    B, S, nh = x["B"], x["S"], x["nh"]
    up = lambda a, dt_: _in(torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dt_))      # noqa: E731
    return (up(fd["o"].reshape(B * S, nh * 64), dtype), up(fd["o_soft"].reshape(B * S, nh * 64), dtype), up(fd["lse"], torch.float32),
            up(fd["corr"], torch.float32))


def _attn_lens(lens):
    return None if lens is None else _in(torch.tensor(lens, dtype=torch.int32, device=DEV))


def check_attention_bounded(dtype, S, lens=None, chained=False, B=2, nh=3):
    """tav_attn_fwd / tav_attn_bwd (the _len forms with `lens`), every mask mode, pre-scaled or not: o, o_soft, corr, lse each within its own
    per-element bound of the fp64 reference; the backward ISOLATED (fed the reference's o, o_soft, lse, corr rounded to the storage types): dq, dk,
    dv and the delta workspace within theirs.  chained: the backward fed the kernel's own forward, against the composed bounds."""
    dname = _GDT[dtype]
    rs = []
    B = len(lens) if lens is not None else B
    for mode, pre in ((0, True), (1, False), (2, True)) if chained else [(m, p_) for m in (0, 1, 2) for p_ in (False, True)]:
        x = AR.make_inputs(B, S, nh, dname, seed=11, **AR.bound_config(S, mode, pre, lens))
        ref = AR.attn_ref(x)
        ops_in, sl = _attn_operands(x, dtype), _attn_lens(lens)
        tag = f"attn.bound[{dname},mode{mode},S{S},B{B},nh{nh},pre{int(pre)},lens{lens}]"
        f = _attn_fwd(x, ops_in, sl)
        for n in AR.FWD_OUT:
            if n == "corr" and mode != 2:
                continue
            rs.append(_bounded(f"{tag}.{n}", f[n].reshape(ref[n].shape), ref[n], ref[n + "_bound"]))
        if chained:
            got, gap = _attn_bwd(x, ops_in, sl, f["o"], f["o_soft"], f["lse"], f["corr"], tag)
        else:
            got, gap = _attn_bwd(x, ops_in, sl, *_attn_fed(x, AR.fed(ref, x), dtype), tag)
        sfx = "_bound_chained" if chained else "_bound"
        rs += [_bounded(f"{tag}.{n}{'.chained' if chained else ''}", got[n], ref[n], ref[n + sfx]) for n in AR.BWD_OUT] + [gap]
    return rs


def check_attention_exact(dtype, S, mode, nh=2):
    """The exact selections of attn_ref.exact_case, plain and with lengths, pre-scaled or not: o, o_soft, corr equal to the one right answer (lse: 0
    where one key is selected, under its bound elsewhere), padded rows exactly zero; with one key per query and the backward fed lse = 0 and the
    exact o: delta, dq = dk = 0 and dv exact, and tav_attn_probs exact."""
    dname = _GDT[dtype]
    rs = []
    for pre in (False, True):
        for lens in (None, _ALENS_EXACT[S]):
            for single in (False, True):
                B = 2 if lens is None else len(lens)
                x = AR.exact_case(B, S, nh, dname, mode, pre, lens=lens, single=single)
                assert AR.exact_ok(x)
                w = AR.exact_want(x)
                ops_in, sl = _attn_operands(x, dtype), _attn_lens(lens)
                tag = f"attn.exact[{dname},mode{mode},S{S},pre{int(pre)},lens{lens},single{int(single)}]"
                want = lambda n, dt_=dtype: torch.from_numpy(w[n]).to(DEV).to(dt_)      # noqa: E731
                f = _attn_fwd(x, ops_in, sl)
                rs += [_exact(f"{tag}.o", f["o"].reshape(B, S, nh, 64), want("o")), _exact(f"{tag}.o_soft", f["o_soft"].reshape(B, S, nh, 64), want("o_soft"))]
                if mode == 2:
                    rs.append(_exact(f"{tag}.corr", f["corr"], want("corr", torch.float32)))
                one = torch.from_numpy(~np.isnan(w["lse"])).to(DEV)
                rs.append(_exact(f"{tag}.lse where l = 1", torch.where(one, f["lse"], torch.zeros_like(f["lse"])), torch.zeros_like(f["lse"])))
                rs.append(_bounded(f"{tag}.lse", f["lse"], w["lse_full"], AR.attn_ref(x)["lse_bound"]))
                if not single:
                    continue
                zero_lse = _in(torch.zeros(B, nh, S, device=DEV))
                o_fed = _in(want("o").reshape(B * S, nh * 64))
                os_fed = _in(want("o_soft").reshape(B * S, nh * 64))
                got, gap = _attn_bwd(x, ops_in, sl, o_fed, os_fed, zero_lse, _in(want("corr", torch.float32)), tag)
                rs += [_exact(f"{tag}.{n}", got[n], want(n)) for n in ("dq", "dk", "dv")] + [_exact(f"{tag}.delta", got["delta"], want("delta", torch.float32)), gap]
                if lens is None:
                    q, k, _, _, mask = ops_in
                    pr = ops.attn_probs(q, k, zero_lse, B, S, nh, key_mask=mask, mask_mode=mode, q_prescaled=pre)
                    rs.append(_exact(f"{tag}.probs", pr, want("probs", torch.float32)))
    return rs


def check_attn_probs_bounded(dtype, S, B=2, nh=3):
    """tav_attn_probs fed the reference's lse: every element within its bound (entries under a mode-1 mask: bound 0, exactly zero), without and
    with head factors of spread magnitude in both layouts."""
    dname = _GDT[dtype]
    rs = []
    rng = np.random.default_rng(S)
    for mode in (0, 1, 2):
        for pre in (False, True):
            x = AR.make_inputs(B, S, nh, dname, seed=12, **AR.bound_config(S, mode, pre))
            ref = AR.attn_ref(x)
            q, k, _, _, mask = _attn_operands(x, dtype)
            lse = _in(torch.from_numpy(ref["lse"]).to(DEV).float())
            for name, hs in (("none", None), ("[nh]", rng.standard_normal(nh) * 2.0 ** (3 * np.arange(nh) - 3)),
                             ("[B,nh]", rng.standard_normal((B, nh)) * 2.0 ** (3 * np.arange(nh) - 3))):
                hs_t = None if hs is None else _in(torch.from_numpy(hs).to(DEV).float())
                want, bound = AR.probs_ref(x, ref, None if hs is None else hs_t.double().cpu().numpy())
                got = ops.attn_probs(q, k, lse, B, S, nh, key_mask=mask, mask_mode=mode, q_prescaled=pre, head_scale=hs_t)
                rs.append(_bounded(f"attn_probs.bound[{dname},S{S},mode{mode},pre{int(pre)},hs{name}]", got, want, bound))
    return rs


def check_head_scale_bounded(dtype, B=2, S=37, nh=3):
    """tav_head_scale, out = a + (c0 + hs[b, h]) * b with head factors of spread magnitude: every element within two f32 roundings and the store."""
    dname = _GDT[dtype]
    rng = np.random.default_rng(37)
    H = nh * 64
    a = GR.round_to(rng.standard_normal((B * S, nh, 64)) * AR.v_scale(), dname)[0]
    b = GR.round_to(rng.standard_normal((B * S, nh, 64)) * AR.do_scale(), dname)[0]
    rs = []
    for name, hs in (("[nh]", rng.standard_normal(nh) * 2.0 ** (3 * np.arange(nh) - 3)), ("[B,nh]", rng.standard_normal((B, nh)) * 2.0 ** (3 * np.arange(nh) - 3))):
        hs_t = _in(torch.from_numpy(hs).to(DEV).float())
        for use_a in (False, True):
            for c0 in (-1.0, 1.0):
                f = np.broadcast_to((np.float32(c0) + hs_t.cpu().numpy().reshape(-1, nh)).astype(np.float64), (B, nh)).repeat(S, 0)
                want, bound = AR.head_scale_ref(a if use_a else None, b, f, dname)
                at = _in(torch.from_numpy(a.reshape(B * S, H)).to(DEV).to(dtype), 8) if use_a else None
                bt = _in(torch.from_numpy(b.reshape(B * S, H)).to(DEV).to(dtype), 16)
                wide = _blank((B * S, H + 16), dtype)
                out = ops.head_scale(at, bt, hs_t, c0, B, S, nh, out=wide[:, 8:8 + H])
                tag = f"head_scale.bound[{dname},a{int(use_a)},hs{name},c0{c0:g}]"
                rs += [_bounded(tag, out.reshape(B * S, nh, 64), want, bound), _all_ff(tag + ".gap", wide[:, :8], wide[:, 8 + H:])]
    return rs


def attention_fp64_checks():
    """The attention cases against fp64, in the order all_checks() appends them."""
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        for S in AR.BOUND_S:
            out.append(lambda d=dtype, s=S: check_attention_bounded(d, s))
        for S, lens_list in AR.LEN_CASES.items():
            for lens in lens_list:
                out.append(lambda d=dtype, s=S, ln=lens: check_attention_bounded(d, s, lens=list(ln), nh=2))
        out.append(lambda d=dtype: check_attention_bounded(d, AR.CHAINED_S, chained=True))
        for S in AR.EXACT_S:
            for mode in (0, 1, 2):
                out.append(lambda d=dtype, s=S, m=mode: check_attention_exact(d, s, m))
        for S in (1, 65, 193):
            out.append(lambda d=dtype, s=S: check_attn_probs_bounded(d, s))
        out.append(lambda d=dtype: check_head_scale_bounded(d))
    return out


# ================================================================================================= normalisation against fp64
# tests/norm_ref.py: per-element bounds at operands of spread magnitude, integer cases with ONE right answer, an atypical first row in front of
# the group norm's statistics.  The library is called through the C ABI: pitched outputs, accumulation, a bf16 dy, hand-fed mean / rstd / stats
# and workspaces at exactly the advertised size are things the ops wrappers (rightly) cannot express.
def _dev(a, dtype, pitch=0):
    return _in(torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype), pitch)


def _wide(rows, W, dtype, pitch):
    """An all-0xFF [rows][W + pitch] buffer and the [rows][W] view the kernel is to fill."""
    w = _blank((rows, W + pitch), dtype)
    return w, w[:, :W]


def _filled(a):
    t = _blank(tuple(a.shape), torch.float32)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV).float())
    return t


def _ln_dev(p, pitch=0):
    return _dev(p["x"], _TDT[p["xdt"]], pitch), _dev(p["gamma"], torch.float32), _dev(p["beta"], torch.float32)


def _ln_base(p, dev, act):
    a = ops.L.LnArgs()
    xt, gam, bet = dev
    a.x, a.x_dtype, a.gamma, a.beta = ops.ptr(xt), ops.dt(xt), ops.ptr(gam), ops.ptr(bet)
    a.rows, a.W, a.ld_x, a.eps, a.act = p["rows"], p["W"], xt.stride(0), 1e-5, act
    return a


def _ln_fwd_abi(p, dev, *, act=0, want32=True, lp=True, pitch=0, stats=True):
    """tav_ln_fwd -> (dict y_f32, y_lp, mean, rstd (None where not asked for), the pitch gaps of the outputs)."""
    rows, W = p["rows"], p["W"]
    a = _ln_base(p, dev, act)
    y32w, y32 = _wide(rows, W, torch.float32, pitch) if want32 else (None, None)
    ylw, yl = _wide(rows, W, torch.bfloat16, pitch) if lp else (None, None)
    mean, rstd = (_blank((rows,), torch.float32), _blank((rows,), torch.float32)) if stats else (None, None)
    a.y_f32, a.y_lp, a.lp_dtype, a.mean, a.rstd, a.ld_y = ops.ptr(y32), ops.ptr(yl), ops.dt(torch.bfloat16) if lp else 0, ops.ptr(mean), ops.ptr(rstd), W + pitch
    ops.check(ops.lib().tav_ln_fwd(ops.C.byref(a), ops.stream()), "ln_fwd")
    return dict(y_f32=y32, y_lp=yl, mean=mean, rstd=rstd), [w[:, W:] for w in (y32w, ylw) if w is not None]


def _ln_bwd_abi(p, dev, dyt, mean, rstd, *, act=0, want32=True, lp=True, pitch=0, add=None, grads=True, prev=None, defer=False):
    """tav_ln_bwd -> (dict dx_f32, dx_lp, dgamma, dbeta, partials, nb; gaps).  prev: (dgamma, dbeta) contents to accumulate onto."""
    rows, W = p["rows"], p["W"]
    a = _ln_base(p, dev, act)
    nb = ops.lib().tav_ln_bwd_partials(rows)
    d32w, d32 = _wide(rows, W, torch.float32, pitch) if want32 else (None, None)
    dlw, dl = _wide(rows, W, torch.bfloat16, pitch) if lp else (None, None)
    dg = db = part = None
    if grads:
        dg, db = (_filled(prev[0]), _filled(prev[1])) if prev is not None else (_blank((W,), torch.float32), _blank((W,), torch.float32))
        part = _blank((nb * 2 * W,), torch.float32)
    a.mean, a.rstd, a.dy, a.dy_dtype, a.dx_add, a.ld_dy = ops.ptr(mean), ops.ptr(rstd), ops.ptr(dyt), ops.dt(dyt), ops.ptr(add), dyt.stride(0)
    a.dx_f32, a.dx_lp, a.lp_dtype, a.ld_dx = ops.ptr(d32), ops.ptr(dl), ops.dt(torch.bfloat16) if lp else 0, W + pitch
    a.dgamma, a.dbeta, a.partials, a.accumulate_params, a.defer_param_reduce = ops.ptr(dg), ops.ptr(db), ops.ptr(part), int(prev is not None), int(defer)
    ops.check(ops.lib().tav_ln_bwd(ops.C.byref(a), ops.stream()), "ln_bwd")
    return dict(dx_f32=d32, dx_lp=dl, dgamma=dg, dbeta=db, partials=part, nb=nb), [w[:, W:] for w in (d32w, dlw) if w is not None]


def _ln_reduce_multi(items):
    """items: (partials, dgamma, dbeta, nblocks, W, accumulate) -> one tav_ln_param_reduce_multi launch."""
    arr = (ops.L.LnReduceItem * len(items))()
    for j, (part, dg, db, nb, W, acc) in enumerate(items):
        arr[j].partials, arr[j].dgamma, arr[j].dbeta, arr[j].nblocks, arr[j].W, arr[j].accumulate = ops.ptr(part), ops.ptr(dg), ops.ptr(db), nb, W, acc
    ops.check(ops.lib().tav_ln_param_reduce_multi(arr, len(items), ops.stream()), "ln_param_reduce_multi")


@functools.lru_cache(maxsize=4)
def _ln_fwd_reference(rows, W, xdt, act, lp):
    return NR.ln_ref_fwd(NR.ln_inputs(rows, W, xdt, "f32"), act, lp)                # (x, gamma and beta do not depend on the dtype of dy)


def _some(rs, got, ref, tag, names):
    for n in names:
        if got.get(n) is not None:
            rs.append(_bounded(f"{tag}.{n}", got[n], ref[n], ref[n + "_b"]))


def _ln_bounded_one(rs, rows, W, xdt, dydt, *, act, lp, both, pitch, add, accumulate, chained=False, fwd=True):
    """One forward and one backward launch of the spread-magnitude problem, every output within its bound, every pitch gap still 0xFF."""
    p = NR.ln_inputs(rows, W, xdt, dydt)
    dev = _ln_dev(p, 4 if pitch else 0)
    tag = f"ln.bound[x {xdt},dy {dydt},lp{int(lp)},W{W},rows{rows},act{act},pitch{pitch},add{int(add)},acc{int(accumulate)}]"
    want32 = both or not lp
    ref = _ln_fwd_reference(rows, W, xdt, act, lp)
    f = None
    if fwd or chained:
        f, gaps = _ln_fwd_abi(p, dev, act=act, want32=want32, lp=lp, pitch=pitch)
        _some(rs, f, ref, tag, NR.LN_FWD_OUT)
        rs.append(_all_ff(tag + ".y gaps", *gaps))
    if chained:
        mean, rstd, mv, rv, sfx = f["mean"], f["rstd"], ref["_mean"], ref["_rstd"], ".chained"
    else:
        (mv, m32), (rv, r32) = NR.fed(ref["mean"]), NR.fed(ref["rstd"])
        mean, rstd, sfx = _dev(m32, torch.float32), _dev(r32, torch.float32), ""
    kw = dict(act=act, lp=lp, add=add, accumulate=accumulate)
    b, gaps = _ln_bwd_abi(p, dev, _dev(p["dy"], _TDT[dydt], 8 if pitch else 0), mean, rstd, act=act, want32=want32, lp=lp, pitch=pitch,
                          add=_dev(p["add"], torch.float32, pitch) if add else None, prev=(p["prev_g"], p["prev_b"]) if accumulate else None)
    _some(rs, b, NR.ln_ref_bwd(p, mv, rv, **kw), tag + sfx, NR.LN_BWD_OUT)
    rs.append(_all_ff(tag + ".dx gaps", *gaps))


def check_layernorm_bounded(xdt, W):
    """tav_ln_fwd / tav_ln_bwd at one width, rows 1, 5, 17, 333: x f32 | bf16 (per group) x dy f32 | bf16 x low-precision output none | bf16 --
    with this group's twin all eight backward instantiations --; the backward isolated, at W = 768 also chained.  The forward does not read dy,
    so it is launched with the f32 dy only (di = 0).  The options of a case follow from ri (index of rows), di (0: dy f32, 1: bf16), li (0: no
    bf16 output, 1: one) and k = ri + di + li + W / 4:

        act          k odd                                 pitched rows     k / 2 odd   (x + 4, dy + 8, outputs and dx_add + 8 elements)
        dx_add       ri + li even                          accumulate       ri + di + li divisible by 3
        outputs      li = 0: f32 only;   li = 1: f32 and bf16 where ri + di is even, bf16 only where it is odd

    W / 4 is odd for W = 4, 252 and 260 and even for the other widths, so each (rows, dy, output) cell meets both values of act across the
    widths, and k / 2 takes both parities within every group (k runs over four consecutive values)."""
    rs = []
    for ri, rows in enumerate(NR.LN_ROWS):
        for di, dydt in enumerate(("f32", "bf16")):
            for li, lp in enumerate((False, True)):
                k = ri + di + li + W // 4
                _ln_bounded_one(rs, rows, W, xdt, dydt, act=k % 2, lp=lp, both=(ri + di) % 2 == 0, pitch=8 * ((k // 2) % 2), add=(ri + li) % 2 == 0,
                                accumulate=(ri + di + li) % 3 == 0, fwd=di == 0)
    if W == 768:
        for act in (0, 1):
            _ln_bounded_one(rs, 333, W, xdt, xdt, act=act, lp=True, both=True, pitch=0, add=True, accumulate=False, chained=True)
    return rs


def check_layernorm_bounded_big(xdt, W, act):
    """8192 + 37 rows: past the grid caps of both kernels, so the row loops and the backward's prefetch pipeline run more than once per wave."""
    rs = []
    _ln_bounded_one(rs, NR.LN_ROWS_BIG, W, xdt, xdt, act=act, lp=xdt == "bf16", both=True, pitch=8 if W == 64 else 0, add=True, accumulate=W == 64)
    return rs


def check_layernorm_options():
    """The corners of the argument struct: mean = rstd = NULL in a forward, param_grads off (partials = NULL, the early return), and the deferred
    reduce through tav_ln_param_reduce_multi with 1, 3 and 64 items of mixed W and nblocks (1, 63, 65 and 512 among them), accumulating on some:
    bit-equal to the immediate form, inside the bound against fp64, and nothing stored into dgamma / dbeta before the reduce."""
    rs = []
    p = NR.ln_inputs(333, 260, "f32", "f32")
    dev = _ln_dev(p)
    ref = _ln_fwd_reference(333, 260, "f32", 0, True)
    f, gaps = _ln_fwd_abi(p, dev, lp=True, pitch=8, stats=False)
    _some(rs, f, ref, "ln.fwd without mean / rstd", ("y_f32", "y_lp"))
    rs.append(_all_ff("ln.fwd without mean / rstd.gaps", *gaps))
    (mv, m32), (rv, r32) = NR.fed(ref["mean"]), NR.fed(ref["rstd"])
    b, gaps = _ln_bwd_abi(p, dev, _dev(p["dy"], torch.float32), _dev(m32, torch.float32), _dev(r32, torch.float32), grads=False)
    _some(rs, b, NR.ln_ref_bwd(p, mv, rv, add=False), "ln.bwd without param grads", ("dx_f32", "dx_lp"))
    shapes = [(333, 260), (5, 4), (16 * 63, 64), (16 * 65 - 3, 252), (NR.LN_ROWS_BIG, 64)] + [(1 + 7 * i % 40, NR.LN_W[i % 7]) for i in range(59)]
    runs = []
    for i, (rows, W) in enumerate(shapes):
        xdt = ("f32", "bf16")[i % 2]
        q = NR.ln_inputs(rows, W, xdt, xdt)
        qd = _ln_dev(q)
        qref = _ln_fwd_reference(rows, W, xdt, 0, False)
        (qm, m32), (qr, r32) = NR.fed(qref["mean"]), NR.fed(qref["rstd"])
        mt, rt, dyt = _dev(m32, torch.float32), _dev(r32, torch.float32), _dev(q["dy"], _TDT[xdt])
        acc = i % 3 == 1
        prev = (q["prev_g"], q["prev_b"]) if acc else None
        imm, _ = _ln_bwd_abi(q, qd, dyt, mt, rt, lp=False, prev=prev)
        dfr, _ = _ln_bwd_abi(q, qd, dyt, mt, rt, lp=False, prev=prev, defer=True)
        if not acc:
            rs.append(_all_ff(f"ln.deferred[{i}] dgamma / dbeta untouched by the backward", dfr["dgamma"], dfr["dbeta"]))
        if i < 5:
            _some(rs, imm, NR.ln_ref_bwd(q, qm, qr, lp=False, add=False, accumulate=acc), f"ln.immediate[rows{rows},W{W},nb{imm['nb']},acc{int(acc)}]", ("dgamma", "dbeta"))
        runs.append((imm, dfr, q["W"], acc))
    assert {r[0]["nb"] for r in runs} >= {1, 63, 65, 512}
    for lo, hi in ((0, 1), (1, 4), (0, 64)):
        fresh = []
        for k, (imm, dfr, W, acc) in enumerate(runs[lo:hi]):
            i = lo + k
            q = NR.ln_inputs(shapes[i][0], W, ("f32", "bf16")[i % 2], ("f32", "bf16")[i % 2])
            dg, db = (_filled(q["prev_g"]), _filled(q["prev_b"])) if acc else (_blank((W,), torch.float32), _blank((W,), torch.float32))
            fresh.append((dfr["partials"], dg, db, dfr["nb"], W, int(acc)))
        _ln_reduce_multi(fresh)
        bad_g = sum(int((it[1] != run[0]["dgamma"]).sum()) + int(it[1].isnan().sum()) for it, run in zip(fresh, runs[lo:hi]))
        bad_b = sum(int((it[2] != run[0]["dbeta"]).sum()) + int(it[2].isnan().sum()) for it, run in zip(fresh, runs[lo:hi]))
        rs += [(f"ln.reduce_multi x{hi - lo} dgamma bitwise", float(bad_g), 0.0, bad_g == 0), (f"ln.reduce_multi x{hi - lo} dbeta bitwise", float(bad_b), 0.0, bad_b == 0)]
    return rs


def _want(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def check_layernorm_exact(xdt, dydt):
    """The integer construction of norm_ref.ln_exact_case fed mean = 0, rstd = 1: dx_f32 equal to the fp64 value bit for bit, dx_lp to its
    round-to-nearest-even, dgamma / dbeta to the fp64 sums -- accumulated onto integer contents, through the immediate and the deferred reduce,
    pitched, with and without the saturated GELU, at 333 rows and past the grid caps."""
    rs = []
    for rows, W, pitch in ((333, 64, 8), (333, 512, 0), (17, 1024, 8), (NR.LN_ROWS_BIG, 64, 0), (NR.LN_ROWS_BIG, 1024, 8)):
        for act in (0, 1):
            if rows > 1000 and act != (W == 64):
                continue
            assert NR.exact_ok(rows, W)
            p = NR.ln_exact_case(rows, W, xdt, dydt, act)
            dev = _ln_dev(p)
            zero, one = _dev(np.zeros(rows), torch.float32), _dev(np.ones(rows), torch.float32)
            dyt, add = _dev(p["dy"], _TDT[dydt], 8 if pitch else 0), _dev(p["add"], torch.float32, pitch)
            tag = f"ln.exact[x {xdt},dy {dydt},rows{rows},W{W},act{act},pitch{pitch}]"
            want_g, want_b = _want(p["want_dg"] + p["prev_g"], torch.float32), _want(p["want_db"] + p["prev_b"], torch.float32)
            b, gaps = _ln_bwd_abi(p, dev, dyt, zero, one, act=act, pitch=pitch, add=add, prev=(p["prev_g"], p["prev_b"]))
            rs += [_exact(tag + ".dx_f32", b["dx_f32"], _want(p["want_dx"], torch.float32)), _exact(tag + ".dx_lp", b["dx_lp"], _want(p["want_dx"], torch.bfloat16)),
                   _exact(tag + ".dgamma", b["dgamma"], want_g), _exact(tag + ".dbeta", b["dbeta"], want_b), _all_ff(tag + ".gaps", *gaps)]
            d, _ = _ln_bwd_abi(p, dev, dyt, zero, one, act=act, pitch=pitch, add=add, prev=(p["prev_g"], p["prev_b"]), defer=True)
            _ln_reduce_multi([(d["partials"], d["dgamma"], d["dbeta"], d["nb"], W, 1)])
            rs += [_exact(tag + ".deferred dgamma", d["dgamma"], want_g), _exact(tag + ".deferred dbeta", d["dbeta"], want_b)]
    return rs


def check_norm_exact_statistics():
    """Forward statistics with one right answer: LayerNorm rows of +-a in equal number (mean exactly 0) and constant integer rows (mean = the
    constant, y = beta exactly); group norm on integers over a power-of-two T (mean exact, rstd within the bounded term)."""
    rs = []
    for xdt in ("f32", "bf16"):
        for W in (64, 512, 1024):
            p = NR.ln_stats_case(33, W)
            p["xdt"] = xdt
            f, _ = _ln_fwd_abi(p, _ln_dev(p), lp=False)
            rs += [_exact(f"ln.exact mean[{xdt},W{W}]", f["mean"], _want(p["want_mean"], torch.float32)),
                   _exact(f"ln.exact y = beta[{xdt},W{W}]", f["y_f32"][1::2], _want(np.broadcast_to(p["beta"], (16, W)), torch.float32))]
        for T in (1, 64, 1024):
            p = NR.gn_exact_case(3, T, 64, xdt)
            f = _gn_fwd_abi(p)
            ref = NR.gn_ref_fwd(p)
            rs += [_exact(f"gn.exact mean[{xdt},T{T}]", f["mean"], _want(p["want_mean"], torch.float32)),
                   _bounded(f"gn.exact rstd[{xdt},T{T}]", f["rstd"], ref["rstd"], ref["rstd_b"])]
    return rs


def _gn_ws(B, C):
    n = ops.lib().tav_gn_workspace_floats(B, C)
    assert n == NR.gn_workspace_floats(B, C)
    return _blank((n,), torch.float32)                                              # exactly the advertised size, under guard


def _gn_fwd_abi(p):
    B, T, C, dtype = p["B"], p["T"], p["C"], _TDT[p["dt"]]
    x, gam, bet = _dev(p["x"], dtype), _dev(p["gamma"], torch.float32), _dev(p["beta"], torch.float32)
    y, stats = _blank((B, T, C), dtype), _blank((B, C, 2), torch.float32)
    ops.check(ops.lib().tav_gn_gelu_fwd(ops.ptr(x), ops.ptr(y), ops.dt(dtype), ops.ptr(gam), ops.ptr(bet), ops.ptr(stats), ops.ptr(_gn_ws(B, C)), B, T, C,
                                        1e-5, ops.stream()), "gn_gelu_fwd")
    return dict(y=y, stats=stats, mean=stats[..., 0], rstd=stats[..., 1], dev=(x, gam, bet))


def _gn_bwd_abi(p, dev, stats, prev=None):
    B, T, C, dtype = p["B"], p["T"], p["C"], _TDT[p["dt"]]
    x, gam, bet = dev
    dy, dx = _dev(p["dy"], dtype), _blank((B, T, C), dtype)
    dg, db = (_filled(prev[0]), _filled(prev[1])) if prev is not None else (_blank((C,), torch.float32), _blank((C,), torch.float32))
    ops.check(ops.lib().tav_gn_gelu_bwd(ops.ptr(x), ops.ptr(dy), ops.ptr(dx), ops.dt(dtype), ops.ptr(gam), ops.ptr(bet), ops.ptr(stats), ops.ptr(_gn_ws(B, C)),
                                        ops.ptr(dg), ops.ptr(db), B, T, C, int(prev is not None), ops.stream()), "gn_gelu_bwd")
    return dict(dx=dx, dgamma=dg, dbeta=db)


def _gn_bounded_one(rs, B, T, C, dt, accumulate, chained=False, onset=False):
    p = NR.gn_inputs(B, T, C, dt, onset=onset)
    ref = NR.gn_ref_fwd(p)
    tag = f"gn.bound[{dt},B{B},T{T},C{C},acc{int(accumulate)}{',onset' if onset else ''}]"
    f = _gn_fwd_abi(p)
    _some(rs, f, ref, tag, NR.GN_FWD_OUT)
    if onset:
        return
    prev = (p["prev_g"], p["prev_b"]) if accumulate else None
    (mv, m32), (rv, r32) = NR.fed(ref["mean"]), NR.fed(ref["rstd"])
    _some(rs, _gn_bwd_abi(p, f["dev"], _dev(np.stack([m32, r32], -1), torch.float32), prev), NR.gn_ref_bwd(p, mv, rv, accumulate), tag, NR.GN_BWD_OUT)
    if chained:
        _some(rs, _gn_bwd_abi(p, f["dev"], f["stats"], prev), NR.gn_ref_bwd(p, ref["_mean"], ref["_rstd"], accumulate), tag + ".chained", NR.GN_BWD_OUT)


def check_group_norm_bounded(dt, C, half):
    """tav_gn_gelu_fwd / _bwd at one channel count and six of the twelve lengths (empty splits, one row per split, a ragged last split, one and
    two unrolled chunks plus a tail in both statistics kernels, both branches of the apply block), B = 1 | 3 and accumulate alternating: stats
    (mean, rstd), y, and -- fed the reference's stats -- dx, dgamma, dbeta within their bounds; T = 1599 also chained."""
    rs = []
    for i, T in enumerate(NR.GN_T[6 * half:6 * half + 6]):
        k = i + C // 64
        _gn_bounded_one(rs, 1 if k % 2 else 3, T, C, dt, accumulate=(k // 2) % 2 == 1, chained=T == 1599)
    return rs


def check_group_norm_exact(dt):
    """norm_ref.gn_exact_case fed stats = (0, 1): the saturated GELU is exactly the identity, so dx, dgamma and dbeta (accumulated onto integer
    contents) have one right answer."""
    rs = []
    for T, C in ((1, 64), (64, 320), (1024, 64)):
        p = NR.gn_exact_case(3, T, C, dt)
        dev = (_dev(p["x"], _TDT[dt]), _dev(p["gamma"], torch.float32), _dev(p["beta"], torch.float32))
        stats = _dev(np.stack([np.zeros((3, C)), np.ones((3, C))], -1), torch.float32)
        b = _gn_bwd_abi(p, dev, stats, (p["prev_g"], p["prev_b"]))
        tag = f"gn.exact[{dt},T{T},C{C}]"
        rs += [_exact(tag + ".dx", b["dx"], _want(p["want_dx"], _TDT[dt])), _exact(tag + ".dgamma", b["dgamma"], _want(p["want_dg"] + p["prev_g"], torch.float32)),
               _exact(tag + ".dbeta", b["dbeta"], _want(p["want_db"] + p["prev_b"], torch.float32))]
    return rs


def check_group_norm_onset(dt):
    """An atypical FIRST row -- 32 sigma off in the even channels, 256 sigma in the odd ones, T = 1599 -- against the statistics bound with kappa
    capped at what a typical row is allowed (norm_ref.KAPPA_CAP): the pivot of the statistics pass must not be that row."""
    rs = []
    _gn_bounded_one(rs, 2, 1599, 64, dt, False, onset=True)
    return rs


def norm_fp64_checks():
    """The normalisation cases against fp64, in the order all_checks() appends them."""
    out = []
    for dt_ in ("f32", "bf16"):
        for W in NR.LN_W:
            out.append(lambda d=dt_, w=W: check_layernorm_bounded(d, w))
        for W, act in ((64, 0), (64, 1), (1024, int(dt_ == "bf16"))):
            out.append(lambda d=dt_, w=W, a=act: check_layernorm_bounded_big(d, w, a))
        for dydt in ("f32", "bf16"):
            out.append(lambda d=dt_, e=dydt: check_layernorm_exact(d, e))
        for C in NR.GN_C:
            for half in (0, 1):
                out.append(lambda d=dt_, c=C, h=half: check_group_norm_bounded(d, c, h))
        out.append(lambda d=dt_: check_group_norm_exact(d))
        out.append(lambda d=dt_: check_group_norm_onset(d))
    out += [check_layernorm_options, check_norm_exact_statistics]
    return out


# ================================================================================================= front-end, pooling, head, loss against fp64
# tests/front_ref.py: per-element bounds at operands of spread magnitude and integer cases with ONE right answer for the kernels the chains
# above judge only through later stages: the rest of csrc/audio_frontend.hip, tav_colsum, the stand-alone GELU pair, the pools, the head, tanh,
# the cross entropy and the index kernels.  The C ABI is called directly: accumulation, NULL outputs and workspaces at exactly the advertised
# size are things the ops wrappers cannot express.  Every output starts as 0xFF.
_F32 = torch.float32


def _fb(rs, tag, got, ref, names):
    for n in names:
        if got.get(n) is not None:
            rs.append(_bounded(f"{tag}.{n}", got[n], ref[n], ref[n + "_b"]))


def _fx(rs, tag, got, want, dtype=torch.float32):
    want = np.asarray(want)
    rs.append(_exact(tag, got, _want(want.reshape(tuple(got.shape)) if want.size == got.numel() else want, dtype)))


def _ints_dev(a, dtype):
    return _in(torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV))


def _conv0_fwd_abi(p, bias, dtype):
    wave, w = _dev(p["wave"], _F32), _dev(p["w"], _F32)
    b = _dev(p["bias"], _F32) if bias else None
    y = _blank((p["B"], p["T_out"], p["C"]), dtype)
    ops.check(ops.lib().tav_conv0_fwd(ops.ptr(wave), ops.ptr(w), ops.ptr(b), ops.ptr(y), ops.dt(dtype), p["B"], p["T_in"], p["T_out"], p["C"], p["K"],
                                      p["stride"], ops.stream()), "conv0_fwd")
    return dict(y=y)


def check_conv0_fwd_fp64(dt):
    """tav_conv0_fwd: C = 4 (one quad), 12 (85 time groups and an idle thread), 512 (the model's), 1028 (a second quad pass) x T_out = 1, 127,
    128, 129, 257 (around one and two blocks of C0_TT), (K, stride) cycling through (10, 5), (16, 8), (1, 1), (3, 2), B = 1 | 3, bias on | off,
    T_in exact | 7 longer; every fourth shape also on integers (one right answer)."""
    rs, i = [], 0
    for C in (4, 12, 512, 1028):
        for T_out in (1, 127, 128, 129, 257):
            K, s = ((10, 5), (16, 8), (1, 1), (3, 2))[i % 4]
            B, bias, extra = (1, 3)[i % 2], i % 3 != 0, 7 * ((i // 2) % 2)
            for exact in (False, True) if i % 4 == 1 else (False,):
                p = FR.conv0_inputs(B, T_out, C, K, s, extra=extra, exact=exact)
                tag = f"conv0.fwd[{dt},B{B},T{T_out},C{C},K{K},s{s},bias{int(bias)},+{extra}{',int' if exact else ''}]"
                got, ref = _conv0_fwd_abi(p, bias, _TDT[dt]), FR.conv0_ref_fwd(p, bias, dt)
                if exact:
                    _fx(rs, tag + ".y", got["y"], FR.held(ref["y"], dt), _TDT[dt])
                else:
                    _fb(rs, tag, got, ref, ("y",))
            i += 1
    return rs


def _conv0_bwd_abi(p, want_bias, accumulate):
    B, T_out, C, K = p["B"], p["T_out"], p["C"], p["K"]
    wave, dy = _dev(p["wave"], _F32), _dev(p["dy"], _TDT[p["dydt"]])
    n = ops.lib().tav_conv0_bwd_partials(B, T_out, C, K)
    assert n == B * -(-T_out // FR.C0_BT) * C * (K + 1)
    part = _blank((n,), _F32)                                                       # exactly the advertised size, under guard
    dw = _filled(p["prev_w"]) if accumulate else _blank((C, K), _F32)
    db = None if not want_bias else (_filled(p["prev_b"]) if accumulate else _blank((C,), _F32))
    ops.check(ops.lib().tav_conv0_bwd_w(ops.ptr(wave), ops.ptr(dy), ops.dt(dy), ops.ptr(dw), ops.ptr(db), ops.ptr(part), B, p["T_in"], T_out, C, K,
                                        p["stride"], int(accumulate), ops.stream()), "conv0_bwd_w")
    return dict(dw=dw, dbias=db)


def check_conv0_bwd_fp64(dydt, Cs):
    """tav_conv0_bwd_w at two of the widths C = 8, 64 (threads idle in the channel loop), 512, 520 (a second, ragged pass of it) x T_out = 1, 3,
    511, 512, 513, 1025, 1537, 2050 (one chunk of C0_BT, a ragged second one, up to five: t0 > 0 and the cross-chunk reduce), B in {1, 3, 5} and
    K in {1, 3, 10} cycling -- nblocks % 4 takes all four values: 1537 with B = 1 gives 4 blocks, which no odd B reaches at the other lengths --,
    dbias NULL | given, accumulate 0 | 1; T_out = 513 and the extremes also on integers."""
    rs, i = [], 0
    for C in Cs:
        for T_out in (1, 3, 511, 512, 513, 1025, 1537, 2050):
            B = 1 if T_out == 1537 else (1, 3, 5)[i % 3]
            K = (1, 3, 10)[(i + i // 3) % 3]
            s = {1: 1, 3: 2, 10: 5}[K]
            want_bias, acc = i % 2 == 0, (i // 2) % 2 == 1
            p = FR.conv0_inputs(B, T_out, C, K, s, dydt=dydt)
            tag = f"conv0.bwd[dy {dydt},B{B},T{T_out},C{C},K{K},db{int(want_bias)},acc{int(acc)}]"
            _fb(rs, tag, _conv0_bwd_abi(p, want_bias, acc), FR.conv0_ref_bwd_w(p, acc), ("dw", "dbias"))
            if T_out == 513 or (C, T_out) in ((8, 2050), (520, 3)):
                q = FR.conv0_inputs(B, T_out, C, K, s, dydt=dydt, exact=True)
                got, ref = _conv0_bwd_abi(q, True, True), FR.conv0_ref_bwd_w(q, True)
                _fx(rs, tag + ".int dw", got["dw"], ref["dw"])
                _fx(rs, tag + ".int dbias", got["dbias"], ref["dbias"])
            i += 1
    return rs


def _wn_fwd_abi(p, dtype, which, v, g):
    H, Cg, K = p["H"], p["Cg"], p["K"]
    nb = ops.lib().tav_weight_norm_partials(H, Cg)
    assert nb == FR.wn_blocks(H, Cg)[0]
    norms, part = _blank((K,), _F32), _blank((nb * K,), _F32)
    w = _blank((p["G"], Cg, K, Cg), dtype) if which != "w_flip" else None
    wf = _blank((p["G"], Cg, K, Cg), dtype) if which != "w" else None
    ops.check(ops.lib().tav_weight_norm_fwd(ops.ptr(v), ops.ptr(g), ops.ptr(norms), ops.ptr(part), ops.ptr(w), ops.ptr(wf), ops.dt(dtype), H, Cg, K,
                                            ops.stream()), "weight_norm_fwd")
    return dict(norms=norms, w=w, w_flip=wf)


def _wn_bwd_abi(p, norms, accumulate, v, g):
    H, Cg, K = p["H"], p["Cg"], p["K"]
    ws = _blank((FR.wn_bwd_workspace_floats(H, Cg, K),), _F32)
    dv, dg = (_filled(p["prev_v"]), _filled(p["prev_g"])) if accumulate else (_blank((H, Cg, K), _F32), _blank((K,), _F32))
    ops.check(ops.lib().tav_weight_norm_bwd(ops.ptr(v), ops.ptr(g), ops.ptr(norms), ops.ptr(_dev(p["dw"], _F32)), ops.ptr(ws), ops.ptr(dv), ops.ptr(dg),
                                            H, Cg, K, int(accumulate), ops.stream()), "weight_norm_bwd")
    return dict(dv=dv, dg=dg)


def check_weight_norm_fp64(H, Cg, K, parts="fb"):
    """tav_weight_norm_fwd / _bwd at one (H, Cg, K): norms, w, w_flip (w only, w_flip only, both; both dtypes) and -- fed the reference's norms
    rounded to f32 (isolated) and the kernel's own (chained) -- dv, dg, accumulating and not; then the construction with ||v|| = 2^k, bit for bit.
    parts: "f" the forward, "b" the backward (the model's shape is split in two groups)."""
    rs = []
    big = H * Cg * K > 1 << 20
    p, q = FR.wn_inputs(H, Cg, K), FR.wn_inputs(H, Cg, K, exact=True)
    v, g = _dev(p["v"], _F32), _dev(p["g"], _F32)
    qv, qg = _dev(q["v"], _F32), _dev(q["g"], _F32)
    tag = f"wn[H{H},Cg{Cg},K{K}]"
    if "f" in parts:
        for dt in ("f32", "bf16"):
            ref = FR.wn_ref_fwd(p, dt)
            for which in (("w", "w_flip") if dt == "f32" else ("both",)) if big else ("w", "w_flip", "both"):
                _fb(rs, f"{tag}.fwd[{dt},{which}]", _wn_fwd_abi(p, _TDT[dt], which, v, g), ref, ("norms", "w", "w_flip"))
            got, want = _wn_fwd_abi(q, _TDT[dt], "both", qv, qg), FR.wn_ref_fwd(q, dt)
            _fx(rs, f"{tag}.int norms[{dt}]", got["norms"], want["norms"])
            _fx(rs, f"{tag}.int w[{dt}]", got["w"], FR.held(want["w"], dt), _TDT[dt])
            _fx(rs, f"{tag}.int w_flip[{dt}]", got["w_flip"], FR.held(want["w_flip"], dt), _TDT[dt])
    if "b" in parts:
        ref = FR.wn_ref_fwd(p, "f32")
        nv, n32 = FR.fed(ref["norms"])
        fed = _dev(n32, _F32)
        for acc in ((True,) if big else (False, True)):                              # (a big shape: isolated accumulating, chained not)
            _fb(rs, f"{tag}.bwd[acc{int(acc)}]", _wn_bwd_abi(p, fed, acc, v, g), FR.wn_ref_bwd(p, nv, acc), ("dv", "dg"))
        own = _wn_fwd_abi(p, _F32, "w", v, g)["norms"]
        acc = not big and (H // Cg) % 2 == 0
        _fb(rs, f"{tag}.bwd.chained[acc{int(acc)}]", _wn_bwd_abi(p, own, acc, v, g), FR.wn_ref_bwd(p, ref["_norms"], acc), ("dv", "dg"))
        got, want = _wn_bwd_abi(q, _dev(FR.wn_ref_fwd(q, "f32")["norms"], _F32), True, qv, qg), FR.wn_ref_bwd(q, FR.V(FR.wn_ref_fwd(q, "f32")["norms"]), True)
        _fx(rs, f"{tag}.int dv", got["dv"], want["dv"])
        _fx(rs, f"{tag}.int dg", got["dg"], want["dg"])
    return rs


def check_group_pad_fp64():
    """tav_group_pad is a copy with zero frames: bit for bit in all three dtype pairs (f32 -> bf16 with its round-to-nearest-even), at the smallest
    launch, the positional conv's forward (64, 64) and backward (63, 64) frames, sixteen groups with a short right frame, and no left frame."""
    rs = []
    for B, T, H, G, pl, pr in ((1, 1, 8, 2, 0, 0), (2, 49, 256, 4, 64, 64), (2, 49, 256, 4, 63, 64), (3, 5, 768, 16, 64, 63), (2, 3, 16, 2, 0, 5), (1, 70, 16, 1, 1, 0)):
        for sdt, ddt in (("f32", "bf16"), ("f32", "f32"), ("bf16", "bf16")):
            x = FR.gp_inputs(B, T, H, sdt)
            xt = _dev(x, _TDT[sdt])
            xg = _blank((B, G, pl + T + pr, H // G), _TDT[ddt])
            ops.check(ops.lib().tav_group_pad(ops.ptr(xt), ops.dt(xt), ops.ptr(xg), ops.dt(xg), B, T, H, G, pl, pr, ops.stream()), "group_pad")
            _fx(rs, f"group_pad[{sdt}->{ddt},B{B},T{T},H{H},G{G},{pl}+{pr}]", xg, FR.gp_ref(x, G, pl, pr, ddt), _TDT[ddt])
    return rs


def check_col2im_fp64(dt):
    """tav_col2im_1d on its own: (K, stride) = (3, 2), (2, 2), (10, 5), (3, 1), T_in exact and 3 longer (rows no tap reaches: exactly zero), with
    and without the gelu' product, one and many workgroups; on integers with pre in [16, 48], where gelu' is exactly 1."""
    rs, i = [], 0
    dtype = _TDT[dt]
    for K, s in ((3, 2), (2, 2), (10, 5), (3, 1)):
        for extra in (0, 3):
            for with_pre in (False, True):
                B, T_out, C = ((1, 1, 4), (2, 7, 8), (2, 130, 68))[i % 3]
                for exact in (False, True) if i % 2 == 0 else (False,):
                    p = FR.c2i_inputs(B, T_out, C, K, s, extra, dt, exact=exact)
                    dcol, pre = _dev(p["dcol"], dtype), _dev(p["pre"], dtype) if with_pre else None
                    dx = _blank((B, p["T_in"], C), dtype)
                    ops.check(ops.lib().tav_col2im_1d(ops.ptr(dcol), ops.ptr(dx), ops.ptr(pre), ops.dt(dtype), B, p["T_in"], T_out, C, K, s, ops.stream()), "col2im_1d")
                    tag = f"col2im[{dt},B{B},T{T_out},C{C},K{K},s{s},+{extra},pre{int(with_pre)}{',int' if exact else ''}]"
                    ref = FR.c2i_ref(p, with_pre and not exact)
                    if exact:
                        _fx(rs, tag, dx, FR.held(ref["dx"], dt), dtype)
                    else:
                        _fb(rs, tag, dict(dx=dx), ref, ("dx",))
                i += 1
    return rs


def check_gelu_tanh_fp64():
    """tav_gelu_fwd (no other caller in the tests) and tav_gelu_bwd per element over [-12, 12], +-0 and +-40 at n = 4, 1020, 1028, both dtypes;
    tav_tanh_fwd / _bwd over [-10, 10], +-0 and +-90."""
    rs = []
    for dt in ("f32", "bf16"):
        for n in (4, 1020, 1028):
            p = FR.gelu_inputs(n, dt)
            x, dy = _dev(p["x"], _TDT[dt]), _dev(p["dy"], _TDT[dt])
            y, dx = _blank((n,), _TDT[dt]), _blank((n,), _TDT[dt])
            ops.check(ops.lib().tav_gelu_fwd(ops.ptr(x), ops.ptr(y), ops.dt(x), n, ops.stream()), "gelu_fwd")
            ops.check(ops.lib().tav_gelu_bwd(ops.ptr(x), ops.ptr(dy), ops.ptr(dx), ops.dt(x), n, ops.stream()), "gelu_bwd")
            _fb(rs, f"gelu[{dt},n{n}]", dict(y=y, dx=dx), FR.gelu_ref(p), ("y", "dx"))
    for n in (5, 260, 1029):
        p = FR.tanh_inputs(n)
        x, yin, dy = _dev(p["x"], _F32), _dev(p["y"], _F32), _dev(p["dy"], _F32)
        y, dx = _blank((n,), _F32), _blank((n,), _F32)
        ops.check(ops.lib().tav_tanh_fwd(ops.ptr(x), ops.ptr(y), n, ops.stream()), "tanh_fwd")
        ops.check(ops.lib().tav_tanh_bwd(ops.ptr(yin), ops.ptr(dy), ops.ptr(dx), n, ops.stream()), "tanh_bwd")
        _fb(rs, f"tanh[n{n}]", dict(y=y, dx=dx), FR.tanh_ref(p), ("y", "dx"))
    return rs


def _colsum_abi(p, nparts, accumulate, pitch):
    M, N = p["M"], p["N"]
    x = _dev(p["x"], _TDT[p["dt"]], pitch)
    part = _blank((nparts * N,), _F32)
    out = _filled(p["prev"]) if accumulate else _blank((N,), _F32)
    ops.check(ops.lib().tav_colsum(ops.ptr(x), ops.dt(x), M, N, x.stride(0), ops.ptr(part), nparts, ops.ptr(out), int(accumulate), ops.stream()), "colsum")
    return dict(out=out)


def check_colsum_fp64(dt):
    """tav_colsum: M = 1, 15, 17, 1000, 4097 x N = 1, 255, 257, 768, dense and with ld = N + 8, accumulating and not, nparts what ops.colsum
    computes, 1 (one block takes every row) and 256 (blocks without a row); M = 17 and 4097 also on integers."""
    rs, i = [], 0
    for M in (1, 15, 17, 1000, 4097):
        for N in (1, 255, 257, 768):
            nparts = (FR.colsum_nparts(M), 1, 256)[i % 3]
            pitch, acc = 8 * (i % 2), (i // 2) % 2 == 1
            p = FR.colsum_inputs(M, N, dt)
            tag = f"colsum[{dt},M{M},N{N},nparts{nparts},ld+{pitch},acc{int(acc)}]"
            _fb(rs, tag, _colsum_abi(p, nparts, acc, pitch), FR.colsum_ref(p, nparts, acc), ("out",))
            if M in (17, 4097):
                q = FR.colsum_inputs(M, N, dt, exact=True)
                _fx(rs, tag + ".int", _colsum_abi(q, nparts, True, pitch)["out"], FR.colsum_ref(q, nparts, True)["out"])
            i += 1
    return rs


def _pool_abi(p, lens, want32, lp):
    B, S, W = p["B"], p["S"], p["W"]
    x, dy = _dev(p["x"], _F32), _dev(p["dy"], _F32)
    y = _blank((B, W), _F32)
    dx = _blank((B, S, W), _F32) if want32 else None
    dl = _blank((B, S, W), torch.bfloat16) if lp else None
    lpd = ops.dt(torch.bfloat16) if lp else 0
    if lens is None:
        ops.check(ops.lib().tav_mean_pool_fwd(ops.ptr(x), ops.ptr(y), B, S, W, ops.stream()), "mean_pool_fwd")
        ops.check(ops.lib().tav_mean_pool_bwd(ops.ptr(dy), ops.ptr(dx), ops.ptr(dl), lpd, B, S, W, ops.stream()), "mean_pool_bwd")
    else:
        lt = _ints_dev(np.asarray(lens), torch.int32)
        ops.check(ops.lib().tav_mean_pool_fwd_len(ops.ptr(x), ops.ptr(y), ops.ptr(lt), B, S, W, ops.stream()), "mean_pool_fwd_len")
        ops.check(ops.lib().tav_mean_pool_bwd_len(ops.ptr(dy), ops.ptr(dx), ops.ptr(dl), lpd, ops.ptr(lt), B, S, W, ops.stream()), "mean_pool_bwd_len")
    return dict(y=y, dx_f32=dx, dx_lp=dl)


def check_mean_pool_fp64():
    """The mean pools, plain and length-aware: W = 4, 68 (the c < W guard of the last block decides), 768 x S = 1, 15, 16, 17, 77 x B = 1 | 3,
    lens among 0, 1, S and S + 5 (clamped), backward into f32 only, bf16 only and both; S = 16 | 64 and L_b powers of two on integers."""
    rs, i = [], 0
    for W in (4, 68, 768):
        for S in (1, 15, 16, 17, 77):
            B = (1, 3)[i % 2]
            want32, lp = ((True, False), (False, True), (True, True))[i % 3]
            for lens in (None, ((S + 5,), (0, 1, S + 5), (S,), (S, max(1, S // 2), 0))[(i % 2) + 2 * ((i // 2) % 2)]):
                p = FR.pool_inputs(B, S, W)
                tag = f"pool[B{B},S{S},W{W},lens{lens},f32{int(want32)},bf16{int(lp)}]"
                _fb(rs, tag, _pool_abi(p, lens, want32, lp), FR.pool_ref(p, lens), ("y", "dx_f32", "dx_lp"))
            i += 1
        for S, lens in ((16, None), (64, (16, 64, 0)), (64, (1, 69, 32))):
            q = FR.pool_inputs(3, S, W, exact=True)
            got, ref = _pool_abi(q, lens, True, True), FR.pool_ref(q, lens)
            tag = f"pool.int[S{S},W{W},lens{lens}]"
            _fx(rs, tag + ".y", got["y"], ref["y"])
            _fx(rs, tag + ".dx_f32", got["dx_f32"], ref["dx_f32"])
            _fx(rs, tag + ".dx_lp", got["dx_lp"], FR.held(ref["dx_lp"], "bf16"), torch.bfloat16)
    return rs


def _head_abi(p, bias, need_dx, need_db, accumulate):
    B, K, N = p["B"], p["K"], p["N"]
    x, W, dy = _dev(p["x"], _F32), _dev(p["W"], _F32), _dev(p["dy"], _F32)
    b = _dev(p["bias"], _F32) if bias else None
    y = _blank((B, N), _F32)
    ops.check(ops.lib().tav_head_fwd(ops.ptr(x), ops.ptr(W), ops.ptr(b), ops.ptr(y), B, K, N, ops.stream()), "head_fwd")
    dx = _blank((B, K), _F32) if need_dx else None
    dW = _filled(p["prev_W"]) if accumulate else _blank((N, K), _F32)
    db = None if not need_db else (_filled(p["prev_b"]) if accumulate else _blank((N,), _F32))
    ops.check(ops.lib().tav_head_bwd(ops.ptr(x), ops.ptr(W), ops.ptr(dy), ops.ptr(dx), ops.ptr(dW), ops.ptr(db), B, K, N, int(accumulate), ops.stream()), "head_bwd")
    return dict(y=y, dx=dx, dW=dW, db=db)


def check_head_fp64():
    """tav_head_fwd / _bwd: K = 1, 63, 65 (lanes idle in the dot product), 3072 x N = 1, 7, 256 x B = 1 | 5; bias NULL; the backward without
    dx, without db, and accumulating; half of the shapes also on integers."""
    rs, i = [], 0
    for K in (1, 63, 65, 3072):
        for N in (1, 7, 256):
            for B in (1, 5):
                bias = i % 3 != 1
                need_dx, need_db, acc = ((True, True, False), (False, True, False), (True, False, False), (True, True, True))[i % 4]
                for exact in (False, True) if i % 2 == 0 else (False,):
                    p = FR.head_inputs(B, K, N, exact=exact)
                    tag = f"head[B{B},K{K},N{N},bias{int(bias)},dx{int(need_dx)},db{int(need_db)},acc{int(acc)}{',int' if exact else ''}]"
                    got, ref = _head_abi(p, bias, need_dx, need_db, acc), FR.head_ref(p, bias, acc)
                    if exact:
                        for n in ("y", "dx", "dW", "db"):
                            if got[n] is not None:
                                _fx(rs, f"{tag}.{n}", got[n], ref[n])
                    else:
                        _fb(rs, tag, got, ref, ("y", "dx", "dW", "db"))
                i += 1
    return rs


def check_cross_entropy_fp64():
    """tav_cross_entropy: C = 1, 2, 7, 64 x B = 1, 3, 255, 257, 600 (the loop over B > 256), rows of randn 2^(r % 5), rows offset by +-80 and
    +-3e4, rows with one logit 60 above the rest; class weights 2^-3 .. 2^3 or none, grad_scale 1, 1 / 8, 3, loss only, dlogits only, both."""
    rs, i = [], 0
    for C in (1, 2, 7, 64):
        for B in (1, 3, 255, 257, 600):
            weighted, gs = i % 2 == 0, (1.0, 0.125, 3.0)[i % 3]
            want_loss, want_grad = ((True, True), (True, False), (False, True))[(i // 2) % 3]
            p = FR.ce_inputs(B, C)
            z, t = _dev(p["z"], _F32), _ints_dev(p["t"], torch.int64)
            cw = _dev(p["cw"], _F32) if weighted else None
            loss = _blank((1,), _F32) if want_loss else None
            dl = _blank((B, C), _F32) if want_grad else None
            ops.check(ops.lib().tav_cross_entropy(ops.ptr(z), ops.ptr(t), ops.ptr(cw), ops.ptr(loss), ops.ptr(dl), B, C, gs, ops.stream()), "cross_entropy")
            _fb(rs, f"ce[B{B},C{C},cw{int(weighted)},gs{gs},loss{int(want_loss)},grad{int(want_grad)}]", dict(loss=loss, dlogits=dl), FR.ce_ref(p, weighted, gs),
                ("loss", "dlogits"))
            i += 1
    return rs


def check_text_index_fp64():
    """text_pos_ids_kernel and the three-table sum on integers: S = 63, 64, 65, 512, 513, 1024 (the scan width changes at 64, 128, ... 1024),
    pads at the front, in the interior, as a suffix, a row of all pads and one without, pad_id = 1, 0, -1: pos_ids and pre bit for bit."""
    rs = []
    one, zero = np.ones(8), np.zeros(8)
    for S in (63, 64, 65, 512, 513, 1024):
        for pad_id in (1, 0, -1):
            p = FR.text_inputs(5, S, pad_id)
            ref = FR.text_ref(p)
            _, _, pre, pos_ids, _, _ = ops.text_embed_fwd(_ints_dev(p["ids"], torch.int64), _dev(p["word"], _F32), _dev(p["pos"], _F32), _dev(p["type"], _F32),
                                                          _dev(one, _F32), _dev(zero, _F32), 1e-5, pad_id)
            rs += [_exact(f"text.pos_ids[S{S},pad{pad_id}]", pos_ids, torch.from_numpy(ref["pos_ids"]).to(DEV)),
                   _exact(f"text.pre[S{S},pad{pad_id}]", pre, _want(ref["pre"], _F32))]
    return rs


def check_embed_add_fp64():
    """tav_embed_add_fwd / _bwd on integers: ntable = 1, 3, 8 (the register array's size), rows = 1, 257, 65536 + 300 (past the 256-part cap),
    accumulating and not."""
    rs, i = [], 0
    for ntable in (1, 3, 8):
        for rows in (1, 257, 65536 + 300):
            W = 4 if rows > 1000 else 260
            acc = i % 2 == 0
            p = FR.embed_inputs(rows, W, ntable)
            ref = FR.embed_ref(p, acc)
            ids, x, table, dy = _ints_dev(p["ids"], torch.int64), _dev(p["x"], _F32), _dev(p["table"], _F32), _dev(p["dy"], _F32)
            out = _blank((rows, W), _F32)
            ops.check(ops.lib().tav_embed_add_fwd(ops.ptr(x), ops.ptr(ids), ops.ptr(table), ops.ptr(out), rows, W, ntable, ops.stream()), "embed_add_fwd")
            nparts = ops.lib().tav_embed_add_bwd_parts(rows)
            assert nparts == FR.embed_parts(rows)
            part = _blank((nparts * ntable * W,), _F32)
            d = _filled(p["prev"]) if acc else _blank((ntable, W), _F32)
            ops.check(ops.lib().tav_embed_add_bwd(ops.ptr(dy), ops.ptr(ids), ops.ptr(d), ops.ptr(part), rows, W, ntable, int(acc), ops.stream()), "embed_add_bwd")
            tag = f"embed_add[rows{rows},W{W},ntable{ntable},acc{int(acc)}]"
            _fx(rs, tag + ".fwd", out, ref["out"])
            _fx(rs, tag + ".dtable", d, ref["dtable"])
            i += 1
    return rs


def check_scatter_add_fp64():
    """tav_scatter_add_rows on integers onto integer contents: rows = 1, 17, 1025, 4096 x W = 4, 132, 1024, one index carried by 1, 16, 17 rows
    and by a quarter of them (one wave, sixteen waves, a second round of the waves)."""
    rs = []
    for rows in (1, 17, 1025, 4096):
        for W in (4, 132, 1024):
            p = FR.scatter_inputs(rows, W)
            d, idx, table = _dev(p["d"], _F32), _ints_dev(p["idx"], torch.int64), _filled(p["prev"])
            ops.check(ops.lib().tav_scatter_add_rows(ops.ptr(d), ops.ptr(idx), ops.ptr(table), rows, W, p["ntable"], ops.stream()), "scatter_add_rows")
            _fx(rs, f"scatter_add[rows{rows},W{W}]", table, FR.scatter_ref(p)["dtable"])
    return rs


def check_index_copies_fp64():
    """mask_to_index at n = 255, 256, 257, 1568 with nkeep = 1 and nkeep = n, both keep values, a row without a kept token; gather_rows and
    patchify on spread data with indices past both ends (clamped): every one a copy with one right answer."""
    rs = []
    rng = np.random.default_rng(5)
    for n in (255, 256, 257, 1568):
        mask = (rng.random((3, n)) < 0.4).astype(np.uint8)
        mask[2] = 0
        mask[0, -1] = 1
        for keep in (1, 0):
            for nkeep in (1, n):
                idx, counts = ops.mask_to_index(_ints_dev(mask, torch.uint8), keep, nkeep)
                wi, wc = FR.mask_to_index_ref(mask, keep, nkeep)
                rs += [_exact(f"mask_to_index[n{n},keep{keep},nkeep{nkeep}].idx", idx, torch.from_numpy(wi).to(DEV)),
                       _exact(f"mask_to_index[n{n},keep{keep},nkeep{nkeep}].counts", counts, torch.from_numpy(wc).to(DEV))]
    table = FR.gp_inputs(1, 37, 260, "f32")[0]
    gi = np.concatenate([rng.integers(0, 37, size=300), [-3, 37, 1 << 20, 0, 36]]).astype(np.int32)
    _fx(rs, "gather_rows", ops.gather_rows(_dev(table, _F32), _ints_dev(gi, torch.int32)), FR.gather_ref(table, gi))
    video = FR.f32(rng.standard_normal((2, 4, 3, 32, 48)) * 2.0 ** (np.arange(48) % 7 - 3.0))
    keep = np.array([[0, 5, 11, 3], [7, 1 << 20, -1, 6]], dtype=np.int32)
    for dt in ("f32", "bf16"):
        got = ops.patchify(_dev(video, _F32), _ints_dev(keep, torch.int32), _TDT[dt])
        _fx(rs, f"patchify[{dt}]", got, FR.held(FR.patchify_ref(video, keep), dt), _TDT[dt])
    return rs


def front_fp64_checks():
    """The front-end, pooling, head, loss and index cases against fp64, in the order all_checks() appends them."""
    out = []
    for dt_ in ("f32", "bf16"):
        out.append(lambda d=dt_: check_conv0_fwd_fp64(d))
        for Cs in ((8, 64), (512, 520)):
            out.append(lambda d=dt_, c=Cs: check_conv0_bwd_fp64(d, c))
        out.append(lambda d=dt_: check_col2im_fp64(d))
        out.append(lambda d=dt_: check_colsum_fp64(d))
    for shape in ((8, 4, 3), (256, 64, 128), (260, 4, 1), (1024, 256, 4)):
        out.append(lambda s=shape: check_weight_norm_fp64(*s))
    out += [lambda: check_weight_norm_fp64(768, 48, 128, "f"), lambda: check_weight_norm_fp64(768, 48, 128, "b")]
    out += [check_group_pad_fp64, check_gelu_tanh_fp64, check_mean_pool_fp64, check_head_fp64, check_cross_entropy_fp64, check_text_index_fp64,
            check_embed_add_fp64, check_scatter_add_fp64, check_index_copies_fp64]
    return out


# ------------------------------------------------------------------------------------------------ non-finite values ("Non-finite values")
# Every case launches its kernel clean once and once per placement with ONE operand element replaced by a poison pattern (tests/nonfinite_ref.py),
# and NF.verdict() holds the two launches against the three sets the fp64 reference of the same two problems gives: non-finite exactly where the
# reference is, bit-equal to the clean launch where the reference did not move, inside the family's existing bound where it moved.
@contextlib.contextmanager
def _poisoned(t, index, pat):
    """Inside: element `index` of the device tensor holds pattern `pat`, written through an integer view; afterwards its own bits are back (the
    guard's snapshot of an operand must still match)."""
    dn = "f32" if t.dtype == torch.float32 else "bf16"
    v = t.view(torch.int32 if dn == "f32" else torch.int16)
    old = v[index].clone()
    v[index] = NF.signed_bits(pat, dn)
    try:
        yield
    finally:
        v[index] = old


def _np(t):
    return t.detach().double().cpu().numpy()


def _fp8_bytes(t):
    return NF.e4m3_decode(t.view(torch.uint8).cpu().numpy())


def _quantize_form(x, state, want_t, delayed):
    rows, cols = x.shape
    rows_pad = (rows + ops.FP8_KPAD - 1) // ops.FP8_KPAD * ops.FP8_KPAD
    q = _blank((rows, cols), torch.uint8)
    qt = _blank((cols, rows_pad), torch.uint8) if want_t else None
    fn = ops.lib().tav_fp8_quantize_delayed if delayed else ops.lib().tav_fp8_quantize
    ops.check(fn(ops.ptr(x), ops.dt(x), rows, cols, x.stride(0), ops.ptr(state), ops.ptr(q), cols, ops.ptr(qt), rows_pad, rows_pad, ops.stream()), "fp8_quantize")
    return q, qt


def check_nonfinite_fp8_quantize(dtype, delayed):
    """tav_fp8_quantize / tav_fp8_quantize_delayed, streaming kernel (q only, cols % 8 == 0) and tiled kernel (q + qt; q only with cols % 8 != 0),
    at a scale that saturates half the range: a NaN or +-Inf input element becomes an e4m3 NaN byte in q and in the matching byte of qt, every
    other byte is the clean launch's, the padding of qt stays zero; state[0..2] are untouched, state[3] is the maximum over the FINITE elements
    bit for bit (the plain entry leaves state[3] alone)."""
    dn = _GDT[dtype]
    rs, launch = [], 0
    for rows, cols0 in NF.FP8_SHAPES:
        for form, cols, want_t in (("stream", cols0, False), ("tiled q+qt", cols0, True), ("tiled cols%8", cols0 - 4, False)):
            x64 = NF.fp8_inputs(rows, cols, dn)
            x = _up(x64, dtype)
            a0 = float(NF.finite_amax(x64)) * 0.5
            state = _fp8_state(a0)
            scale = float(state[0].item())
            qc, qtc = _quantize_form(x, state, want_t, delayed)
            for site in NF.fp8_sites(rows, cols):
                pat = launch % NF.NPAT
                launch += 1
                xp, _, rp, sets, _ = NF.fp8_quantize_case(rows, cols, dn, site, pat, scale)
                state = _fp8_state(a0)
                s0 = state.clone()
                with _poisoned(x, site, pat):
                    q, qt = _quantize_form(x, state, want_t, delayed)
                tag = f"nonfinite.fp8.{'delayed' if delayed else 'plain'}[{dn},{rows}x{cols},{form},{NF.NAMES[pat]}@{site}]"
                rs += NF.verdict(tag + ".q", _fp8_bytes(qc), _fp8_bytes(q), rp, None, sets)
                if want_t:
                    tsets = {k: v.T for k, v in sets.items()}
                    rs += NF.verdict(tag + ".qt", _fp8_bytes(qtc[:, :rows]), _fp8_bytes(qt[:, :rows]), rp.T, None, tsets)
                    pad = int(qt[:, rows:].ne(0).sum().item())
                    rs.append((tag + ".qt_pad bytes zero", float(pad), 0.0, pad == 0))
                rs.append(_exact(tag + ".state[0:3] unchanged", _bits(state[:3]), _bits(s0[:3])))
                want3 = torch.tensor([float(NF.finite_amax(xp))], device=DEV) if delayed else s0[3:4]
                rs.append(_exact(tag + ".state[3] over the finite elements", _bits(state[3:4]), _bits(want3)))
                rs.append(_all_ff(tag + ".gap", state[4:]))
    return rs


def check_nonfinite_fp8_saturation():
    """A hand-made state with amax 1e-30: state[0] = 4.48e32 is finite and x state[0] overflows f32 for the finite x = +-1e10, which must still
    saturate to +-448 (0x7e / 0xfe) next to a NaN and an Inf that become NaN bytes: the class of the INPUT decides.  Both kernels, both entries,
    both dtypes."""
    vals = [1e10, -1e10, 1e-32, 0.0, 1e30, -1e-30, 1.0, -1.0] * 4
    rs = []
    for dtype in (torch.float32, torch.bfloat16):
        dn = _GDT[dtype]
        x64 = GR.round_to(np.array(vals).reshape(4, 8), dn)[0]
        for delayed in (False, True):
            for want_t in (False, True):
                x = _up(x64, dtype)
                xp = x64
                sites = [((1, 0), 0), ((2, 1), 3), ((3, 6), 4), ((3, 7), 1)]
                state = _fp8_state(1e-30)
                scale = float(state[0].item())
                with np.errstate(over="ignore"):
                    assert np.isfinite(scale) and np.isinf(np.float32(1e10) * np.float32(scale))
                with contextlib.ExitStack() as es:
                    for site, pat in sites:
                        es.enter_context(_poisoned(x, site, pat))
                        xp = NF.plant(xp, site, pat, dn)
                    q, qt = _quantize_form(x, state, want_t, delayed)
                ref = NF.e4m3_quantize(xp, scale)
                got = _fp8_bytes(q)
                tag = f"nonfinite.fp8.saturation[{dn},{'delayed' if delayed else 'plain'},{'q+qt' if want_t else 'q'}]"
                same = np.isnan(ref) == np.isnan(got)
                bad = int((~same).sum()) + int((np.nan_to_num(ref, nan=0.0) != np.nan_to_num(got, nan=0.0)).sum())
                rs.append((tag + ".q bytes (finite inputs saturate, non-finite inputs are NaN bytes)", float(bad), 0.0, bad == 0))
                sat, want_sat = (int((np.abs(np.nan_to_num(t_, nan=0.0)) == 448.0).sum()) for t_ in (got, ref))
                assert want_sat >= 8                                  # (+-1e10 in every row: the reference itself saturates)
                rs.append((tag + f".saturated elements {sat} (reference {want_sat})", float(abs(sat - want_sat)), 0.0, sat == want_sat))
                if want_t:
                    gt = _fp8_bytes(qt[:, :4]).T
                    bad = int((np.isnan(gt) != np.isnan(got)).sum()) + int((np.nan_to_num(gt, nan=0.0) != np.nan_to_num(got, nan=0.0)).sum())
                    rs.append((tag + ".qt == q^T", float(bad), 0.0, bad == 0))
                if delayed:
                    rs.append(_exact(tag + ".state[3]", _bits(state[3:4]), _bits(torch.tensor([float(NF.finite_amax(xp))], device=DEV))))
    return rs


def check_nonfinite_fp8_amax():
    """tav_fp8_amax: a NaN is not counted (the scales are those of the finite elements, bit for bit), an Inf falls back to scale 1; no word of
    the scales is ever non-finite."""
    rs = []
    for dtype in (torch.float32, torch.bfloat16):
        dn = _GDT[dtype]
        for rows, cols in NF.FP8_SHAPES:
            x64 = NF.fp8_inputs(rows, cols, dn)
            x = _up(x64, dtype)
            top = tuple(int(i) for i in np.unravel_index(np.abs(x64).argmax(), x64.shape))
            for k, site in enumerate(NF.fp8_sites(rows, cols) + [top]):            # (the largest element itself poisoned as well)
                for pat in ((k % NF.NPAT, (k + 3) % NF.NPAT) if site != top else range(NF.NPAT)):
                    scales = _blank((5,), torch.float32)
                    part = ops.workspace("fp8_amax", ops.lib().tav_fp8_amax_partials(rows, cols), x.device)
                    with _poisoned(x, site, pat):
                        ops.check(ops.lib().tav_fp8_amax(ops.ptr(x), ops.dt(x), rows, cols, x.stride(0), ops.ptr(part), ops.ptr(scales), ops.stream()), "fp8_amax")
                    want = torch.from_numpy(NF.amax_scales(NF.plant(x64, site, pat, dn))).to(DEV)
                    tag = f"nonfinite.fp8.amax[{dn},{rows}x{cols},{NF.NAMES[pat]}@{site}]"
                    rs.append(_exact(tag, _bits(scales[:3]), _bits(want)))
                    rs.append(_all_ff(tag + ".tail", scales[3:]))
    return rs


@functools.lru_cache(maxsize=None)
def _nf_fp8_nt(M, N, K):
    x = GR.nt_inputs(M, N, K, "fp8", seed=9100 + M + N + K)
    return x, GR.nt_ref(x, bias=True, out_dtype="f32")


def _fp8_dev(a):
    return _in(torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV).to(ops.FP8))


@contextlib.contextmanager
def _nan_byte(t, index, pat):
    v = t.view(torch.uint8)
    old = v[index].clone()
    v[index] = NF.E4M3_NAN[pat % 2]
    try:
        yield
    finally:
        v[index] = old


def check_nonfinite_fp8_gemm(M, N, K, hint):
    """The fp8 tav_gemm_nt with an e4m3 NaN byte (0x7f / 0xff) planted in a q operand: an A byte poisons its output row, a B byte its column,
    everything else is the clean launch bit for bit."""
    x, rc = _nf_fp8_nt(M, N, K)
    a8, b8 = _fp8_dev(x["a"]), _fp8_dev(x["b"])
    sa, sb = _in(torch.tensor([x["sa"]], dtype=torch.float32, device=DEV)), _in(torch.tensor([x["sb"]], dtype=torch.float32, device=DEV))
    bias = _up(x["bias"], torch.float32)

    def run():
        return ops.gemm_nt(a8, b8, a_dequant=sa, b_dequant=sb, bias=bias, out_dtype=torch.float32, tile_m=hint)
    clean = _np(run())
    bad = int((~np.isfinite(clean)).sum())
    rs = [(f"nonfinite.fp8.gemm_nt[M{M},N{N},K{K},tm{hint}].clean launch finite", float(bad), 0.0, bad == 0)]
    for launch, (tensor, index, kind) in enumerate(NF.fp8_nt_sites(M, N, K, hint)):
        rp, sets = NF.fp8_nt_case(x, rc, tensor, index)
        with _nan_byte(a8 if tensor == "a" else b8, index, launch):
            got = _np(run())
        tag = f"nonfinite.fp8.gemm_nt[M{M},N{N},K{K},tm{hint},{tensor}{index} byte {NF.E4M3_NAN[launch % 2]:#x}]"
        rs += NF.verdict(tag, clean, got, rp["out"], rp["out_bound"], sets)
    return rs


def check_nonfinite_fp8_wgrad(T=333, N1=132, N2=256):
    """ops.wgrad_fp8 (the NT GEMM of the transposed copies in eight K-slices + tav_splitk_reduce): a NaN byte in dY^T poisons a dW row, one in
    X^T a dW column, at the first token, the last one and one of a middle slice."""
    ops.clear_workspaces()
    p = NF.fp8_wgrad_problem(T, N1, N2)
    rows_pad = p["at"].shape[1]
    at, bt = _fp8_dev(p["at"]), _fp8_dev(p["bt"])
    sa, sb = _in(torch.tensor([1.0, p["sa"], 1.0], dtype=torch.float32, device=DEV)), _in(torch.tensor([1.0, p["sb"], 1.0], dtype=torch.float32, device=DEV))
    dy8, x8 = ops.Fp8(None, at, sa, T, N1), ops.Fp8(None, bt, sb, T, N2)
    clean = _np(ops.wgrad_fp8(dy8, x8))
    rc = NF.fp8_wgrad_ref(p)
    bad = int((~np.isfinite(clean)).sum())
    rs = [(f"nonfinite.fp8.wgrad[T{T},N1{N1},N2{N2},Kp{rows_pad}].clean launch finite", float(bad), 0.0, bad == 0)]
    for launch, (tensor, index) in enumerate(NF.fp8_wgrad_sites(T, N1, N2)):
        rp, sets = NF.fp8_wgrad_case(p, rc, tensor, index)
        with _nan_byte(at if tensor == "at" else bt, index, launch):
            got = _np(ops.wgrad_fp8(dy8, x8))
        rs += NF.verdict(f"nonfinite.fp8.wgrad[T{T},{tensor}{index} byte {NF.E4M3_NAN[launch % 2]:#x}]", clean, got, rp["out"], rp["out_bound"], sets)
    return rs


@functools.lru_cache(maxsize=4)                                       # (a few 333 x 384 fp64 arrays each: only a site two hints share is worth keeping)
def _nf_nt_case(dname, flavour, tensor, index, pat):
    M, N, K = NF.NT_SHAPE
    return NF.nt_case(_nt_problem(dname, M, N, K), _nt_reference(dname, M, N, K, flavour), flavour, tensor, index, pat)


def check_nonfinite_gemm_nt(dtype, hint):
    """tav_gemm_nt at M 333, N 384, K 256, the flavours NF.nt_flavours(): poison in A (an output row, and C_pre's), B (a column), the bias (a
    column), the f32 residual, gelu_in and the accumulate-prev tensor (one element each), at the first row / column, the last one (the ragged
    tail tile) and one on a tile boundary, with k = 0, K - 1 and a k of a middle K-tile; the pattern rotates with every launch."""
    dname = _GDT[dtype]
    M, N, K = NF.NT_SHAPE
    x = _nt_problem(dname, M, N, K)
    dev = {"a": _up(x["a"], dtype), "b": _up(x["b"], dtype)}
    rs, launch = [], 0
    for name in NF.nt_flavours(dname):
        kw = GR.FLAVOURS[name]
        odt = torch.float32 if (dtype == torch.float32 or kw.get("out_dtype") == "f32") else torch.bfloat16
        prev = "cprev_" + ("f32" if odt == torch.float32 else "bf16")
        for key, tensor, dt_ in (("bias", "bias", torch.float32), ("resid", "resid", torch.float32), ("gelu_in", kw.get("gelu_in"), dtype), ("accumulate", prev, odt)):
            if kw.get(key) and tensor not in dev:
                dev[tensor] = _up(x[tensor], dt_)

        def run():
            args = dict(tile_m=hint, out_dtype=odt, act=kw.get("act", 0), want_pre=kw.get("want_pre", False), alpha=kw.get("alpha", 1.0))
            for key, tensor in (("bias", "bias"), ("resid", "resid"), ("gelu_in", kw.get("gelu_in"))):
                if kw.get(key):
                    args[key] = dev[tensor]
            if kw.get("accumulate"):
                out = _blank((M, N), odt)
                out.copy_(dev[prev])
                args.update(out=out, accumulate=True)
            res = ops.gemm_nt(dev["a"], dev["b"], **args)
            out, pre = res if isinstance(res, tuple) else (res, None)
            return _np(out), (None if pre is None else _np(pre))
        clean, clean_pre = run()
        for tensor, index, kind in NF.nt_sites(dname, hint, name):
            pat = launch % NF.NPAT
            launch += 1
            rp, sets, pre_sets = _nf_nt_case(dname, name, tensor, index, pat)
            with _poisoned(dev[tensor], index, pat):
                got, got_pre = run()
            tag = f"nonfinite.gemm_nt[{dname},tm{hint},{name},{NF.NAMES[pat]}@{tensor}{index}]"
            rs += NF.verdict(tag, clean, got, rp["out"], rp["out_bound"], sets)
            if pre_sets is not None:
                rs += NF.verdict(tag + ".pre", clean_pre, got_pre, rp["pre"], rp["pre_bound"], pre_sets)
    return rs


_NF_TN_VARIANTS = [("plain", dict(), 0), ("chunk64,scale", dict(scale=0.37), 64), ("conv perm", dict(perm=(88, 3)), 0)]


def check_nonfinite_gemm_tn(dtype, rows, nbatch):
    """tav_gemm_tn at check_gemm_tn_bounded's widths and a token count that is no multiple of the 64-row K-tile: an A element poisons one dW
    row and that element of dbias (dbias is A's column sum: tavhip.h), a B element one dW column and nothing of dbias."""
    dname = _GDT[dtype]
    N1, N2 = NF.TN_WIDTHS
    x = _tn_problem(dname, rows * nbatch, N1, N2)
    dev = dict(a=_up(x["a"], dtype), b=_up(x["b"], dtype))
    rs, launch = [], 0
    for name, kw, chunk in _NF_TN_VARIANTS:
        ops.clear_workspaces()
        out, dbias, ns = _tn_call(dev["a"], dev["b"], N1, N2, rows, nbatch, chunk_rows=chunk, **kw)
        clean, clean_b = _np(out), _np(dbias)
        rc = GR.tn_ref(x, nsplit=ns, **kw)
        for tensor, index in NF.tn_sites(rows * nbatch, N1, N2):
            pat = launch % NF.NPAT
            launch += 1
            rp, sets, bsets = NF.tn_case(x, rc, tensor, index, pat, nsplit=ns, **kw)
            with _poisoned(dev[tensor], index, pat):
                out, dbias, _ = _tn_call(dev["a"], dev["b"], N1, N2, rows, nbatch, chunk_rows=chunk, **kw)
            tag = f"nonfinite.gemm_tn[{dname},rows{rows},nb{nbatch},{name},{NF.NAMES[pat]}@{tensor}{index}]"
            rs += NF.verdict(tag, clean, _np(out), rp["out"], rp["out_bound"], sets)
            rs += NF.verdict(tag + ".dbias", clean_b, _np(dbias), rp["dbias"], rp["dbias_bound"], bsets)
    return rs


def check_nonfinite_gemm_tn_grouped(dtype, rows=130):
    """tav_gemm_tn_grouped (what a too small workspace falls back to) and every tav_gemm_tn_grouped_ws form: the poison sits in problem 1 of
    four; its dW / db follow tav_gemm_tn's rule, the other three problems are the clean launch bit for bit."""
    dname = _GDT[dtype]
    xs = [_tn_problem(dname, rows, n1, n2, seed=50 + k) for k, (n1, n2) in enumerate(_GROUP_SHAPES)]
    pairs = [(_up(x["a"], dtype), _up(x["b"], dtype)) for x in xs]
    N1, N2 = _GROUP_SHAPES[1]
    rs, launch = [], 0
    for name, flags, nsplit in _grouped_forms(dtype, rows):
        clean = [(_np(dW), _np(db)) for dW, db in _grouped_run(pairs, flags)]
        rc = GR.tn_ref(xs[1], nsplit=nsplit)
        for tensor, index in NF.tn_sites(rows, N1, N2):
            pat = launch % NF.NPAT
            launch += 1
            rp, sets, bsets = NF.tn_case(xs[1], rc, tensor, index, pat, nsplit=nsplit)
            with _poisoned(pairs[1][0 if tensor == "a" else 1], index, pat):
                got = [(_np(dW), _np(db)) for dW, db in _grouped_run(pairs, flags)]
            tag = f"nonfinite.gemm_tn_grouped[{dname},rows{rows},{name},{NF.NAMES[pat]}@{tensor}1{index}]"
            rs += NF.verdict(tag + ".dW1", clean[1][0], got[1][0], rp["out"], rp["out_bound"], sets)
            rs += NF.verdict(tag + ".db1", clean[1][1], got[1][1], rp["dbias"], rp["dbias_bound"], bsets)
            for k in (0, 2, 3):                                     # the other problems: all of it U
                for j, what in enumerate(("dW", "db")):
                    every = np.ones(clean[k][j].shape, dtype=bool)
                    rs += NF.verdict(f"{tag}.{what}{k}", clean[k][j], got[k][j], clean[k][j], None, dict(N=~every, U=every, C=~every))[:2]
    return rs


def _nf_arena(sizes, flat, mis=False):
    A = _Arena(sizes, mis)
    A.put(flat)
    return A


@contextlib.contextmanager
def _poisoned_flat(arena, site, pat):
    """Element `site` of the concatenated tensors of an _Arena holds pattern `pat`."""
    with _poisoned(arena.buf, int(arena.idx[site].item()), pat):
        yield


def check_nonfinite_sumsq():
    """tav_sumsq_multi, tav_sumsq_chunked and tav_sum_partials: one NaN among the gradients gives a NaN sum, one +-Inf gives +Inf -- the class
    and the kind the fp64 sum of squares has."""
    L = ops.lib()
    sizes = SR.SIZE_LISTS[NF.STEP_SIZES]
    nt = len(sizes)
    _, g0 = SR.make_inputs(sum(sizes), seed=77 + nt)
    rs, launch = [], 0
    for mis in (False, True):
        G = _nf_arena(sizes, g0, mis)
        t_g, t_s = G.table(), _i64(sizes)
        pre, nchunks = SR.chunk_prefix(sizes, int(L.tav_optim_chunk_elems()))
        t_c = _i32(pre)
        n_part = int(L.tav_sumsq_partials(nt))
        for site in NF.step_sites(sizes):
            for k in range(2 if launch else NF.NPAT):                # all five patterns at the first site, two (rotating) at the others
                pat = (launch + k) % NF.NPAT
                want = NF.sumsq_ref(NF.plant(g0, site, pat))
                outs, part_c, part_m = _blank((4,), torch.float32), _blank((nchunks,), torch.float32), _blank((n_part,), torch.float32)
                with _poisoned_flat(G, site, pat):
                    ops.check(L.tav_sumsq_chunked(ops.ptr(t_g), ops.ptr(t_s), ops.ptr(t_c), nt, nchunks, ops.ptr(part_c), ops.ptr(outs[0:1]), ops.stream()), "sumsq_chunked")
                    ops.check(L.tav_sumsq_multi(ops.ptr(t_g), ops.ptr(t_s), nt, ops.ptr(part_m), ops.ptr(outs[1:2]), ops.stream()), "sumsq_multi")
                    ops.check(L.tav_sum_partials(ops.ptr(part_c), nchunks, ops.ptr(outs[2:3]), ops.stream()), "sum_partials")
                got = outs[:3].cpu().numpy().astype(np.float64)
                for form, v in zip(("chunked", "multi", "sum_partials"), got):
                    ok = bool(np.isnan(v)) if np.isnan(want) else bool(v == want)
                    rs.append((f"nonfinite.sumsq[{'+4B' if mis else 'aligned'},{NF.NAMES[pat]}@{site}].{form} = {v} (fp64: {want})", 0.0 if ok else 1.0, 0.0, ok))
                rs.append(_all_ff("nonfinite.sumsq.gap", G.gaps(), outs[3:4]))
            launch += 2
    return rs


def _adamw_launch(form, A, G, sizes, scal, step, wd):
    L = ops.lib()
    nt = len(sizes)
    tp, tm, tv = (A[k].table() for k in "pmv")
    t_g, t_s = G.table(), _i64(sizes)
    pre, nchunks = SR.chunk_prefix(sizes, int(L.tav_optim_chunk_elems()))
    b1, b2 = SR.BETAS
    coef, lr, bc = ops.ptr(scal[1:2]), ops.ptr(scal[4:5]), ops.ptr(scal[5:7])
    if form == "multi":
        ops.check(L.tav_adamw_multi(ops.ptr(tp), ops.ptr(t_g), ops.ptr(tm), ops.ptr(tv), ops.ptr(t_s), nt, coef, lr, b1, b2, SR.EPS, wd, ops.ptr(step), bc,
                                    ops.stream()), "adamw_multi")
    elif form == "chunked":
        ops.check(L.tav_adamw_chunked(ops.ptr(tp), ops.ptr(t_g), ops.ptr(tm), ops.ptr(tv), ops.ptr(t_s), ops.ptr(_i32(pre)), nt, nchunks, coef, lr, b1, b2,
                                      SR.EPS, wd, ops.ptr(step), bc, ops.stream()), "adamw_chunked")
    else:
        hyper = _in(torch.tensor([[float(scal[4].item()), wd]], dtype=torch.float32, device=DEV))
        ops.check(L.tav_adamw_chunked_groups(ops.ptr(tp), ops.ptr(t_g), ops.ptr(tm), ops.ptr(tv), ops.ptr(t_s), ops.ptr(_i32(pre)), nt, nchunks, coef,
                                             ops.ptr(_i32([0] * nt)), ops.ptr(hyper), 1, b1, b2, SR.EPS, ops.ptr(step), bc, ops.stream()), "adamw_chunked_groups")
    return {k: A[k].get() for k in "pmv"}


def check_nonfinite_adamw(form):
    """tav_adamw_multi / _chunked / _chunked_groups, step 2 from non-zero moments with a clip coefficient of 0.37: a NaN or +-Inf gradient
    element makes exactly that element of p, exp_avg and exp_avg_sq non-finite (an Inf second moment gives inf / inf in the update) and leaves
    every other element the clean launch's bits; a NaN clip coefficient makes EVERY element of all three non-finite."""
    sizes = SR.SIZE_LISTS[NF.STEP_SIZES]
    p0, g0, m0, v0 = NF.adamw_state(SR)
    G = _nf_arena(sizes, g0, True)

    def run(site, pat):
        A = dict(p=_nf_arena(sizes, p0), m=_nf_arena(sizes, m0), v=_nf_arena(sizes, v0))
        scal, step = _blank((8,), torch.float32), _blank((1,), torch.int32)
        step.fill_(1)
        scal[4] = SR.LR
        scal[1] = SR.CLIP_STEP2
        with contextlib.ExitStack() as es:
            if site is not None:
                es.enter_context(_poisoned_flat(G, site, pat))
            elif pat is not None:
                es.enter_context(_poisoned(scal, 1, pat))
            got = _adamw_launch(form, A, G, sizes, scal, step, SR.WD)
        gaps = _all_ff(f"nonfinite.adamw[{form}].gap", *[A[k].gaps() for k in "pmv"], scal[0:1], scal[2:4], scal[7:8])
        return got, gaps
    clean, gap = run(None, None)
    rs = [gap]
    cases = [(site, (i + j) % NF.NPAT) for i, site in enumerate(NF.step_sites(sizes)) for j in ((0, 3, 4) if i == 0 else (1 + i, 3 + i))] + [(None, 0), (None, 1)]
    for site, pat in cases:
        rc, rp, sets = NF.adamw_case(p0, g0, m0, v0, 2, SR.f32(SR.LR), SR.WD, SR.CLIP_STEP2, site, pat, SR.ref_step)
        got, gap = run(site, pat)
        rs.append(gap)
        for k, nm in zip("pmv", ("p", "exp_avg", "exp_avg_sq")):
            tag = f"nonfinite.adamw[{form},{NF.NAMES[pat]}@{'clip coefficient' if site is None else site}].{nm}"
            rs += NF.verdict(tag, clean[k], got[k], rp[k], rp[k + "_bound"], sets[k])
    return rs


def check_nonfinite_cross_entropy():
    """tav_cross_entropy with a NaN, +Inf or -Inf logit at the target class and off it (B 3 and 257, C 7, class weights, loss and dlogits), the
    loss and every dlogits element against the class the fp64 reference gives them; then tav_step_stats on that loss word: `nonfinite` goes up
    by exactly one when the loss is NaN or Inf, and not at all when it is a number."""
    rs, launch = [], 0
    for B, C, weighted, gs in ((3, 7, True, 1.0), (257, 7, False, 0.125)):
        p = FR.ce_inputs(B, C)
        rc = FR.ce_ref(p, weighted, gs)
        z, t = _dev(p["z"], _F32), _ints_dev(p["t"], torch.int64)
        cw = _dev(p["cw"], _F32) if weighted else None

        def run():
            loss, dl = _blank((1,), _F32), _blank((B, C), _F32)
            ops.check(ops.lib().tav_cross_entropy(ops.ptr(z), ops.ptr(t), ops.ptr(cw), ops.ptr(loss), ops.ptr(dl), B, C, gs, ops.stream()), "cross_entropy")
            return loss, dl
        loss_c, dl_c = run()
        for row, col, where in NF.ce_sites(p):
            for pat in (launch % 3, 3, 4):                            # a NaN pattern (rotating), +Inf and -Inf at every site
                rp, lsets, dsets = NF.ce_case(p, rc, FR.ce_ref, weighted, gs, row, col, pat)
                with _poisoned(z, (row, col), pat):
                    loss, dl = run()
                tag = f"nonfinite.ce[B{B},C{C},{NF.NAMES[pat]}@({row},{col}) {where}]"
                rs += NF.verdict(tag + ".loss", _np(loss_c), _np(loss), rp["loss"], rp["loss_b"], lsets)
                rs += NF.verdict(tag + ".dlogits", _np(dl_c), _np(dl), rp["dlogits"], rp["dlogits_b"], dsets)
                acc = ops.loop_acc_new(DEV)
                ops.step_stats(logits=z, target=t, cm=torch.zeros(C * C, dtype=torch.int64, device=DEV), loss=loss, acc=acc)
                n_bad = ops.loop_acc_read(acc)["nonfinite"]
                want = int(lsets["N"].any())
                rs.append((tag + f".step_stats nonfinite {n_bad} (want {want})", float(abs(n_bad - want)), 0.0, n_bad == want))
            launch += 1
    return rs


def check_nonfinite_layernorm(xdt, act):
    """tav_ln_fwd and the isolated tav_ln_bwd at W 768 and 5 rows, f32 output alone and f32 + bf16, the parameter reduce immediate and deferred
    (tav_ln_param_reduce_multi): poison in x, dy, gamma and dx_add against the sets NF.ln_expect() spells out."""
    rows, W = NF.LN_SHAPE
    p = NR.ln_inputs(rows, W, xdt, xdt)
    dev = _ln_dev(p)
    dyt, add = _dev(p["dy"], _TDT[xdt]), _dev(p["add"], torch.float32)
    tensors = dict(x=dev[0], gamma=dev[1], dy=dyt, add=add)
    rs, launch = [], 0

    def run(fed, lp, defer):
        f, _ = _ln_fwd_abi(p, dev, act=act, want32=True, lp=lp)
        b, _ = _ln_bwd_abi(p, dev, dyt, _dev(fed[0], torch.float32), _dev(fed[1], torch.float32), act=act, want32=True, lp=lp, add=add, defer=defer)
        if defer:
            _ln_reduce_multi([(b["partials"], b["dgamma"], b["dbeta"], b["nb"], W, 0)])
        return {n: _np(t) for n, t in list(f.items()) + list(b.items()) if n in NR.LN_FWD_OUT + NR.LN_BWD_OUT and t is not None}
    for lp in (False, True):
        for defer in (False, True):
            clean = None
            for tensor, index in NF.ln_sites(rows, W):
                pat = launch % NF.NPAT
                launch += 1
                c = NF.ln_case(NR, p, tensor, index, pat, act, lp)
                if clean is None:
                    clean = run(c["fed_clean"], lp, defer)
                with _poisoned(tensors[tensor], index, pat):
                    got = run(c["fed"], lp, defer)
                tag = f"nonfinite.ln[{xdt},act{act},lp{int(lp)},{'deferred' if defer else 'immediate'},{NF.NAMES[pat]}@{tensor}{index}]"
                for side, names in (("fwd", NR.LN_FWD_OUT), ("bwd", NR.LN_BWD_OUT)):
                    for n in names:
                        if n in got:
                            rs += NF.verdict(f"{tag}.{n}", clean[n], got[n], c[side][n], c[side][n + "_b"], c[side + "_sets"][n])
    return rs


def check_nonfinite_attention(dtype, S):
    """tav_attn_fwd and the isolated tav_attn_bwd at B 2, nh 3, every mask mode, raw and pre-scaled q: one poisoned element of Q, K, V, the
    mask or dO per launch (NF.attn_site rotates rows, entries, heads and patterns) against the sets NF.attn_expect() spells out -- the other
    (batch, head) slices are the clean launch bit for bit.  The backward is fed the reference's own (poisoned) o, o_soft, lse and corr."""
    dname = _GDT[dtype]
    rs, cfg = [], 0
    for mode in (0, 1, 2):
        for pre in (False, True):
            x = AR.make_inputs(2, S, 3, dname, seed=11, **AR.bound_config(S, mode, pre, None))
            ops_in = _attn_operands(x, dtype)
            dev = dict(zip(("q", "k", "v", "do", "mask"), ops_in))
            names = [n for n in AR.FWD_OUT + AR.BWD_OUT if not (n == "corr" and mode != 2)]

            def run(ref, tag):
                f = _attn_fwd(x, ops_in, None)
                got, gap = _attn_bwd(x, ops_in, None, *_attn_fed(x, AR.fed(ref, x), dtype), tag)
                got.update(f)
                return {n: _np(got[n]).reshape(ref[n].shape) for n in names}, gap
            clean = {}
            for i in range(len(NF.ATTN_SITES)):
                site = NF.attn_site(S, mode, cfg, i)
                if site is None:
                    continue
                tensor, index = site
                pat = NF.attn_pattern(tensor, cfg + i, mode, pre)
                xp, rc, rp, sets = NF.attn_case(AR, x, tensor, index, pat)
                tag = f"nonfinite.attn[{dname},S{S},mode{mode},pre{int(pre)},{NF.NAMES[pat]}@{tensor}{index}]"
                kind = "o_bound" in rp                                # (the clean launch is fed the clean reference of the same model)
                if kind not in clean:
                    clean[kind], gap = run(rc, tag + ".clean")
                    rs.append(gap)
                at = index if tensor == "mask" else (index[0] * S + index[1], index[2] * 64 + index[3])
                with _poisoned(dev[tensor], at, pat):
                    got, gap = run(rp, tag)
                rs.append(gap)
                for n in names:
                    rs += NF.verdict(f"{tag}.{n}", clean[kind][n], got[n], rp[n], rp.get(n + "_bound"), sets[n])
            cfg += 1
    return rs


def _nf_cast_rows(tag, clean, got, ref_c, ref_p):
    return NF.verdict(tag, _np(clean), _np(got), ref_p, None, NF.classify(ref_c, ref_p))


def check_nonfinite_casts():
    """tav_cast_weight, tav_cast2d, tav_cast_weights_multi (with the scaled q rows and a scaled bias row) and tav_cast_conv_weight: a poisoned
    source element is non-finite in the normal and in the transposed copy (and exactly once in the per-phase operand, a permutation of the
    weights), everything else is the clean launch bit for bit."""
    rs, launch = [], 0
    R, Cc = 65, 127
    w = _rnd(R, Cc, seed=1500)
    w64 = _np(w)
    sites = [(0, 0), (R - 1, Cc - 1), (32, 64)]
    for dtype in (torch.bfloat16, torch.float32):
        dn = _GDT[dtype]
        n_c, t_c = ops.cast_weight(w, dtype)
        ref_c = NF.cast_ref(w64, dn)
        for site in sites:
            pat = launch % NF.NPAT
            launch += 1
            ref_p = NF.cast_ref(NF.plant(w64, site, pat), dn)
            with _poisoned(w, site, pat):
                n, t = ops.cast_weight(w, dtype)
            tag = f"nonfinite.cast[{dn},{NF.NAMES[pat]}@{site}]"
            rs += _nf_cast_rows(tag + ".cast_weight.n", n_c, n, ref_c, ref_p) + _nf_cast_rows(tag + ".cast_weight.t", t_c, t, ref_c.T, ref_p.T)
    for src in (torch.float32, torch.bfloat16):                        # tav_cast2d, every pair of dtypes
        xs = _rnd(33, 64, dtype=src, seed=1501)
        xs64 = _np(xs)
        for dtype in (torch.bfloat16, torch.float32):
            c2_c = ops.cast2d(xs, dtype)
            for site in ((0, 0), (32, 63), (16, 32)):
                pat = launch % NF.NPAT
                launch += 1
                with _poisoned(xs, site, pat):
                    c2 = ops.cast2d(xs, dtype)
                rs += _nf_cast_rows(f"nonfinite.cast2d[{_GDT[src]}->{_GDT[dtype]},{NF.NAMES[pat]}@{site}]", c2_c, c2, NF.cast_ref(xs64, _GDT[dtype]),
                                    NF.cast_ref(NF.plant(xs64, site, pat, _GDT[src]), _GDT[dtype]))
    # the multi-tensor launch: q rows scaled in dst and not in dst_t, a scaled f32 bias row
    H, K, bf, qs = 64, 128, torch.bfloat16, ops.ATTN_Q_PRESCALE
    wq, bq = _rnd(H, K, seed=1600), _rnd(1, H, seed=1610)
    outs = dict(n=_blank((H, K), bf), t=_blank((K, H), bf), b=_blank((H,), torch.float32))
    descs, tiles = ops.make_cast_descs([(wq, outs["n"], outs["t"], qs), (bq, outs["b"].view(1, H), None, qs)], DEV)
    descs = _in(descs)

    def multi():
        for b_ in outs.values():
            _refill(b_)
        ops.cast_weights_multi(descs, 2, 3)
        return {k: v.clone() for k, v in outs.items()}
    clean = multi()
    wq64, bq64 = _np(wq), _np(bq)
    for src, s64, site in ((wq, wq64, (0, 0)), (wq, wq64, (H - 1, K - 1)), (wq, wq64, (32, 64)), (bq, bq64, (0, H - 1))):
        pat = launch % NF.NPAT
        launch += 1
        with _poisoned(src, site, pat):
            got = multi()
        tag = f"nonfinite.cast_multi[{NF.NAMES[pat]}@{'bias' if src is bq else 'wq'}{site}]"
        pw = NF.plant(wq64, site, pat) if src is wq else wq64
        pb = NF.plant(bq64, site, pat) if src is bq else bq64
        rs += _nf_cast_rows(tag + ".dst (scaled)", clean["n"], got["n"], NF.cast_ref(wq64, "bf16", qs), NF.cast_ref(pw, "bf16", qs))
        rs += _nf_cast_rows(tag + ".dst_t", clean["t"], got["t"], NF.cast_ref(wq64, "bf16").T, NF.cast_ref(pw, "bf16").T)
        rs += _nf_cast_rows(tag + ".bias (scaled)", clean["b"], got["b"], NF.cast_ref(bq64, "f32", qs)[0], NF.cast_ref(pb, "f32", qs)[0])
    # conv weights [co][ci][k]: dst[c][kk ci + i] = W[c][i][kk], dst_t its transpose, the per-phase operand a permutation
    co, ci, k = 16, 8, 3
    wc = _rnd(co, ci, k, seed=1700)
    wc64 = _np(wc)
    for dtype in (torch.bfloat16, torch.float32):
        dn = _GDT[dtype]
        n_c, t_c, ph_c = ops.cast_conv_weight(wc, dtype, conv_stride=2)
        for site in ((0, 0, 0), (co - 1, ci - 1, k - 1), (7, 3, 1)):
            pat = launch % NF.NPAT
            launch += 1
            with _poisoned(wc, site, pat):
                n, t, ph = ops.cast_conv_weight(wc, dtype, conv_stride=2)
            lay = lambda a: NF.cast_ref(a, dn).transpose(0, 2, 1).reshape(co, k * ci)          # noqa: E731
            ref_c, ref_p = lay(wc64), lay(NF.plant(wc64, site, pat))
            tag = f"nonfinite.cast_conv[{dn},{NF.NAMES[pat]}@{site}]"
            rs += _nf_cast_rows(tag + ".dst", n_c, n, ref_c, ref_p) + _nf_cast_rows(tag + ".dst_t", t_c, t, ref_c.T, ref_p.T)
            bad = ~np.isfinite(_np(ph))
            same = int(((_np(ph) != _np(ph_c)) & ~bad).sum())
            rs.append((tag + f".phase operand: {int(bad.sum())} non-finite element(s), {same} others changed", float(abs(int(bad.sum()) - 1) + same), 0.0,
                       int(bad.sum()) == 1 and same == 0))
    return rs


def check_nonfinite_dropout():
    """tav_dropout_fwd / tav_dropout_bwd (y = keep ? x / (1 - p) : 0, a select): a kept poison stays non-finite, a dropped one is exactly 0, the
    mask bytes are those of the clean launch, every other element is the clean launch bit for bit."""
    n, p, seed = 5003, 0.3, 1234
    x, dy = _rnd(n, seed=1800), _rnd(n, seed=1801)
    y_c, mask_c = ops.dropout_fwd(x, p, seed, 0)
    dx_c = ops.dropout_bwd(dy, mask_c, p)
    keep = mask_c.cpu().numpy() != 0
    x64, dy64 = _np(x), _np(dy)
    kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
    rs = [("nonfinite.dropout: kept and dropped elements both present", 0.0, 0.0, len(kept) > 2 and len(dropped) > 2)]
    sites = [("kept", int(kept[0])), ("kept", int(kept[-1])), ("dropped", int(dropped[0])), ("dropped", int(dropped[-1])), ("kept", int(kept[len(kept) // 2]))]
    for launch, (what, i) in enumerate(sites):
        for pat in (launch % NF.NPAT, (launch + 3) % NF.NPAT):
            with _poisoned(x, i, pat):
                y, mask = ops.dropout_fwd(x, p, seed, 0)
            with _poisoned(dy, i, pat):
                dx = ops.dropout_bwd(dy, mask_c, p)
            tag = f"nonfinite.dropout[{NF.NAMES[pat]}@{i} ({what})]"
            rs.append(_exact(tag + ".mask bytes", mask, mask_c))
            ref_c, ref_p = NF.dropout_ref(x64, keep, p), NF.dropout_ref(NF.plant(x64, i, pat), keep, p)
            rs += NF.verdict(tag + ".fwd", _np(y_c), _np(y), ref_p, None, NF.classify(ref_c, ref_p))
            ref_c, ref_p = NF.dropout_ref(dy64, keep, p), NF.dropout_ref(NF.plant(dy64, i, pat), keep, p)
            rs += NF.verdict(tag + ".bwd", _np(dx_c), _np(dx), ref_p, None, NF.classify(ref_c, ref_p))
            if what == "dropped":
                z = float(y[i].abs().item()) + float(dx[i].abs().item())
                rs.append((tag + ".dropped poison is exactly 0", z, 0.0, z == 0.0))
    return rs


def nonfinite_checks():
    """The non-finite cases, in the order all_checks() appends them."""
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        for delayed in (False, True):
            out.append(lambda d=dtype, l=delayed: check_nonfinite_fp8_quantize(d, l))
    out += [check_nonfinite_fp8_saturation, check_nonfinite_fp8_amax, lambda: check_nonfinite_fp8_gemm(130, 132, 128, 4),
            lambda: check_nonfinite_fp8_gemm(257, 260, 256, 16), check_nonfinite_fp8_wgrad]
    out.append(lambda: check_nonfinite_gemm_nt(torch.float32, 0))
    for hint in (0, 8, 16):
        out.append(lambda h=hint: check_nonfinite_gemm_nt(torch.bfloat16, h))
    for dtype in (torch.float32, torch.bfloat16):
        out.append(lambda d=dtype: check_nonfinite_gemm_tn(d, 130, 1))
        out.append(lambda d=dtype: check_nonfinite_gemm_tn(d, 249, 3))
        out.append(lambda d=dtype: check_nonfinite_gemm_tn_grouped(d))
    out.append(check_nonfinite_sumsq)
    for form in ("multi", "chunked", "chunked_groups"):
        out.append(lambda f=form: check_nonfinite_adamw(f))
    out.append(check_nonfinite_cross_entropy)
    for xdt in ("f32", "bf16"):
        for act in (0, 1):
            out.append(lambda x=xdt, a=act: check_nonfinite_layernorm(x, a))
    for dtype in (torch.float32, torch.bfloat16):
        for S in NF.ATTN_S:
            out.append(lambda d=dtype, s=S: check_nonfinite_attention(d, s))
    out += [check_nonfinite_casts, check_nonfinite_dropout]
    return out


def all_checks():
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        out.append(lambda d=dtype: check_gemm_nt(d))
        out.append(lambda d=dtype: check_gemm_nt(d, M=1000, N=768, K=768, act=1, pre=True, resid=False))
        out.append(lambda d=dtype: check_gemm_nt(d, M=129, N=2304, K=768, resid=False))
        for tmh in (2, 3, 4):
            out.append(lambda d=dtype, t=tmh: check_gemm_nt(d, M=333, N=384, K=256, tile_m=t))
        if dtype == torch.bfloat16:          # 8-wave 256x128 tile (bf16 only): ragged M and N, short and long K, every epilogue
            out.append(lambda d=dtype: check_gemm_nt(d, M=333, N=384, K=256, tile_m=8))
            out.append(lambda d=dtype: check_gemm_nt(d, M=700, N=768, K=64, tile_m=8, out_f32=True))
            out.append(lambda d=dtype: check_gemm_nt(d, M=1000, N=3072, K=768, act=1, pre=True, resid=False, tile_m=8))
            out.append(lambda d=dtype: check_gemm_nt(d, M=513, N=132, K=1536, tile_m=8))
            # 8-wave 256x256 tile, two-pass epilogue: ragged M / N, short and long K, every epilogue flavour
            out.append(lambda d=dtype: check_gemm_nt(d, M=333, N=384, K=256, tile_m=16))
            out.append(lambda d=dtype: check_gemm_nt(d, M=700, N=768, K=64, tile_m=16, out_f32=True))
            out.append(lambda d=dtype: check_gemm_nt(d, M=1000, N=3072, K=768, act=1, pre=True, resid=False, tile_m=16))
            out.append(lambda d=dtype: check_gemm_nt(d, M=513, N=132, K=1536, tile_m=16))
            # interior tiles (the bounds-check-free pass) of the plain and residual flavours: no bias / bias, bf16 / f32 out, with and without the
            # f32 residual; the gelu pair below covers the other two flavours
            for kw in (dict(resid=False), dict(resid=False, bias=False), dict(resid=False, out_f32=True), dict(resid=False, bias=False, out_f32=True),
                       dict(out_f32=True), dict(bias=False, out_f32=True)):
                out.append(lambda d=dtype, k=kw: check_gemm_nt(d, M=700, N=768, K=192, tile_m=16, **k))
            # ... and every length of its 3 + 2 image ring's prologue / tail: 1, 2, 3 and 5 K-tiles
            for kk in (128, 192, 320):
                out.append(lambda d=dtype, k=kk: check_gemm_nt(d, M=300, N=260, K=k, tile_m=16))
        if dtype == torch.bfloat16:
            out.append(check_gemm_nt_mixed_schedule)
        if dtype == torch.bfloat16:
            out.append(check_gemm_tn_grouped_big)
            # the weight-gradient tile's ring with one, two and three K-tiles per split (the last one ragged)
            out.append(lambda: check_gemm_tn_grouped_big(M=130))
            out.append(lambda: check_gemm_tn_grouped_big(M=64))
        out.append(lambda d=dtype: check_gemm_nt_gelu_bwd(d))
        out.append(lambda d=dtype: check_gemm_nt_gelu_derivative_pair(d))
        if dtype == torch.bfloat16:
            out.append(lambda d=dtype: check_gemm_nt_gelu_derivative_pair(d, M=700, N=768, K=128, tile_m=16))
        out.append(lambda d=dtype: check_gemm_tn(d))
        out.append(lambda d=dtype: check_gemm_tn(d, M=249, N1=768, N2=512, nbatch=3))
        out.append(lambda d=dtype: check_gemm_tn_grouped(d))
        out.append(lambda d=dtype: check_gemm_tn_grouped(d, M=64))
        out.append(lambda d=dtype: check_conv_as_gemm(d))
        out.append(lambda d=dtype: check_conv_as_gemm(d, k=2, T_in=100))
        out.append(lambda d=dtype: check_conv_chain(d))
        out.append(lambda d=dtype: check_conv_chain(d, B=2, T=1000, Cc=128))      # even length: the phases end on different rows
        for mode in (0, 1, 2):
            out.append(lambda d=dtype, m=mode: check_attention(d, m))
        out.append(lambda d=dtype: check_attention(d, 0, B=1, S=64, nh=1))
        out.append(lambda d=dtype: check_attention(d, 2, B=1, S=481, nh=12))
        out.append(lambda d=dtype: check_attention(d, 2, B=2, S=481, nh=12, ref_style_mask=True))
        # size extremes of the path: 1 token, the text model's longest sequence (514 positions -> 512 tokens, pre-softmax mask), the
        # 32-frame video of BASELINE config 5 (3136 tokens before masking), 10 s audio (499 frames)
        out.append(lambda d=dtype: check_attention(d, 0, B=2, S=1, nh=2))
        out.append(lambda d=dtype: check_attention(d, 1, B=1, S=512, nh=2))
        out.append(lambda d=dtype: check_attention(d, 0, B=1, S=3136, nh=1))
        out.append(lambda d=dtype: check_attention(d, 0, B=1, S=499, nh=2))
        # tav_attn_args.q_prescaled (what the engine's layers run): every mask mode, the ragged / single-tile / long cases, the reference-style
        # post-softmax mask, and key spikes that force the forward kernel's lazy rescale late in the key loop (moderate and extreme jumps)
        for mode in (0, 1, 2):
            out.append(lambda d=dtype, m=mode: check_attention(d, m, pre=True))
        out.append(lambda d=dtype: check_attention(d, 0, B=1, S=64, nh=1, pre=True))
        out.append(lambda d=dtype: check_attention(d, 0, B=2, S=1, nh=2, pre=True))
        out.append(lambda d=dtype: check_attention(d, 0, B=1, S=3136, nh=1, pre=True))
        out.append(lambda d=dtype: check_attention(d, 0, B=2, S=1464, nh=2, pre=True))
        # odd slice / tile counts: the one-dimensional XCD-banded grid (attn_tile) must stay a bijection when tiles * heads * batch % 8 != 0
        out.append(lambda d=dtype: check_attention(d, 0, B=3, S=300, nh=5, pre=True))
        out.append(lambda d=dtype: check_attention(d, 2, B=3, S=135, nh=3))
        out.append(lambda d=dtype: check_attention(d, 2, B=2, S=481, nh=12, ref_style_mask=True, pre=True))
        out.append(lambda d=dtype: check_attention(d, 0, B=2, S=328, nh=2, pre=True, spike=6.0))
        out.append(lambda d=dtype: check_attention(d, 0, B=1, S=328, nh=2, pre=True, spike=300.0))
        out.append(lambda d=dtype: check_attention(d, 2, B=1, S=300, nh=2, pre=True, spike=40.0))
        out.append(lambda d=dtype: check_attention(d, 0, B=1, S=328, nh=2, spike=40.0))
        out.append(lambda d=dtype: check_layernorm(d))
        out.append(lambda d=dtype: check_layernorm(d, W=512, act=1))
        out.append(lambda d=dtype: check_layernorm(d, W=1024))
        if dtype == torch.float32:
            out.append(check_layernorm_deferred_param_reduce)
        out.append(lambda d=dtype: check_conv0_gn(d))
        out.append(lambda d=dtype: check_posconv(d))
    out.append(lambda: check_gemm_nt(torch.bfloat16, out_f32=True))
    out += [check_cast_weight, check_colsum, check_text_embed, lambda: check_text_embed(-1), check_patchify,
            check_pool_head_ce, check_embed_add, check_scatter_deterministic, check_index_safety, check_fp8,
            lambda: check_fp8(M=1000, N=768, K=256, tile_m=16), lambda: check_fp8(M=130, N=132, K=128, tile_m=4)]
    # guard-band edge cases (appended, so the indices of the cases above stay what they were)
    for dtype in (torch.float32, torch.bfloat16):
        for hint in (0, 2, 3, 4, 17) + ((8, 16) if dtype == torch.bfloat16 else ()):
            out.append(lambda d=dtype, h=hint: check_gemm_nt_edges(d, h))
        out.append(lambda d=dtype: check_gemm_tn_edges(d))
        out.append(lambda d=dtype: check_gemm_tn_grouped_edges(d))
        for mode in (0, 1, 2):
            for S in (1, 63, 64, 65, 127, 129):
                out.append(lambda d=dtype, m=mode, s=S: check_attention_edges(d, m, s, pre=bool(s % 2)))
            out.append(lambda d=dtype, m=mode: check_attention_edges(d, m, 65, lens=[0, 65, 33]))
            out.append(lambda d=dtype, m=mode: check_attention_edges(d, m, 129, lens=[129, 0, 64], pre=True))
        for S in (1, 65, 200):
            out.append(lambda d=dtype, s=S: check_attn_probs(d, s))
        out.append(lambda d=dtype: check_head_scale(d))
        # audio front-end at the smallest sizes the host validation accepts (one output step, one batch entry; both together at the end of
        # the list) and one step past a chunk
        out.append(lambda d=dtype: check_conv0_gn(d, B=2, T_in=10, ref64=True))
        out.append(lambda d=dtype: check_conv0_gn(d, B=1, T_in=15, ref64=True))
        out.append(lambda d=dtype: check_conv0_gn(d, B=1, T_in=512 * 5 + 10, ref64=True))
        out.append(_in64(lambda d=dtype: check_conv_as_gemm(d, B=1, T_in=3)))
        out.append(_in64(lambda d=dtype: check_posconv(d, B=1, T=1)))
    out += [check_fp8_quantize_edges, lambda: check_fp8(M=1, N=132, K=128, tile_m=4), lambda: check_fp8(M=129, N=132, K=128, tile_m=4),
            lambda: check_fp8(M=1, N=768, K=256, tile_m=16), lambda: check_fp8(M=257, N=768, K=256, tile_m=16),
            check_elementwise_tails, _in64(check_layernorm_edges), check_transpose2d, check_zero_pad_rows, _in64(check_small_counts)]
    # the fp8 epilogue with strided outputs and side tensors: check_fp8's three shapes plus M = 1 and tile + 1 of both fp8 tiles
    for M, N, K, tm in ((700, 384, 1024, 0), (1000, 768, 256, 16), (130, 132, 128, 4), (1, 132, 128, 4), (129, 132, 128, 4),
                        (1, 260, 256, 16), (257, 260, 256, 16)):
        out.append(lambda a=(M, N, K, tm): check_fp8_edges(*a))
    # the smallest launch of the audio front-end: one batch entry, one output step (hand-written fp64 group norm: torch's refuses it)
    for dtype in (torch.float32, torch.bfloat16):
        out.append(lambda d=dtype: check_conv0_gn(d, B=1, T_in=10, ref64=True))
    # step-end kernels: gradient norm, clip coefficient, AdamW, operand casts, fp8 states
    out += step_end_checks()
    # the GEMM family against fp64: per-element bounds and exact integer operands
    out += gemm_fp64_checks()
    # the attention family against fp64: per-element bounds, exact selections, isolated and chained backward, the two helper kernels
    out += attention_fp64_checks()
    # the normalisation family against fp64: per-element bounds, exact integer cases, the group norm's pivot on an atypical first row
    out += norm_fp64_checks()
    # the audio front-end, colsum, the GELU pair, pools, head, tanh, cross entropy and the index kernels against fp64
    out += front_fp64_checks()
    # non-finite values: a poisoned operand element stays loud where the fp64 reference says so and reaches nothing else
    out += nonfinite_checks()
    return out
