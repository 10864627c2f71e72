"""GPU: length-aware attention (tav_attn_fwd_len / tav_attn_bwd_len) and mean pool (tav_mean_pool_*_len).

Row b of a length-aware launch over a padded [B, S] layout must be BITWISE equal to the plain kernel run on that row alone with S = L_b,
padded rows must come out exactly zero, all-full lengths must reproduce the plain kernel, and two runs must agree bit for bit.

Every test runs inside the guard-band allocator (tests/guarded.py): outputs start as 0xFF (NaN), so "exactly zero" and "bitwise equal" cannot
be met by what an earlier launch left in a recycled block, and stores outside a tensor or into an operand are reported by verify()."""
import functools

import pytest
import torch

import guarded
import tav_amd  # noqa: F401
from tav_amd import ops

pytestmark = pytest.mark.gpu

def _g(t):
    """An operand inside a watched 0xFF buffer while a guard is active (None stays None)."""
    return t if t is None or guarded.current() is None else guarded.guarded_input(t)


def under_guard(fn):
    @functools.wraps(fn)
    def run(*args, **kw):
        with guarded.active() as g:
            fn(*args, **kw)
            assert g.allocs
            g.verify()
    return run


NH = 2
H = NH * 64
LENS = [1, 63, 64, 65, 130, 200]          # S = 200: single tiles, tile edges, several tiles, the full row
S = max(LENS)


def _inputs(dtype, mode, lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    qkv = (torch.randn(B * S, 3 * H, generator=g) * 0.5).to(dtype)
    dout = (torch.randn(B * S, H, generator=g) * 0.5).to(dtype)
    mask = None
    if mode == 1:
        mask = torch.where(torch.rand(B, S, generator=g) < 0.2, -10000.0, 0.0)
    elif mode == 2:
        mask = torch.where(torch.rand(B, S, generator=g) < 0.2, -1.0, 0.0) + 0.01 * torch.randn(B, S, generator=g)
    dev = "cuda"
    return _g(qkv.to(dev)), _g(dout.to(dev)), None if mask is None else _g(mask.float().contiguous().to(dev))


def _run(qkv, dout, mask, B, S_, mode, pre, seq_lens=None):
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    o, lse, corr = ops.attn_fwd(q, k, v, B, S_, NH, key_mask=mask, mask_mode=mode, q_prescaled=pre, seq_lens=seq_lens)
    dqkv = ops.attn_bwd(q, k, v, o, dout, lse, corr, B, S_, NH, key_mask=mask, mask_mode=mode, q_prescaled=pre, seq_lens=seq_lens)
    out = dict(o=o.clone(), lse=lse.clone(), dqkv=dqkv.clone())
    if mode == 2:
        out["corr"], out["o_soft"] = corr[0].clone(), corr[1].clone()
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _poison_fill(t, region):
    """t[region] := the five poison patterns of tests/nonfinite_ref.py in turn (quiet NaN, all ones, signalling NaN, +Inf, -Inf), written
    through an integer view: what a reused buffer may hold just as well as finite garbage."""
    import nonfinite_ref as NF
    dn = "bf16" if t.dtype == torch.bfloat16 else "f32"
    sub = t.view(torch.int16 if dn == "bf16" else torch.int32)[region]
    pats = torch.tensor([NF.signed_bits(i, dn) for i in range(NF.NPAT)], dtype=sub.dtype, device=t.device)
    sub.copy_(pats[torch.arange(sub.numel(), device=t.device) % NF.NPAT].view(sub.shape))


def _same_class(a, b):
    """Non-finite in the same places (NaN for Inf passes) and bitwise equal everywhere else."""
    fa, fb = torch.isfinite(a), torch.isfinite(b)
    return torch.equal(fa, fb) and _same(torch.where(fa, a, torch.zeros_like(a)), torch.where(fb, b, torch.zeros_like(b)))


CASES = [(dt, mode, pre) for dt in (torch.bfloat16, torch.float32) for mode in (0, 1, 2) for pre in (False, True)]


@pytest.mark.parametrize("dtype,mode,pre", CASES, ids=[f"{'bf16' if d == torch.bfloat16 else 'f32'}-m{m}-{'pre' if p else 'raw'}" for d, m, p in CASES])
@under_guard
def test_attention_rows_bitwise_equal_to_batch1(gpu, dtype, mode, pre):
    B = len(LENS)
    qkv, dout, mask = _inputs(dtype, mode, LENS)
    sl = _g(torch.tensor(LENS, dtype=torch.int32, device="cuda"))
    rag = _run(qkv, dout, mask, B, S, mode, pre, seq_lens=sl)
    again = _run(qkv, dout, mask, B, S, mode, pre, seq_lens=sl)
    for key in rag:
        assert _same(rag[key], again[key]), f"{key}: two runs differ"
    for b, L in enumerate(LENS):
        r0, r1 = b * S, b * S + L
        m1 = None if mask is None else _g(mask[b:b + 1, :L].contiguous())
        one = _run(qkv[r0:r1], dout[r0:r1], m1, 1, L, mode, pre)
        assert _same(rag["o"][r0:r1], one["o"]), f"row {b} (L={L}): o"
        assert _same(rag["lse"][b, :, :L], one["lse"][0]), f"row {b} (L={L}): lse"
        assert _same(rag["dqkv"][r0:r1], one["dqkv"]), f"row {b} (L={L}): dq/dk/dv"
        if mode == 2:
            assert _same(rag["corr"][b], one["corr"][0]), f"row {b} (L={L}): corr"
            assert _same(rag["o_soft"][r0:r1], one["o_soft"]), f"row {b} (L={L}): o_soft"
        # padded rows: exactly zero, never left uninitialised
        assert not rag["o"][r1:(b + 1) * S].float().abs().sum().item(), f"row {b}: padded o"
        assert not rag["lse"][b, :, L:].abs().sum().item(), f"row {b}: padded lse"
        assert not rag["dqkv"][r1:(b + 1) * S].float().abs().sum().item(), f"row {b}: padded dq/dk/dv"
        if mode == 2:
            assert not rag["o_soft"][r1:(b + 1) * S].float().abs().sum().item(), f"row {b}: padded o_soft"


@pytest.mark.parametrize("dtype,mode,pre", CASES, ids=[f"{'bf16' if d == torch.bfloat16 else 'f32'}-m{m}-{'pre' if p else 'raw'}" for d, m, p in CASES])
@under_guard
def test_attention_full_lengths_equal_plain_kernel(gpu, dtype, mode, pre):
    B = 3
    qkv, dout, mask = _inputs(dtype, mode, [S] * B, seed=1)
    full = _g(torch.full((B,), S, dtype=torch.int32, device="cuda"))
    rag = _run(qkv, dout, mask, B, S, mode, pre, seq_lens=full)
    plain = _run(qkv, dout, mask, B, S, mode, pre)
    for key in plain:
        assert _same(rag[key], plain[key]), key


@pytest.mark.parametrize("dtype,mode,pre", CASES, ids=[f"{'bf16' if d == torch.bfloat16 else 'f32'}-m{m}-{'pre' if p else 'raw'}" for d, m, p in CASES])
@under_guard
def test_attention_padding_content_and_empty_rows(gpu, dtype, mode, pre):
    """What the padded slots hold does not reach the valid rows; a row of length 0 (and lengths past S, clamped) is handled."""
    lens = [0, 37, S + 50, 129]
    B = len(lens)
    qkv, dout, mask = _inputs(dtype, mode, lens, seed=2)
    sl = _g(torch.tensor(lens, dtype=torch.int32, device="cuda"))
    a = _run(qkv, dout, mask, B, S, mode, pre, seq_lens=sl)
    qkv2, dout2 = qkv.clone(), dout.clone()
    mask2 = None if mask is None else mask.clone()
    for b, L in enumerate(lens):
        L = min(L, S)
        qkv2[b * S + L:(b + 1) * S] = torch.randn_like(qkv2[b * S + L:(b + 1) * S].float()).to(qkv2.dtype) * 30
        dout2[b * S + L:(b + 1) * S] = 7
        if mask2 is not None:
            mask2[b, L:] = 123.0
    c = _run(_g(qkv2), _g(dout2), _g(mask2), B, S, mode, pre, seq_lens=sl)
    for key in a:
        assert _same(a[key], c[key]), f"mode {mode}: {key} depends on the padded slots"
    assert not a["o"][:S].float().abs().sum().item() and not a["dqkv"][:S].float().abs().sum().item()
    assert not a["lse"][0].abs().sum().item()
    if mode == 2:
        assert not a["corr"][0].abs().sum().item()
    full = _run(qkv[2 * S:3 * S], dout[2 * S:3 * S], None if mask is None else _g(mask[2:3].contiguous()), 1, S, mode, pre)
    assert _same(a["o"][2 * S:3 * S], full["o"]) and _same(a["dqkv"][2 * S:3 * S], full["dqkv"])
    # ... and neither does NaN / Inf there: the padded slots hold the five poison patterns instead of finite garbage
    qkv3, dout3 = qkv.clone(), dout.clone()
    mask3 = None if mask is None else mask.clone()
    for b, L in enumerate(lens):
        L = min(L, S)
        _poison_fill(qkv3, slice(b * S + L, (b + 1) * S))
        _poison_fill(dout3, slice(b * S + L, (b + 1) * S))
        if mask3 is not None:
            _poison_fill(mask3, (b, slice(L, S)))
    assert not torch.isfinite(qkv3[37:S].float()).any() and not torch.isfinite(dout3[S + 37:2 * S].float()).any()
    d = _run(_g(qkv3), _g(dout3), _g(mask3), B, S, mode, pre, seq_lens=sl)
    for key in c:
        assert _same(c[key], d[key]), f"mode {mode}: {key} depends on NaN / Inf in the padded slots"
    for b, L in enumerate(lens):
        r1 = b * S + min(L, S)
        assert not d["o"][r1:(b + 1) * S].float().abs().sum().item() and not d["dqkv"][r1:(b + 1) * S].float().abs().sum().item(), f"row {b}: padded outputs"
        assert not d["lse"][b, :, min(L, S):].abs().sum().item(), f"row {b}: padded lse"


@pytest.mark.parametrize("dtype,mode,pre", CASES, ids=[f"{'bf16' if d == torch.bfloat16 else 'f32'}-m{m}-{'pre' if p else 'raw'}" for d, m, p in CASES])
@under_guard
def test_attention_poison_in_last_valid_row(gpu, dtype, mode, pre):
    """A NaN / Inf in the LAST valid row of a batch entry: the ragged tile's clamp re-reads that row for the keys past L_b.  The entry must
    come out exactly as the plain kernel run on that row alone with the same poison (non-finite in the same places, bitwise equal elsewhere),
    its padded slots exactly zero, and the other entries bit for bit as without the poison."""
    import nonfinite_ref as NF
    lens = [65, 37, 129]
    B, b, L = len(lens), 1, 37
    qkv, dout, mask = _inputs(dtype, mode, lens, seed=4)
    sl = _g(torch.tensor(lens, dtype=torch.int32, device="cuda"))
    clean = _run(qkv, dout, mask, B, S, mode, pre, seq_lens=sl)
    r0, r1, last = b * S, b * S + L, b * S + L - 1
    dn = "bf16" if dtype == torch.bfloat16 else "f32"
    for i, (name, col) in enumerate((("q", 5), ("k", H + 70), ("v", 2 * H + 3), ("dout", 9))):
        pat = i + mode + int(pre)                                     # every pattern over the cases
        qkv2, dout2 = qkv.clone(), dout.clone()
        t = dout2 if name == "dout" else qkv2
        t.view(torch.int16 if dn == "bf16" else torch.int32)[last, col] = NF.signed_bits(pat, dn)
        qkv2, dout2 = _g(qkv2), _g(dout2)
        rag = _run(qkv2, dout2, mask, B, S, mode, pre, seq_lens=sl)
        m1 = None if mask is None else _g(mask[b:b + 1, :L].contiguous())
        one = _run(qkv2[r0:r1], dout2[r0:r1], m1, 1, L, mode, pre)
        tag = f"{NF.NAMES[pat % NF.NPAT]} in {name}, last valid row"
        assert not torch.isfinite(rag["dqkv"][r0:r1].float()).all(), f"{tag}: laundered"
        assert _same_class(rag["o"][r0:r1], one["o"]), f"{tag}: o"
        assert _same_class(rag["lse"][b, :, :L], one["lse"][0]), f"{tag}: lse"
        assert _same_class(rag["dqkv"][r0:r1], one["dqkv"]), f"{tag}: dq/dk/dv"
        if mode == 2:
            assert _same_class(rag["o_soft"][r0:r1], one["o_soft"]), f"{tag}: o_soft"
        assert not rag["o"][r1:(b + 1) * S].float().abs().sum().item() and not rag["dqkv"][r1:(b + 1) * S].float().abs().sum().item(), f"{tag}: padded slots"
        for key in clean:
            for other in (0, 2):
                x, y = (clean[key][other], rag[key][other]) if key in ("lse", "corr") else (clean[key][other * S:(other + 1) * S], rag[key][other * S:(other + 1) * S])
                assert _same(x, y), f"{tag}: {key} of entry {other} changed"


@under_guard
def test_mean_pool_len_bitwise(gpu):
    lens = [0, 1, 15, 16, 17, 100, S]
    B, W = len(lens), 136
    g = torch.Generator().manual_seed(3)
    x = _g(torch.randn(B * S, W, generator=g).cuda())
    dy = _g(torch.randn(B, W, generator=g).cuda())
    sl = _g(torch.tensor(lens, dtype=torch.int32, device="cuda"))
    y = ops.mean_pool_fwd(x, B, S, seq_lens=sl)
    assert _same(y, ops.mean_pool_fwd(x, B, S, seq_lens=sl))
    dx, dxlp = ops.mean_pool_bwd(dy, B, S, lp_dtype=torch.bfloat16, seq_lens=sl)
    for b, L in enumerate(lens):
        if L == 0:
            assert not y[b].abs().sum().item()
        else:
            assert _same(y[b:b + 1], ops.mean_pool_fwd(x[b * S:b * S + L], 1, L)), f"row {b} (L={L})"
            ref, reflp = ops.mean_pool_bwd(dy[b:b + 1], 1, L, lp_dtype=torch.bfloat16)
            assert _same(dx[b * S:b * S + L], ref) and _same(dxlp[b * S:b * S + L], reflp), f"row {b} (L={L}): backward"
        assert not dx[b * S + L:(b + 1) * S].abs().sum().item() and not dxlp[b * S + L:(b + 1) * S].float().abs().sum().item()
    # NaN / Inf in the padded slots of x: the valid rows' means are bit for bit the same, an empty row's mean stays exactly zero
    x2 = x.clone()
    for b, L in enumerate(lens):
        _poison_fill(x2, slice(b * S + L, (b + 1) * S))
    assert not torch.isfinite(x2[:S]).any()
    y2 = ops.mean_pool_fwd(_g(x2), B, S, seq_lens=sl)
    assert _same(y, y2) and not y2[0].abs().sum().item()
    full = _g(torch.full((B,), S, dtype=torch.int32, device="cuda"))
    assert _same(ops.mean_pool_fwd(x, B, S, seq_lens=full), ops.mean_pool_fwd(x, B, S))
    assert _same(ops.mean_pool_bwd(dy, B, S, seq_lens=full)[0], ops.mean_pool_bwd(dy, B, S)[0])


# ------------------------------------------------------------------------------------------------ one encoder layer (engine level)
def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30)).item()


def _layer(H, F, seed):
    g = torch.Generator().manual_seed(seed)

    def P(*shape, scale=0.05, base=0.0):
        return torch.nn.Parameter((base + torch.randn(*shape, generator=g) * scale).cuda())
    return [P(H, base=1.0), P(H), P(H, H), P(H), P(H, H), P(H), P(H, H), P(H), P(H, H), P(H), P(H, base=1.0), P(H), P(F, H), P(F), P(H, F), P(H)]


def _layer_step(policy, params, x, gy, B, S, mode, key_mask, seq_lens):
    from tav_amd import engine, runtime
    ectx = runtime.set_precision(policy)
    for p in params:
        p.grad = None
    x = x.clone().requires_grad_(True)
    spec = engine.LayerSpec(B, S, 2, 1e-12, pre_ln=True, mask_mode=mode, branch="video" if mode == 0 else "fusion", seq_lens=seq_lens)
    y, _ = engine.encoder_layer(ectx, spec, x, None, key_mask, params)
    (y * gy).sum().backward()
    torch.cuda.synchronize()
    return y.detach().clone(), x.grad.clone(), [p.grad.clone() for p in params]


@pytest.mark.parametrize("mode", [0, 2])
@under_guard
def test_encoder_layer_ragged_rows(gpu, mode):
    """LayerSpec(seq_lens=...): valid rows match the rows run alone (fp32 policy), the padded slots' content changes nothing (bitwise,
    fp32 and bf16), their gradient is exactly zero, and the parameter gradients are the sums of the per-row ones."""
    H, F, S_, lens = 128, 256, 70, [70, 33, 1, 64]
    B = len(lens)
    params = _layer(H, F, 5)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B * S_, H, generator=g).cuda()
    gy = torch.randn(B * S_, H, generator=g).cuda()
    valid = torch.zeros(B * S_, 1, device="cuda")
    for b, L in enumerate(lens):
        valid[b * S_:b * S_ + L] = 1
    gy = gy * valid                                               # what a length-aware pool hands back: nothing on padded rows
    km = (torch.where(torch.rand(B, S_, generator=g) < 0.3, -1.0, 0.0)).cuda() if mode == 2 else None
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for policy in ("fp32", "bf16"):
        y, dx, dps = _layer_step(policy, params, x, gy, B, S_, mode, km, sl)
        x2 = torch.where(valid.bool(), x, torch.randn_like(x) * 10)
        km2 = None if km is None else torch.where(valid.view(B, S_).bool(), km, torch.full_like(km, 55.0))
        y2, dx2, dps2 = _layer_step(policy, params, x2, gy, B, S_, mode, km2, sl)
        vb = valid.bool().expand_as(y)
        assert torch.equal(y[vb], y2[vb]), f"{policy}: outputs depend on padded slots"
        assert torch.equal(dx, dx2) and all(torch.equal(a, c) for a, c in zip(dps, dps2)), f"{policy}: gradients depend on padded slots"
        assert not dx[~valid.bool().expand_as(dx)].abs().sum().item(), f"{policy}: padded rows got a gradient"
        assert all(torch.isfinite(t).all() for t in dps)
    # fp32: row by row against B = 1 runs of the same utterances
    y, dx, dps = _layer_step("fp32", params, x, gy, B, S_, mode, km, sl)
    acc = None
    for b, L in enumerate(lens):
        r = slice(b * S_, b * S_ + L)
        kb = None if km is None else km[b:b + 1, :L].contiguous()
        y1, dx1, dp1 = _layer_step("fp32", params, x[r].contiguous(), gy[r].contiguous(), 1, L, mode, kb, None)
        assert rel(y[r], y1) < 1e-5, (b, rel(y[r], y1))
        assert rel(dx[r], dx1) < 1e-5, (b, rel(dx[r], dx1))
        acc = dp1 if acc is None else [a + c for a, c in zip(acc, dp1)]
    for i, (a, c) in enumerate(zip(dps, acc)):
        if i == 5:         # key bias: its gradient is exactly zero in exact arithmetic (softmax ignores a shift shared by all keys), only rounding is left
            assert max(a.abs().max().item(), c.abs().max().item()) < 1e-4 * dps[7].abs().max().item()
        else:
            assert rel(a, c) < 1e-4, (i, rel(a, c))
