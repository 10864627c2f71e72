"""GPU: engine.encoder_layer, one layer at a time -- what an fp8 layer is, bit for bit.

An fp8 layer is the plain layer plus its e4m3 sites (Policy.fp8_fwd / fp8_bwd / fp8_wgrad8) and f32 outputs of the two dgrads that feed a
LayerNorm backward.  With every e4m3 site switched off it must therefore reproduce the bf16 layer with f32 dgrad outputs exactly: the
output, the input gradient and all 16 parameter gradients.  And with its sites on, the saved-tensor layout (None in the slots a path does
not keep) must carry a backward that two runs from the same inputs and fresh scaling states repeat bit for bit.

Shapes: wide = 10 heads (H 640), FFN 2560, 2 x 64 tokens: 100 + 100 + 25 + 75 = 300 weight-gradient tiles >= 256, the grouped launch;
narrow = 2 heads (H 128), FFN 512, 2 x 37 tokens: 12 tiles, one TN GEMM per weight, and a partial attention tile."""
import pytest
import torch

import tav_amd  # noqa: F401
from tav_amd import engine, runtime

pytestmark = pytest.mark.gpu

SHAPES = {"wide": (10, 2560, 2, 64), "narrow": (2, 512, 2, 37)}        # nheads, FFN, B, S


@pytest.fixture(autouse=True)
def _leave_the_default_policy():
    yield
    runtime.set_precision("bf16")


def _layer(H, F, seed):
    g = torch.Generator().manual_seed(seed)

    def P(*shape, scale=0.05, base=0.0):
        return torch.nn.Parameter((base + torch.randn(*shape, generator=g) * scale).cuda())
    return [P(H, base=1.0), P(H), P(H, H), P(H), P(H, H), P(H), P(H, H), P(H), P(H, H), P(H), P(H, base=1.0), P(H), P(F, H), P(F), P(H, F), P(H)]


def _case(shape):
    nh, F, B, S = SHAPES[shape]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B * S, nh * 64, generator=g).cuda()
    gy = torch.randn(B * S, nh * 64, generator=g).cuda()
    return _layer(nh * 64, F, 7), x, gy


def _step(policy, shape, pre_ln, params, x, gy, finite=True):
    """One forward + backward under a FRESH context (new operand cache, new delayed-scaling states) -> [x2, dx, 16 parameter gradients].
    finite=False: the caller feeds a poisoned gy and judges the outputs itself."""
    nh, _, B, S = SHAPES[shape]
    ectx = runtime.set_precision(policy)
    for p in params:
        p.grad = None
    x = x.clone().requires_grad_(True)
    spec = engine.LayerSpec(B, S, nh, 1e-12, pre_ln=pre_ln, branch="video")
    y, _ = engine.encoder_layer(ectx, spec, x, None, None, params)
    (y * gy).sum().backward()
    torch.cuda.synchronize()
    out = [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in params]
    assert len(out) == 18 and (not finite or all(torch.isfinite(t).all() for t in out))
    return out


@pytest.mark.parametrize("pre_ln", [True, False])
@pytest.mark.parametrize("shape", ["wide", "narrow"])
def test_fp8_layer_without_e4m3_sites_is_the_bf16_layer(gpu, shape, pre_ln):
    params, x, gy = _case(shape)
    pol = engine.Policy("fp8", fp8_fwd=0, fp8_bwd=0)
    assert pol.fp8 and "video" in pol.fp8_stacks and pol.fp8_fwd == 0 and pol.fp8_bwd == 0 and not pol.fp8_wgrad8
    plain = engine.Policy("bf16")
    plain.dgrad_lp = False                       # f32 dgrad outputs, as an fp8 layer forces them
    got = _step(pol, shape, pre_ln, params, x, gy)
    ref = _step(plain, shape, pre_ln, params, x, gy)
    names = ["x2", "dx"] + [f"param {i}" for i in range(16)]
    diff = [n for n, a, b in zip(names, got, ref) if not torch.equal(a, b)]
    print(f"[{shape}, pre_ln={pre_ln}] tensors that differ: {diff or 'none'}")
    assert not diff, diff


@pytest.mark.parametrize("policy", ["fp8", "fp8-all", "fp8-wgrad8"])
@pytest.mark.parametrize("pre_ln", [True, False])
@pytest.mark.parametrize("shape", ["wide", "narrow"])
def test_fp8_layer_replays_bitwise(gpu, shape, pre_ln, policy):
    params, x, gy = _case(shape)
    first = _step(policy, shape, pre_ln, params, x, gy)
    again = _step(policy, shape, pre_ln, params, x, gy)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    sts = runtime.ctx().cache._fp8_states
    assert sts is not None and sts.calibrated                # the layer did run its e4m3 sites


@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp8-all", "fp8-wgrad8"])
@pytest.mark.parametrize("pre_ln", [True, False])
def test_poisoned_output_gradient_stays_loud(gpu, pre_ln, policy):
    """One NaN or Inf element of gy in batch entry 0 ("Non-finite values"): the forward is untouched; attention spreads the row to
    every token of ITS entry and to no token of the other one; every parameter gradient sums over the poisoned rows, so the gradient norm and the
    clip coefficient are non-finite -- the step cannot go on quietly; and no fp8 scaling state takes a non-finite word, before or after
    tav_fp8_roll_states."""
    import nonfinite_ref as NF
    from tav_amd import ops, optim
    _, _, B, S = SHAPES["narrow"]
    params, x, gy = _case("narrow")
    clean = _step(policy, "narrow", pre_ln, params, x, gy)
    pat = ["bf16", "fp8", "fp8-all", "fp8-wgrad8"].index(policy) + (0 if pre_ln else 1)          # all five patterns over the eight cases
    bad = gy.clone()
    bad.view(torch.int32)[S - 1, 77] = NF.signed_bits(pat, "f32")                                # the last token of entry 0
    got = _step(policy, "narrow", pre_ln, params, x, bad, finite=False)
    y, dx, grads = got[0], got[1], got[2:]
    assert torch.equal(y, clean[0])
    rows = torch.isfinite(dx).all(1)
    print(f"[{policy}, pre_ln={pre_ln}, {NF.NAMES[pat % NF.NPAT]}] finite dx rows: entry 0 {int(rows[:S].sum())}/{S}, entry 1 {int(rows[S:].sum())}/{S}; "
          f"parameter gradients without a non-finite element: {[i for i, g in enumerate(grads) if torch.isfinite(g).all()]}")
    assert not rows[:S].any(), "a token of the poisoned entry has a finite input gradient"
    assert rows[S:].all(), "the poison reached the other batch entry"
    assert len(grads) == 16 and not any(torch.isfinite(g).all() for g in grads)
    norm = optim.grad_norm(params)
    scal = torch.stack([norm[0] * norm[0], norm[0], norm[0]]).contiguous()
    ops.check(ops.lib().tav_clip_coef(ops.ptr(scal[0:1]), 1.0, ops.ptr(scal[1:2]), ops.ptr(scal[2:3]), ops.stream()), "clip_coef")
    assert not torch.isfinite(norm).any() and not torch.isfinite(scal[1:]).any()
    sts = runtime.ctx().cache._fp8_states
    assert (sts is not None and bool(sts.calibrated)) == (policy != "bf16")
    if sts is not None:
        assert torch.isfinite(sts.dev).all()
        ops.fp8_roll_all()
        assert torch.isfinite(sts.dev).all()
