"""GPU: the dense 3-D convolution entry points (csrc/conv3d.hip, include/tavhip_conv.h) against their fp64 model with per-element bounds
(tests/conv3d_ref.py), exact-integer and structural cases whose answer does not depend on rounding, VisualClassification against a float64
torch twin under a gate computed from the reference alone, and two epochs of the visual training loop.

The kernel tests run inside the guard-band allocator (tests/guarded.py): every operand sits in a watched 0xFF buffer, every output and
workspace is allocated under guard, and verify() reports any store outside a tensor or into an operand.  The activations of this ABI are
dense channels-last tensors without stride arguments, so the operands carry no padded row pitch; a read past one lands in 0xFF = NaN.

Later stages are fed the kernels' own earlier outputs (dZ from the kernel's g, dX and dW from the kernel's dZ), so every bound is the bound
of one launch."""
import numpy as np
import pytest
import torch

import conv3d_ref as R
import guarded
import tav_amd  # noqa: F401
from tav_amd import ops

pytestmark = pytest.mark.gpu
TW = 32                                                       # asserted against the plan
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _dev(a, dtype="f32"):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(TORCH_DT[dtype]).cuda()


def _host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _th(Cin, Cout, dtype, dims=(1, 5, 8, 40)):
    p = ops.conv3d_plan(*dims, Cin, Cout, TORCH_DT[dtype])
    assert p["tw"] == TW and p["th"] in (1, 2, 4) and p["block"] == 64 * p["th"] and p["lds_bytes"] <= 160 * 1024 and p["wg_lds_bytes"] <= 160 * 1024
    assert p["cin_p"] == R.cp(Cin) and p["cout_p"] == R.cp(Cout) and p["n_tiles"] * p["n_passes"] >= p["cout_p"] // 16
    return p["th"]


def _layer(x, dtype, *, gelu=True, nslabs=0, bias=True):
    """Forward, dZ, input gradient and weight gradient of one layer under guard (call inside guarded.active()).  -> dict of host arrays in
    torch layouts, the pad channels of every channels-last output under *_pad."""
    Cin, Cout, td = x["Cin"], x["Cout"], TORCH_DT[dtype]
    xd = guarded.guarded_input(_dev(R.to_cl(x["x"]), dtype))
    w32 = guarded.guarded_input(_dev(x["w"]))
    w_op, w_flip = ops.conv3d_pack_weight(w32, td), ops.conv3d_pack_weight(w32, td, flip_transpose=True)
    bp = None
    if bias:
        bp = np.zeros(R.cp(Cout))
        bp[:Cout] = x["b"]
        bp = guarded.guarded_input(_dev(bp))
    y, g = ops.conv3d_fwd(xd, w_op, bp, Cin, Cout, gelu=gelu, want_g=gelu)
    dy = guarded.guarded_input(_dev(R.to_cl(x["dy"]), dtype))
    dz = ops.conv3d_dz(dy, g)
    dx = ops.conv3d_dgrad(dz, w_flip, Cin, Cout)
    dw, db = ops.conv3d_wgrad(xd, dz, Cin, Cout, nslabs=nslabs)
    k = dict(dw=_host(dw), db=_host(db))
    for name, t, Cn in (("y", y, Cout), ("g", g, Cout), ("dz", dz, Cout), ("dx", dx, Cin)):
        if t is not None:
            k[name], k[name + "_pad"] = R.from_cl(_host(t), Cn)
    return k


def _check_layer(x, dtype, k, th, nslabs_eff, gelu=True, bias=True):
    f = R.forward_ref(x["x"], x["w"], x["b"] if bias else None, dtype, gelu_on=gelu)
    res = R.check(k, f, ("y", "g") if gelu else ("y",))
    res.update(R.check(k, R.dz_ref(x["dy"], k["g"] if gelu else 1.0, dtype), ("dz",)))
    res.update(R.check(k, R.dgrad_ref(k["dz"], x["w"], dtype), ("dx",)))
    res.update(R.check(k, R.wgrad_ref(x["x"], k["dz"], dtype, th, nslabs_eff), ("dw", "db")))
    for name in ("y", "g", "dz", "dx"):
        if name + "_pad" in k:
            assert not k[name + "_pad"].any(), f"pad channels of {name} are not exactly zero"
    return res


def _dims(th, case):
    """(B, D', H', W') of the case list: D' in {1, 2, 3}, H' in {1, TH - 1, TH + 1}, W' in {1, TW - 1, TW, TW + 1, 2 TW + 3}."""
    return {"a": (1, 1, 1, 1), "b": (3, 2, th + 1, TW + 1), "c": (1, 3, max(th - 1, 1), 2 * TW + 3), "d": (3, 1, th + 1, TW - 1), "e": (1, 2, max(th - 1, 1), TW),
            "f": (3, 3, 1, TW + 1)}[case]


CASES = [((3, 32), "a", True), ((3, 32), "b", True), ((32, 32), "b", True), ((32, 32), "e", False), ((16, 48), "c", True), ((16, 48), "d", False),
         ((1, 16), "d", True), ((1, 16), "f", True), ((32, 32), "c", True)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("chan,case,gelu", CASES)
def test_forward_dgrad_wgrad_per_element(gpu, chan, case, gelu, dtype):
    Cin, Cout = chan
    th = _th(Cin, Cout, dtype)
    B, od, oh, ow = _dims(th, case)
    x = R.inputs(B, Cin, Cout, od + 2, oh + 2, ow + 2, dtype, 1000 * Cin + 10 * Cout + ord(case))
    plan = ops.conv3d_plan(B, od + 2, oh + 2, ow + 2, Cin, Cout, TORCH_DT[dtype])
    assert (plan["th"], plan["od"], plan["oh"], plan["ow"]) == (th, od, oh, ow) and plan["patches"] == B * od * -(-oh // th) * -(-ow // TW)
    with guarded.active() as g:
        k = _layer(x, dtype, gelu=gelu, bias=gelu)
        g.verify()
    res = _check_layer(x, dtype, k, th, plan["wg_nslabs"], gelu=gelu, bias=gelu)
    print(f"{chan} {case} {dtype} gelu {gelu} th {th}:", " ".join(f"{n} {v:.3f}" for n, v in res.items()))
    assert R.passed(res), res


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("chan", [(3, 32), (32, 32), (16, 48), (1, 16)])
def test_exact_integer_operands_bit_for_bit(gpu, chan, dtype):
    Cin, Cout = chan
    th = _th(Cin, Cout, dtype)
    B, od, oh, ow = 3, 2, th + 1, TW + 1
    x = R.int_inputs(B, Cin, Cout, od + 2, oh + 2, ow + 2, 5 + Cin)
    with guarded.active() as g:
        k = _layer(x, dtype, gelu=False)
        g.verify()
    rt = R.bf16_rne if dtype == "bf16" else (lambda a: a)
    z = R.conv(x["x"], x["w"]) + x["b"][None, :, None, None, None]
    dw, db = R.conv_wgrad(x["x"], x["dy"])
    assert np.array_equal(k["y"], rt(z)) and np.array_equal(k["dz"], x["dy"]) and np.array_equal(k["dx"], rt(R.conv_dgrad(x["dy"], x["w"])))
    assert np.array_equal(k["dw"], dw) and np.array_equal(k["db"], db)
    assert not k["y_pad"].any() and not k["dx_pad"].any() and not k["dz_pad"].any()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pack_input_and_weight_are_exact_with_zero_pads(gpu, dtype):
    x = R.inputs(2, 3, 20, 4, 5, 37, dtype, 3)
    td = TORCH_DT[dtype]
    with guarded.active() as g:
        cl = ops.conv3d_pack_input(guarded.guarded_input(_dev(x["x"])), td)
        w32 = guarded.guarded_input(_dev(x["w"]))
        w_op, w_flip = _host(ops.conv3d_pack_weight(w32, td)), _host(ops.conv3d_pack_weight(w32, td, flip_transpose=True))
        g.verify()
    assert np.array_equal(_host(cl), R.to_cl(x["x"]))
    ks = 32 if dtype == "bf16" else 16
    want = np.zeros((32, -(-27 * 16 // ks) * ks))
    want[:20, :27 * 16] = np.pad(np.moveaxis(x["w"].reshape(20, 3, 27), 1, 2), ((0, 0), (0, 0), (0, 13))).reshape(20, -1)
    assert np.array_equal(w_op, want)
    want = np.zeros((16, -(-27 * 32 // ks) * ks))
    wf = R.flip_t(x["w"])                                                      # [Cin][Cout][taps reversed]
    want[:3, :27 * 32] = np.pad(np.moveaxis(wf.reshape(3, 20, 27), 1, 2), ((0, 0), (0, 0), (0, 12))).reshape(3, -1)
    assert np.array_equal(w_flip, want)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_batch_row_alone_equals_the_row_inside_a_batch(gpu, dtype):
    Cin, Cout = 16, 48
    th = _th(Cin, Cout, dtype)
    x = R.inputs(3, Cin, Cout, 4, th + 3, TW + 3, dtype, 21)
    one = dict(x, x=x["x"][1:2], dy=x["dy"][1:2])
    with guarded.active() as g:
        kb, k1 = _layer(x, dtype), _layer(one, dtype)
        g.verify()
    for name in ("y", "g", "dz", "dx"):
        assert np.array_equal(kb[name][1:2], k1[name]), name


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_weight_gradient_is_repeatable_and_independent_of_the_slab_count(gpu, dtype):
    Cin, Cout = 32, 32
    th = _th(Cin, Cout, dtype)
    B, od, oh, ow = 1, 1, 2 * th + 1, TW + 1                                     # 3 x 2 = 6 patches... asserted below
    dims = (B, od + 2, oh + 2, ow + 2)
    patches = ops.conv3d_plan(*dims, Cin, Cout, TORCH_DT[dtype])["patches"]
    assert patches == 6
    xi, xr = R.int_inputs(*dims[:1], Cin, Cout, *dims[1:], 9), R.inputs(*dims[:1], Cin, Cout, *dims[1:], dtype, 10)
    got = {}
    for ns in (1, 2, 5, patches + 3, 1):
        with guarded.active() as g:
            ki, kr = _layer(xi, dtype, gelu=False, nslabs=ns), _layer(xr, dtype, nslabs=ns)
            g.verify()
        got.setdefault(ns, []).append(kr)
        dw, db = R.conv_wgrad(xi["x"], xi["dy"])
        assert np.array_equal(ki["dw"], dw) and np.array_equal(ki["db"], db), ns
        res = R.check(kr, R.wgrad_ref(xr["x"], kr["dz"], dtype, th, ns), ("dw", "db"))
        print(f"{dtype} nslabs {ns}:", res)
        assert R.passed(res), (ns, res)
    assert np.array_equal(got[1][0]["dw"], got[1][1]["dw"]) and np.array_equal(got[1][0]["db"], got[1][1]["db"])


# ---------------------------------------------------------------------------------------------- flatten + Linear, sigmoid
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nparts", [0, 2, 4, 200])
def test_flat_linear_and_sigmoid(gpu, dtype, nparts):
    B, Cn, D, H, W, O = 3, 20, 3, 5, 7, 7                                      # 20 channels are carried as 32; S = 105 is no multiple of any split
    rng = np.random.default_rng(4 + nparts)
    x = R.round_to(rng.standard_normal((B, Cn, D, H, W)) * (2.0 ** (np.arange(Cn) % 7 - 3.0))[None, :, None, None, None], dtype)[0]
    w = (0.05 * rng.standard_normal((O, Cn * D * H * W))).astype(np.float32).astype(np.float64)
    b = rng.standard_normal(O).astype(np.float32).astype(np.float64)
    dy = rng.standard_normal((B, O)).astype(np.float32).astype(np.float64)
    lin = torch.nn.Linear(Cn * D * H * W, O).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w)), lin.bias.copy_(torch.from_numpy(b))
    want = lin(torch.from_numpy(x).view(B, -1)).detach().numpy()               # torch's flatten order, on the NCDHW view
    with guarded.active() as g:
        xd, wd, bd, dyd = (guarded.guarded_input(t) for t in (_dev(R.to_cl(x), dtype), _dev(w), _dev(b), _dev(dy)))
        out = ops.flat_linear_fwd(xd, wd, bd, Cn, nparts=nparts)
        again = ops.flat_linear_fwd(xd, wd, bd, Cn, nparts=nparts)
        dx, dw, db = ops.flat_linear_bwd(xd, wd, dyd, Cn)
        sy = ops.sigmoid_fwd(out)
        sdx = ops.sigmoid_bwd(sy, dyd)
        g.verify()
    eff = nparts or 1                                                            # tav_flat_linear_parts(105) = 1
    ref = R.flat_ref(x, w, b, eff, dtype, dy)
    assert R.rel_max(ref["out"], want) < 1e-12
    dxk, dx_pad = R.from_cl(_host(dx), Cn)
    k = dict(out=_host(out), dx=dxk, dw=_host(dw), db=_host(db))
    res = R.check(k, ref, ("out", "dx", "dw", "db"))
    s = R.sigmoid_ref(k["out"], dy)
    res.update(R.check(dict(y=_host(sy)), s, ("y",)))
    res.update(R.check(dict(dx=_host(sdx)), R.sigmoid_ref(k["out"], dy) | dict(dx=dy * _host(sy) * (1 - _host(sy))), ("dx",)))
    print(f"flat {dtype} nparts {nparts}:", res)
    assert R.passed(res), res
    assert torch.equal(out, again) and not dx_pad.any()


# ---------------------------------------------------------------------------------------------- the model against a float64 torch twin
def _twin(hidden, clip, O):
    m = torch.nn.Module()
    m.in_layer = torch.nn.Conv3d(3, hidden[0], 3)
    m.hidden_layers = torch.nn.ModuleList(torch.nn.Conv3d(hidden[i], hidden[i + 1], 3) for i in range(len(hidden) - 1))
    T, H, W = (s - 2 * len(hidden) for s in clip)
    m.out_layer = torch.nn.Linear(hidden[-1] * T * H * W, O)
    return m


@pytest.mark.parametrize("policy,dtype", [("fp32", "f32"), ("bf16", "bf16")])
def test_model_matches_a_float64_torch_twin_within_four_chain_errors(gpu, policy, dtype):
    from tav_amd import runtime
    from tav_amd.SingleModels.models.visual import VisualClassification
    from tav_amd.utils.global_functions import CrossEntropyLoss
    clip, hidden, B, O = (6, 12, 20), [16, 32], 3, 7
    torch.manual_seed(11)
    twin = _twin(hidden, clip, O).double()
    x = torch.randn(B, 3, *clip, dtype=torch.float64)
    target, cw = torch.tensor([2, 0, 5]), torch.linspace(0.6, 0.95, O, dtype=torch.float64)
    # the twin, float64 on the CPU
    a = x
    for layer in [twin.in_layer, *twin.hidden_layers]:
        a = torch.nn.functional.gelu(layer(a))
    logits = torch.sigmoid(twin.out_layer(a.view(B, -1)))
    loss = torch.nn.functional.cross_entropy(logits, target, weight=cw)
    loss.backward()
    names = [n for n, _ in twin.named_parameters()]
    want = dict(logits=logits.detach().numpy(), loss=float(loss), grads=[p.grad.numpy() for p in twin.parameters()])
    # the gate, from the reference alone
    P = {n: p.detach().numpy() for n, p in twin.named_parameters()}
    convs = [(P["in_layer.weight"], P["in_layer.bias"])] + [(P[f"hidden_layers.{i}.weight"], P[f"hidden_layers.{i}.bias"]) for i in range(len(hidden) - 1)]
    args = (x.numpy(), convs, P["out_layer.weight"], P["out_layer.bias"], target.numpy(), cw.numpy(), dtype)
    exact, chained = R.chain(*args, "exact"), R.chain(*args, "chained")
    assert R.rel_max(exact["logits"], want["logits"]) < 1e-12 and abs(exact["loss"] - want["loss"]) < 1e-12 * abs(want["loss"])
    assert all(R.rel_max(e, w) < 1e-11 for e, w in zip(exact["grads"], want["grads"]))
    gate = dict(logits=R.rel_max(chained["logits"], exact["logits"]), loss=abs(chained["loss"] - exact["loss"]) / abs(exact["loss"]),
                **{n: R.rel_max(c, e) for n, c, e in zip(names, chained["grads"], exact["grads"])})
    # Every compared quantity is read from an f32 buffer, so no e_chain is taken below u = 2^-24, half an f32 ulp of the largest element:
    # the draw of a single scalar (the loss) can land on an f32 value by chance and would then demand an exact result.
    gate = {n: max(v, R.U) for n, v in gate.items()}
    # the product
    runtime.set_precision(policy)
    try:
        ours = VisualClassification({"input_dim": 3, "output_dim": O, "hidden_layers": hidden, "clip_shape": clip})
        ours.load_state_dict({k: v.float() for k, v in twin.state_dict().items()})
        ours.cuda()
        out = ours(x.float().cuda().unsqueeze(1))
        lo = CrossEntropyLoss(weight=cw.float())(out, target.cuda())
        lo.backward()
        torch.cuda.synchronize()
        got = dict(logits=R.rel_max(_host(out), exact["logits"]), loss=abs(float(lo) - exact["loss"]) / abs(exact["loss"]),
                   **{n: R.rel_max(_host(p.grad), e) for (n, p), e in zip(ours.named_parameters(), exact["grads"])})
    finally:
        runtime.set_precision("bf16")
    for n in got:
        print(f"model {policy} {n}: error {got[n]:.3e}  e_chain {gate[n]:.3e}  ratio {got[n] / max(gate[n], 1e-300):.2f}")
    assert tuple(out.shape) == (B, O) and all(np.isfinite(v) for v in got.values())
    bad = {n: (got[n], gate[n]) for n in got if got[n] > 4 * gate[n]}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- the loop
def test_two_epochs_of_the_visual_loop_on_synthetic_clips(gpu):
    from tav_amd import runtime
    from tav_amd.SingleModels import visual_nn as V
    from tav_amd.SingleModels.models.visual import VisualClassification
    from tav_amd.SingleModels.train_model.visual_training import evaluate_visual, visual_train
    from tav_amd.utils.global_functions import CrossEntropyLoss, Metrics
    clip, O = (6, 12, 20), 7
    torch.manual_seed(0)
    runtime.set_precision("bf16")
    model = VisualClassification({"input_dim": 3, "output_dim": O, "hidden_layers": "16,32", "clip_shape": clip}).cuda()
    crit = CrossEntropyLoss(weight=torch.linspace(0.6, 0.95, O))
    metric = Metrics(num_classes=O, rank="cuda")
    train = V.prepare_dataloader(V.SyntheticClips(6, clip, O, 1), 3, clip_shape=clip, shuffle=False)
    val = V.prepare_dataloader(V.SyntheticClips(3, clip, O, 2), 3, clip_shape=clip, shuffle=False)
    log = []
    visual_train(model, train, val, crit, 1e-3, 2, 1e-4, 2, metric, patience=None, clip=1.0, log=log)
    assert len(log) == 2 and all(np.isfinite(e["train/train_loss"]) and np.isfinite(e["val/total_loss_val"]) for e in log)
    assert all(int(e["train/cm"].sum()) == 6 and int(e["val/cm"].sum()) == 3 for e in log)
    res = evaluate_visual(model, val, metric)
    assert int(res["test/ConfusionMatrix"].sum()) == 3
    # a repeated batch: the loss falls
    from tav_amd.optim import FusedAdamW
    opt = FusedAdamW(list(model.parameters()), lr=1e-3, weight_decay=0.0)
    xb, yb = next(iter(train))
    losses = []
    for _ in range(4):
        loss = crit(model(xb), yb.long().cuda())
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("repeated batch:", losses)
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0]
