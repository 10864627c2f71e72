"""CPU: the dense 3-D convolution's host side.

tests/conv3d_ref.py against torch.nn.functional.conv3d, its autograd gradients and nn.Linear in float64; the mutants of that reference, each
caught by the inputs the GPU tests use; csrc/conv3d_plan.h alone under ASan + UBSan as a program of its own (tests/host_program.py);
include/tavhip_conv.h against its row of _lib.ABIS type by type and the families kept apart (tests/abi_check.py); argument faults through
the built library; and the pieces of VisualClassification and its entrypoint that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abi_check
import conv3d_ref as R
import tav_amd  # noqa: F401
from host_program import run_alone_under_sanitizers
from tav_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_ALIGN = -1, -2, -3, -4


# ---------------------------------------------------------------------------------------------- against torch, fp64
@pytest.mark.parametrize("chan", [(3, 8), (5, 5)])
def test_reference_equals_torch_conv3d_and_its_gradients_in_float64(chan):
    Cin, Cout = chan
    x = R.inputs(2, Cin, Cout, 5, 6, 7, "f32", 1)
    X, W, b = (torch.tensor(x[k], requires_grad=True) for k in ("x", "w", "b"))
    z = torch.nn.functional.conv3d(X, W, b)
    y = torch.nn.functional.gelu(z)
    (y * torch.tensor(x["dy"])).sum().backward()
    f = R.forward_ref(x["x"], x["w"], x["b"], "f32")
    assert R.rel_max(f["y"], y.detach().numpy()) < 1e-12
    assert R.rel_max(R.forward_ref(x["x"], x["w"], x["b"], "f32", gelu_on=False)["y"], z.detach().numpy()) < 1e-12
    dz = x["dy"] * f["g"]
    assert R.rel_max(R.conv_dgrad(dz, x["w"]), X.grad.numpy()) < 1e-12
    assert R.rel_max(R.conv(dz, R.flip_t(x["w"]), 2), X.grad.numpy()) < 1e-12          # the halo-2 forward on the flipped, transposed weights
    dw, db = R.conv_wgrad(x["x"], dz)
    assert R.rel_max(dw, W.grad.numpy()) < 1e-12 and R.rel_max(db, b.grad.numpy()) < 1e-12
    assert (f["y_bound"] > 0).all() and (f["g_bound"] > 0).all()


def test_reference_equals_nn_linear_on_the_ncdhw_view_in_float64():
    rng = np.random.default_rng(2)
    B, Cn, D, H, W, O = 3, 5, 2, 3, 4, 7
    x, dy = rng.standard_normal((B, Cn, D, H, W)), rng.standard_normal((B, O))
    lin = torch.nn.Linear(Cn * D * H * W, O).double()
    X = torch.tensor(x, requires_grad=True)
    out = lin(X.view(B, -1))
    (torch.sigmoid(out) * torch.tensor(dy)).sum().backward()
    w, b = lin.weight.detach().numpy(), lin.bias.detach().numpy()
    s = R.sigmoid_ref(out.detach().numpy(), dy)
    ref = R.flat_ref(x, w, b, 3, "f32", s["dx"])
    assert R.rel_max(ref["out"], out.detach().numpy()) < 1e-12 and R.rel_max(s["y"], torch.sigmoid(out).detach().numpy()) < 1e-12
    assert R.rel_max(ref["dx"], X.grad.numpy()) < 1e-6 and R.rel_max(ref["dw"], lin.weight.grad.numpy()) < 1e-6          # (s["dx"] reads the f32-stored y)
    assert R.rel_max(ref["db"], lin.bias.grad.numpy()) < 1e-6
    # channels-last round trip of the layout helpers, pads zero
    cl = R.to_cl(x)
    back, pad = R.from_cl(cl, Cn)
    assert cl.shape == (B, D, H, W, 16) and np.array_equal(back, x) and not pad.any()


def test_whole_step_reference_equals_torch_autograd_in_float64():
    torch.manual_seed(5)
    clip, hidden, B, O = (5, 6, 7), [4, 6], 2, 7
    convs = [torch.nn.Conv3d(3, 4, 3).double(), torch.nn.Conv3d(4, 6, 3).double()]
    lin = torch.nn.Linear(6 * 1 * 2 * 3, O).double()
    x, target, cw = torch.randn(B, 3, *clip, dtype=torch.float64), torch.tensor([1, 6]), torch.linspace(0.6, 0.95, O, dtype=torch.float64)
    a = x
    for c in convs:
        a = torch.nn.functional.gelu(c(a))
    logits = torch.sigmoid(lin(a.view(B, -1)))
    loss = torch.nn.functional.cross_entropy(logits, target, weight=cw)
    loss.backward()
    params = [p for c in convs for p in (c.weight, c.bias)] + [lin.weight, lin.bias]
    args = (x.numpy(), [(c.weight.detach().numpy(), c.bias.detach().numpy()) for c in convs], lin.weight.detach().numpy(), lin.bias.detach().numpy(),
            target.numpy(), cw.numpy())
    e = R.chain(*args, "f32", "exact")
    assert R.rel_max(e["logits"], logits.detach().numpy()) < 1e-12 and abs(e["loss"] - float(loss.detach())) < 1e-12
    for got, p in zip(e["grads"], params):
        assert R.rel_max(got, p.grad.numpy()) < 1e-11
    # the chained mode is near, and nearer in f32 than in bf16
    errs = {}
    for dtype in ("f32", "bf16"):
        c = R.chain(*args, dtype, "chained")
        errs[dtype] = max(R.rel_max(c["logits"], e["logits"]), *(R.rel_max(g, w) for g, w in zip(c["grads"], e["grads"])))
    print("chained vs exact:", errs)
    assert 0 < errs["f32"] < 1e-4 and errs["f32"] < errs["bf16"] < 0.2


# ---------------------------------------------------------------------------------------------- the tester tested
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_clean_reference_accepts_and_every_mutant_is_caught(dtype):
    x = R.inputs(2, 4, 4, 5, 6, 37, dtype, 7)                                     # the GPU tests' inputs at a small size; Cin == Cout for mutant 3
    rng = np.random.default_rng(8)
    fw, fb = 0.1 * rng.standard_normal((7, 4 * 3 * 4 * 35)), rng.standard_normal(7)
    clean = R.verdict(x, dtype, R.simulate(x, dtype, fw, fb), fw, fb)
    assert R.passed(clean), clean
    for mut, name in R.MUTANTS.items():
        v = R.verdict(x, dtype, R.simulate(x, dtype, fw, fb, mut), fw, fb)
        assert not R.passed(v), f"mutant {name} survives"
    assert len(R.MUTANTS) == 6


def test_exact_integer_generator_and_chain_lengths():
    x = R.int_inputs(3, 32, 32, 4, 7, 35, 1)
    for k in ("x", "w", "b", "dy"):
        assert np.array_equal(x[k], np.rint(x[k])) and np.abs(x[k]).max() == 7
    assert np.abs(R.conv(np.abs(x["x"]), np.abs(x["w"]))).max() + 7 < 2 ** 24
    assert R.chain_len(32, "bf16") == 32 + 1 + 27 and R.chain_len(3, "bf16") == 32 + 1 + 14 and R.chain_len(32, "f32") == 4 + 1 + 216
    assert R.wgrad_chain(1, 1, 9, 33, 4, 2, "bf16") == 32 + 1 + 3 * 4 + 2 and R.wgrad_chain(1, 1, 9, 33, 4, 9, "bf16") == 32 + 1 + 4 + 9


# ---------------------------------------------------------------------------------------------- conv3d_plan.h alone
def test_conv3d_plan_header_alone_under_sanitizers(tmp_path):
    run_alone_under_sanitizers("conv3d_plan_check.cpp", tmp_path)


# ---------------------------------------------------------------------------------------------- header against binding
def test_conv_binding_matches_its_header_type_by_type(tmp_path):
    assert len(abi_check.check_binding(abi_check.abi("tavhip_conv.h"), tmp_path)) == 14


def test_the_other_three_symbol_tables_are_unchanged():
    abi_check.check_families_apart()


# ---------------------------------------------------------------------------------------------- argument faults, nothing launches
def _fwd_args(**kw):
    a = _lib.Conv3dFwdArgs()
    for f in ("x", "w", "y"):
        setattr(a, f, 4096)                                   # only tested for NULL-ness and alignment before a fault is found
    a.B, a.D, a.H, a.W, a.Cin, a.Cout, a.dtype = 2, 5, 6, 40, 3, 32, _lib.TAV_BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _wgrad_args(**kw):
    a = _lib.Conv3dWgradArgs()
    for f in ("x", "dz", "workspace", "dw"):
        setattr(a, f, 4096)
    a.B, a.D, a.H, a.W, a.Cin, a.Cout, a.dtype, a.nslabs = 2, 5, 6, 40, 3, 32, _lib.TAV_F32, 2
    a.workspace_bytes = _lib.lib().tav_conv3d_wgrad_ws_bytes(2, 5, 6, 40, 3, 32, _lib.TAV_F32, 2)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _flat_args(cls, **kw):
    a = cls()
    for f in ("x", "w", "out", "workspace", "dy", "dw"):
        if hasattr(a, f):
            setattr(a, f, 4096)
    a.B, a.S, a.C, a.O, a.dtype = 3, 105, 20, 7, _lib.TAV_BF16
    if hasattr(a, "workspace_bytes"):
        a.workspace_bytes = 3 * 7 * 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_invalid_arguments_are_refused_before_any_launch():
    h = _lib.lib()
    fwd = lambda **kw: h.tav_conv3d_fwd(C.byref(_fwd_args(**kw)), None)                 # noqa: E731
    wg = lambda **kw: h.tav_conv3d_wgrad(C.byref(_wgrad_args(**kw)), None)              # noqa: E731
    ff = lambda **kw: h.tav_flat_linear_fwd(C.byref(_flat_args(_lib.FlatLinearFwdArgs, **kw)), None)      # noqa: E731
    fb = lambda **kw: h.tav_flat_linear_bwd(C.byref(_flat_args(_lib.FlatLinearBwdArgs, **kw)), None)      # noqa: E731
    assert h.tav_conv3d_fwd(None, None) == ERR_NULL and h.tav_conv3d_wgrad(None, None) == ERR_NULL
    assert h.tav_flat_linear_fwd(None, None) == ERR_NULL and h.tav_flat_linear_bwd(None, None) == ERR_NULL
    for f in ("x", "w", "y"):
        assert fwd(**{f: None}) == ERR_NULL, f
    for f in ("x", "dz", "workspace", "dw"):
        assert wg(**{f: None}) == ERR_NULL, f
    assert fwd(dtype=_lib.TAV_FP8) == ERR_DTYPE and fwd(dtype=9) == ERR_DTYPE and wg(dtype=_lib.TAV_FP8) == ERR_DTYPE and ff(dtype=_lib.TAV_FP8) == ERR_DTYPE
    assert fwd(Cin=0) == ERR_SHAPE and fwd(Cout=129) == ERR_SHAPE and fwd(D=2) == ERR_SHAPE and fwd(pad=1) == ERR_SHAPE and fwd(B=0) == ERR_SHAPE
    assert fwd(g=4096) == ERR_SHAPE and fwd(gelu=2) == ERR_SHAPE
    assert fwd(dtype=_lib.TAV_F32, Cin=113) == ERR_SHAPE                              # the f32 halo of 128 channels does not fit the LDS
    assert fwd(x=4104) == ERR_ALIGN and fwd(bias=4100) == ERR_ALIGN and fwd(x=4104, Cin=0) == ERR_SHAPE and fwd(x=4104, y=None) == ERR_NULL
    assert wg(nslabs=-1) == ERR_SHAPE and wg(nslabs=4097) == ERR_SHAPE and wg(workspace_bytes=64) == ERR_SHAPE and wg(dz=4104) == ERR_ALIGN
    assert ff(O=17) == ERR_SHAPE and ff(O=0) == ERR_SHAPE and ff(nparts=2) == ERR_SHAPE and ff(nparts=4097) == ERR_SHAPE and ff(x=4104) == ERR_ALIGN
    assert fb(O=17) == ERR_SHAPE and fb(x=None) == ERR_NULL and fb(dx=4104) == ERR_ALIGN and fb(C=129) == ERR_SHAPE
    p = _lib.Conv3dPlan()
    assert h.tav_conv3d_get_plan(8, 14, 222, 222, 32, 32, 0, _lib.TAV_BF16, C.byref(p)) == 0
    assert (p.cin_p, p.cout_p, p.tw, p.th, p.block, p.n_tiles, p.n_passes, p.k_steps, p.kp) == (32, 32, 32, 4, 256, 2, 1, 27, 864)
    assert (p.od, p.oh, p.ow, p.patches) == (12, 220, 220, 8 * 12 * 55 * 7) and p.lds_bytes <= 64 * 1024 and p.wg_lds_bytes <= 64 * 1024
    assert (p.wg_block, p.wg_ci_tiles, p.wg_co_tiles, p.wg_groups, p.wg_slab_floats) == (256, 2, 2, 1, 28 * 32 * 32) and 1 <= p.wg_nslabs <= 4096
    assert h.tav_conv3d_wgrad_ws_bytes(8, 14, 222, 222, 32, 32, _lib.TAV_BF16, 0) == p.wg_nslabs * p.wg_slab_floats * 4
    assert h.tav_conv3d_get_plan(8, 16, 224, 224, 3, 32, 0, _lib.TAV_BF16, C.byref(p)) == 0 and (p.cin_p, p.k_steps) == (16, 14)
    assert h.tav_conv3d_get_plan(8, 12, 220, 220, 32, 32, 2, _lib.TAV_F32, C.byref(p)) == 0 and (p.od, p.oh, p.ow, p.wg_block) == (14, 222, 222, 0)
    assert h.tav_conv3d_get_plan(8, 14, 222, 222, 32, 32, 0, _lib.TAV_BF16, None) == ERR_NULL
    assert h.tav_conv3d_get_plan(8, 14, 222, 222, 32, 32, 0, _lib.TAV_FP8, C.byref(p)) == ERR_DTYPE
    assert h.tav_conv3d_wgrad_ws_bytes(8, 14, 222, 222, 32, 32, _lib.TAV_FP8, 0) == ERR_DTYPE
    assert h.tav_conv3d_pack_input(None, 4096, 1, 3, 4, 4, 4, _lib.TAV_BF16, None) == ERR_NULL
    assert h.tav_conv3d_pack_input(4096, 4096, 1, 129, 4, 4, 4, _lib.TAV_BF16, None) == ERR_SHAPE
    assert h.tav_conv3d_pack_weight(4096, None, 32, 3, 0, _lib.TAV_BF16, None) == ERR_NULL and h.tav_conv3d_pack_weight(4096, 4096, 32, 3, 2, _lib.TAV_BF16, None) == ERR_SHAPE
    assert h.tav_conv3d_pack_weight(4096, 4096, 32, 3, 0, _lib.TAV_FP8, None) == ERR_DTYPE
    assert h.tav_conv3d_dz(None, None, 4096, 64, _lib.TAV_F32, None) == ERR_NULL and h.tav_conv3d_dz(4096, None, 4096, 6, _lib.TAV_F32, None) == ERR_SHAPE
    assert h.tav_conv3d_dz(4096, 4100, 4096, 64, _lib.TAV_F32, None) == ERR_ALIGN and h.tav_conv3d_dz(4096, None, 4096, 64, _lib.TAV_FP8, None) == ERR_DTYPE
    assert h.tav_flat_linear_parts(105) == 1 and h.tav_flat_linear_parts(580800) == 568 and h.tav_flat_linear_ws_bytes(8, 580800, 7, 0) == 8 * 568 * 7 * 4
    sg, sb = h.tav_sigmoid_fwd, h.tav_sigmoid_bwd
    assert sg(None, 64, 4, None) == ERR_NULL and sg(64, None, 4, None) == ERR_NULL and sg(64, 64, 0, None) == ERR_SHAPE
    assert sb(None, 64, 64, 4, None) == ERR_NULL and sb(64, None, 64, 4, None) == ERR_NULL and sb(64, 64, None, 4, None) == ERR_NULL and sb(64, 64, 64, -1, None) == ERR_SHAPE


# ---------------------------------------------------------------------------------------------- VisualClassification without a GPU
def _twin(input_dim, hidden, n_features, O):
    m = torch.nn.Module()
    m.in_layer = torch.nn.Conv3d(input_dim, hidden[0], 3)
    m.hidden_layers = torch.nn.ModuleList(torch.nn.Conv3d(hidden[i], hidden[i + 1], 3) for i in range(len(hidden) - 1))
    m.out_layer = torch.nn.Linear(n_features, O)
    return m


def test_state_dict_is_torchs_and_default_in_features_is_the_references():
    from tav_amd.SingleModels.models.visual import ResNet50Classification, VisualClassification
    ours = VisualClassification({"input_dim": 3, "output_dim": 7, "hidden_layers": [16, 32], "clip_shape": (6, 12, 20)})
    ref = _twin(3, [16, 32], 32 * 2 * 8 * 16, 7)
    assert list(ours.state_dict()) == list(ref.state_dict()) == ["in_layer.weight", "in_layer.bias", "hidden_layers.0.weight", "hidden_layers.0.bias",
                                                                  "out_layer.weight", "out_layer.bias"]
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    missing, unexpected = ours.load_state_dict(ref.state_dict())
    assert not missing and not unexpected and all(p.requires_grad for p in ours.parameters())
    with torch.device("meta"):                                                  # the default geometry: 130 M weights, never materialised here
        big = VisualClassification({"input_dim": 3, "output_dim": 7, "hidden_layers": "32,32"})
    assert big.out_layer.in_features == 18585600 == 32 * 12 * 220 * 220 and big.clip_shape == (16, 224, 224)
    for form in ("16,32", [16, 32], (16, 32)):
        assert VisualClassification({"input_dim": 3, "output_dim": 2, "hidden_layers": form, "clip_shape": (6, 12, 20)}).hidden_dim == [16, 32]
    with pytest.raises(ValueError, match="leave nothing"):
        VisualClassification({"input_dim": 3, "output_dim": 2, "hidden_layers": "8,8", "clip_shape": (4, 12, 20)})
    with pytest.raises(RuntimeError, match="GPU"):
        ours(torch.zeros(1, 1, 3, 6, 12, 20))
    with pytest.raises(RuntimeError, match="hub"):
        ResNet50Classification({"input_dim": 3, "output_dim": 7, "hidden_layers": [32]})


def test_cli_parses_and_fp8_is_refused():
    from tav_amd import engine as E
    from tav_amd.SingleModels import visual_nn as V
    a = V.parse_args(["--hidden_layers", "32,32", "--batch_size", "8", "--epoch", "1", "--synthetic", "16"])
    assert (a.clip_shape, a.hidden_layers, a.batch_size, a.epoch, a.synthetic, a.clip) == ((16, 224, 224), "32,32", 8, 1, 16, 1.0)
    a = V.parse_args(["--clip-shape", "6,12,20", "--clip", "0.5", "--model", "Video"])
    assert a.clip_shape == (6, 12, 20) and a.clip == 0.5 and a.model == "Video"
    with pytest.raises(SystemExit):
        V.parse_args(["--clip-shape", "6,12"])
    ds = V.SyntheticClips(4, (6, 12, 20), 7, 1)
    frames, label = ds[2]
    assert len(ds) == 4 and frames.dtype == torch.uint8 and tuple(frames.shape) == (8, 13, 22, 3) and 0 <= label < 7 and torch.equal(ds[2][0], frames)
    root = os.path.join(ROOT, "SingleModels", "visual_nn.py")
    assert "tav_amd.SingleModels.visual_nn" in open(root).read()
    ectx = E.Ctx("fp8")
    w = torch.nn.Parameter(torch.zeros(16, 3, 3, 3, 3))
    with pytest.raises(ValueError, match="bf16 and fp32"):
        E.Conv3dGeluFn.apply(torch.zeros(1, 3, 3, 3, 16), w, None, ectx)
    with pytest.raises(ValueError, match="bf16 and fp32"):
        E.FlatLinearSigmoidFn.apply(torch.zeros(1, 1, 1, 1, 16), torch.zeros(2, 16), None, 16, ectx)
