"""CPU: the LSTM recurrence's host side.

tests/lstm_ref.py against torch.nn.LSTM in float64 (outputs, final states and every gradient, 1 and 2 layers, with and without initial
states); the mutants of that reference, each caught in both modes by the inputs the GPU tests use; the chained caps; csrc/lstm_plan.h alone
under ASan + UBSan as a program of its own (tests/host_program.py); include/tavhip_rnn.h against its row of _lib.ABIS type by type and
the families kept apart (tests/abi_check.py); argument faults through the built library; and the pieces of LSTMClassifier that need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check
import lstm_ref as R
import tav_amd  # noqa: F401
from host_program import run_alone_under_sanitizers
from tav_amd import _lib

ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_ALIGN = -1, -2, -3, -4


# ---------------------------------------------------------------------------------------------- against torch.nn.LSTM, fp64
def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-300))


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("with_state", [False, True])
def test_reference_equals_torch_lstm_in_float64(layers, with_state):
    torch.manual_seed(3 + layers)
    H, T, B = 20, 7, 3
    m = torch.nn.LSTM(H, H, num_layers=layers, batch_first=True).double()
    x = torch.randn(B, T, H, dtype=torch.float64, requires_grad=True)
    state = None
    if with_state:
        state = (torch.randn(layers, B, H, dtype=torch.float64, requires_grad=True), torch.randn(layers, B, H, dtype=torch.float64, requires_grad=True))
    out, (hT, cT) = m(x, state)
    dout, dh, dc = torch.randn_like(out), torch.randn_like(hT), torch.randn_like(cT)
    ((out * dout).sum() + (hT * dh).sum() + (cT * dc).sum()).backward()
    P = {k: v.detach().numpy() for k, v in m.named_parameters()}
    inp, saved, hs, cs = x.detach().numpy(), [], [], []
    for k in range(layers):
        h0 = state[0][k].detach().numpy() if with_state else None
        c0 = state[1][k].detach().numpy() if with_state else None
        inp, h, c, s = R.layer_forward(inp, P[f"weight_ih_l{k}"], P[f"weight_hh_l{k}"], P[f"bias_ih_l{k}"], P[f"bias_hh_l{k}"], h0, c0)
        saved.append(s), hs.append(h), cs.append(c)
    assert _rel(inp, out.detach().numpy()) < 1e-12 and _rel(np.stack(hs), hT.detach().numpy()) < 1e-12 and _rel(np.stack(cs), cT.detach().numpy()) < 1e-12
    d = dout.numpy()
    for k in range(layers - 1, -1, -1):
        g = R.layer_backward(saved[k], d, dh[k].numpy(), dc[k].numpy())
        for name, key in (("weight_ih", "dW_ih"), ("weight_hh", "dW_hh"), ("bias_ih", "db_ih"), ("bias_hh", "db_hh")):
            assert _rel(g[key], getattr(m, f"{name}_l{k}").grad.numpy()) < 1e-12, (name, k)
        if with_state:
            assert _rel(g["dh0"], state[0].grad[k].numpy()) < 1e-12 and _rel(g["dc0"], state[1].grad[k].numpy()) < 1e-12
        d = g["dx"]
    assert _rel(d, x.grad.numpy()) < 1e-12


# ---------------------------------------------------------------------------------------------- the tester tested
def _both_modes(x, dtype, mut, fk, bk):
    """Forward and backward verdicts of the reference (mutant `mut`) on the stand-in kernel outputs, step-fed and chained."""
    H = x["H"]
    out = {}
    for mode in ("fed", "chained"):
        ff = dict(y=fk["y"], cells=fk["cells"]) if mode == "fed" else None
        fref = R.forward(x["W"], x["b"], x["xp"], x["h0"], x["c0"], dtype, fed=ff, mut=mut, H=H)
        fb = dict(gates=fk["gates"], cells=fk["cells"], dz=bk["dz"], trace=bk["trace"]) if mode == "fed" else None
        bref = R.backward(x["W"], fref, x["dy"], x["dh_T"], x["dc_T"], dtype, fed=fb, mut=mut)
        out[mode] = (R.check_forward(fk, fref, H), R.check_backward(bk, bref, H))
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_clean_reference_accepts_and_every_mutant_is_caught_in_both_modes(dtype):
    # the GPU tests' inputs at a small size: torch scale for the step-fed mode, contracting weights for the chained one; H = 100 has pads
    cases = {"fed": R.inputs(100, 5, 3, dtype, 11, "torch"), "chained": R.inputs(100, 5, 3, dtype, 12, "contract")}
    sims = {k: R.simulate(x["W"], x["b"], x["xp"], x["h0"], x["c0"], x["dy"], x["dh_T"], x["dc_T"], dtype) for k, x in cases.items()}
    for mode, x in cases.items():
        res = _both_modes(x, dtype, 0, *sims[mode])[mode]
        assert R.passed(res[0]) and R.passed(res[1]), (mode, res)
    for mut, name in R.MUTANTS.items():
        for mode, x in cases.items():
            f, b = _both_modes(x, dtype, mut, *sims[mode])[mode]
            assert not (R.passed(f) and R.passed(b)), f"mutant {name} survives the {mode} mode"


def test_chained_bound_stays_under_the_cap():
    for H in (64, 300):
        for dtype in ("f32", "bf16"):
            bound = R.chained_last_h_bound(H, 70, dtype)
            print(f"H {H} {dtype}: propagated bound on h at step 70 = {bound:.3e}")
            assert 0.0 < bound <= R.CHAINED_CAP[dtype]


def test_logsigmoid_reference():
    x = np.array([0.0, 2.0 ** -30, -2.0 ** -30, 100.0, -100.0, 3.5, -3.5])
    y, dx = R.logsigmoid_bounds(x, np.ones_like(x))
    want = torch.nn.functional.logsigmoid(torch.tensor(x, dtype=torch.float64))
    assert np.abs(y.v - want.numpy()).max() < 1e-14 and np.abs(dx.v - torch.sigmoid(torch.tensor(-x)).numpy()).max() < 1e-14
    assert (y.e <= 32 * R.U * (np.abs(y.v) + 1)).all() and (dx.e <= 32 * R.U).all() and (y.e > 0).all()


# ---------------------------------------------------------------------------------------------- lstm_plan.h alone
def test_lstm_plan_header_alone_under_sanitizers(tmp_path):
    run_alone_under_sanitizers("lstm_plan_check.cpp", tmp_path)


# ---------------------------------------------------------------------------------------------- header against binding
def test_rnn_binding_matches_its_header_type_by_type(tmp_path):
    assert len(abi_check.check_binding(abi_check.abi("tavhip_rnn.h"), tmp_path)) == 7


def test_the_other_two_symbol_tables_are_unchanged():
    abi_check.check_families_apart()


# ---------------------------------------------------------------------------------------------- argument faults, nothing launches
def _fwd_args(**kw):
    a = _lib.LstmFwdArgs()
    for f in ("xproj", "w_hh", "y", "workspace"):
        setattr(a, f, 4096)                                   # only tested for NULL-ness and alignment before a fault is found
    a.B, a.T, a.H, a.dtype, a.xp_stride_b, a.xp_stride_t = 5, 70, 300, _lib.TAV_BF16, 70 * 1280, 1280
    a.workspace_bytes = _lib.lib().tav_lstm_ws_bytes(5, 70, 300, _lib.TAV_BF16)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bwd_args(**kw):
    a = _lib.LstmBwdArgs()
    for f in ("dy", "w_hh_t", "workspace", "dz"):
        setattr(a, f, 4096)
    a.B, a.T, a.H, a.dtype = 5, 70, 300, _lib.TAV_F32
    a.dy_stride_b, a.dy_stride_t, a.dz_stride_b, a.dz_stride_t = 320, 5 * 320, 1280, 5 * 1280
    a.workspace_bytes = _lib.lib().tav_lstm_ws_bytes(5, 70, 300, _lib.TAV_F32)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_invalid_arguments_are_refused_before_any_launch():
    h = _lib.lib()
    fwd = lambda **kw: h.tav_lstm_fwd(C.byref(_fwd_args(**kw)), None)          # noqa: E731
    bwd = lambda **kw: h.tav_lstm_bwd(C.byref(_bwd_args(**kw)), None)          # noqa: E731
    assert h.tav_lstm_fwd(None, None) == ERR_NULL and h.tav_lstm_bwd(None, None) == ERR_NULL
    for f in ("xproj", "w_hh", "y", "workspace"):
        assert fwd(**{f: None}) == ERR_NULL, f
    for f in ("dy", "w_hh_t", "workspace", "dz"):
        assert bwd(**{f: None}) == ERR_NULL, f
    assert fwd(dtype=_lib.TAV_FP8) == ERR_DTYPE and fwd(dtype=9) == ERR_DTYPE and bwd(dtype=_lib.TAV_U8) == ERR_DTYPE
    assert fwd(H=1025) == ERR_SHAPE and fwd(H=0) == ERR_SHAPE and fwd(B=0) == ERR_SHAPE and fwd(T=0) == ERR_SHAPE and bwd(H=577) == ERR_SHAPE
    assert fwd(xp_stride_t=1272) == ERR_SHAPE and fwd(workspace_bytes=64) == ERR_SHAPE and bwd(dy_stride_b=312) == ERR_SHAPE
    assert fwd(xp_stride_t=1284) == ERR_ALIGN and fwd(xp_stride_b=70 * 1280 + 4) == ERR_ALIGN and bwd(dz_stride_t=5 * 1280 + 4) == ERR_ALIGN
    assert fwd(h0=4100) == ERR_ALIGN and fwd(xproj=4104) == ERR_ALIGN and bwd(dc_trace=4100) == ERR_ALIGN
    assert fwd(xp_stride_t=1284, H=1025) == ERR_SHAPE and fwd(xp_stride_t=1284, y=None) == ERR_NULL          # pointers, then sizes, then strides
    p = _lib.LstmPlan()
    assert h.tav_lstm_get_plan(5, 70, 300, _lib.TAV_BF16, C.byref(p)) == 0
    assert (p.block, p.rows_per_wg, p.Hp, p.tiles_per_wave) == (640, 16, 320, 2) and p.lds_bytes <= 160 * 1024
    assert p.ws_gates_off == 0 and p.ws_cell_off >= 70 * 5 * 1280 * 4 and p.ws_bytes >= p.ws_cell_off + 71 * 5 * 320 * 4
    assert h.tav_lstm_ws_bytes(5, 70, 300, _lib.TAV_BF16) == p.ws_bytes
    assert h.tav_lstm_get_plan(5, 70, 300, _lib.TAV_BF16, None) == ERR_NULL and h.tav_lstm_get_plan(5, 70, 1025, _lib.TAV_BF16, C.byref(p)) == ERR_SHAPE
    assert h.tav_lstm_get_plan(5, 70, 600, _lib.TAV_F32, C.byref(p)) == ERR_SHAPE and h.tav_lstm_get_plan(5, 70, 600, _lib.TAV_BF16, C.byref(p)) == 0
    assert h.tav_lstm_ws_bytes(5, 70, 300, _lib.TAV_FP8) == ERR_DTYPE and h.tav_lstm_ws_bytes(0, 70, 300, _lib.TAV_F32) == ERR_SHAPE
    ls, lb = h.tav_logsigmoid_fwd, h.tav_logsigmoid_bwd
    assert ls(None, 64, 4, None) == ERR_NULL and ls(64, None, 4, None) == ERR_NULL and ls(64, 64, 0, None) == ERR_SHAPE
    assert lb(None, 64, 64, 4, None) == ERR_NULL and lb(64, None, 64, 4, None) == ERR_NULL and lb(64, 64, None, 4, None) == ERR_NULL and lb(64, 64, 64, -1, None) == ERR_SHAPE


# ---------------------------------------------------------------------------------------------- LSTMClassifier without a GPU
class _Vec:
    def __init__(self, V, E, seed=0):
        self.vectors = torch.randn(V, E, generator=torch.Generator().manual_seed(seed))


def _torch_assembly(V, H, layers, O):
    m = torch.nn.Module()
    m.embedding = torch.nn.Embedding(V, H)
    m.lstm = torch.nn.LSTM(H, H, num_layers=layers, batch_first=True)
    m.fc2 = torch.nn.Linear(H, O)
    return m


def test_classifier_state_dict_is_torchs_and_round_trips():
    from tav_amd.SingleModels.models.text import LSTMClassifier
    for layers in (1, 2):
        ours = LSTMClassifier(_Vec(50, 20), {"output_dim": 7, "hidden_layers": [20, 20], "lstm_layers": layers})
        ref = _torch_assembly(50, 20, layers, 7)
        assert list(ours.state_dict()) == list(ref.state_dict())
        assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        missing, unexpected = ours.load_state_dict(ref.state_dict())
        assert not missing and not unexpected
        for k, v in ref.state_dict().items():
            assert torch.equal(ours.state_dict()[k], v), k
        assert not ours.embedding.weight.requires_grad and all(p.requires_grad for n, p in ours.named_parameters() if not n.startswith("embedding"))
        k = 1.0 / 20 ** 0.5
        fresh = LSTMClassifier(_Vec(50, 20), {"output_dim": 7, "hidden_layers": 20, "lstm_layers": layers})
        assert all(float(p.detach().abs().max()) <= k for n, p in fresh.lstm.named_parameters()) and float(fresh.lstm.weight_hh_l0.detach().abs().max()) > 0.5 * k


def test_classifier_hidden_layers_forms_and_refusals():
    from tav_amd.SingleModels.models.text import LSTMClassifier
    for form in (24, [24], [24, 99], (24,), "24", "24,32"):
        assert LSTMClassifier(_Vec(9, 24), {"output_dim": 3, "hidden_layers": form, "lstm_layers": 1}).hidden_dim == 24
    with pytest.raises(ValueError, match="embedding width"):
        LSTMClassifier(_Vec(9, 20), {"output_dim": 3, "hidden_layers": 24, "lstm_layers": 1})
    m = LSTMClassifier(_Vec(9, 24), {"output_dim": 3, "hidden_layers": 24, "lstm_layers": 1})
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(2, 5, dtype=torch.long))
