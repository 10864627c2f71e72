"""GPU: tav_lstm_fwd / tav_lstm_bwd and tav_logsigmoid_* (csrc/lstm.hip) against their fp64 model with per-element bounds (tests/lstm_ref.py),
structural cases whose answer does not depend on rounding, and LSTMClassifier against torch.nn.LSTM in float64 on the CPU.

The kernel tests run inside the guard-band allocator (tests/guarded.py): the projection and dY sit in watched buffers with a padded row pitch
(0xFF = NaN between the rows), every output is allocated under guard, and verify() reports any store outside a tensor or into an operand.

STEP-FED checks feed every step of the reference the kernel's own previous state, so each bound is a one-step bound; CHAINED checks propagate
the bound through all 70 steps with contracting weights (lstm_ref's docstring)."""
import numpy as np
import pytest
import torch

import guarded
import lstm_ref as R
import tav_amd  # noqa: F401
from tav_amd import ops

pytestmark = pytest.mark.gpu
ROWS = 16                                                     # rows of a workgroup; asserted against the plan below
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _dev(a, dtype="f32"):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(TORCH_DT[dtype]).cuda()


def _host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _forward(x, dtype, state=True, time_major=False):
    """One tav_lstm_fwd under guard (call inside guarded.active()) -> (saved, dict of host arrays y, cells, gates)."""
    xp = _dev(x["xp"] if time_major else x["xp"].transpose(1, 0, 2), dtype)
    xp = guarded.guarded_input(xp, pitch_extra=8)
    assert xp.stride(1) == xp.shape[2] + 8
    W = guarded.guarded_input(_dev(x["W"], dtype))
    b = guarded.guarded_input(_dev(x["b"])) if x["b"] is not None else None
    h0 = guarded.guarded_input(_dev(x["h0"])) if state and x["h0"] is not None else None
    c0 = guarded.guarded_input(_dev(x["c0"])) if state and x["c0"] is not None else None
    s = ops.lstm_fwd(xp, W, b, h0, c0, H=x["H"], time_major=time_major)
    return s, dict(y=_host(s.y), cells=_host(ops.lstm_cells(s)), gates=_host(ops.lstm_gates(s)))


def _backward(x, dtype, s, state=True):
    dy = guarded.guarded_input(_dev(x["dy"].transpose(1, 0, 2), dtype), pitch_extra=8)
    Wt = guarded.guarded_input(_dev(x["W"].T, dtype))
    dh_T = guarded.guarded_input(_dev(x["dh_T"])) if state and x["dh_T"] is not None else None
    dc_T = guarded.guarded_input(_dev(x["dc_T"])) if state and x["dc_T"] is not None else None
    dz, dh0, dc0, trace = ops.lstm_bwd(s, dy, Wt, dh_T, dc_T, want_trace=True)
    return dict(dz=_host(dz), dh0=_host(dh0), dc0=_host(dc0), trace=_host(trace))


def _no_state(x):
    return dict(x, h0=None, c0=None, dh_T=None, dc_T=None)


def _report(tag, *results):
    for res in results:
        print(tag, " ".join(f"{k} {v:.3f}" if not isinstance(v, bool) else f"{k} {v}" for k, v in res.items()))


def test_plan_rows():
    for H in (64, 100, 300):
        for dt in TORCH_DT.values():
            assert ops.lstm_plan(5, 70, H, dt)["rows_per_wg"] == ROWS


@pytest.mark.parametrize("T", [1, 2, 3, 70])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("H", [64, 100, 300])
def test_forward_and_backward_step_fed(gpu, H, dtype, T):
    for B in (1, 5, ROWS, ROWS + 1, 2 * ROWS + 3):
        for state in (True, False):
            x = R.inputs(H, T, B, dtype, 1000 * H + 10 * T + B, "torch")
            if not state:
                x = _no_state(x)
            with guarded.active() as g:
                s, fk = _forward(x, dtype, state)
                bk = _backward(x, dtype, s, state)
                g.verify()
            fref = R.forward(x["W"], x["b"], x["xp"], x["h0"], x["c0"], dtype, fed=fk, H=H)
            bref = R.backward(x["W"], fref, x["dy"], x["dh_T"], x["dc_T"], dtype, fed=dict(fk, **bk))
            rf, rb = R.check_forward(fk, fref, H), R.check_backward(bk, bref, H)
            _report(f"H {H} {dtype} T {T} B {B} state {state}:", rf, rb)
            assert np.isfinite(fk["y"]).all() and np.isfinite(bk["dz"]).all()
            assert R.passed(rf) and R.passed(rb), (B, state, rf, rb)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("H", [64, 300])
def test_chained_against_the_propagated_bound(gpu, H, dtype):
    T, B = 70, 5
    x = R.inputs(H, T, B, dtype, 77 + H, "contract")
    with guarded.active() as g:
        s, fk = _forward(x, dtype)
        bk = _backward(x, dtype, s)
        g.verify()
    fref = R.forward(x["W"], x["b"], x["xp"], x["h0"], x["c0"], dtype, H=H)
    bref = R.backward(x["W"], fref, x["dy"], x["dh_T"], x["dc_T"], dtype)
    rf, rb = R.check_forward(fk, fref, H), R.check_backward(bk, bref, H)
    last = float(fref["h"][-1].e.max())
    _report(f"chained H {H} {dtype} (bound on h_T {last:.2e}):", rf, rb)
    assert last <= R.CHAINED_CAP[dtype]
    assert R.passed(rf) and R.passed(rb), (rf, rb)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_saturated_forget_gate_carries_c0_bit_for_bit(gpu, dtype):
    """z_f = +64 (s is exactly 1.0f), z_i = -64 (i g is below half an ulp of c0), the o rows of W_hh zero and the o, g projections constant in
    time: c_t is c0 bit for bit at every step and h_t = o tanhf(c0) is the same at every t -- whatever the rounding."""
    H, T, B = 100, 9, ROWS + 3
    x = R.inputs(H, T, B, dtype, 5, "torch")
    Hp = R.hp_of(H)
    xp = x["xp"].copy()
    xp[:, :, 0 * Hp:0 * Hp + H] = -64.0
    xp[:, :, 1 * Hp:1 * Hp + H] = 64.0
    xp[:, :, 2 * Hp:] = xp[0:1, :, 2 * Hp:]
    W = x["W"].copy()
    W[3 * Hp:] = 0.0
    rng = np.random.default_rng(9)
    c0 = R.rnd(R.pad_cols(rng.uniform(0.5, 1.5, (B, H)) * rng.choice([-1.0, 1.0], (B, H)), H), "f32")
    x = dict(x, xp=xp, W=W, c0=c0)
    with guarded.active() as g:
        s, fk = _forward(x, dtype)
        g.verify()
    for t in range(T + 1):
        assert np.array_equal(fk["cells"][t], c0), t
    for t in range(1, T + 1):
        assert np.array_equal(fk["y"][t], fk["y"][1]), t
    assert (fk["gates"][:, :, 1, :H] == 1.0).all() and (fk["gates"][:, :, 0, :H] < 1e-24).all()
    fref = R.forward(x["W"], x["b"], x["xp"], x["h0"], x["c0"], dtype, fed=fk, H=H)
    assert R.passed(R.check_forward(fk, fref, H))
    assert np.abs(fk["y"][1][:, :H]).min() > 0.01                           # (a dead output would pass the comparisons above)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_zero_recurrent_weights_every_step_is_a_one_step_launch(gpu, dtype):
    H, T, B = 100, 4, 5
    x = R.inputs(H, T, B, dtype, 6, "torch")
    x = dict(x, W=np.zeros_like(x["W"]))
    with guarded.active() as g:
        s, fk = _forward(x, dtype)
        for t in range(T):
            one = dict(x, xp=x["xp"][t:t + 1], h0=fk["y"][t], c0=fk["cells"][t])
            _, f1 = _forward(one, dtype)
            assert np.array_equal(f1["y"][1], fk["y"][t + 1]) and np.array_equal(f1["cells"][1], fk["cells"][t + 1]), t
            assert np.array_equal(f1["gates"][0], fk["gates"][t]), t
        g.verify()
    assert np.abs(fk["y"][T][:, :H]).max() > 0.05


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rows_do_not_depend_on_their_tile_and_launches_repeat(gpu, dtype):
    H, T, B = 100, 3, 2 * ROWS + 3
    x = R.inputs(H, T, B, dtype, 8, "torch")
    with guarded.active() as g:
        s, fk = _forward(x, dtype)
        bk = _backward(x, dtype, s)
        s2, fk2 = _forward(x, dtype)
        bk2 = _backward(x, dtype, s2)
        for k in fk:
            assert np.array_equal(fk[k], fk2[k]), k
        for k in bk:
            assert np.array_equal(bk[k], bk2[k]), k
        for b in (0, ROWS - 1, ROWS, 2 * ROWS + 2):
            one = {k: (v[:, b:b + 1] if k in ("xp", "dy") else (v[b:b + 1] if k in ("h0", "c0", "dh_T", "dc_T") else v)) for k, v in x.items()}
            s1, f1 = _forward(one, dtype)
            b1 = _backward(one, dtype, s1)
            for k in ("y", "cells", "gates"):
                assert np.array_equal(f1[k][:, 0], fk[k][:, b]), (k, b)
            for k in ("dz", "trace"):
                assert np.array_equal(b1[k][:, 0], bk[k][:, b]), (k, b)
            assert np.array_equal(b1["dh0"][0], bk["dh0"][b]) and np.array_equal(b1["dc0"][0], bk["dc0"][b]), b
        g.verify()


def test_time_major_projection_gives_the_same_bits(gpu):
    x = R.inputs(100, 3, 5, "bf16", 21, "torch")
    with guarded.active() as g:
        _, a = _forward(x, "bf16")
        _, b = _forward(x, "bf16", time_major=True)
        g.verify()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("n", [1, 63, 64, 4097])
def test_logsigmoid_per_element(gpu, n):
    rng = np.random.default_rng(n)
    rest = np.where(np.arange(n) % 2 == 0, rng.uniform(-100, 100, n), rng.standard_normal(n) * 3)
    x = R.rnd(np.concatenate([[0.0, 2.0 ** -30, -2.0 ** -30, 100.0, -100.0, 88.0, -88.0, 104.0], rest])[:n], "f32")
    dy = R.rnd(rng.standard_normal(n) * 2.0 ** rng.integers(-3, 4, n), "f32")
    with guarded.active() as g:
        xd, dyd = guarded.guarded_input(_dev(x)), guarded.guarded_input(_dev(dy))
        y = _host(ops.logsigmoid_fwd(xd))
        dx = _host(ops.logsigmoid_bwd(xd, dyd))
        g.verify()
    wy, wdx = R.logsigmoid_bounds(x, dy)
    print(f"n {n}: worst y {R.worst(y, wy):.3f} dx {R.worst(dx, wdx):.3f}")
    assert R.worst(y, wy) <= 1.0 and R.worst(dx, wdx) <= 1.0


# ---------------------------------------------------------------------------------------------- LstmLayerFn, LSTMClassifier, text_nn
class _Vec:
    def __init__(self, V, E, seed=0):
        self.vectors = torch.randn(V, E, generator=torch.Generator().manual_seed(seed)) * 0.4


def _classifier(H, layers, O=7, V=97, seed=0):
    from tav_amd.SingleModels.models.text import LSTMClassifier
    torch.manual_seed(seed)
    return LSTMClassifier(_Vec(V, H, seed), {"output_dim": O, "hidden_layers": [H], "lstm_layers": layers})


def _torch_reference(model, x, wts):
    """The reference's forward in float64 on the CPU with the model's weights -> (output, {parameter name: gradient})."""
    H, layers = model.hidden_dim, model.LSTM_layers
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    lstm = torch.nn.LSTM(H, H, num_layers=layers, batch_first=True).double()
    lstm.load_state_dict({k[5:]: v for k, v in sd.items() if k.startswith("lstm.")})
    fc = torch.nn.Linear(H, model.output_dim).double()
    fc.load_state_dict({"weight": sd["fc2.weight"], "bias": sd["fc2.bias"]})
    out, _ = lstm(sd["embedding.weight"][x.cpu()])
    out = torch.nn.functional.logsigmoid(fc(out).mean(1))
    (out * wts.double().cpu()).sum().backward()
    grads = {"lstm." + k: p.grad for k, p in lstm.named_parameters()}
    grads.update({"fc2.weight": fc.weight.grad, "fc2.bias": fc.bias.grad})
    return out.detach(), grads


@pytest.mark.parametrize("policy,budget", [("fp32", 1e-3), ("bf16", 1e-2)])
@pytest.mark.parametrize("H,T,layers,B", [(64, 16, 2, 5), (300, 70, 1, 4)])
def test_model_against_torch_in_float64(gpu, H, T, layers, B, policy, budget):
    from tav_amd import runtime
    runtime.set_precision(policy)
    try:
        model = _classifier(H, layers).cuda().eval()
        g = torch.Generator().manual_seed(T)
        x = torch.randint(0, 97, (B, T), generator=g)
        wts = torch.randn(B, 7, generator=g)
        want, wgrads = _torch_reference(model, x, wts)
        out = model(x.cuda())
        (out * wts.cuda()).sum().backward()
        torch.cuda.synchronize()
        err = float((out.detach().double().cpu() - want).abs().max() / want.abs().max())
        print(f"H {H} T {T} layers {layers} B {B} {policy}: logits {err:.3e}")
        worst = {"logits": err}
        for name, p in model.named_parameters():
            if name.startswith("embedding"):
                assert p.grad is None
                continue
            assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, name
            worst[name] = float((p.grad.double().cpu() - wgrads[name]).abs().max() / wgrads[name].abs().max())
            print(f"    {name}: {worst[name]:.3e}")
        assert all(v <= budget for v in worst.values()), worst
    finally:
        runtime.set_precision("bf16")


def test_training_mode_draws_from_the_seed_words(gpu):
    from tav_amd import runtime
    runtime.set_precision("bf16")
    model = _classifier(64, 1).cuda()
    x = torch.randint(0, 97, (4, 12), generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        model.train()
        model._drop_calls = 0
        a = model(x).clone()
        model._drop_calls = 0
        b = model(x).clone()
        c = model(x).clone()
        model.eval()
        e1, e2 = model(x).clone(), model(x).clone()
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all() and torch.isfinite(c).all()
    assert torch.equal(e1, e2) and not torch.equal(e1, a)


def test_captured_forward_and_backward_replays_the_eager_bits(gpu):
    from tav_amd import runtime
    runtime.set_precision("bf16")
    model = _classifier(64, 2).cuda().eval()
    gen = torch.Generator().manual_seed(2)
    x = torch.randint(0, 97, (5, 16), generator=gen).cuda()
    wts = torch.randn(5, 7, generator=gen).cuda()
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        out = model(x)
        (out * wts).sum().backward()
        return out

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            for p in params:
                p.grad = None
            eager = step().detach().clone()
        torch.cuda.synchronize()
        eager_grads = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with runtime.capture(graph, s):
            static_out = step()
        for p in params:
            p.grad.zero_()
        static_out.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out.detach(), eager)
        for p, gexp in zip(params, eager_grads):
            assert torch.equal(p.grad, gexp)


def test_entrypoint_trains_the_lstm_baseline(gpu, capsys, monkeypatch):
    from tav_amd import runtime
    from tav_amd.SingleModels import text_nn
    start = {}

    class Spy(text_nn.LSTMClassifier):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            start.update({k: v.detach().clone() for k, v in self.state_dict().items()})

    monkeypatch.setattr(text_nn, "LSTMClassifier", Spy)
    try:
        model = text_nn.main(["--model", "LSTM", "--hidden_layers", "64", "--lstm_layers", "2", "--synthetic", "32", "--batch_size", "4", "--epoch", "2", "--dtype", "bf16"])
    finally:
        runtime.set_precision("bf16")
    losses = [float(ln.split()[-1]) for ln in capsys.readouterr().out.splitlines() if "loss" in ln]
    assert len(losses) == 4 and all(np.isfinite(losses))
    assert model.LSTM_layers == 2 and model.hidden_dim == 64 and len(start) == 11
    for name, v in model.state_dict().items():
        if name.startswith("embedding"):
            assert torch.equal(v.cpu(), start[name]), name
        else:
            assert not torch.equal(v.cpu(), start[name]), f"{name} has not moved"
