"""GPU: tav_soft_f_loss (csrc/loss.hip) against its fp64 twin with per-element bounds (tests/soft_f_ref.py), under the guard-band allocator
(tests/guarded.py); non-finite logits; engine.SoftFLossFn under autograd; FBetaLoss through the training loop, eager against captured
graphs and sync="step" against sync="log", bit for bit; the tav_nn entry point with --loss FBeta.

Every named case runs once with all three outputs, once loss-only and once gradient-only; the variants (grad_scale 1, 1/8, 3; a logits row
pitch of C + 3; the class-weight vector) rotate over the cases of a group so that every combination occurs in every group."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset

import guarded
import soft_f_ref as R
import tav_amd  # noqa: F401
from tav_amd import config as C
from tav_amd import engine as E
from tav_amd import ops, runtime, synthetic
from tav_amd.models.tav import PreFormer, TAVForMAE
from tav_amd.train_model import tav_train as T
from tav_amd.utils.global_functions import FBetaLoss, Metrics

pytestmark = pytest.mark.gpu
GRAD_SCALES = (1.0, 0.125, 3.0)
WORST = {"loss": 0.0, "dlogits": 0.0, "stats": 0.0}


def _variant(i):
    """(grad_scale, weighted, pitch_extra) of the i-th case of a group: all 12 combinations in every 12 consecutive cases."""
    return GRAD_SCALES[i % 3], bool((i // 3) % 2), 3 if (i // 6) % 2 else 0


def _run(z, t, w, beta, mode, grad_scale, pitch):
    """The full call, the loss-only call and the gradient-only call under guard -> dict of host arrays; asserts that the partial calls
    give the full call's bits."""
    with guarded.active() as g:
        zd = guarded.guarded_input(z.cuda(), pitch_extra=pitch)
        td = guarded.guarded_input(t.cuda())
        wd = None if w is None else guarded.guarded_input(w.cuda())
        assert zd.stride(0) == z.shape[1] + pitch or z.shape[0] == 1
        stats = g.empty(3, z.shape[1], dtype=torch.float32, device="cuda")
        loss, dl = ops.soft_f_loss(zd, td, wd, beta, mode, grad_scale=grad_scale, stats=stats)
        loss_only, none_g = ops.soft_f_loss(zd, td, wd, beta, mode, grad_scale=grad_scale, want_grad=False)
        none_l, grad_only = ops.soft_f_loss(zd, td, wd, beta, mode, grad_scale=grad_scale, want_loss=False)
        g.verify()
        assert none_g is None and none_l is None
        assert torch.equal(loss_only, loss) or (torch.isnan(loss).all() and torch.isnan(loss_only).all())
        assert torch.equal(grad_only.view(torch.int32), dl.view(torch.int32))
        return dict(loss=loss.cpu().numpy().astype(np.float64), dlogits=dl.cpu().numpy().astype(np.float64), stats=stats.cpu().numpy().astype(np.float64))


def _check(got, ref, what):
    for fam in WORST:
        r = R.ratio(got[fam], ref[fam], ref[fam + "_b"])
        WORST[fam] = max(WORST[fam], r)
        assert r <= 1.0, f"{what}: {fam} error / bound = {r:.3f}"


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("Cn", R.CS)
def test_named_cases_against_the_twin_per_element(gpu, Cn, mode):
    group = [c for c in R.NAMED if c[1] == Cn and c[3] == mode]
    assert len(group) == 144 and {_variant(i) for i in range(len(group))} == {(s, w, p) for s in GRAD_SCALES for w in (False, True) for p in (0, 3)}
    for i, (B, _, beta, _, scale, seed) in enumerate(group):
        gs, weighted, pitch = _variant(i)
        z, t = R.named_inputs(B, Cn, scale, seed)
        ref = R.named_reference(B, Cn, beta, mode, scale, seed, weighted, gs)
        got = _run(z, t, R.class_weights(Cn) if weighted else None, beta, mode, gs, pitch)
        _check(got, ref, f"B {B} C {Cn} beta {beta} {mode} x{scale} seed {seed} grad_scale {gs} weighted {weighted} pitch +{pitch}")
    print(f"soft_f worst error / bound after C {Cn} {mode}: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


@pytest.mark.parametrize("name", R.EXACT_INPUTS)
def test_exact_cases_against_the_twin_per_element(gpu, name):
    z, t = R.exact_inputs(name)
    Cn = z.shape[1]
    for i, (_, beta, mode) in enumerate(c for c in R.EXACT if c[0] == name):
        for j in range(2):
            gs, weighted, pitch = _variant(2 * i + j)
            ref = R.exact_reference(name, beta, mode, weighted, gs)
            got = _run(z, t, R.class_weights(Cn) if weighted else None, beta, mode, gs, pitch)
            _check(got, ref, f"{name} beta {beta} {mode} grad_scale {gs} weighted {weighted} pitch +{pitch}")
            clamped = ref["branch"] != 0
            if name == "saturated":                          # every class clamped: the gradient is exactly 0 and the sums are the integers
                assert clamped.all() and not got["dlogits"].any()
                assert np.array_equal(got["stats"], [[8, 8, 8, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
            if name == "absent_p0":                          # p = 0 exactly in the absent class: its column of dlogits is exactly 0
                assert clamped[2] and not got["dlogits"][:, 2].any() and got["stats"][0, 2] == 0 and got["stats"][1, 2] == 0
            if name == "out_of_range":                       # rows 0 and 2 belong to no class: tp + fn counts the four rows that do
                assert np.abs((got["stats"][0] + got["stats"][2]).sum() - 4.0) < 1e-5 and np.abs(got["stats"][:2].sum() - 6.0) < 1e-5
    print("soft_f worst error / bound after the exact cases: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


def test_two_runs_are_bitwise_equal(gpu):
    for B, Cn in ((257, 7), (1000, 16), (3, 2)):
        z, t = R.named_inputs(B, Cn, 3.0, 1)
        zd, td, wd = z.cuda(), t.cuda(), R.class_weights(Cn).cuda()
        runs = []
        for _ in range(3):
            stats = torch.empty(3, Cn, device="cuda")
            loss, dl = ops.soft_f_loss(zd, td, wd, 0.5, "FBeta", stats=stats)
            runs.append(torch.cat([loss, dl.reshape(-1), stats.reshape(-1)]).view(torch.int32).clone())
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("B", [3, 257])
def test_non_finite_logits_are_not_laundered(gpu, B):
    Cn = 7
    z0, t = R.named_inputs(B, Cn, 1.0, 0)
    row = 1
    on, off = int(t[row]), (int(t[row]) + 1) % Cn
    for mode in R.MODES:
        for val in (float("nan"), float("inf")):
            for col in (on, off):
                z = z0.clone()
                z[row, col] = val
                got = _run(z, t, None, 1.0, mode, 1.0, 0)
                assert np.isnan(got["loss"]).all(), (mode, val, col)
                assert not np.isfinite(got["dlogits"]).any(), (mode, val, col)
        z = z0.clone()
        z[row, off] = float("-inf")                          # a legal logit: p = 0 there
        ref = R.reference(z, t, None, 1.0, mode)
        got = _run(z, t, None, 1.0, mode, 1.0, 3)
        _check(got, ref, f"-Inf off the target, B {B} {mode}")
        assert np.isfinite(got["dlogits"]).all() and got["dlogits"][row, off] == 0
        z[row, :] = float("-inf")                            # the whole row: no probabilities to speak of
        got = _run(z, t, None, 1.0, mode, 1.0, 0)
        assert np.isnan(got["loss"]).all() and not np.isfinite(got["dlogits"]).any()


def test_debug_checks_refuse_a_target_outside_the_classes(gpu, monkeypatch):
    z, t = R.exact_inputs("out_of_range")
    loss, _ = ops.soft_f_loss(z.cuda(), t.cuda(), None, 1.0, "FBeta")
    assert torch.isfinite(loss).all()
    monkeypatch.setattr(ops, "_DEBUG_CHECKS", True)
    with pytest.raises(ValueError, match="outside"):
        ops.soft_f_loss(z.cuda(), t.cuda(), None, 1.0, "FBeta")


@pytest.mark.parametrize("mode", R.MODES)
def test_autograd_function_scales_the_twins_gradient(gpu, mode):
    B, Cn, beta = 65, 7, 2.0
    z, t = R.named_inputs(B, Cn, 1.0, 2)
    ref = R.named_reference(B, Cn, beta, mode, 1.0, 2, True, 1.0)
    zd = z.cuda().requires_grad_(True)
    loss = E.SoftFLossFn.apply(zd, t.cuda(), R.class_weights(Cn).cuda(), beta, mode, 1e-7)
    assert loss.shape == () and R.ratio(loss.detach().cpu().numpy().reshape(1), ref["loss"], ref["loss_b"]) <= 1.0
    (loss * 0.25).backward()
    want = 0.25 * ref["dlogits"]
    assert R.ratio(zd.grad.cpu().numpy(), want, 0.25 * ref["dlogits_b"] + R.U * np.abs(want)) <= 1.0       # (one more product, by a power of two)
    crit = FBetaLoss(Cn, beta=beta, weights=R.class_weights(Cn)) if mode == "FBeta" else None
    if crit is not None:
        assert torch.equal(crit(z.cuda(), t.cuda(), epoch=3), loss.detach()) and crit.weights.is_cuda


# ---------------------------------------------------------------------------------------------- through the loop
ARGS = dict(output_dim=7, dropout=0.5, learn_PosEmbeddings=True, num_layers=12)
_LOG = T.log
_RUNS = {}


class _Dialogues(Dataset):
    """Pre-collated batches plus the reference data loader's dialogue bookkeeping (retGradAccum -> (dialogue length, running end))."""

    def __init__(self, cfg, sizes, dialogues, seed):
        self.items = [synthetic.make_batch(cfg, b, seed=seed + i, s_text=16, t_audio=8000, n_visual_true=4) for i, b in enumerate(sizes)]
        self.grad, self.grad_sum, self.ctr = list(dialogues), [int(v) for v in np.cumsum(dialogues)], 0

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]

    def retGradAccum(self, i):
        r, s = self.grad[self.ctr], self.grad_sum[self.ctr]
        if i + 1 == self.grad_sum[self.ctr]:
            self.ctr += 1
        if self.ctr == len(self.grad):
            self.ctr = 0
        return r, s


def _train(graphs, sync):
    """Preset B-tiny, FBetaLoss(7, beta = 0.5), four training steps an epoch (batches of 2 in dialogues of 2), two epochs with
    epoch_switch = 2: one through each accumulation mode.  -> the logged losses and the parameters the run leaves (cached per mode)."""
    if (graphs, sync) in _RUNS:
        return _RUNS[(graphs, sync)]
    runtime.set_precision("bf16")
    cfg = C.preset("B-tiny")
    cfg["audio"]["mask_time_prob"] = 0.0           # SpecAugment off: torch's Philox stream differs between eager calls and replays
    torch.manual_seed(0)
    pre, model = PreFormer(cfg), TAVForMAE(ARGS, cfg)
    synthetic.seeded_init_(pre, 1)
    synthetic.seeded_init_(model, 2)
    pre.cuda()
    model.cuda()
    train = DataLoader(_Dialogues(cfg, [2, 2, 2, 2], [2, 2], 100), batch_size=None)
    val = DataLoader(_Dialogues(cfg, [2], [1], 200), batch_size=None)
    crit = FBetaLoss(7, beta=0.5)
    logged = []
    T.log = lambda M, loss, check="train": (logged.append((check, loss)), _LOG(M, loss, check))
    T.PATIENCE_ITER = 0
    try:
        T.train_tav_network(model, pre, train, val, crit, 1e-4, 2, 1e-4, 2, Metrics(7, rank="cuda", on_device=(sync == "log")), 10, 1.0, 2, path=None,
                            log_val=3, graphs=graphs, sync=sync)
        torch.cuda.synchronize()
    finally:
        T.log = _LOG
    _RUNS[(graphs, sync)] = dict(logged=logged, params=[p.detach().clone() for p in list(model.parameters()) + list(pre.parameters())])
    return _RUNS[(graphs, sync)]


def _same_run(a, b):
    assert len(a["logged"]) == len(b["logged"]) >= 2 and all(np.isfinite(v) for _, v in a["logged"])
    assert a["logged"] == b["logged"], (a["logged"], b["logged"])
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))


def test_captured_graphs_equal_eager_through_the_loop(gpu):
    eager, graphed = _train(False, "step"), _train(True, "step")
    _same_run(eager, graphed)
    start = _fresh_parameters()
    assert any(not torch.equal(x.cpu(), y) for x, y in zip(eager["params"], start)), "the loss moved no parameter"


def test_log_sync_equals_step_sync_through_the_loop(gpu):
    _same_run(_train(False, "step"), _train(False, "log"))


def _fresh_parameters():
    cfg = C.preset("B-tiny")
    torch.manual_seed(0)
    pre, model = PreFormer(cfg), TAVForMAE(ARGS, cfg)
    synthetic.seeded_init_(pre, 1)
    synthetic.seeded_init_(model, 2)
    return [p.detach().clone() for p in list(model.parameters()) + list(pre.parameters())]


# ---------------------------------------------------------------------------------------------- entry point
def test_tav_nn_trains_with_the_f_beta_loss(gpu, capsys, monkeypatch):
    import tav_amd.tav_nn as tav_nn
    calls = []
    real = ops.soft_f_loss

    def rec(logits, target, weight, beta, mode, *a, **k):
        out = real(logits, target, weight, beta, mode, *a, **k)
        calls.append((logits.detach().float().cpu().clone(), target.cpu().clone(), weight, beta, mode, out[0].detach().cpu().clone()))
        return out
    monkeypatch.setattr(ops, "soft_f_loss", rec)
    try:
        tav_nn.main(["--preset", "B-tiny", "--epoch", "1", "--batch_size", "2", "--synthetic", "8", "--dtype", "bf16", "--loss", "FBeta", "--beta", "0.5"])
    finally:
        C.set_default_preset("A")
    out = capsys.readouterr().out
    assert "nan" not in out.lower() and "in train" in out and "in val" in out
    assert len(calls) >= 4 and all(c[2] is None and c[3] == 0.5 and c[4] == "FBeta" for c in calls)
    z, t, _, _, _, loss = calls[0]
    ref = R.reference(z, t, None, 0.5, "FBeta")
    assert np.isfinite(loss.numpy()).all() and R.ratio(loss.numpy().astype(np.float64), ref["loss"], ref["loss_b"]) <= 1.0
    ce = torch.nn.functional.cross_entropy(z.double(), t).item()
    assert abs(float(loss) - ce) > 1e-3, "the first step's loss is the cross entropy's"
