"""-m gpu: tav_step_stats (ops.step_stats, the loop accumulator, Metrics(on_device=True)) against the numpy reference of
tests/step_stats_ref.py.  Every comparison is exact.  Every test runs inside the guard-band allocator (tests/guarded.py): operands sit in
watched buffers that verify() compares bit for bit, the confusion matrix and the accumulator sit between 0xFF bands that must stay 0xFF."""
import functools

import numpy as np
import pytest
import torch

import guarded
import step_stats_ref as R
import tav_amd  # noqa: F401
from tav_amd import ops
from tav_amd.utils.global_functions import Metrics

pytestmark = pytest.mark.gpu


def under_guard(fn):
    @functools.wraps(fn)
    def run(*args, **kw):
        with guarded.active() as g:
            fn(*args, **kw)
            assert g.allocs
            g.verify()
    return run


def _in(a):
    """A numpy array as a watched device operand."""
    return guarded.guarded_input(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def _cm(Cn, fill=None):
    """An int64 [C, C] matrix between guard bands (in-out: not a watched operand)."""
    cm = guarded.current().zeros(Cn, Cn, dtype=torch.int64, device="cuda")
    if fill is not None:
        cm.copy_(torch.from_numpy(fill))
    return cm


def _scalar(v, dtype):
    return guarded.guarded_input(torch.tensor([v], dtype=dtype).cuda())


def _same_acc(got, want):
    assert set(got) == set(want)
    for k in want:
        if k == "loss_sum" and np.isnan(want[k]):
            assert np.isnan(got[k])
        else:
            assert got[k] == want[k] and type(got[k]) is type(want[k]), (k, got[k], want[k])


@pytest.mark.parametrize("Cn", R.CLASSES)
@pytest.mark.parametrize("B", R.BATCHES)
@under_guard
def test_logits_and_preds_forms_equal_the_reference(gpu, B, Cn):
    """Both forms into a matrix that starts with 2^31 + 5 in one bin (the add carries past 32 bits) and into one accumulator: special rows
    (all equal, repeated maximum, last column, -inf, +inf, one and two NaNs), targets -1 and C, the given preds out of range as well."""
    logits, target = R.make_case(B, Cn)
    preds = R.argmax_rows(logits)
    preds[1::13] = -1
    preds[2::13] = Cn
    start = np.zeros((Cn, Cn), np.int64)
    start[Cn - 1, Cn // 2] = (1 << 31) + 5
    want_cm, want_acc = start.copy(), R.new_acc()
    R.step(Cn, target, logits=logits, cm=want_cm, loss=np.float32(0.625), status=0, acc=want_acc)
    R.step(Cn, target, preds=preds, cm=want_cm, loss=np.float32(1.5), status=0, acc=want_acc)
    cm, acc = _cm(Cn, start), ops.loop_acc_new("cuda")
    t = _in(target)
    ops.step_stats(logits=_in(logits), target=t, cm=cm, loss=_scalar(0.625, torch.float32), status=_scalar(0, torch.int32), acc=acc)
    ops.step_stats(preds=_in(preds), target=t, cm=cm, loss=_scalar(1.5, torch.float32), status=_scalar(0, torch.int32), acc=acc)
    assert torch.equal(cm.cpu(), torch.from_numpy(want_cm))
    _same_acc(ops.loop_acc_read(acc), want_acc)
    assert want_acc["rows"] == 2 * B and int(want_cm.sum()) - int(start.sum()) + want_acc["bad_rows"] == 2 * B


@pytest.mark.parametrize("Cn", R.CLASSES)
@under_guard
def test_special_rows_pick_torch_argmax(gpu, Cn):
    """The seven special rows alone, target = row index modulo C: the matrix equals the one built from torch.argmax on the device."""
    sp = R.special_rows(Cn)
    target = np.arange(len(sp), dtype=np.int64) % Cn
    cm = _cm(Cn)
    z = _in(sp)
    ops.step_stats(logits=z, target=_in(target), cm=cm)
    pred = torch.argmax(z, dim=1).cpu()
    assert torch.equal(pred, torch.from_numpy(R.argmax_rows(sp)))
    want = torch.zeros(Cn, Cn, dtype=torch.int64)
    want.index_put_((torch.from_numpy(target), pred), torch.ones(len(sp), dtype=torch.int64), accumulate=True)
    assert torch.equal(cm.cpu(), want)


@under_guard
def test_five_calls_sum_in_double_and_keep_the_first_bad_step(gpu):
    """Five calls into one matrix and one accumulator.  Losses 1e8, 1, 1, -1e8, 0.1: a float32 running sum gives 0.1f, the accumulator
    Python's sum of the same floats.  Status words 0, 0, 4, 0, 2 -> status 6, first_bad_step 2.  A sixth call with a NaN loss counts in
    nonfinite.  loop_acc_reset() then returns the accumulator to its initial state without a host read."""
    Cn, losses, words = 7, [1e8, 1.0, 1.0, -1e8, 0.1], [0, 0, 4, 0, 2]
    cm, acc = _cm(Cn), ops.loop_acc_new("cuda")
    want_cm, want_acc, py_sum = np.zeros((Cn, Cn), np.int64), R.new_acc(), 0.0
    for i, (v, w) in enumerate(zip(losses, words)):
        logits, target = R.make_case(65 + i, Cn, seed=i)
        ops.step_stats(logits=_in(logits), target=_in(target), cm=cm, loss=_scalar(v, torch.float32), status=_scalar(w, torch.int32), acc=acc)
        R.step(Cn, target, logits=logits, cm=want_cm, loss=np.float32(v), status=w, acc=want_acc)
        py_sum += torch.tensor(v, dtype=torch.float32).item()
    got = ops.loop_acc_read(acc)
    _same_acc(got, want_acc)
    assert got["loss_sum"] == py_sum and got["loss_sum"] != float(np.float32(0.1))
    assert (got["steps"], got["status"], got["first_bad_step"], got["nonfinite"]) == (5, 6, 2, 0)
    assert torch.equal(cm.cpu(), torch.from_numpy(want_cm))
    logits, target = R.make_case(3, Cn)
    ops.step_stats(logits=_in(logits), target=_in(target), loss=_scalar(float("nan"), torch.float32), acc=acc)
    R.step(Cn, target, logits=logits, loss=np.float32("nan"), acc=want_acc)
    got = ops.loop_acc_read(acc)
    _same_acc(got, want_acc)
    assert got["nonfinite"] == 1 and got["steps"] == 6 and np.isnan(got["loss_sum"])
    ops.loop_acc_reset(acc)
    _same_acc(ops.loop_acc_read(acc), R.new_acc())


@pytest.mark.parametrize("inf", [float("inf"), float("-inf")])
@under_guard
def test_infinite_loss_counts_as_nonfinite(gpu, inf):
    acc = ops.loop_acc_new("cuda")
    ops.step_stats(preds=_in(np.array([0], np.int64)), target=_in(np.array([0], np.int64)), loss=_scalar(inf, torch.float32), acc=acc, num_classes=1)
    got = ops.loop_acc_read(acc)
    assert got["nonfinite"] == 1 and got["loss_sum"] == inf and got["bad_rows"] == 0 and got["rows"] == 1


@under_guard
def test_matrix_alone_and_accumulator_alone(gpu):
    """cm=None leaves a matrix that was not passed untouched and still counts the out-of-range rows; acc=None leaves the accumulator
    untouched and still fills the matrix; without loss / status the accumulator's sum and status do not move."""
    Cn, B = 7, 257
    logits, target = R.make_case(B, Cn)
    cm, acc = _cm(Cn), ops.loop_acc_new("cuda")
    cm0, acc0 = cm.clone(), acc.clone()
    z, t = _in(logits), _in(target)
    ops.step_stats(logits=z, target=t, cm=cm)
    want_cm = np.zeros((Cn, Cn), np.int64)
    R.step(Cn, target, logits=logits, cm=want_cm)
    assert torch.equal(acc, acc0) and torch.equal(cm.cpu(), torch.from_numpy(want_cm))
    cm1 = cm.clone()
    ops.step_stats(logits=z, target=t, acc=acc)
    want_acc = R.new_acc()
    R.step(Cn, target, logits=logits, acc=want_acc)
    assert torch.equal(cm, cm1) and not torch.equal(cm, cm0)
    _same_acc(ops.loop_acc_read(acc), want_acc)
    assert want_acc["bad_rows"] > 0 and want_acc["loss_sum"] == 0.0 and want_acc["first_bad_step"] == -1
    with pytest.raises(RuntimeError, match="step_stats"):
        ops.step_stats(logits=z, target=t)                        # neither: TAV_ERR_NULL from the library
    with pytest.raises(RuntimeError, match="step_stats"):
        ops.step_stats(logits=z, preds=t, target=t, cm=cm)        # both forms


@under_guard
def test_on_device_metrics_equal_the_host_class(gpu):
    """Metrics(on_device=True): update_from_logits and update_metrics count what the host class counts for in-range rows, compute_scores
    returns the host class's ten values, reset_metrics zeroes on the device."""
    Cn = 7
    dev_m, host_m = Metrics(Cn, rank="cuda", on_device=True), Metrics(Cn)
    assert dev_m.cm.is_cuda and dev_m.on_device
    for B in (2, 65, 1000):
        logits, target = R.make_case(B, Cn)
        ok = (target >= 0) & (target < Cn)
        z, t = torch.from_numpy(logits[ok]), torch.from_numpy(target[ok])
        td = guarded.guarded_input(t.cuda())
        dev_m.update_from_logits(guarded.guarded_input(z.cuda()), td)
        host_m.update_from_logits(z, t)
        p = torch.argmax(z, dim=1)
        dev_m.update_metrics(guarded.guarded_input(p.cuda()), td)
        host_m.update_metrics(p, t)
    assert torch.equal(dev_m.cm.cpu(), host_m.cm)
    a, b = dev_m.compute_scores("val"), host_m.compute_scores("val")
    assert len(a) == len(b) == 10 and a[:9] == b[:9] and torch.equal(a[9], b[9]) and not a[9].is_cuda
    dev_m.reset_metrics()
    assert dev_m.cm.is_cuda and int(dev_m.cm.abs().sum()) == 0
