"""CPU: the numpy reference of tav_step_stats against torch.argmax and the host Metrics' bincount, the new symbol in the header and the binding
(ABI still 7), its argument checks (error codes before anything is launched), and what the on-device forms do without a GPU tensor."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import step_stats_ref as R
import tav_amd  # noqa: F401
from tav_amd import _lib, ops
from tav_amd.train_model import tav_train as T
from tav_amd.utils.global_functions import Metrics, arg_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("Cn", R.CLASSES)
def test_reference_argmax_is_torch_argmax(Cn):
    sp = R.special_rows(Cn)
    assert torch.equal(torch.from_numpy(R.argmax_rows(sp)), torch.argmax(torch.from_numpy(sp), dim=1))
    if Cn >= 7:
        # all equal -> 0; repeated maximum -> its first place; last column; -inf everywhere -> 0; +inf; the NaN beats the +inf; the first NaN
        assert R.argmax_rows(sp).tolist() == [0, Cn // 3, Cn - 1, 0, Cn // 2, Cn - 1, Cn // 2]
    for B in R.BATCHES:
        logits, _ = R.make_case(B, Cn)
        assert torch.equal(torch.from_numpy(R.argmax_rows(logits)), torch.argmax(torch.from_numpy(logits), dim=1)), (B, Cn)


@pytest.mark.parametrize("Cn", R.CLASSES)
def test_reference_matrix_is_the_host_metrics_bincount(Cn):
    for B in (7, 257, 1000):
        logits, target = R.make_case(B, Cn)
        ok = (target >= 0) & (target < Cn)
        cm = np.zeros((Cn, Cn), np.int64)
        acc = R.new_acc()
        R.step(Cn, target, logits=logits, cm=cm, acc=acc)
        m = Metrics(Cn)
        m.update_from_logits(torch.from_numpy(logits[ok]), torch.from_numpy(target[ok]))
        assert torch.equal(torch.from_numpy(cm), m.cm)
        assert acc["bad_rows"] == int((~ok).sum()) and acc["rows"] == B and cm.sum() == int(ok.sum())
        cm2 = np.zeros((Cn, Cn), np.int64)
        R.step(Cn, target, preds=R.argmax_rows(logits), cm=cm2)
        assert np.array_equal(cm, cm2)


def test_reference_accumulator_sums_in_double_and_keeps_the_first_bad_step():
    acc = R.new_acc()
    losses = [1e8, 1.0, 1.0, -1e8, 0.1]
    for v, w in zip(losses, [0, 0, 4, 0, 2]):
        R.step(2, [0, 1], preds=[0, 5], loss=np.float32(v), status=w, acc=acc)
    want = 0.0
    f32 = np.float32(0.0)
    for v in losses:
        want += float(np.float32(v))
        f32 = np.float32(f32 + np.float32(v))
    assert acc["loss_sum"] == want and want != float(f32)               # (a float32 running sum loses the two 1.0)
    assert (acc["steps"], acc["rows"], acc["bad_rows"], acc["status"], acc["first_bad_step"], acc["nonfinite"]) == (5, 10, 5, 6, 2, 0)
    R.step(2, [0], preds=[0], loss=np.float32("nan"), acc=acc)
    assert acc["nonfinite"] == 1 and np.isnan(acc["loss_sum"])


def test_symbol_is_declared_bound_and_abi_stays_7():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tavhip.h")).read(), flags=re.S)
    assert re.search(r"\btav_step_stats\s*\(", src) and "tav_loop_acc" in src
    assert "tav_step_stats" in _lib.declared_symbols()
    h = _lib.lib()
    assert hasattr(h, "tav_step_stats")
    assert _lib.ABI_VERSION == 7 and h.tav_version() == 7
    assert ops.LOOP_ACC_WORDS * 8 == 64


def test_argument_checks_return_error_codes_before_any_launch():
    h = _lib.lib()
    p = 0x1000                                                   # never dereferenced: every call below is rejected on the host
    NULL, SHAPE = -1, -2
    call = h.tav_step_stats
    assert call(p, None, None, p, None, None, p, 4, 7, None) == NULL            # no target
    assert call(None, None, p, p, None, None, p, 4, 7, None) == NULL            # neither logits nor preds
    assert call(p, p, p, p, None, None, p, 4, 7, None) == NULL                  # both
    assert call(p, None, p, None, p, p, None, 4, 7, None) == NULL               # neither cm nor acc
    for B, Cn in [(0, 7), (-1, 7), (1 << 31, 7), (4, 0), (4, 65), (4, -3)]:
        assert call(p, None, p, p, None, None, p, B, Cn, None) == SHAPE, (B, Cn)
        assert call(None, p, p, None, None, None, p, B, Cn, None) == SHAPE, (B, Cn)
    assert h.tav_error_string(SHAPE).decode() == "unsupported shape"


def test_on_device_forms_refuse_host_tensors():
    """The counting kernel has no host form: Metrics(on_device=True) on a CPU device and ops.step_stats on CPU tensors raise ValueError
    that says so, the default Metrics is the host class, and sync="log" refuses a host-resident Metrics."""
    with pytest.raises(ValueError, match="on_device=True.*GPU"):
        Metrics(7, rank="cpu", on_device=True)
    m = Metrics(7, rank="cpu")
    assert m.on_device is False and m.cm.device.type == "cpu"
    with pytest.raises(ValueError, match="on the GPU"):
        ops.step_stats(preds=torch.zeros(3, dtype=torch.long), target=torch.zeros(3, dtype=torch.long), cm=m.cm)
    with pytest.raises(ValueError, match="target is required"):
        ops.step_stats(preds=torch.zeros(3, dtype=torch.long), cm=m.cm)
    with pytest.raises(ValueError, match="on_device=True"):
        T.LogSync(m)
    with pytest.raises(ValueError, match="on_device=True"):
        T.train_tav_network(None, None, [], [], None, 1e-6, 1, 1e-4, 2, m, 10, 1.0, 2, sync="log")
    with pytest.raises(ValueError, match="sync must be"):
        T.train_tav_network(None, None, [], [], None, 1e-6, 1, 1e-4, 2, m, 10, 1.0, 2, sync="epoch")
    assert arg_parse("TAV", []).loop_sync == "step" and arg_parse("TAV", ["--loop-sync", "log"]).loop_sync == "log"
