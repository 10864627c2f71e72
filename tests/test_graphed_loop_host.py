"""CPU: graph mode of the training loop (train_model/graphed.py) -- the --graph flag, the device-seed dropout entry point of ABI v7 (argument
validation only: nothing is launched without a GPU), the dropout-seed bookkeeping of runtime under a capture, and the host scheduling of the
graphed loop against stub graphs, stepper and scheduler."""
import ctypes as C

import numpy as np
import pytest
import torch

import tav_amd  # noqa: F401
from tav_amd import _lib, runtime
from tav_amd.train_model import graphed as G
from tav_amd.train_model import tav_train as T
from tav_amd.utils.global_functions import arg_parse


def test_graph_flag_parses():
    assert arg_parse("TAV", ["--graph", "1"]).graph == 1
    assert arg_parse("TAV", []).graph == 0
    with pytest.raises(SystemExit):
        arg_parse("TAV", ["--graph", "2"])


def test_dropout_fwd_dev_is_abi_v7_and_validates_arguments():
    h = _lib.lib()
    assert h.tav_version() == _lib.ABI_VERSION == 7
    assert "tav_dropout_fwd_dev" in _lib.declared_symbols() and hasattr(h, "tav_dropout_fwd_dev")
    f = h.tav_dropout_fwd_dev
    x, y, m, s = (C.c_void_p(4096 * (i + 1)) for i in range(4))          # never dereferenced: every call below is rejected first
    assert f(None, y, m, 8, 0.5, s, 0, None) == -1
    assert f(x, None, m, 8, 0.5, s, 0, None) == -1
    assert f(x, y, None, 8, 0.5, s, 0, None) == -1
    assert f(x, y, m, 8, 0.5, None, 0, None) == -1                        # the seed word is required
    assert f(x, y, m, -3, 0.5, s, 0, None) == -2
    assert f(x, y, m, 0, 0.5, s, 0, None) == -2
    assert f(x, y, m, 8, 1.0, s, 0, None) == -2
    assert f(x, y, m, 8, -0.1, s, 0, None) == -2


def test_dropout_seeds_do_not_advance_under_a_capture():
    """Eager: the counter advances and the seeds are initial_seed + GOLDEN * k.  Under a capture: no advance, the site is recorded with its
    seed words; each advance_seeds() (= before each replay) advances the counter as the eager call would and writes the seeds of those draws."""
    class M:
        _calls = 0
    m = M()
    torch.manual_seed(123)
    want = lambda k: (torch.initial_seed() + 0x9E3779B97F4A7C15 * k) & 0xFFFFFFFFFFFFFFFF     # noqa: E731
    assert runtime.dropout_seeds(m, "_calls", 2) == [want(1), want(2)] and m._calls == 2
    g = runtime.guard_only(object())
    with g:
        words = runtime.dropout_seeds(m, "_calls", 3)
        assert runtime.dropout_seeds(m, "_calls", 1, draw=False) == [0]
    assert m._calls == 2 and len(g.seeds) == 2 and all(w.shape == (1,) and w.dtype == torch.int64 for w in words)
    for r in range(2):
        runtime.advance_seeds(g.seeds)
        base = 2 + r * 4
        assert m._calls == base + 4
        got = [int(np.int64(w.item()).astype(np.uint64)) for w in words]
        assert got == [want(base + 1), want(base + 2), want(base + 3)]        # (the p = 0 site took draw base + 4 without a word)
    assert runtime.dropout_seeds(m, "_calls", 1) == [want(11)]


# ---------------------------------------------------------------------------------------------- the graphed loop against stubs
class _Loss:
    def __init__(self, v, calls):
        self.v, self.calls = v, calls

    def __truediv__(self, d):
        return _Loss(self.v / d, self.calls)

    def item(self):
        return self.v

    def backward(self):
        self.calls.append(("backward", self.v))


class _Opt:
    def __init__(self, calls):
        self.calls, self.lr, self.generation = calls, 0.5, 0

    def sync_lr(self):
        self.calls.append(("lr", self.lr))

    def captures_released(self):
        self.calls.append(("released",))


class _Crit:
    epoch_switch = 2


class _Stepper:
    reducer = None

    def __init__(self, calls):
        self.calls, self.opt, self.criterion, self.model, self.pre = calls, _Opt(calls), _Crit(), None, None

    def update(self, clip=True):
        self.calls.append(("update",) if clip else ("update-unclipped",))


class _Sched:
    def __init__(self, opt, calls):
        self.opt, self.calls = opt, calls

    def step(self, e):
        self.opt.lr = round(0.5 + e, 4)                  # a new learning rate after every batch
        self.calls.append(("sched", round(e, 4)))


class _Metric:
    def __init__(self, calls):
        self.calls = calls

    def update_metrics(self, preds, target):
        self.calls.append(("metrics", preds.tolist(), target.tolist()))


class _Graph:
    def __init__(self, tag, calls):
        self.tag, self.calls = tag, calls
        self.loss, self.logits, self.label = torch.tensor(0.25), torch.tensor([[0.0, 1.0], [3.0, 0.0]]), torch.tensor([1, 1])

    def feed(self, input, label):
        self.calls.append(("feed", self.tag, int(label[0])))

    def set_scale(self, v):
        self.calls.append(("scale", v))

    def replay(self):
        self.calls.append(("replay", self.tag))

    def release(self):
        self.calls.append(("release", self.tag))


def _batch(B, s_text, tag):
    vm = torch.zeros(B, 8, dtype=torch.bool)
    vm[:, :3] = True
    return ([{"input_ids": torch.zeros(B, s_text, dtype=torch.int64), "attention_mask": torch.ones(B, s_text)},
             {"audio_features": torch.zeros(B, 800), "attention_mask": torch.ones(B, 800)},
             {"visual_embeds": torch.zeros(B, 16, 3, 32, 32), "attention_mask": vm}], torch.full((B,), float(tag)))


def _setup(monkeypatch, max_graphs=1):
    calls, logged = [], []
    st = _Stepper(calls)
    gs = G.GraphedSteps(st, max_graphs=max_graphs)
    tags = iter(range(100))

    def capture(self, input, label, epoch, accum, nv):
        t = next(tags)
        calls.append(("capture", t, epoch, accum, nv))
        return _Graph(t, calls)
    monkeypatch.setattr(G.GraphedSteps, "_capture", capture)
    monkeypatch.setattr(T, "get_statistics", lambda input, label, *a, **k: (calls.append(("eager", int(label[0]))), _Loss(6.0, calls))[1])
    monkeypatch.setattr(T, "validate", lambda *a, **k: 0.5)
    monkeypatch.setattr(T, "log", lambda Metric, loss, check="train": logged.append((check, loss)))
    T.PATIENCE_ITER = 0
    return calls, logged, st, gs


def test_graphed_not_grad_accum_schedule(monkeypatch):
    """First batch of a signature: the eager step, then its capture.  Later batches of that signature: batch -> static buffers, the scheduler's
    learning rate -> device, replay, metrics from the static logits, the static loss into the running total.  A batch of another signature
    (different text length; the short last batch) runs eagerly when the cache is full."""
    calls, logged, st, gs = _setup(monkeypatch, max_graphs=1)
    dl = [_batch(2, 16, 0), _batch(2, 16, 1), _batch(2, 24, 2), _batch(2, 16, 3), _batch(1, 16, 4)]
    best = T.not_grad_accum(0, dl, None, None, None, _Crit(), st, _Sched(st.opt, calls), 10, _Metric(calls), 100, 2400, None, graphs=gs)
    assert best == 0.5
    assert calls == [
        ("eager", 0), ("backward", 6.0), ("update",), ("capture", 0, 0, False, 3), ("sched", 0.0),
        ("feed", 0, 1), ("lr", 0.5), ("replay", 0), ("metrics", [1, 0], [1, 1]), ("sched", 0.2),
        ("eager", 2), ("backward", 6.0), ("update",), ("sched", 0.4),                                   # other text length: eager, cache full
        ("feed", 0, 3), ("lr", 0.9), ("replay", 0), ("metrics", [1, 0], [1, 1]), ("sched", 0.6),
        ("eager", 4), ("backward", 6.0), ("update",), ("sched", 0.8)]                                    # short last batch
    assert logged == [("train", (6.0 + 0.25 + 6.0 + 0.25 + 6.0) / 5)]
    assert (gs.eager_steps, gs.captures, gs.replays) == (3, 1, 2)


def test_graphed_grad_accum_scale_recapture_per_epoch_and_after_reload(monkeypatch, tmp_path):
    """grad_accum: 1 / dialogue length (float32, as torch's division by a Python scalar) goes to the device before each replay; the unclipped
    dialogue-end update stays eager.  one_epoch frees the epoch's graphs; the next epoch captures anew.  A reload of the optimizer state
    (load_model -> FusedAdamW.load_state_dict bumps .generation) frees them as well, mid-epoch."""
    calls, logged, st, gs = _setup(monkeypatch, max_graphs=2)

    class DS:
        grad, grad_sum, ctr = [2, 3], [2, 5], 0

        def retGradAccum(self, i):
            r, s = self.grad[self.ctr], self.grad_sum[self.ctr]
            if i + 1 == self.grad_sum[self.ctr]:
                self.ctr += 1
            if self.ctr == len(self.grad):
                self.ctr = 0
            return r, s

    class DL(list):
        dataset = DS()
    dl = DL([_batch(2, 16, i) for i in range(5)])
    sched = _Sched(st.opt, calls)
    T.one_epoch(1, dl, None, None, None, _Crit(), st, sched, 2, 10, None, 100, path=None, graphs=gs)
    third = float(np.float32(1.0) / np.float32(3.0))
    assert third != 1.0 / 3.0
    assert calls == [
        ("eager", 0), ("backward", 3.0), ("update",), ("capture", 0, 1, True, 3), ("sched", 1.0),
        ("feed", 0, 1), ("scale", 0.5), ("lr", 1.5), ("replay", 0), ("sched", 1.2), ("update-unclipped",), ("sched", 1.2),
        ("feed", 0, 2), ("scale", third), ("lr", 1.7), ("replay", 0), ("sched", 1.4),
        ("feed", 0, 3), ("scale", third), ("lr", 1.9), ("replay", 0), ("sched", 1.6),
        ("feed", 0, 4), ("scale", third), ("lr", 2.1), ("replay", 0), ("sched", 1.8), ("update-unclipped",), ("sched", 1.8),
        ("release", 0), ("released",)]                                                      # end of the epoch
    assert logged == [("train", (3.0 + 4 * 0.25) / 5)]
    del calls[:]
    T.one_epoch(2, [_batch(2, 16, 7), _batch(2, 16, 8)], None, None, None, _Crit(), st, sched, 2, 10, None, 100, path=None, graphs=gs)
    assert calls[:4] == [("eager", 7), ("backward", 6.0), ("update",), ("capture", 1, 2, False, 3)]        # new epoch, new capture
    assert ("replay", 1) in calls and calls[-2:] == [("release", 1), ("released",)]
    del calls[:]
    gs.step(*_batch(2, 16, 9), 4, None)
    st.opt.generation += 1                                          # what load_model does to the optimizer
    gs.step(*_batch(2, 16, 10), 4, None)
    assert calls == [("eager", 9), ("backward", 6.0), ("update",), ("capture", 2, 4, False, 3),
                     ("release", 2), ("released",), ("eager", 10), ("backward", 6.0), ("update",), ("capture", 3, 4, False, 3)]


def test_graphed_loop_refuses_a_reducer_and_fp8():
    st = _Stepper([])
    st.reducer = object()
    with pytest.raises(ValueError, match="data-parallel"):
        G.GraphedSteps(st)
    prev = runtime.precision()
    runtime.set_precision("fp8")
    try:
        with pytest.raises(ValueError, match="fp8"):
            G.GraphedSteps(_Stepper([]))
    finally:
        runtime.set_precision(prev)
