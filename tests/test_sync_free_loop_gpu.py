"""-m gpu: the training loop's sync="log" mode (train_model/tav_train.LogSync).  Loss sum, ragged status word and confusion matrix stay on the
device and are read where the loops log: everything a run leaves equals sync="step" bit for bit, eager and from captured graphs; replayed
steps between two log points make no host read at all; the status word of a bucketed ragged run reaches the accumulator; the tav_nn
entrypoint with --loop-sync log."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset

import tav_amd  # noqa: F401
from tav_amd import config as C
from tav_amd import ops, runtime, synthetic
from tav_amd.models.tav import PreFormer, TAVForMAE
from tav_amd.train_model import graphed as G
from tav_amd.train_model import tav_train as T
from tav_amd.utils.global_functions import Metrics, NewCrossEntropyLoss

pytestmark = pytest.mark.gpu
ARGS = dict(output_dim=7, dropout=0.5, learn_PosEmbeddings=True, num_layers=12)
_LOG = T.log


@pytest.fixture
def restore_rows():
    yield
    runtime.set_visual_rows("equal")


class _Dialogues(Dataset):
    """Pre-collated batches plus the reference data loader's dialogue bookkeeping (retGradAccum -> (dialogue length, running end)).
    device="cuda": the batches live on the device and carry their per-row video token counts, as collate_batch_device hands them over."""

    def __init__(self, cfg, sizes, dialogues, seed, t_audio=8000, device="cpu"):
        self.items = [synthetic.make_batch(cfg, b, seed=seed + i, s_text=16, t_audio=t_audio, n_visual_true=4, device=device) for i, b in enumerate(sizes)]
        if device != "cpu":
            for (_, _, vi), _ in self.items:
                vi["n_visual_true"] = [4] * vi["attention_mask"].shape[0]
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


def _train(monkeypatch, policy, graphs, sync, path, device="cpu", epochs=2, around_replay=None):
    """The harness of test_graphed_loop_gpu._train: preset B-tiny, batches of 2, 2, 2, 2, 2, 1 in dialogues of 2 and 4, log_val = 3, two
    epochs with epoch_switch = 2 (both loops, both loss branches), validate() mid-epoch, best.pt saved and reloaded.  sync="log" runs with an
    on-device Metrics.  around_replay(before: bool): called on entry to and exit from every GraphedSteps._replay."""
    runtime.set_precision(policy)
    cfg = C.preset("B-tiny")
    cfg["audio"]["mask_time_prob"] = 0.0           # SpecAugment off: torch's Philox stream differs between eager calls and replays
    torch.manual_seed(0)
    pre, model = PreFormer(cfg), TAVForMAE(ARGS, cfg)
    synthetic.seeded_init_(pre, 1)
    synthetic.seeded_init_(model, 2)
    pre.cuda()
    model.cuda()
    train = DataLoader(_Dialogues(cfg, [2, 2, 2, 2, 2, 1], [2, 4], 100, device=device), batch_size=None)
    val = DataLoader(_Dialogues(cfg, [2, 2], [2], 200, device=device), batch_size=None)
    crit = NewCrossEntropyLoss(class_weights=torch.linspace(0.6, 0.95, 7).cuda(), epoch_switch=2)
    made, logged, replays, reads, stats = [], [], [], [], []

    class Rec(T.TrainStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    replay, read, step_stats = G.GraphedSteps._replay, T.LogSync.read, ops.step_stats

    def rec_replay(self, *a, **k):
        replays.append(1)
        if around_replay is not None:
            around_replay(True)
        try:
            return replay(self, *a, **k)
        finally:
            if around_replay is not None:
                around_replay(False)

    def rec_read(acc, what):
        r = read(acc, what)
        reads.append((what, r))
        return r

    def rec_stats(**k):
        stats.append({name: v is not None for name, v in k.items()})
        return step_stats(**k)
    monkeypatch.setattr(T, "TrainStep", Rec)
    monkeypatch.setattr(G.GraphedSteps, "_replay", rec_replay)
    monkeypatch.setattr(T.LogSync, "read", staticmethod(rec_read))
    monkeypatch.setattr(ops, "step_stats", rec_stats)
    monkeypatch.setattr(T, "log", lambda M, loss, check="train": (logged.append((check, loss, M.cm.cpu().clone())), _LOG(M, loss, check)))
    T.PATIENCE_ITER = 0
    metric = Metrics(7, rank="cuda", on_device=(sync == "log"))
    try:
        T.train_tav_network(model, pre, train, val, crit, 1e-4, epochs, 1e-4, 2, metric, 10, 1.0, 2, path=None if path is None else str(path), log_val=3,
                            graphs=graphs, sync=sync)
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    opt = made[-1].opt
    return dict(params=[p.detach().clone() for p in list(model.parameters()) + list(pre.parameters())],
                moments=[tuple(t.clone() for t in opt.state[p]) if p in opt.state else None for p in opt.params],
                step=opt.step_count, lr=opt.lr, logged=logged, replays=len(replays), reads=reads, stats=stats)


@pytest.mark.parametrize("policy", ["fp32", "bf16"])
@pytest.mark.parametrize("graphs", [False, True])
def test_log_sync_equals_step_sync_bit_for_bit(gpu, monkeypatch, tmp_path, graphs, policy):
    """Parameters, AdamW moments, step count, learning rate, every logged loss (float ==) and every logged confusion matrix of a sync="log"
    run equal the sync="step" run's, with both loss branches, mid-epoch validation, save and reload."""
    a = _train(monkeypatch, policy, graphs, "step", tmp_path / "step")
    b = _train(monkeypatch, policy, graphs, "log", tmp_path / "log")
    assert a["replays"] == b["replays"] == (8 if graphs else 0)          # batches 2-5 of each epoch
    assert not a["reads"] and not a["stats"]
    assert len(a["logged"]) == 8 and [x[0] for x in a["logged"]] == [x[0] for x in b["logged"]]
    for (ca, la, cma), (_, lb, cmb) in zip(a["logged"], b["logged"]):
        assert la == lb and torch.equal(cma, cmb), (ca, la, lb)
    assert all(np.isfinite(x[1]) for x in b["logged"]) and any(int(x[2].sum()) > 0 for x in b["logged"])
    assert a["step"] == b["step"] > 0 and a["lr"] == b["lr"]
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))
    for ma, mb in zip(a["moments"], b["moments"]):
        assert (ma is None) == (mb is None) and (ma is None or (torch.equal(ma[0], mb[0]) and torch.equal(ma[1], mb[1])))
    assert any(m is not None for m in a["moments"])
    # one launch per training and validation batch, each with the matrix, the loss and the accumulator; one read per log
    assert len(b["stats"]) == 2 * (6 + 2 * 2) and all(s["logits"] and s["cm"] and s["loss"] and s["acc"] for s in b["stats"])
    assert [w for w, _ in b["reads"]] == ["train", "val"] * 4
    train_reads = [r for w, r in b["reads"] if w == "train"]
    assert [r["steps"] for r in train_reads] == [3, 6, 3, 6] and [r["rows"] for r in train_reads] == [6, 11, 6, 11]     # reset per epoch
    assert all(r["steps"] == 2 and r["rows"] == 4 for w, r in b["reads"] if w == "val")                                  # reset per validate()
    assert all(r["status"] == 0 and r["first_bad_step"] == -1 and r["nonfinite"] == 0 and r["bad_rows"] == 0 for _, r in b["reads"])


_COUNTED = [(torch.Tensor, "item"), (torch.Tensor, "cpu"), (torch.Tensor, "tolist"), (torch.cuda, "synchronize"),
            (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize")]


def _replay_windows(monkeypatch, sync):
    """One not_grad_accum epoch in graph mode on device-resident batches that carry n_visual_true, with every host read / wait counted:
    -> [(count on entry, count on exit)] per replay (batches 1, 2, 3, 4; the loop logs after batch 2)."""
    n = [0]
    marks = []

    def counting(owner, name):
        orig = getattr(owner, name)

        def wrapped(*a, **k):
            n[0] += 1
            return orig(*a, **k)
        return wrapped
    with monkeypatch.context() as m:
        for owner, name in _COUNTED:
            m.setattr(owner, name, counting(owner, name))
        _train(monkeypatch, "bf16", True, sync, None, device="cuda", epochs=1, around_replay=lambda before: marks.append(n[0]))
    assert len(marks) == 8
    return list(zip(marks[0::2], marks[1::2]))


def test_replayed_steps_make_no_host_read_under_log_sync(gpu, monkeypatch):
    """Tensor.item / .cpu / .tolist, torch.cuda.synchronize, Stream.synchronize and Event.synchronize are counted.  Under sync="log" no call
    falls inside a replayed step, nor between two replays without a log point between them (batches 1 -> 2 and 3 -> 4: the scheduler
    step and the next batch's feed included).  The same harness under sync="step" counts at least one per replayed step (the control)."""
    w = _replay_windows(monkeypatch, "log")
    assert all(exit_ == entry for entry, exit_ in w), w
    assert w[1][0] == w[0][1] and w[3][0] == w[2][1], w
    assert w[2][0] > w[1][1], w                                          # the log point between batches 2 and 3 does read
    s = _replay_windows(monkeypatch, "step")
    assert all(exit_ - entry >= 1 for entry, exit_ in s), s


PAIRS = [[5, 7], [6, 8], [7, 5], [8, 6], [5, 6], [7, 8], [6, 7], [8, 5]]          # all inside bucket 4: capacities (8, 28), no two alike


def test_ragged_status_word_reaches_the_accumulator(gpu, monkeypatch, restore_rows):
    """Ragged rows at a bucketed capacity (the counts of test_ragged_capture_gpu's loop, all inside one bucket), graph mode, sync="log":
    every training and validation launch hands the step's status word over -- the model's after an eager step, the captured step's after
    a replay -- and every read finds it 0."""
    make = synthetic.make_batch

    def ragged(cfg, b, *, seed=1234, **kw):
        kw["n_visual_true"] = PAIRS[seed % len(PAIRS)] if b == 2 else [6]
        return make(cfg, b, seed=seed, **kw)
    runtime.set_visual_rows("ragged", bucket=4)
    monkeypatch.setattr(synthetic, "make_batch", ragged)
    out = _train(monkeypatch, "bf16", True, "log", None, epochs=1)
    assert out["replays"] == 4
    assert len(out["stats"]) == 6 + 2 * 2 and all(s["status"] and s["acc"] for s in out["stats"])
    assert len(out["reads"]) == 4 and all(r["status"] == 0 and r["first_bad_step"] == -1 and r["bad_rows"] == 0 for _, r in out["reads"])
    assert all(np.isfinite(x[1]) for x in out["logged"])


def test_tav_nn_log_sync_runs_one_tiny_epoch(gpu, capsys, monkeypatch):
    import tav_amd.tav_nn as tav_nn
    replays = []
    replay = G.GraphedSteps._replay
    monkeypatch.setattr(G.GraphedSteps, "_replay", lambda self, *a, **k: (replays.append(k.get("sync")), replay(self, *a, **k))[1])
    try:
        tav_nn.main(["--preset", "B-tiny", "--epoch", "1", "--batch_size", "2", "--synthetic", "8", "--dtype", "bf16", "--graph", "1",
                     "--loop-sync", "log"])
    finally:
        C.set_default_preset("A")
    out = capsys.readouterr().out
    assert "nan" not in out.lower() and "in train" in out and "in val" in out and "in test" in out
    assert len(replays) == 3 and all(s is not None for s in replays)
    losses = [float(line.split("loss = ")[1].split()[0]) for line in out.splitlines() if "loss = " in line]
    assert len(losses) >= 3 and all(np.isfinite(v) for v in losses) and any(v > 0 for v in losses)
