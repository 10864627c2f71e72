"""-m gpu: graph mode of the training loop.  The device-seed dropout kernel (ABI v7) against the by-value one; replays of captured
train-mode forwards draw fresh masks, the same ones eager calls draw, in any interleaving with eager calls; train_tav_network(graphs=True)
equals graphs=False bit for bit; SpecAugment and dropout draw anew per replay; the tav_nn entrypoint with --graph 1."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset

import tav_amd  # noqa: F401
from tav_amd import config as C
from tav_amd import engine as E
from tav_amd import ops, runtime, synthetic
from tav_amd.models.tav import PreFormer, TAVForMAE
from tav_amd.train_model import graphed as G
from tav_amd.train_model import tav_train as T
from tav_amd.utils.global_functions import CrossEntropyLoss, Metrics, NewCrossEntropyLoss
from tav_amd.utils.TAVFormer import TransformerEncoder

pytestmark = pytest.mark.gpu
ARGS = dict(output_dim=7, dropout=0.5, learn_PosEmbeddings=True, num_layers=12)
_LOG = T.log


def _i64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def test_dropout_fwd_dev_equals_by_value(gpu):
    """tav_dropout_fwd_dev reads the seed word when it runs: output and mask equal tav_dropout_fwd's bit for bit (odd n, seeds above 2^63,
    the offsets TransformerBlockFn uses), and a captured launch follows what the host wrote into the word before the replay."""
    torch.manual_seed(0)
    for n, p, seed, off in [(1001, 0.5, 12345, 0), (3 * 768 + 5, 0.1, (1 << 64) - 17, 1 << 40), (77777, 0.9, (1 << 63) + 5, 2 << 40)]:
        x = torch.randn(n, device="cuda")
        y0, m0 = ops.dropout_fwd(x, p, seed, off)
        w = torch.tensor([_i64(seed)], dtype=torch.int64, device="cuda")
        y1, m1 = ops.dropout_fwd(x, p, w, off)
        assert torch.equal(y0, y1) and torch.equal(m0, m1)
        assert 0 < int(m0.sum()) < n
    s = torch.cuda.Stream()
    x = torch.randn(4097, device="cuda")
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with runtime.capture(g, s):
            y, m = ops.dropout_fwd(x, 0.5, w, 7)
        outs = []
        for seed in (99, (1 << 64) - 1):
            w.fill_(_i64(seed))
            g.replay()
            outs.append((y.clone(), m.clone(), *ops.dropout_fwd(x, 0.5, seed, 7)))
        torch.cuda.synchronize()
    for yr, mr, ye, me in outs:
        assert torch.equal(yr, ye) and torch.equal(mr, me)
    assert not torch.equal(outs[0][1], outs[1][1])


def _interleaved(make, run):
    """Module A: eager train call (warm-up), capture of a train call, then replay / eager val / replay / eager train / replay.  Its twin B (same
    weights, same torch seed): the same sequence, every call eager.  -> (outputs of A, outputs of B) after the warm-up."""
    s = torch.cuda.Stream()
    seq = ["R", "val", "R", "train", "R"]
    with torch.cuda.stream(s), torch.no_grad():
        a = make()
        run(a, True)
        torch.cuda.synchronize()
        cap = runtime.capture(torch.cuda.CUDAGraph(), s)
        with cap:
            static = run(a, True)
        got = []
        for step in seq:
            if step == "R":
                cap.replay()
                got.append(static.clone())
            else:
                got.append(run(a, step == "train").clone())
        b = make()
        run(b, True)
        want = [run(b, step != "val").clone() for step in seq]
        torch.cuda.synchronize()
    return got, want


def _check_interleaved(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.isfinite(g).all() and torch.equal(g, w), f"call {i + 2}: replay / eager differ from the all-eager twin"
    r = [got[0], got[2], got[4]]
    assert not torch.equal(r[0], r[1]) and not torch.equal(r[1], r[2]) and not torch.equal(r[0], r[2]), "replays drew the same masks"


def test_replayed_tav_head_draws_like_eager(gpu):
    """TAVForMAE forward + loss, check="train" (TailFn's head dropout, p = 0.5)."""
    cfg = C.preset("B-tiny")
    runtime.set_precision("bf16")
    torch.manual_seed(0)
    pre = synthetic.seeded_init_(PreFormer(cfg), 1).cuda().eval()
    (tx, au, vi), lab = synthetic.make_batch(cfg, 2, s_text=16, t_audio=8000, n_visual_true=4, device="cuda")
    with torch.no_grad():
        tav, emb, amask = pre(input_ids=tx["input_ids"], audio_features=au["audio_features"], video_embeds=vi["visual_embeds"], text_mask=tx["attention_mask"],
                              audio_mask=au["attention_mask"], visual_mask=vi["attention_mask"], device="cuda", train=False, n_visual_true=4)
    torch.cuda.synchronize()

    def make():
        torch.manual_seed(0)                     # (seeded_init_ keeps each tensor's init scale: the construction draws must match too)
        return synthetic.seeded_init_(TAVForMAE(ARGS, cfg), 2).cuda()

    def run(m, train):
        logits = m(tx["input_ids"], tx["attention_mask"], au["audio_features"], vi["visual_embeds"], vi["attention_mask"], tav, emb, amask,
                   batch_size=2, check="train" if train else "val", n_visual_true=4)
        loss = E.CrossEntropyFn.apply(logits, lab.long(), None)
        return torch.cat([logits.reshape(-1), loss.reshape(1)])
    _check_interleaved(*_interleaved(make, run))


def test_replayed_bert_classifier_head_draws_like_eager(gpu):
    """BertClassifier (HeadFn)."""
    from tav_amd.SingleModels.models.text import BertClassifier
    cfg = C.preset("B-tiny")
    runtime.set_precision("bf16")
    torch.manual_seed(0)
    (tx, _, _), _ = synthetic.make_batch(cfg, 3, s_text=16, text_only=True, device="cuda")

    def make():
        torch.manual_seed(0)
        return synthetic.seeded_init_(BertClassifier(dict(output_dim=7, dropout=0.5), config=cfg), 3).cuda()
    _check_interleaved(*_interleaved(make, lambda m, train: m(tx["input_ids"], tx["attention_mask"], "train" if train else "val")))


def test_replayed_transformer_encoder_draws_like_eager(gpu):
    """TransformerEncoder: one draw per layer, three masks per block (TransformerBlockFn)."""
    runtime.set_precision("fp32")
    torch.manual_seed(0)
    x = torch.randn(2, 11, 768, device="cuda")
    m = torch.zeros(2, 1, 1, 11, device="cuda")
    m[..., 8:] = -1e4

    def make():
        torch.manual_seed(0)
        return synthetic.seeded_init_(TransformerEncoder(768, num_layers=2, dropout=0.2), 4).cuda()

    def run(te, train):
        te.train(train)
        return te(x, m)
    _check_interleaved(*_interleaved(make, run))


def test_plain_graph_replay_after_the_capture_object_is_gone(gpu):
    """`with runtime.capture(g, s):` without keeping the capture object, then plain g.replay(): the seed words belong to the graph and start
    out with the seeds of the draws that followed the capture -- every replay repeats that draw (counters unmoved), equal to the eager call a
    twin makes next, even after the allocator released its free memory and handed it out again.  A capture that draws nothing passes its
    seed buffer on to the next capture instead of keeping one."""
    import gc
    runtime.set_precision("fp32")
    x = torch.randn(2, 11, 768, device="cuda")

    def make():
        torch.manual_seed(0)
        return synthetic.seeded_init_(TransformerEncoder(768, num_layers=2, dropout=0.2), 4).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s), torch.no_grad():
        a, b = make(), make()
        a(x)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with runtime.capture(g, s):
            static = a(x)
        assert a._calls == 2
        gc.collect()
        torch.cuda.empty_cache()
        junk = torch.full((1 << 22,), -1, dtype=torch.int64, device="cuda")       # reuse whatever was freed
        outs = []
        for _ in range(2):
            g.replay()
            outs.append(static.clone())
        del junk
        b(x)
        want = b(x)
        a.eval()
        g2, g3 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with runtime.capture(g2, s):
            a(x)
        spare = runtime._spare_words.get(str(x.device))
        with runtime.capture(g3, s):
            a(x)
        torch.cuda.synchronize()
    assert a._calls == 2 and torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], want)
    assert not hasattr(g2, "_tav_seed_words") and spare is not None and runtime._spare_words.get(str(x.device)) is spare


# ---------------------------------------------------------------------------------------------- the loop
class _Dialogues(Dataset):
    """Pre-collated batches plus the reference data loader's dialogue bookkeeping (retGradAccum -> (dialogue length, running end))."""

    def __init__(self, cfg, sizes, dialogues, seed, t_audio=8000):
        self.items = [synthetic.make_batch(cfg, b, seed=seed + i, s_text=16, t_audio=t_audio, n_visual_true=4) for i, b in enumerate(sizes)]
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


def _train(monkeypatch, policy, like_1_10, graphs, path):
    runtime.set_precision(policy)
    cfg = C.preset("B-tiny")
    cfg["audio"]["mask_time_prob"] = 0.0           # SpecAugment off: torch's Philox stream differs between eager calls and replays
    torch.manual_seed(0)
    pre, model = PreFormer(cfg), TAVForMAE(ARGS, cfg)
    synthetic.seeded_init_(pre, 1)
    synthetic.seeded_init_(model, 2)
    pre.cuda()
    model.cuda()
    train = DataLoader(_Dialogues(cfg, [2, 2, 2, 2, 2, 1], [2, 4], 100), batch_size=None)          # two dialogues, a short last batch
    val = DataLoader(_Dialogues(cfg, [2, 2], [2], 200), batch_size=None)
    crit = NewCrossEntropyLoss(class_weights=torch.linspace(0.6, 0.95, 7).cuda(), epoch_switch=2)
    made, logged, replays = [], [], []

    class Rec(T.TrainStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    replay = G.GraphedSteps._replay

    def rec_replay(self, *a, **k):
        replays.append(1)
        return replay(self, *a, **k)
    monkeypatch.setattr(T, "TrainStep", Rec)
    monkeypatch.setattr(G.GraphedSteps, "_replay", rec_replay)
    monkeypatch.setattr(T, "log", lambda M, loss, check="train": (logged.append((check, loss, M.cm.clone())), _LOG(M, loss, check)))
    T.PATIENCE_ITER = 0
    T.train_tav_network(model, pre, train, val, crit, 1e-4, 2, 1e-4, 2, Metrics(7), 10, 1.0, 2, path=str(path), log_val=3,
                        zero_grad_like_torch_1_10=like_1_10, graphs=graphs)
    torch.cuda.synchronize()
    opt = made[-1].opt
    out = dict(params=[p.detach().clone() for p in list(model.parameters()) + list(pre.parameters())],
               moments=[tuple(t.clone() for t in opt.state[p]) if p in opt.state else None for p in opt.params],
               step=opt.step_count, lr=opt.lr, logged=logged, replays=len(replays))
    monkeypatch.undo()
    return out


@pytest.mark.parametrize("policy", ["fp32", "bf16"])
@pytest.mark.parametrize("like_1_10", [False, True])
def test_graphed_training_loop_equals_eager(gpu, monkeypatch, tmp_path, policy, like_1_10):
    """Two epochs with epoch_switch = 2 (not_grad_accum with unweighted CE, then grad_accum with class-weighted CE and its unclipped
    dialogue-end steps), dialogues of 2 and 4 batches, a short last batch, validate() mid-epoch, best.pt saved and reloaded after each epoch:
    parameters, AdamW moments, step count, learning rate, logged losses and confusion matrices equal bit for bit with and without graphs."""
    a = _train(monkeypatch, policy, like_1_10, False, tmp_path / "eager")
    b = _train(monkeypatch, policy, like_1_10, True, tmp_path / "graph")
    assert a["replays"] == 0 and b["replays"] == 8                  # batches 2-5 of each epoch
    assert len(a["logged"]) == 8 and [x[0] for x in a["logged"]] == [x[0] for x in b["logged"]]
    for (ca, la, cma), (_, lb, cmb) in zip(a["logged"], b["logged"]):
        assert la == lb and torch.equal(cma, cmb), (ca, la, lb)
    assert a["step"] == b["step"] > 0 and a["lr"] == b["lr"]
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))
    for ma, mb in zip(a["moments"], b["moments"]):
        assert (ma is None) == (mb is None) and (ma is None or (torch.equal(ma[0], mb[0]) and torch.equal(ma[1], mb[1])))
    assert any(m is not None for m in a["moments"])


class _Same(Dataset):
    def __init__(self, batch, n):
        self.batch, self.n = batch, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.batch


@pytest.mark.parametrize("dropout", [0.5, 0.0])
def test_graphed_loop_draws_fresh_specaugment_and_dropout(gpu, monkeypatch, dropout):
    """SpecAugment on (the preset's mask_time_prob), graphs=True, learning rate 0 so that the parameters stay put: one epoch on the same batch
    gives finite losses, and consecutive replays differ -- with dropout 0 the SpecAugment draws alone make the difference."""
    runtime.set_precision("bf16")
    cfg = C.preset("B-tiny")
    torch.manual_seed(0)
    pre, model = synthetic.seeded_init_(PreFormer(cfg), 1).cuda(), synthetic.seeded_init_(TAVForMAE(dict(ARGS, dropout=dropout), cfg), 2).cuda()
    before = [p.detach().clone() for p in list(model.parameters()) + list(pre.parameters())]
    batch = synthetic.make_batch(cfg, 2, seed=5, s_text=16, t_audio=16000, n_visual_true=4)
    losses = []
    replay = G.GraphedSteps._replay
    monkeypatch.setattr(G.GraphedSteps, "_replay", lambda self, *a, **k: (losses.append(replay(self, *a, **k)), losses[-1])[1])
    T.PATIENCE_ITER = 0
    T.train_tav_network(model, pre, DataLoader(_Same(batch, 5), batch_size=None), DataLoader(_Same(batch, 1), batch_size=None), CrossEntropyLoss(),
                        0.0, 1, 1e-4, 2, None, 10, 1.0, 2, log_val=100, graphs=True)
    torch.cuda.synchronize()
    assert len(losses) == 4 and all(np.isfinite(losses))
    assert all(losses[i] != losses[i + 1] for i in range(3)), losses
    assert all(torch.equal(p.detach(), q) for p, q in zip(list(model.parameters()) + list(pre.parameters()), before))


def test_tav_nn_graph_mode_runs_one_tiny_epoch(gpu, capsys, monkeypatch):
    import tav_amd.tav_nn as tav_nn
    replays = []
    replay = G.GraphedSteps._replay
    monkeypatch.setattr(G.GraphedSteps, "_replay", lambda self, *a, **k: (replays.append(1), replay(self, *a, **k))[1])
    try:
        tav_nn.main(["--preset", "B-tiny", "--epoch", "1", "--batch_size", "2", "--synthetic", "8", "--dtype", "bf16", "--graph", "1"])
    finally:
        C.set_default_preset("A")
    out = capsys.readouterr().out
    assert "nan" not in out.lower() and "in train" in out
    assert len(replays) == 3
