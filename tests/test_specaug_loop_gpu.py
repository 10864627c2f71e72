"""-m gpu: SpecAugment through libtavhip in the model and in the training loop.

"device" mode: the k-th train=True forward of a PreFormer draws the same masks whether it ran eagerly or as a replay of a captured forward, in any
interleaving, and they are the masks of the host model (tests/specaug_ref.py) for that call's seed; train_tav_network(graphs=True) equals
graphs=False bit for bit WITH SpecAugment on.  "reference" mode: exactly the rows and channels HF `_compute_mask_indices` selects under
np.random.seed(s) are replaced / zeroed, and a capture is refused."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import specaug_ref as R
import tav_amd  # noqa: F401
from tav_amd import config as C
from tav_amd import ops, runtime, synthetic
from tav_amd.models.tav import PreFormer, TAVForMAE
from tav_amd.train_model import graphed as G
from tav_amd.train_model import tav_train as T
from tav_amd.utils.global_functions import Metrics, NewCrossEntropyLoss
from test_graphed_loop_gpu import _LOG, ARGS, _Dialogues

pytestmark = pytest.mark.gpu
FEATURE = dict(mask_feature_prob=0.2, mask_feature_length=4, mask_feature_min_masks=1)


@pytest.fixture
def device_mode():
    runtime.set_specaugment("device")
    yield
    runtime.set_specaugment("torch")


def _cfg(**audio):
    cfg = C.preset("B-tiny")
    cfg["audio"].update(FEATURE)
    cfg["audio"].update(audio)
    return cfg


def test_preformer_replays_draw_what_eager_calls_draw(gpu, device_mode, monkeypatch):
    runtime.set_precision("bf16")
    cfg = _cfg()
    B, St = 3, 16
    (tx, au, vi), _ = synthetic.make_batch(cfg, B, s_text=St, t_audio=16000, n_visual_true=4, device="cuda")      # row 0: 20 % padding

    def make():
        torch.manual_seed(0)
        return synthetic.seeded_init_(PreFormer(cfg), 1).cuda()

    def run(pre, train=True):
        return pre(input_ids=tx["input_ids"], audio_features=au["audio_features"], video_embeds=vi["visual_embeds"], text_mask=tx["attention_mask"],
                   audio_mask=au["attention_mask"], visual_mask=vi["attention_mask"], device="cuda", train=train, n_visual_true=4)[0]
    drawn = []
    draw = ops.specaug_draw

    def rec_draw(valid, *a, **k):
        m = draw(valid, *a, **k)
        drawn.append((None if valid is None else valid.clone(), m.clone(), a))
        return m
    s = torch.cuda.Stream()
    with torch.cuda.stream(s), torch.no_grad():
        a = make()
        monkeypatch.setattr(ops, "specaug_draw", rec_draw)
        first = [run(a).clone() for _ in range(5)]
        monkeypatch.undo()
        plain = run(a, train=False).clone()
        assert a._spec_calls == 5
        b = make()
        second = [run(b).clone()]
        torch.cuda.synchronize()
        cap = runtime.capture(torch.cuda.CUDAGraph(), s)
        with cap:
            static = run(b)
        assert b._spec_calls == 1                           # the capture drew nothing
        for _ in range(3):
            cap.replay()
            second.append(static.clone())
        second.append(run(b).clone())
        assert b._spec_calls == 5
        torch.cuda.synchronize()
    for j, (x, y) in enumerate(zip(first, second)):
        assert torch.isfinite(x).all() and torch.equal(x, y), f"call {j + 1}: eager and eager / replay runs differ"
    assert all(not torch.equal(first[j], first[j + 1]) for j in range(4)), "consecutive calls drew the same masks"
    # text and video tokens are untouched, the audio segment is not
    Sa = a.wav2vec2.conv_out_len(16000)
    assert Sa == 49 and first[0].shape[1] == St + Sa + 4
    for x in first:
        assert torch.equal(x[:, :St], plain[:, :St]) and torch.equal(x[:, St + Sa:], plain[:, St + Sa:])
        assert not torch.equal(x[:, St:St + Sa], plain[:, St:St + Sa])
    # the masks themselves: two draws per call (time with the frame mask, feature without), equal to the host model for the call's seed
    assert len(drawn) == 10
    H = cfg["audio"]["hidden"]
    for k in range(5):
        seed = runtime.dropout_seed(k + 1)
        (valid, tm, ta), (fvalid, fm, fa) = drawn[2 * k], drawn[2 * k + 1]
        assert fvalid is None and valid.dtype == torch.bool and ta[:2] == (B, Sa) and fa[:2] == (B, H) and ta[5] == fa[5] == seed
        lens = valid.sum(1).tolist()
        assert lens[0] < Sa and lens[1] == lens[2] == Sa
        want_t = R.draw(valid.cpu().numpy(), B, Sa, 0.05, 10, 2, seed, R.TAG_TIME)[0]
        want_f = R.draw(None, B, H, 0.2, 4, 1, seed, R.TAG_FEATURE)[0]
        assert np.array_equal(tm.cpu().numpy(), want_t) and np.array_equal(fm.cpu().numpy(), want_f)
        assert tm.any(1).all() and fm.any(1).all()
        assert not (tm.bool() & ~valid).any(), "a masked frame lies in a row's padding"


def _train(monkeypatch, policy, graphs, path, mode="device", **audio):
    """The scenario of test_graphed_loop_gpu._train with SpecAugment ON: 16000 samples (49 frames), the preset's time masking plus feature masking."""
    runtime.set_precision(policy)
    runtime.set_specaugment(mode)
    cfg = _cfg(**audio)
    torch.manual_seed(0)
    pre, model = PreFormer(cfg), TAVForMAE(ARGS, cfg)
    synthetic.seeded_init_(pre, 1)
    synthetic.seeded_init_(model, 2)
    pre.cuda()
    model.cuda()
    embed0 = pre.masked_spec_embed.detach().clone()
    train = DataLoader(_Dialogues(cfg, [2, 2, 2, 2, 2, 1], [2, 4], 100, t_audio=16000), batch_size=None)          # two dialogues, a short last batch
    val = DataLoader(_Dialogues(cfg, [2, 2], [2], 200, t_audio=16000), batch_size=None)
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
    try:
        T.train_tav_network(model, pre, train, val, crit, 1e-4, 2, 1e-4, 2, Metrics(7), 10, 1.0, 2, path=str(path), log_val=3,
                            zero_grad_like_torch_1_10=False, graphs=graphs)
        torch.cuda.synchronize()
    finally:
        runtime.set_specaugment("torch")
        monkeypatch.undo()
    opt = made[-1].opt
    return dict(params=[p.detach().clone() for p in list(model.parameters()) + list(pre.parameters())],
                moments=[tuple(t.clone() for t in opt.state[p]) if p in opt.state else None for p in opt.params],
                step=opt.step_count, lr=opt.lr, logged=logged, replays=len(replays), embed0=embed0, embed=pre.masked_spec_embed.detach().clone(),
                spec_calls=pre._spec_calls)


@pytest.mark.parametrize("policy", ["fp32", "bf16"])
def test_graphed_training_loop_equals_eager_with_specaugment(gpu, monkeypatch, tmp_path, policy):
    """test_graphed_training_loop_equals_eager's two epochs (epoch_switch = 2, dialogues of 2 and 4 batches, a short last batch, mid-epoch
    validate(), best.pt reload) with SpecAugment drawn by the kernels: parameters, AdamW moments, step count, learning rate, logged losses
    and confusion matrices equal bit for bit with and without graphs -- and the masking really happened: the losses differ from a run with
    both probabilities 0, and masked_spec_embed was trained."""
    a = _train(monkeypatch, policy, False, tmp_path / "eager")
    b = _train(monkeypatch, policy, True, tmp_path / "graph")
    off = _train(monkeypatch, policy, False, tmp_path / "off", mask_time_prob=0.0, mask_feature_prob=0.0)
    assert a["replays"] == 0 and b["replays"] == 8                  # batches 2-5 of each epoch
    assert a["spec_calls"] == b["spec_calls"] == 12 and off["spec_calls"] == 0          # one draw per training batch, none in validate()
    assert len(a["logged"]) == 8 and [x[0] for x in a["logged"]] == [x[0] for x in b["logged"]]
    for (ca, la, cma), (_, lb, cmb) in zip(a["logged"], b["logged"]):
        assert la == lb and torch.equal(cma, cmb), (ca, la, lb)
    assert a["step"] == b["step"] > 0 and a["lr"] == b["lr"]
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))
    for ma, mb in zip(a["moments"], b["moments"]):
        assert (ma is None) == (mb is None) and (ma is None or (torch.equal(ma[0], mb[0]) and torch.equal(ma[1], mb[1])))
    assert any(m is not None for m in a["moments"])
    train_a = [l for c, l, _ in a["logged"] if c == "train"]
    train_off = [l for c, l, _ in off["logged"] if c == "train"]
    assert len(train_a) == len(train_off) > 0 and all(x != y for x, y in zip(train_a, train_off)), (train_a, train_off)
    assert not torch.equal(a["embed"], a["embed0"]) and torch.equal(a["embed"], b["embed"])


@pytest.mark.parametrize("seed", [3, 11])
def test_reference_mode_masks_what_hf_selects(gpu, seed):
    """np.random.seed(s): the hidden states come back with `masked_spec_embed` on exactly the frames, and zeros on exactly the channels, that the
    two direct HF calls select; everything else is the input.  Under a capture the mode raises (the guard state runtime.capture sets)."""
    from transformers.models.wav2vec2.modeling_wav2vec2 import _compute_mask_indices
    runtime.set_precision("bf16")
    cfg = _cfg()
    B, Tn, H = 3, 49, cfg["audio"]["hidden"]
    torch.manual_seed(0)
    pre = synthetic.seeded_init_(PreFormer(cfg), 1).cuda()
    amask = (torch.arange(Tn)[None, :] < torch.tensor([39, 49, 49])[:, None]).cuda()
    x = torch.randn(B * Tn, H, device="cuda") + 3.0          # (no zeros, nothing equal to the embedding)
    runtime.set_specaugment("reference")
    try:
        np.random.seed(seed)
        y = pre._mask_hidden_states(x, B, Tn, amask, training=True)
        np.random.seed(seed)
        tm = torch.from_numpy(_compute_mask_indices((B, Tn), mask_prob=0.05, mask_length=10, attention_mask=amask.cpu().long(), min_masks=2)).cuda()
        fm = torch.from_numpy(_compute_mask_indices((B, H), mask_prob=0.2, mask_length=4, min_masks=1)).cuda()
        want = torch.where(tm.reshape(B * Tn, 1), pre.masked_spec_embed.detach()[None, :], x)
        want = torch.where(fm[:, None, :].expand(B, Tn, H).reshape(B * Tn, H), torch.zeros((), device="cuda"), want)
        assert tm.any() and fm.any() and pre._spec_calls == 0
        assert torch.equal(y.detach(), want)
        assert torch.equal((y.detach() == 0).view(B, Tn, H), fm[:, None, :].expand(B, Tn, H))
        assert pre._mask_hidden_states(x, B, Tn, amask, training=False) is x
        with runtime.guard_only(torch.cuda.current_stream()):
            with pytest.raises(RuntimeError, match="cannot be captured"):
                pre._mask_hidden_states(x, B, Tn, amask, training=True)
    finally:
        runtime.set_specaugment("torch")
