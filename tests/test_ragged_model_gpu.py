"""GPU: ragged visual rows end to end (runtime.set_visual_rows("ragged")) on preset B-tiny.

A batch whose rows keep different numbers of video tokens computes what separate batch-1 runs of its utterances compute: logits row by row,
parameter gradients as the mean of the per-row ones, the CPU oracle row by row; no utterance sees another one, and the padded slots of the
fusion input do not matter."""
import pytest
import torch

import tav_amd  # noqa: F401
from oracle import tav_oracle as O
from tav_amd import config as C
from tav_amd import engine as E
from tav_amd import runtime, synthetic
from tav_amd.models.tav import PreFormer, TAVForMAE

pytestmark = pytest.mark.gpu

ARGS = dict(output_dim=7, dropout=0.5, learn_PosEmbeddings=True, num_layers=12)
COUNTS = [3, 5, 4, 1]            # True (fusion-side) video tokens per row; the video encoder keeps 32 - n


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


@pytest.fixture
def ragged_mode():
    runtime.set_visual_rows("ragged")
    yield
    runtime.set_visual_rows("equal")


def _models(cfg):
    torch.manual_seed(0)
    pre, model = PreFormer(cfg), TAVForMAE(ARGS, cfg)
    synthetic.seeded_init_(pre, 1)
    synthetic.seeded_init_(model, 2)
    return pre.cuda(), model.cuda()


def _batch(cfg, counts, seed=7):
    (tx, au, vi), lab = synthetic.make_batch(cfg, len(counts), seed=seed, s_text=16, t_audio=8000, n_visual_true=counts)
    return dict(input_ids=tx["input_ids"], text_mask=tx["attention_mask"], audio_features=au["audio_features"], audio_mask=au["attention_mask"],
                video_embeds=vi["visual_embeds"], visual_mask=vi["attention_mask"]), lab


def _rows(batch, lab, b):
    return {k: v[b:b + 1].clone() for k, v in batch.items()}, lab[b:b + 1].clone()


def _step(pre, model, batch, lab, n_visual_true=None, tav_hook=None):
    for p in list(pre.parameters()) + list(model.parameters()):
        p.grad = None
    d = {k: v.cuda() for k, v in batch.items()}
    tav, emb, amask = pre(input_ids=d["input_ids"], audio_features=d["audio_features"], video_embeds=d["video_embeds"], text_mask=d["text_mask"],
                          audio_mask=d["audio_mask"], visual_mask=d["visual_mask"], device="cuda", train=False, n_visual_true=n_visual_true)
    if tav_hook is not None:
        tav = tav_hook(tav)
    logits = model(d["input_ids"], d["text_mask"], d["audio_features"], d["video_embeds"], d["visual_mask"], tav, emb, amask,
                   batch_size=len(lab), check="val", n_visual_true=n_visual_true)
    loss = E.CrossEntropyFn.apply(logits, lab.long().cuda(), None)
    loss.backward()
    torch.cuda.synchronize()
    grads = [None if p.grad is None else p.grad.detach().clone() for p in list(pre.parameters()) + list(model.parameters())]
    return tav.detach(), emb, amask, logits.detach().clone(), loss.detach().clone(), grads


def test_ragged_mode_equal_rows_bitwise_equal_mode(gpu):
    cfg = C.preset("B-tiny")
    runtime.set_precision("bf16")
    pre, model = _models(cfg)
    batch, lab = _batch(cfg, [4, 4, 4])
    ref = _step(pre, model, batch, lab)
    runtime.set_visual_rows("ragged")
    try:
        got = _step(pre, model, batch, lab)
        got2 = _step(pre, model, batch, lab, n_visual_true=[4, 4, 4])
    finally:
        runtime.set_visual_rows("equal")
    for g in (got, got2):
        assert torch.equal(g[3], ref[3]) and torch.equal(g[4], ref[4])
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(g[5], ref[5]))


def test_unequal_rows_still_raise_in_equal_mode(gpu):
    cfg = C.preset("B-tiny")
    runtime.set_precision("bf16")
    pre, model = _models(cfg)
    batch, lab = _batch(cfg, [3, 5, 4, 4])               # (a total that divides by the batch: the per-row check is what refuses it)
    with pytest.raises(ValueError, match="same number"):
        _step(pre, model, batch, lab)
    with pytest.raises(ValueError, match="same number"):
        _step(pre, model, batch, lab, n_visual_true=[3, 5, 4, 4])


@pytest.mark.parametrize("policy", ["fp32", "bf16"])
def test_ragged_batch_equals_batch1_runs(gpu, ragged_mode, policy, capsys):
    cfg = C.preset("B-tiny")
    runtime.set_precision(policy)
    pre, model = _models(cfg)
    batch, lab = _batch(cfg, COUNTS)
    tav, emb, amask, logits, loss, grads = _step(pre, model, batch, lab)
    # the fusion input is rectangular: St + Sa + max n_true, video segment last, padding at the row's end with id 2 / mask 0
    St, Sa = batch["input_ids"].shape[1], pre.wav2vec2.conv_out_len(batch["audio_features"].shape[1])
    assert tuple(tav.shape) == (4, St + Sa + max(COUNTS), 768)
    for b, n in enumerate(COUNTS):
        assert (emb[b, St + Sa:] == 2).all() and not amask[b, 0, 0, St + Sa + n:].abs().sum().item()
    # the same with the counts given (no host read): bitwise the same
    assert torch.equal(_step(pre, model, batch, lab, n_visual_true=COUNTS)[3], logits)
    acc, worst = None, 0.0
    for b, n in enumerate(COUNTS):
        bb, lb = _rows(batch, lab, b)
        _, _, _, l1, _, g1 = _step(pre, model, bb, lb, n_visual_true=n)
        worst = max(worst, rel(logits[b:b + 1], l1))
        if policy == "fp32":
            assert rel(logits[b:b + 1], l1) < 1e-5, (b, rel(logits[b:b + 1], l1))
        acc = g1 if acc is None else [None if x is None else x + y for x, y in zip(acc, g1)]
    with capsys.disabled():
        print(f"\n[ragged {policy}] largest logits difference against batch-1 runs (rel): {worst:.3e}")
    if policy == "fp32":
        for i, (g, a) in enumerate(zip(grads, acc)):
            if g is None:
                assert a is None
                continue
            m = a / len(COUNTS)
            if m.abs().max().item() < 1e-6 * max(x.abs().max().item() for x in acc if x is not None):
                continue                              # a gradient that is zero up to rounding (e.g. key biases): no relative figure
            assert rel(g, m) < 1e-4, (i, rel(g, m))


@pytest.mark.parametrize("policy,tol", [("fp32", 1e-3), ("bf16", 1e-2)])
def test_ragged_batch_against_oracle_row_by_row(gpu, ragged_mode, policy, tol):
    cfg = C.preset("B-tiny")
    runtime.set_precision(policy)
    pre, model = _models(cfg)
    sdp = {k: v.detach().cpu().clone() for k, v in pre.state_dict().items()}
    sdm = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    batch, lab = _batch(cfg, COUNTS, seed=11)
    _, _, _, logits, loss, _ = _step(pre, model, batch, lab)
    o_losses = []
    for b in range(len(COUNTS)):
        bb, lb = _rows(batch, lab, b)
        o_logits, o_loss = O.tav_step(sdm, sdp, cfg, bb, lb.long())
        assert rel(logits[b:b + 1], o_logits) < tol, (b, rel(logits[b:b + 1], o_logits))
        o_losses.append(o_loss)
    o_mean = torch.stack([x.reshape(()) for x in o_losses]).mean()
    assert abs(loss.item() - o_mean.item()) / abs(o_mean.item()) < tol


def test_no_leakage_between_rows_or_from_padding(gpu, ragged_mode):
    cfg = C.preset("B-tiny")
    runtime.set_precision("bf16")
    pre, model = _models(cfg)
    batch, lab = _batch(cfg, COUNTS)
    tav, _, _, logits, _, grads = _step(pre, model, batch, lab)
    b2 = dict(batch)
    b2["video_embeds"] = batch["video_embeds"].clone()
    b2["video_embeds"][1] += torch.randn_like(b2["video_embeds"][1])
    l2 = _step(pre, model, b2, lab)[3]
    assert torch.equal(l2[0], logits[0]) and torch.equal(l2[2:], logits[2:]) and not torch.equal(l2[1], logits[1])
    St, Sa = batch["input_ids"].shape[1], pre.wav2vec2.conv_out_len(batch["audio_features"].shape[1])

    def scramble(t):
        t = t.detach().clone()
        g = torch.Generator(device="cuda").manual_seed(3)
        for b, n in enumerate(COUNTS):
            pad = t[b, St + Sa + n:]
            pad.copy_(torch.randn(pad.shape, device="cuda", generator=g) * 50)
        return t
    _, _, _, l3, _, g3 = _step(pre, model, batch, lab, tav_hook=scramble)
    assert torch.equal(l3, logits)
    model_grads = grads[len(list(pre.parameters())):]
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(g3[len(list(pre.parameters())):], model_grads))


def test_graphed_loop_with_ragged_batches_equals_eager(gpu, monkeypatch, tmp_path, ragged_mode):
    """train_tav_network(graphs=True) in ragged mode on a mix of equal and ragged batches: equal batches are captured and replayed, ragged ones
    run the eager step (they have no fixed shape to capture) -- losses, confusion matrices and final parameters equal graphs=False bit for bit."""
    import test_graphed_loop_gpu as TG
    make = synthetic.make_batch

    def mixed(cfg, b, *, seed=1234, **kw):
        if b == 2 and seed % 2:
            kw["n_visual_true"] = [3, 5]                   # every other two-row batch keeps unequal counts
        return make(cfg, b, seed=seed, **kw)
    runs = []
    for graphs in (False, True):
        monkeypatch.setattr(synthetic, "make_batch", mixed)
        runs.append(TG._train(monkeypatch, "bf16", False, graphs, tmp_path / str(graphs)))      # (_train undoes the patch when it returns)
    a, b = runs
    assert b["replays"] > 0
    assert [x[0] for x in a["logged"]] == [x[0] for x in b["logged"]]
    for (ca, la, cma), (_, lb, cmb) in zip(a["logged"], b["logged"]):
        assert la == lb and torch.equal(cma, cmb), (ca, la, lb)
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))
