"""No GPU: the loop and the entry scaffold the ablation baselines share (train_model/classifier_loop.py, utils/entrypoint.py) through the
names the drop-ins keep: the no-grad pass of audio_training and visual_training against a hand-written loop, the one cosine rule, the
refusal of flags only tav_nn implements, and the classes that became aliases of one."""
import glob
import os

import pytest
import torch
from torch.utils.data import DataLoader

import tav_amd  # noqa: F401
import tav_amd.tav_nn as tav_nn
from tav_amd import config as C
from tav_amd import synthetic
from tav_amd.DoubleModels import text_audio_nn
from tav_amd.DoubleModels.train_model.text_audio_training import TextAudioTrainStep
from tav_amd.SingleModels import audio_nn, text_nn, visual_nn
from tav_amd.SingleModels.train_model import audio_training, visual_training
from tav_amd.SingleModels.train_model.text_training import TextTrainStep
from tav_amd.train_model.classifier_loop import ClipStep
from tav_amd.utils.entrypoint import SyntheticBatches, refuse_tav_only
from tav_amd.utils.global_functions import Metrics, arg_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-modal-emotion_amd")
BASELINES = (audio_nn, visual_nn, text_nn, text_audio_nn)


# ---------------------------------------------------------------------------------------------- the shared no-grad pass
def test_validate_of_both_drop_ins_is_the_hand_written_loop():
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    model = torch.nn.Linear(5, 3)
    rows = [(torch.randn(5, generator=g), float(i % 3)) for i in range(7)]
    loader = DataLoader(rows, batch_size=3, shuffle=False)                       # batches of 3, 3, 1
    criterion = lambda out, lab: torch.nn.functional.cross_entropy(out, lab)     # noqa: E731
    want_cm, total, last, seen = torch.zeros(3, 3, dtype=torch.long), 0.0, None, 0
    with torch.no_grad():
        for x, y in loader:
            out = model(x)
            last = criterion(out, y.long())
            total += last.item()
            seen += len(y)
            for t, p in zip(y.long().tolist(), out.argmax(1).tolist()):
                want_cm[t, p] += 1
    assert seen == len(loader.dataset) == 7                                      # rows seen is the reference's len(dataset) for such a loader
    got = []
    for mod in (audio_training, visual_training):
        metric = Metrics(num_classes=3, rank="cpu")
        batch_loss, mean = mod.validate(loader, model, criterion, metric)
        got.append((float(batch_loss), mean, metric.cm.clone()))
        assert float(batch_loss) == float(last) and mean == total / 7, mod.__name__
        assert int(metric.cm.sum()) == 7 and torch.equal(metric.cm, want_cm), mod.__name__
    assert got[0][:2] == got[1][:2] and torch.equal(got[0][2], got[1][2])
    assert all(not p.requires_grad or p.grad is None for p in model.parameters())


# ---------------------------------------------------------------------------------------------- the one cosine rule
@pytest.mark.parametrize("T_max", [1, 2, 5])
def test_cosine_annealing_lr_is_the_one_rule(T_max):
    """Against torch's CosineAnnealingLR(T_max, eta_min=0) to 1e-12 of the base rate (at epoch T_max the rate itself is 0)."""
    base = 0.05
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_max, eta_min=0)
    for epoch in range(2 * T_max + 1):
        got, want = audio_training.cosine_annealing_lr(base, epoch, T_max), opt.param_groups[0]["lr"]
        assert abs(got - want) <= 1e-12 * base, (epoch, got, want)
        opt.step()
        sched.step()


def test_no_baseline_module_spells_the_cosine_out():
    files = [f for d in ("SingleModels", "DoubleModels") for f in glob.glob(os.path.join(PKG, d, "**", "*.py"), recursive=True)]
    assert len(files) >= 12
    assert not [f for f in files if "math.cos" in open(f).read()]


# ---------------------------------------------------------------------------------------------- flags only tav_nn implements
OTHER_FLAGS = [("--loop-sync", "log"), ("--encoder-lr-scale", "0.5"), ("--no-decay-norm-bias", "1"), ("--visual-rows", "ragged"),
               ("--visual-bucket", "8"), ("--specaugment", "device")]


@pytest.mark.parametrize("mod", BASELINES, ids=lambda m: m.__name__.rsplit(".", 1)[-1])
def test_baseline_mains_refuse_what_only_tav_nn_implements(mod):
    with pytest.raises(SystemExit, match=r"--graph 1: graph mode exists for the tri-modal loop only \(tav_nn\); run this entrypoint with --graph 0"):
        mod.main(["--graph", "1"])
    for flag, value in OTHER_FLAGS:
        with pytest.raises(SystemExit, match=rf"^{flag} .*exists for the tri-modal loop only \(tav_nn\); run this entrypoint with {flag} "):
            mod.main([flag, value])


def test_refuse_tav_only_passes_the_defaults_and_names_the_flag():
    assert refuse_tav_only(arg_parse("Text", [])) is None
    assert refuse_tav_only(audio_nn.parse_args([])) is None and refuse_tav_only(visual_nn.parse_args([])) is None
    assert refuse_tav_only(arg_parse("Text", ["--epoch", "1", "--clip", "0.5", "--preset", "B-tiny", "--dtype", "fp32"])) is None
    for flag, value in [("--graph", "1")] + OTHER_FLAGS:
        with pytest.raises(SystemExit) as e:
            refuse_tav_only(arg_parse("Text", [flag, value]))
        assert str(e.value).startswith(f"{flag} ") and "tav_nn" in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------- aliases
def test_train_steps_are_one_class():
    assert issubclass(TextTrainStep, ClipStep) and issubclass(TextAudioTrainStep, ClipStep)
    assert TextTrainStep.__call__ is TextAudioTrainStep.__call__ is ClipStep.__call__
    assert TextTrainStep.__init__ is TextAudioTrainStep.__init__ is ClipStep.__init__


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_batch_datasets_are_one_class_with_their_old_signatures():
    cfg = C.preset("B-tiny")
    n, bs, seed, i = 8, 2, 1000, 3
    # SyntheticBatches itself: make_batch with the given keywords at seed + i
    kw = dict(s_text=16, t_audio=8000, n_visual_true=4)
    base = SyntheticBatches(cfg, n, bs, seed, **kw)
    assert len(base) == 4 and len(SyntheticBatches(cfg, 1, bs, seed)) == 1
    assert _same(base[i], synthetic.make_batch(cfg, bs, seed=seed + i, **kw))
    # tav_nn: (cfg, n_utterances, batch_size, seed, s_text, t_audio), n_visual_true 4 at a tiny preset
    ds = tav_nn.SyntheticTAVBatches(cfg, n, bs, seed, 16, 8000)
    assert isinstance(ds, SyntheticBatches) and len(ds) == 4
    assert _same(ds[i], synthetic.make_batch(cfg, bs, seed=seed + i, s_text=16, t_audio=8000, n_visual_true=4))
    # text_nn: (cfg, n_utterances, batch_size, seed, s_text)
    ds = text_nn.SyntheticTextBatches(cfg, n, bs, seed, 16)
    (tx, _, _), lab = synthetic.make_batch(cfg, bs, seed=seed + i, s_text=16, t_audio=400, n_visual_true=4, text_only=True)
    assert isinstance(ds, SyntheticBatches) and len(ds) == 4
    assert _same(ds[i], ({"input_ids": tx["input_ids"].unsqueeze(1), "attention_mask": tx["attention_mask"]}, lab))
    # text_audio_nn: (cfg, n_utterances, batch_size, seed, s_text, t_audio)
    ds = text_audio_nn.SyntheticTextAudioBatches(cfg, n, bs, seed, 16, 8000)
    (tx, au, _), lab = synthetic.make_batch(cfg, bs, seed=seed + i, s_text=16, t_audio=8000, with_video=False)
    assert isinstance(ds, SyntheticBatches) and len(ds) == 4
    assert _same(ds[i], ([tx, au], lab))
