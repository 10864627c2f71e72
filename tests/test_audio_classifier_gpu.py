"""-m gpu: the audio-only baseline (SingleModels/models/audio.py, train_model/audio_training.py, audio_nn.py) on libtavhip against the
golden made from the HF module the reference calls and against float64 autograd of the CPU oracle.

The batch (audio_classifier_ref): B = 3, lengths (3200, 2087, 401) zero-padded to 3200, Sa = 9 -- an odd batch size, an odd length, and a
row with one real frame.  Gates: 1e-3 relative under the fp32 policy, 1e-2 under bf16 (BASELINE.json north_star; the gates of
test_model_gpu.py).  Every figure is printed before it is asserted.

Measured on an MI355X (fp32 policy, B-tiny): see profiles/audio_only.txt."""
import functools
import math
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import audio_classifier_ref as R
import closed_form as cf
import tav_amd  # noqa: F401
from tav_amd import config as C
from tav_amd import ops, runtime, synthetic
from tav_amd.models.tav import speech_features_device
from tav_amd.optim import grad_norm
from tav_amd.SingleModels import audio_nn
from tav_amd.SingleModels.models.audio import Wav2Vec2ForSpeechClassification, collate_batch, collate_batch_device
from tav_amd.SingleModels.train_model.audio_training import cosine_annealing_lr, validate
from tav_amd.utils.global_functions import CrossEntropyLoss, Metrics

pytestmark = pytest.mark.gpu
ARGS = dict(output_dim=R.OUTPUT_DIM)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


GRAD_SEED = 7


def _fresh(cfg, seed=0):
    """A freshly initialised model whose init does not depend on what ran before (synthetic.seeded_init_ measures its scales on it), built
    without touching the global generator's state."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return Wav2Vec2ForSpeechClassification(ARGS, config=cfg)


@functools.lru_cache(maxsize=None)
def _state(preset, weights):
    """The weights both sides run on.  "closed": tests/closed_form.py (what the golden was made with); "seeded": synthetic.seeded_init_ at
    the module's own init scale (drawn once: its scale is measured on a freshly initialised module)."""
    model = _fresh(C.preset(preset))
    model = cf.fill_module_(model) if weights == "closed" else synthetic.seeded_init_(model, GRAD_SEED)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _model(preset, weights):
    model = Wav2Vec2ForSpeechClassification(ARGS, config=C.preset(preset))
    model.load_state_dict(_state(preset, weights))
    return model


@functools.lru_cache(maxsize=None)
def _oracle(preset, weights):
    """float64 forward + backward of the oracle, computed once per (preset, weights) and left unchanged."""
    wave, labels = R.batch()
    return R.oracle_run(_state(preset, weights), C.preset(preset)["audio"], wave, labels)


def _product(preset, weights="closed"):
    """The model under the fp32 policy in eval mode, after one forward + backward on the batch."""
    runtime.set_precision("fp32")
    model = _model(preset, weights).cuda().eval()
    wave, labels = R.batch()
    logits = model(wave.cuda())
    loss = CrossEntropyLoss()(logits, labels)
    loss.backward()
    torch.cuda.synchronize()
    return model, logits, loss


@pytest.mark.parametrize("preset", R.PRESETS)
def test_golden_fp32(gpu, preset):
    gold = np.load(R.GOLDEN)
    model, logits, loss = _product(preset)
    assert logits.shape == (3, 7) and logits.dtype == torch.float32
    gn = grad_norm(list(model.parameters())).item()
    errs = dict(logits=rel(logits, gold[f"{preset}_logits"]), loss=abs(loss.item() - gold[f"{preset}_loss"][0]) / gold[f"{preset}_loss"][0],
                gradnorm=abs(gn - gold[f"{preset}_gradnorm"][0]) / gold[f"{preset}_gradnorm"][0])
    print(f"{preset} fp32 vs golden: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < 1e-3


def test_every_parameter_gradient_fp32(gpu):
    """Every parameter's gradient against float64 autograd of the oracle.  g* = the largest float64 gradient magnitude in the model.  A
    tensor whose float64 gradient exceeds 1e-6 g*: max abs error <= 1e-3 of its own max magnitude.  A tensor at or below that (the two
    k_proj.bias, whose gradient is mathematically zero: a key bias shifts every score of a query alike and softmax ignores it): abs error
    <= 1e-6 g*.  Weights: synthetic.seeded_init_ -- under the closed-form weights the B-tiny feature extractor saturates (the three rows get
    the same logits and fourteen tensors' gradients fall below 1e-6 g*), which would leave most of the backward unexamined.  float32
    autograd of the same oracle sits 1.3e-6 (worst tensor, relative to its own max) from float64."""
    o = _oracle("B-tiny", "seeded")
    model, logits, loss = _product("B-tiny", "seeded")
    e_logits = rel(logits, o["logits"])
    print(f"B-tiny fp32, seeded weights, vs float64 oracle: logits {e_logits:.2e}  loss {abs(loss.item() - o['loss']) / o['loss']:.2e}")
    assert e_logits < 1e-3 and o["logits"].std(0).min() > 1e-3        # the rows really differ
    grads = o["grads"]
    named = dict(model.named_parameters())
    assert set(named) == set(grads)
    assert named["wav2vec2.masked_spec_embed"].grad is None and grads["wav2vec2.masked_spec_embed"] is None
    gstar = max(g.abs().max().item() for g in grads.values() if g is not None)
    worst_rel, worst_small, small = (0.0, ""), (0.0, ""), []
    failures = []
    for k, p in named.items():
        if k == "wav2vec2.masked_spec_embed":
            continue
        assert p.grad is not None and grads[k] is not None and p.grad.shape == grads[k].shape, k
        err = (p.grad.detach().double().cpu() - grads[k]).abs().max().item()
        own = grads[k].abs().max().item()
        if own > 1e-6 * gstar:
            worst_rel = max(worst_rel, (err / own, k))
            if not err <= 1e-3 * own:
                failures.append((k, err / own))
        else:
            small.append(k)
            worst_small = max(worst_small, (err / (1e-6 * gstar), k))
            if not err <= 1e-6 * gstar:
                failures.append((k, err / (1e-6 * gstar)))
    print(f"B-tiny fp32 per-parameter gradients vs float64 autograd: {len(named) - 1} tensors, g* {gstar:.3e}; worst err / own max "
          f"{worst_rel[0]:.2e} ({worst_rel[1]}); tensors at or below 1e-6 g*: {small}, worst abs err / (1e-6 g*) {worst_small[0]:.2e} ({worst_small[1]})")
    assert sorted(small) == ["wav2vec2.encoder.layers.0.attention.k_proj.bias", "wav2vec2.encoder.layers.1.attention.k_proj.bias"]
    assert not failures, failures


def test_bf16_vs_oracle(gpu):
    """bf16 policy, seeded-random weights, preset B widths at 2 layers, B = 2, lengths (8000, 5000): logits and loss within 1e-2 of the
    float64 oracle; every gradient finite."""
    cfg = C.preset("B")
    cfg["audio"]["layers"] = 2
    runtime.set_precision("bf16")
    model = synthetic.seeded_init_(_fresh(cfg), 3).eval()
    g = torch.Generator().manual_seed(11)
    wave = torch.zeros(2, 8000)
    wave[0] = torch.randn(8000, generator=g) * 0.1
    wave[1, :5000] = torch.randn(5000, generator=g) * 0.1
    labels = torch.tensor([2, 5])
    o = R.oracle_run({k: v.detach().clone() for k, v in model.state_dict().items()}, cfg["audio"], wave, labels, backward=False)
    model.cuda()
    logits = model(wave.cuda())
    loss = CrossEntropyLoss()(logits, labels)
    loss.backward()
    e_logits, e_loss = rel(logits, o["logits"]), abs(loss.item() - o["loss"]) / o["loss"]
    print(f"bf16 vs float64 oracle: logits {e_logits:.2e}  loss {e_loss:.2e}")
    assert e_logits < 1e-2 and e_loss < 1e-2
    grads = {k: p.grad for k, p in model.named_parameters() if k != "wav2vec2.masked_spec_embed"}
    assert all(v is not None and torch.isfinite(v).all() for v in grads.values()), [k for k, v in grads.items() if v is None or not torch.isfinite(v).all()]


def test_dropout_follows_training_mode_and_validation_keeps_it(gpu):
    runtime.set_precision("bf16")
    model = synthetic.seeded_init_(_fresh(C.preset("B-tiny")), 5).cuda()
    wave = R.batch()[0].cuda()
    assert model.training                                        # a fresh module trains, and nothing below the loops changes that
    a, b = model(wave), model(wave)
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and not torch.equal(a, b)
    model.eval()
    a, b = model(wave), model(wave)
    assert torch.equal(a, b)
    # the reference's loops never call .eval(): validate() runs with dropout on, so two passes over one loader differ
    model.train()
    loader = DataLoader(list(zip(R.utterances(), R.LABELS)), batch_size=2, shuffle=False, collate_fn=collate_batch)
    Metric = Metrics(num_classes=R.OUTPUT_DIM)
    crit = CrossEntropyLoss()
    (_, l1), (_, l2) = validate(loader, model, crit, Metric), validate(loader, model, crit, Metric)
    print(f"validate twice on one loader: {l1:.6f} {l2:.6f}")
    assert math.isfinite(l1) and math.isfinite(l2) and l1 != l2
    assert model.training


def test_collate_batch_device_rows(gpu):
    g = torch.Generator().manual_seed(3)
    items = [({"pcm": torch.randint(-32768, 32768, (2, 3001), generator=g, dtype=torch.int16), "sampling_rate": 44100}, 4),
             ({"pcm": torch.randn(700, generator=g) * 0.1, "sampling_rate": 16000}, 0),
             (torch.randn(1500, generator=g) * 0.1, 6)]
    audio, labels = collate_batch_device(items)
    rows = [speech_features_device(items[0][0]["pcm"], 44100), speech_features_device(items[1][0]["pcm"], 16000), speech_features_device(items[2][0], 16000)]
    lens = [ops.resampled_length(3001, 44100), 700, 1500]
    assert [len(r) for r in rows] == lens and lens[0] == 1089
    assert audio.is_cuda and audio.dtype == torch.float32 and audio.shape == (3, 1500)
    for b, r in enumerate(rows):
        assert torch.equal(audio[b, :lens[b]].view(torch.int32), r.view(torch.int32)), b
        assert not bool(audio[b, lens[b]:].any()), b
    assert torch.equal(audio[2].cpu(), items[2][0])              # a finished 16 kHz waveform passes through unchanged
    assert labels.is_cuda and labels.dtype == torch.float32 and labels.tolist() == [4.0, 0.0, 6.0]
    with pytest.raises(ValueError, match="decoding audio files is outside this package"):
        collate_batch_device([("clips/dia0_utt0.wav", 0)])


def test_entrypoint_trains_validates_and_tests(gpu, capsys):
    argv = ["--preset", "B-tiny", "--epoch", "3", "--batch_size", "2", "--synthetic", "6", "--dtype", "bf16", "--patience", "1", "--audio-seconds", "0.1,0.3",
            "--T_max", "2"]
    try:
        audio_nn.main(argv)
    finally:
        runtime.set_precision("bf16")
    out = capsys.readouterr().out
    print(out)
    assert "nan" not in out.lower()
    num = r"([-+0-9.eE]+)"
    train = re.findall(rf"epoch (\d+): lr {num} train loss {num} batch loss {num}", out)
    val = re.findall(rf"epoch (\d+): val loss {num}", out)
    test = re.findall(rf"test: loss {num}", out)
    assert [int(t[0]) for t in train] == [0, 1, 2] and [int(v[0]) for v in val] == [0, 1, 2] and len(test) == 1
    losses = [float(x) for t in train for x in t[2:]] + [float(v[1]) for v in val] + [float(test[0])]
    assert all(math.isfinite(x) and x > 0 for x in losses), losses
    base = 0.000001                                              # arg_parse's default learning rate
    lrs = [float(t[1]) for t in train]
    want = [cosine_annealing_lr(base, e, 2) for e in range(3)]
    assert want[2] == 0.0 and all(abs(a - b) <= 1e-6 * base for a, b in zip(lrs, want)), (lrs, want)
    with pytest.raises(SystemExit, match="graph mode exists for the tri-modal loop only"):
        audio_nn.main(argv + ["--graph", "1"])
