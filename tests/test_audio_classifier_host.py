"""No GPU: the audio-only baseline's host side -- the classifier's state_dict and refusal to run on the CPU, the host collate contract,
the reference's early-stopping rule, the cosine schedule's closed form, and the golden record against the float64 oracle."""
import os

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pad_sequence

import audio_classifier_ref as R
import tav_amd  # noqa: F401
from tav_amd import config as C
from tav_amd.encoders import AudioEncoder
from tav_amd.SingleModels.models.audio import Wav2Vec2ForSpeechClassification, collate_batch
from tav_amd.SingleModels.train_model.audio_training import cosine_annealing_lr
from tav_amd.utils.early_stopping import EarlyStopping

ARGS = dict(output_dim=R.OUTPUT_DIM)


def test_state_dict_keys_default_width_and_no_cpu_fallback():
    cfg = C.preset("B-tiny")
    model = Wav2Vec2ForSpeechClassification(ARGS, config=cfg)
    want = ["wav2vec2." + k for k in AudioEncoder(cfg["audio"]).state_dict()] + ["out_proj.weight", "out_proj.bias"]
    assert list(model.state_dict()) == want
    with pytest.raises(RuntimeError, match="GPU.* only; there is no CPU fallback"):
        model(torch.zeros(2, 800))
    assert tuple(Wav2Vec2ForSpeechClassification(ARGS, config=C.preset("A-tiny")).out_proj.weight.shape) == (7, 1024)   # the documented deviation
    # config=None is the reference's wav2vec2-base whatever the process default is: build it on the meta device (full depth, no memory)
    before = C._current[0]
    try:
        for default in (before, "A"):
            C.set_default_preset(default)
            with torch.device("meta"):
                m = Wav2Vec2ForSpeechClassification(ARGS)
            assert tuple(m.out_proj.weight.shape) == (7, 768)
            assert m.cfg["audio"] == C.preset("B")["audio"] and len(m.wav2vec2.encoder.layers) == 12
    finally:
        C.set_default_preset(before)


def test_collate_batch_is_pad_sequence():
    utts = R.utterances()
    wave, labels = collate_batch(list(zip(utts, R.LABELS)))
    assert torch.equal(wave, pad_sequence(utts, batch_first=True)) and torch.equal(wave, R.batch()[0])
    assert wave.shape == (3, 3200) and wave.dtype == torch.float32
    for b, L in enumerate(R.LENGTHS):
        assert not wave[b, L:].any() and wave[b, :L].abs().sum() > 0
    assert labels.dtype == torch.float32 and labels.tolist() == [0.0, 3.0, 6.0]
    with pytest.raises(ValueError, match="decoding audio files is outside this package"):
        collate_batch([("clips/dia0_utt0.wav", 0)])
    with pytest.raises(ValueError, match="collate_batch_device"):
        collate_batch([({"pcm": utts[0], "sampling_rate": 44100}, 0)])


def test_early_stopping_rule():
    model = torch.nn.Linear(3, 2)
    es = EarlyStopping("", model, patience=1, model_name="Linear")
    # epoch:   1     2     3     4      5     6     7     8
    scores = [1.0, 0.8, 0.8, 0.9, 0.95, 0.7, 0.75, 0.71]
    #         best  best  best(=) worse  >3+1  best  worse  >6+1
    want = [False, False, False, False, True, False, False, True]
    best_epochs = [1, 2, 3, 3, 3, 6, 6, 6]
    stored = {}
    for i, s in enumerate(scores):
        with torch.no_grad():
            model.weight.fill_(float(i + 1))
            model.bias.fill_(-float(i + 1))
        got = es(model, s)
        assert got is want[i] and es.best_epoch == best_epochs[i], (i, got, es.best_epoch)
        if es.best_epoch == i + 1:
            stored = {k: v.clone() for k, v in model.state_dict().items()}
        assert all(torch.equal(es.best_state_dict["model_state_dict"][k], v) for k, v in stored.items())
    assert es.best_score == 0.7 and es.epoch == 8
    # the stored copy is deep: the live tensors were overwritten twice since epoch 6, and best_state puts epoch 6's back bit for bit
    assert float(model.weight.detach()[0, 0]) == 8.0
    back = es.best_state
    assert back is model
    assert all(torch.equal(model.state_dict()[k], v) for k, v in stored.items()) and float(model.weight.detach()[0, 0]) == 6.0
    assert not [f for f in os.listdir(".") if f.endswith("_Linear.pkl")]              # no path_prefix: nothing is written


def test_early_stopping_restore_invalidates_cached_operands():
    from tav_amd import engine
    model = torch.nn.Linear(2, 2)
    es = EarlyStopping("", model, patience=0)
    es(model, 1.0)
    before = engine._EPOCH[0]
    assert es(model, 2.0) is True
    es.best_state
    assert engine._EPOCH[0] == before + 1


@pytest.mark.parametrize("T_max", [2, 5])
def test_cosine_annealing_lr_is_torch_scheduler(T_max):
    base = 0.05
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_max)
    worst = 0.0
    for epoch in range(2 * T_max + 3):
        worst = max(worst, abs(opt.param_groups[0]["lr"] - cosine_annealing_lr(base, epoch, T_max)))
        opt.step()
        sched.step()
    print(f"T_max {T_max}: worst |closed form - CosineAnnealingLR| {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("preset", R.PRESETS)
def test_golden_is_what_the_oracle_says(preset):
    assert os.path.getsize(R.GOLDEN) < 64 * 1024
    gold = np.load(R.GOLDEN)
    cfg = C.preset(preset)
    sd = R.closed_form_state(Wav2Vec2ForSpeechClassification(ARGS, config=cfg))
    wave, labels = R.batch()
    o = R.oracle_run(sd, cfg["audio"], wave, labels)
    assert o["frames"] == R.SA and o["grads"]["wav2vec2.masked_spec_embed"] is None
    g_logits = torch.as_tensor(gold[f"{preset}_logits"]).double()
    errs = dict(logits=((o["logits"] - g_logits).abs().max() / g_logits.abs().max()).item(),
                pooled=((o["pooled"] - torch.as_tensor(gold[f"{preset}_pooled"]).double()).abs().max() / np.abs(gold[f"{preset}_pooled"]).max()).item(),
                loss=abs(o["loss"] - gold[f"{preset}_loss"][0]) / gold[f"{preset}_loss"][0],
                gradnorm=abs(o["gradnorm"] - gold[f"{preset}_gradnorm"][0]) / gold[f"{preset}_gradnorm"][0])
    print(f"{preset}: oracle (float64) vs golden: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < 1e-5
