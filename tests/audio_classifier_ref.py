"""The batch and the float64 reference shared by the audio-only classifier's golden generator and tests (test_audio_classifier_host.py,
test_audio_classifier_gpu.py, make_audio_classifier_golden.py).

The batch: B = 3 utterances of 3200, 2087 and 401 samples, zero-padded to 3200 (Sa = 9 frames); 401 is one sample above the conv stack's
400-sample receptive field, so the shortest row is one real frame and eight frames of padding.  Labels (0, 3, 6), 7 classes.
The reference: oracle.tav_oracle.w2v2_model on the padded batch, mean over all frames, the linear layer, cross entropy; gradients from
autograd in the same dtype (float64 unless asked otherwise)."""
import os

import numpy as np
import torch

import closed_form as cf
from oracle import tav_oracle as O

LENGTHS = (3200, 2087, 401)
LABELS = (0, 3, 6)
OUTPUT_DIM = 7
SA = 9
PRESETS = ("A-tiny", "B-tiny")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_classifier_golden.npz")


def utterances():
    """The three closed-form waveforms, unpadded (float32, 1-D)."""
    out = []
    for b, L in enumerate(LENGTHS):
        n = np.arange(L, dtype=np.float64)
        w = 0.1 * np.sin(n * 0.0137 * (1.0 + 0.31 * b) + 0.3 + b) + 0.05 * np.sin(n * 0.311 + 0.7 * b)
        out.append(torch.tensor(w, dtype=torch.float32))
    return out


def batch():
    """(f32 [3, 3200] zero-padded waveforms, int64 [3] labels)."""
    wave = torch.zeros(len(LENGTHS), max(LENGTHS))
    for b, u in enumerate(utterances()):
        wave[b, :len(u)] = u
    return wave, torch.tensor(LABELS, dtype=torch.long)


def closed_form_state(model):
    """{key: closed-form f32 tensor} for a module's state_dict keys and shapes (what cf.fill_module_ loads)."""
    return {k: (cf.tensor_for(k, tuple(v.shape)) if v.dtype.is_floating_point else v) for k, v in model.state_dict().items()}


def oracle_run(sd, audio_cfg, wave, labels, dtype=torch.float64, backward=True):
    """-> dict(logits, pooled, loss, gradnorm, grads {key: tensor or None}) of the audio-only classifier in `dtype` on the CPU."""
    sdd = {k: v.detach().to(dtype).clone().requires_grad_(backward) for k, v in sd.items() if v.dtype.is_floating_point}
    with torch.set_grad_enabled(backward):
        hidden = O.w2v2_model(sdd, "wav2vec2", audio_cfg, wave.to(dtype))
        pooled = hidden.mean(1)                                               # every frame of the padded batch
        logits = pooled @ sdd["out_proj.weight"].T + sdd["out_proj.bias"]
        loss = torch.nn.functional.cross_entropy(logits, labels)
    out = dict(logits=logits.detach(), pooled=pooled.detach(), loss=loss.item(), frames=hidden.shape[1])
    if backward:
        loss.backward()
        out["grads"] = {k: v.grad for k, v in sdd.items()}
        out["gradnorm"] = torch.sqrt(sum((g.double() ** 2).sum() for g in out["grads"].values() if g is not None)).item()
    return out
