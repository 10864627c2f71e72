"""Drop-in for the reference's SingleModels/models/audio.py: Wav2Vec2ForSpeechClassification (:41-62) and collate_batch (:20-38), the
audio-only row of the ablation set.

    logits = out_proj(dropout(mean_t(wav2vec2(input_values)[0])))            out_proj: hidden -> output_dim

on libtavhip: encoders.AudioEncoder (the whole wav2vec2 forward and backward in HIP), engine.MeanPoolFn over the Sa frames of the f32
stream, engine.HeadFn (dropout + Linear).  state_dict keys are the reference's: wav2vec2.* (HF names), out_proj.weight, out_proj.bias.

Padding semantics (kept from the reference): the batch is zero-padded to its longest utterance, no attention mask is passed, and the mean
runs over ALL Sa frames of the padded batch, padding frames included.  With the GroupNorm feature extractor (wav2vec2-base, preset B)
the first conv layer normalises over the whole padded time axis, so a row's logits depend on the batch's padded length -- on which other
utterances it was batched with.  Dropout follows self.training; the reference never calls .eval() on this module, so its loops validate
and test with dropout on (train_model/audio_training.py keeps that).  SpecAugment, which HF applies inside Wav2Vec2Model in training
mode when the checkpoint's config asks for it, is not applied: AudioEncoder.forward is the encoder without it.

The one deviation: the reference loads a wav2vec2-base checkpoint and hard-codes Linear(768, output_dim).  config=None therefore means
the audio block of config.preset("B"), whatever the process-wide default preset is; with an explicit `config`, out_proj takes
config["audio"]["hidden"] inputs (1024 for a large encoder), where the reference's 768 would not fit the encoder's output.

The reference's collate_batch decodes and resamples each file with torchaudio; decoding files is outside this package.  collate_batch
takes finished 16 kHz waveforms (the host contract), collate_batch_device also decoded PCM, resampled on the device."""
import numpy as np
import torch
from torch import nn
from torch.nn.utils.rnn import pad_sequence

from ... import config as C
from ... import engine as E
from ... import runtime
from ...encoders import AudioEncoder
from ...models.tav import _decoded_audio, _dev, _pcm_tensor, _resampled_length_checked, speech_features_device


def _no_paths(speech):
    if isinstance(speech, (str, bytes)) or hasattr(speech, "__fspath__"):
        raise ValueError(f"collate_batch: got the path {speech!r}; decoding audio files is outside this package -- pass the decoded waveform "
                         "(a 1-D float tensor at 16 kHz), or decoded PCM as {'pcm', 'sampling_rate'} to collate_batch_device")


def collate_batch(batch):
    """[(speech, label)] with speech a 1-D float waveform at 16 kHz -> (f32 [B, Tmax] zero-padded, labels float [B]) (reference :36-38)."""
    speech_list, label_list = [], []
    for (speech, label) in batch:
        _no_paths(speech)
        if _decoded_audio(speech) is not None:
            raise ValueError("collate_batch takes finished 16 kHz waveforms: decoded PCM is resampled by the HIP kernel only "
                             "(there is no CPU fallback) -- use collate_batch_device")
        speech_list.append(torch.as_tensor(speech).float().reshape(-1))
        label_list.append(label)
    return pad_sequence(speech_list, batch_first=True), torch.Tensor(np.array(label_list))


def collate_batch_device(batch, device="cuda"):
    """[(speech, label)] -> (f32 [B, Tmax] on the device, labels float [B] on the device).  speech: a 1-D waveform at 16 kHz (any float
    type, host or device) or decoded PCM {"pcm": int16 or float [L] / [C, L] / [L, C], "sampling_rate": int}.  Every utterance goes through
    speech_features_device into its row of a zero-initialised batch (one resampler launch per row: resample, channel mean, zero tail);
    Tmax, the longest resampled length, is known on the host, and the samples never come back to it."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"collate_batch_device(device={str(dev)!r}): the waveform transform is a HIP kernel on the GPU only; there is no CPU fallback")
    items, labels = [], []
    for (speech, label) in batch:
        _no_paths(speech)
        decoded = _decoded_audio(speech)
        pcm, sr = decoded if decoded is not None else (speech, 16000)
        pcm = _pcm_tensor(pcm)
        if decoded is None and pcm.dim() != 1:
            raise ValueError(f"collate_batch_device: a finished waveform is 1-D, got {tuple(pcm.shape)}; wrap decoded PCM as {{'pcm', 'sampling_rate'}}")
        items.append((pcm, sr))
        labels.append(float(label))
    T = max(_resampled_length_checked(p, sr, 16000)[1] for (p, sr) in items)
    audio = torch.zeros(len(items), T, dtype=torch.float32, device=_dev(dev))
    for b, (p, sr) in enumerate(items):
        speech_features_device(p, sr, out=audio[b], device=audio.device)
    return audio, torch.tensor(labels, dtype=torch.float32).to(audio.device, non_blocking=True)


class Wav2Vec2ForSpeechClassification(nn.Module):
    def __init__(self, args, dropout=.5, config=None):
        super().__init__()
        cfg = config if config is not None else C.preset("B")            # the reference's checkpoint is a wav2vec2-base (module docstring)
        self.cfg = cfg
        self.output_dim = args["output_dim"]
        self.dropout_p = float(dropout)
        self.wav2vec2 = AudioEncoder(cfg["audio"])
        self.out_proj = nn.Linear(cfg["audio"]["hidden"], self.output_dim)
        self._drop_calls = 0

    def forward(self, input_values):
        dev = self.out_proj.weight.device
        if dev.type != "cuda":
            raise RuntimeError("Wav2Vec2ForSpeechClassification runs on libtavhip (GPU) only; there is no CPU fallback")
        if input_values.dim() != 2:
            raise ValueError(f"Wav2Vec2ForSpeechClassification: expected waveforms [B, T], got {tuple(input_values.shape)}")
        wave = input_values.to(dev, torch.float32).contiguous()
        B = wave.shape[0]
        x, _, Sa = self.wav2vec2(wave)                                     # reference :55
        pooled = E.MeanPoolFn.apply(x, B, Sa)                              # :57, over all Sa frames of the padded batch
        p = self.dropout_p if self.training else 0.0
        seed, = runtime.dropout_seeds(self, "_drop_calls", draw=p > 0.0)
        return E.HeadFn.apply(pooled, p, seed, self.out_proj.weight, self.out_proj.bias)   # :59-60
