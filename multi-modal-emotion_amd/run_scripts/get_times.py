"""Utterance times by CTC forced alignment on the device (reference run_scripts/get_times.py).

The reference's names and signatures -- Point, Segment, get_trellis, backtrack, merge_repeats, get_times -- on tav_ctc_log_softmax and
tav_ctc_align (csrc/ctc_align.hip), plus align_batch for a whole batch in one align launch.  Where this file deviates (INTEGRATION.md,
"Utterance times"):
  * get_times takes the decoded waveform [C, L] at the model's rate where the reference takes a file path (decoding is not part of this
    package; models.tav.speech_features_device resamples).  Like the reference it aligns channel 0.
  * The trellis is a pure function of emission and tokens and the kernel forms it together with the path, so backtrack(trellis, emission,
    tokens) checks the shape of the trellis it is handed and recomputes; it does not read its values.
  * A step that stayed takes its probability from column `blank_id`; the reference reads column literal 0 (its only caller has blank 0).
  * merge_repeats in the reference cannot terminate (its outer loop never advances as the file is indented).  Here it is the evident
    intent: group consecutive equal token_index, score = mean, return the first start and the last end in seconds.
"""
from dataclasses import dataclass

import torch

from .. import ops

# torchaudio.pipelines.WAV2VEC2_ASR_BASE_960H.get_labels(): the blank first, then the word boundary and the letters by frequency
LABELS = ("-", "|", "E", "T", "A", "O", "N", "I", "H", "S", "R", "D", "L", "U", "M", "W", "C", "F", "G", "Y", "P", "B", "V", "K", "'", "X", "J", "Q", "Z")
SAMPLE_RATE = 16000


@dataclass
class Point:
    token_index: int
    time_index: int
    score: float


@dataclass
class Segment:
    label: str
    start: int
    end: int
    score: float

    def __repr__(self):
        return f"{self.label}\t({self.score:4.2f}): [{self.start:5d}, {self.end:5d})"

    @property
    def length(self):
        return self.end - self.start


def _device_problem(emission, tokens):
    """(emission [1, T, V] f32 on the device, tokens [1, N] i32, n_frames [1], n_tokens [1])."""
    if not isinstance(emission, torch.Tensor) or emission.dim() != 2:
        raise ValueError("emission must be a [frames, labels] tensor")
    dev = emission.device if emission.is_cuda else torch.device("cuda")
    em = emission.detach().to(device=dev, dtype=torch.float32)
    if em.stride(-1) != 1 or em.stride(0) % 4 or em.stride(0) < em.shape[1]:      # the kernel wants a row pitch of whole 16 bytes
        padded = torch.zeros(em.shape[0], (em.shape[1] + 3) // 4 * 4, dtype=torch.float32, device=dev)
        padded[:, :em.shape[1]].copy_(em)
        em = padded[:, :em.shape[1]]
    tok = torch.as_tensor(list(tokens) if not isinstance(tokens, torch.Tensor) else tokens, dtype=torch.int32).reshape(1, -1).to(dev)
    if tok.shape[1] == 0:
        tok = torch.zeros(1, 1, dtype=torch.int32, device=dev)
        n_tok = 0
    else:
        n_tok = tok.shape[1]
    n_frames = torch.tensor([em.shape[0]], dtype=torch.int32, device=dev)
    n_tokens = torch.tensor([n_tok], dtype=torch.int32, device=dev)
    return em.unsqueeze(0), tok.contiguous(), n_frames, n_tokens, n_tok


def get_trellis(emission, tokens, blank_id=0):
    """[T + 1, N + 1] f32 on the emission's device (the reference builds it on the host with T torch ops)."""
    em, tok, n_frames, n_tokens, n = _device_problem(emission, tokens)
    out = ops.ctc_align(em, tok, n_frames, n_tokens, blank_id=blank_id, want_trellis=True)
    return out.trellis[0, :, :n + 1]


def _points(path_token, path_prob, span):
    """Host lists -> [Point]; raises the reference's error for a failed row."""
    if span[3] & 1:
        raise ValueError("Failed to align")
    return [Point(path_token[t], t, path_prob[t]) for t in range(span[0], span[1])]


def backtrack(trellis, emission, tokens, blank_id=0):
    """The path as [Point] in ascending frame order.  The trellis is only checked for its shape (see the module docstring)."""
    n = len(tokens)
    if tuple(trellis.shape) != (emission.shape[0] + 1, n + 1):
        raise ValueError(f"trellis {tuple(trellis.shape)} does not belong to {emission.shape[0]} frames and {n} tokens")
    em, tok, n_frames, n_tokens, _ = _device_problem(emission, tokens)
    out = ops.ctc_align(em, tok, n_frames, n_tokens, blank_id=blank_id)
    return _points(out.path_token[0].tolist(), out.path_prob[0].tolist(), out.span[0].tolist())


def merge_repeats(path, ratio, transcript, sr):
    """Consecutive points of one token become a Segment (score = mean); -> (start, end) in seconds of the first and the last segment."""
    i1, i2 = 0, 0
    segments = []
    while i1 < len(path):
        while i2 < len(path) and path[i1].token_index == path[i2].token_index:
            i2 += 1
        score = sum(path[k].score for k in range(i1, i2)) / (i2 - i1)
        segments.append(Segment(transcript[path[i1].token_index], path[i1].time_index, path[i2 - 1].time_index + 1, score))
        i1 = i2
    return (segments[0].start * ratio) / sr, (segments[-1].end * ratio) / sr


def transcript_tokens(text, labels):
    """The reference's transcript handling: upper(), space -> '|'; a character outside `labels` is a KeyError."""
    dictionary = {c: i for i, c in enumerate(labels)}
    transcript = text.upper().replace(" ", "|")
    return transcript, [dictionary[c] for c in transcript]


def get_times(wave, text, model, labels=LABELS, sample_rate=SAMPLE_RATE):
    """(start, end) seconds of `text` inside the decoded waveform `wave` [C, L] (or [L]) at the model's rate, aligned on channel 0."""
    waveform = torch.as_tensor(wave)
    if waveform.dim() == 1:
        waveform = waveform[None]
    with torch.inference_mode():
        logits, _ = model(waveform.to("cuda", torch.float32))
        B, T, V = logits.shape
        rows = torch.empty(B, T, (V + 3) // 4 * 4, dtype=torch.float32, device=logits.device)
        emissions = ops.ctc_log_softmax(logits, out=rows[..., :V])
    emission = emissions[0]
    transcript, tokens = transcript_tokens(text, labels)
    trellis = get_trellis(emission, tokens)
    path = backtrack(trellis, emission, tokens)
    ratio = waveform[0].size(0) / (trellis.size(0) - 1)
    return merge_repeats(path, ratio, transcript, sample_rate)


def align_batch(waves, texts, model, labels=LABELS, sample_rate=SAMPLE_RATE):
    """1-D device waveforms at the model's rate (what speech_features_device returns) and their transcripts -> (times [B, 2] float64
    seconds on the host, status [B] int32 on the host).  Every utterance's emission is computed as a batch of one into its rows of one
    padded buffer (a batch would let GroupNorm over time see the padding), then ONE align launch covers the batch.  Nothing is read back
    before the status words are; a row that failed raises ValueError('Failed to align') there, with the other rows' results attached as
    `.times` and `.status`."""
    B = len(waves)
    if B == 0 or len(texts) != B:
        raise ValueError("align_batch: one transcript per waveform")
    toks = [transcript_tokens(t, labels)[1] for t in texts]
    conv_len = model.wav2vec2.conv_out_len
    frames = [conv_len(int(w.shape[-1])) for w in waves]
    Tmax, Nmax, Vp = max(frames), max(1, max(len(t) for t in toks)), model.vocab_padded
    dev = waves[0].device
    emission = torch.zeros(B, Tmax, Vp, dtype=torch.float32, device=dev)
    for b, w in enumerate(waves):
        if w.dim() != 1 or not w.is_cuda:
            raise ValueError("align_batch takes 1-D waveforms on the device")
        model.emission(w[None].to(torch.float32), out=emission[b:b + 1, :frames[b]])
    tok = torch.zeros(B, Nmax, dtype=torch.int32)
    for b, t in enumerate(toks):
        tok[b, :len(t)] = torch.tensor(t, dtype=torch.int32)
    n_frames = torch.tensor(frames, dtype=torch.int32)
    n_tokens = torch.tensor([len(t) for t in toks], dtype=torch.int32)
    out = ops.ctc_align(emission, tok.to(dev), n_frames.to(dev), n_tokens.to(dev), V=model.vocab)
    span = out.span.cpu()                                  # the one read: frames and status together
    times = torch.full((B, 2), float("nan"), dtype=torch.float64)
    for b in range(B):
        if not int(span[b, 3]) & 1:
            ratio = int(waves[b].shape[-1]) / frames[b]
            times[b, 0] = (int(span[b, 0]) * ratio) / sample_rate
            times[b, 1] = (int(span[b, 1]) * ratio) / sample_rate
    status = span[:, 3].clone()
    if bool((status & 1).any()):
        err = ValueError("Failed to align")
        err.times, err.status = times, status
        raise err
    return times, status
