"""Synthetic MELD-shaped batches: the output contract of the reference's collate_batch
(models/tav.py:174-246) without decoding any file.  Seeded torch.Generator, seed = 1234 + rank."""
import torch


def make_batch(cfg, batch_size, *, seed=1234, s_text=128, t_audio=80000, n_visual_true=104, device="cpu", text_only=False, with_video=True):
    """Returns ([text, audio, visual] dicts exactly as collate_batch yields them, labels float [B]).  text_only / with_video=False skip
    the (large) modalities the single- and dual-modal entrypoints do not read (their dicts come back as None).  n_visual_true: True tokens
    per row of the video mask, an int or one count per row (unequal counts: train with runtime.set_visual_rows("ragged"))."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    tc, vc = cfg["text"], cfg["video"]
    B = batch_size
    ids = torch.randint(3, tc["vocab"], (B, s_text), generator=g)
    npad = s_text // 4
    text_mask = torch.ones(B, s_text)
    if npad:
        ids[:, s_text - npad:] = tc["pad_id"]
        text_mask[:, s_text - npad:] = 0
    if text_only:
        labels = torch.randint(0, 7, (B,), generator=g).float()
        return [{"input_ids": ids.to(device), "attention_mask": text_mask.to(device)}, None, None], labels.to(device)
    audio = torch.randn(B, t_audio, generator=g) * 0.1
    audio_mask = torch.ones(B, t_audio)
    cut = int(0.8 * t_audio)
    audio[0, cut:] = 0
    audio_mask[0, cut:] = 0
    if not with_video:
        labels = torch.randint(0, 7, (B,), generator=g).float()
        return [{"input_ids": ids.to(device), "attention_mask": text_mask.to(device)},
                {"audio_features": audio.to(device), "attention_mask": audio_mask.to(device)}, None], labels.to(device)
    video = torch.randn(B, vc["frames"], 3, vc["image"], vc["image"], generator=g)
    ntok = (vc["image"] // vc["patch"]) ** 2 * (vc["frames"] // vc["tubelet"])
    nts = [int(n_visual_true)] * B if isinstance(n_visual_true, int) else [int(n) for n in n_visual_true]
    if len(nts) != B or not all(0 <= n <= ntok for n in nts):
        raise ValueError(f"n_visual_true {n_visual_true!r}: need {B} counts in [0, {ntok}]")
    vmask = torch.zeros(B, ntok, dtype=torch.bool)
    for b in range(B):
        vmask[b, torch.randperm(ntok, generator=g)[:nts[b]]] = True             # exactly n True per row
    labels = torch.randint(0, 7, (B,), generator=g).float()
    text = {"input_ids": ids.to(device), "attention_mask": text_mask.to(device)}
    audio_d = {"audio_features": audio.to(device), "attention_mask": audio_mask.to(device)}
    visual = {"visual_embeds": video.to(device), "attention_mask": vmask.to(device)}
    return [text, audio_d, visual], labels.to(device)


def make_items(cfg, n, *, raw_video=None, seed=1234, s_text=128, t_audio=80000, speakers=None, raw_audio=None):
    """n seeded items in the collate contract, ([{"input_ids", "attention_mask"}, waveform, video], label), with waveforms of unequal length.
    raw_video=None: video is a finished float clip [frames, 3, image, image].  raw_video=(T, H, W): video is what a decoder yields, uint8
    [T, H, W, 3] frames -- for models.tav.collate_batch_device / video_features_device, which transform them on the device.  speakers: one
    entry per item (None, True, False) wraps the frames as {"frames", "speaker"}.  raw_audio=(sampling_rate, channels): the waveform is what
    an audio decoder yields, {"pcm": int16 [L, channels], "sampling_rate"}, L = the float waveform's length (for
    models.tav.collate_batch_device / speech_features_device, which resample it on the device)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    tc, vc = cfg["text"], cfg["video"]
    items = []
    for i in range(n):
        ids = torch.randint(3, tc["vocab"], (s_text,), generator=g)
        text = {"input_ids": ids, "attention_mask": torch.ones(s_text)}
        wave = torch.randn(t_audio - (i * 997) % max(t_audio // 2, 1), generator=g) * 0.1
        if raw_audio is not None:
            pcm = torch.randint(-32768, 32768, (len(wave), raw_audio[1]), generator=g, dtype=torch.int16)
            wave = {"pcm": pcm, "sampling_rate": int(raw_audio[0])}
        if raw_video is None:
            video = torch.randn(vc["frames"], 3, vc["image"], vc["image"], generator=g)
        else:
            T, H, W = raw_video
            video = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8)
            if speakers is not None:
                video = {"frames": video, "speaker": speakers[i]}
        items.append(([text, wave, video], int(torch.randint(0, 7, (1,), generator=g))))
    return items


def seeded_init_(module, seed=0):
    """Re-draw every parameter from a seeded generator with the module's own init scale (std of the current values),
    so the oracle and the product can be given bit-identical random weights without shipping blobs."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(module.named_parameters()):
            std = float(p.detach().float().std().item()) if p.numel() > 1 else 0.0
            mean = float(p.detach().float().mean().item())
            if std == 0.0:                       # constant tensors (biases = 0, LayerNorm weight = 1): keep, add small noise
                std = 0.02
            new = torch.randn(p.shape, generator=g) * std + mean
            if name.endswith("parametrizations.weight.original0"):
                new = new.abs() + 0.5
            p.copy_(new.to(p.device))
    return module
