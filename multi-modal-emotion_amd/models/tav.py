"""Drop-in for the reference's models/tav.py model classes, executed by libtavhip on MI355X.

  PreFormer   reference models/tav.py:249-417   modality front-ends -> fused token sequence + masks
  TAVForMAE   reference models/tav.py:420-504   3 encoders + fusion encoder + 7-way head
  collate_batch  reference models/tav.py:174-246   (mask / pad logic only: file decoding is out of scope)
  video_features_device  reference models/tav.py:51-121   decoded uint8 frames -> the normalised, resized clip, one HIP launch per clip
  speech_features_device reference models/tav.py:165-169  decoded PCM -> the mono 16 kHz waveform, one HIP launch per utterance

Same constructor arguments, forward() signatures and state_dict keys.  `from_pretrained` checkpoints are not
reachable offline, so sub-models are built from a geometry preset (config.py) and initialised randomly; load a
reference `best.pt` with `load_state_dict(remap_reference_keys(sd))`.
The reference keeps PreFormer on the CPU and ships activations back and forth (models/tav.py:352,359,363); here every
tensor stays resident in HBM: inputs given on the CPU are moved to the GPU once, outputs are returned on the GPU
(the reference's `.to(device)` calls in tav_train.py:39-40 then cost nothing).
"""
import numpy as np
import torch
from torch import nn

from .. import config as C
from .. import engine as E
from .. import ops, runtime
from ..encoders import AudioEncoder, TextEncoder, VideoEncoder
from ..utils.TAVFormer import VideoMAEEncoder

FP16_MIN = float(torch.finfo(torch.float16).min)


def _dev(device):
    d = torch.device(device if device is not None else "cuda")
    if d.type != "cuda":
        d = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else d
    if d.type != "cuda":
        raise RuntimeError("the TAV hot path runs on libtavhip (HIP, MI355X) only: no GPU is visible and there is no CPU fallback")
    return d


def visual_true_counts(visual_mask, n_visual_true=None):
    """Per-row number of True entries of visual_mask (the tokens the fusion stack sees) as a host list, or an int when every row has the
    same count.  n_visual_true: an int, a per-row sequence, or None (ragged mode: one host read of the B counts; equal mode: None back,
    the video encoder counts and checks as it always did).  In equal mode unequal per-row counts are an error."""
    B = visual_mask.shape[0]
    if n_visual_true is None:
        if runtime.visual_rows() != "ragged":
            return None
        n_visual_true = visual_mask.sum(1).cpu().tolist()
    if isinstance(n_visual_true, (int, np.integer)):
        return int(n_visual_true)
    counts = [int(c) for c in (n_visual_true.tolist() if torch.is_tensor(n_visual_true) else n_visual_true)]
    if len(counts) != B:
        raise ValueError(f"n_visual_true has {len(counts)} entries for a batch of {B}")
    if all(c == counts[0] for c in counts):
        return counts[0]
    if runtime.visual_rows() != "ragged":
        raise ValueError(f"visual mask keeps {counts} True tokens per row; every row must keep the same number "
                         "(runtime.set_visual_rows('ragged') trains on unequal rows)")
    return counts


def visual_row_counts(visual_mask, n_visual_true=None):
    """The per-row True counts of visual_mask as a host list of B ints: from n_visual_true (an int, a sequence or a tensor) when given,
    else one host read of the B counts."""
    B = visual_mask.shape[0]
    if n_visual_true is None:
        return [int(c) for c in visual_mask.sum(1).cpu().tolist()]
    if isinstance(n_visual_true, (int, np.integer)):
        return [int(n_visual_true)] * B
    counts = [int(c) for c in (n_visual_true.tolist() if torch.is_tensor(n_visual_true) else n_visual_true)]
    if len(counts) != B:
        raise ValueError(f"n_visual_true has {len(counts)} entries for a batch of {B}")
    return counts


def resolve_visual_caps(visual_mask, n_visual_true=None, caps=None):
    """(cap_true, cap_keep) when the batch runs at a bucketed capacity (runtime.set_visual_rows("ragged", bucket=g), or `caps` given by the
    caller, e.g. a captured step), else None.  With a bucket EVERY batch takes the padded path, equal rows included: the shapes then depend
    on the bucket alone."""
    ntok = visual_mask.shape[1]
    if caps is None:
        g = runtime.visual_bucket()
        if not g:
            return None
        return runtime.visual_capacities(visual_row_counts(visual_mask, n_visual_true), ntok, g)
    cap_true, cap_keep = (int(c) for c in caps)
    if not (0 < cap_true <= ntok and 0 < cap_keep <= ntok):
        raise ValueError(f"visual capacities {(cap_true, cap_keep)} must lie in [1, {ntok}]")
    return cap_true, cap_keep


STATUS_TEXT = {1: "a row keeps more True video tokens than the fusion rows were sized for (cap_true)",
               2: "a row keeps more visible tokens than the video encoder's rows were sized for (cap_keep), or no True token at all"}


class PreFormer(nn.Module):
    """Modality front-ends (reference models/tav.py:249-417)."""

    def __init__(self, config=None):
        super().__init__()
        cfg = config if config is not None else C.default_config()
        self.cfg = cfg
        Ha = cfg["audio"]["hidden"]
        self.bert = TextEncoder(cfg["text"])
        self.wav2vec2 = AudioEncoder(cfg["audio"])
        self.masked_spec_embed = nn.Parameter(torch.FloatTensor(Ha).uniform_())
        self.videomae = VideoEncoder(cfg["video"])
        self.wav_2_768 = nn.Linear(Ha, 768)
        nn.init.xavier_normal_(self.wav_2_768.weight)
        if cfg["video"]["hidden"] != 768:                   # BASELINE config 5 (videomae-large): the bridge the audio branch already has
            self.vid_2_768 = nn.Linear(cfg["video"]["hidden"], 768)
            nn.init.xavier_normal_(self.vid_2_768.weight)
        self.check_shapes = 1
        self._spec_calls = 0             # SpecAugment draws taken in "device" mode (runtime.dropout_seeds)

    # -- reference helpers, same names (models/tav.py:308-342) --
    def _get_feat_extract_output_lengths(self, input_lengths, add_adapter=None):
        for k, s in zip(self.cfg["audio"]["conv_kernel"], self.cfg["audio"]["conv_stride"]):
            input_lengths = torch.div(input_lengths - k, s, rounding_mode="floor") + 1
        return input_lengths

    def _get_feature_vector_attention_mask(self, feature_vector_length, attention_mask, add_adapter=None):
        non_padded = attention_mask.sum(dim=-1)          # == cumsum(-1)[:, -1] of the reference (:329) without a scan kernel
        out_len = self._get_feat_extract_output_lengths(non_padded).to(torch.long)
        # same result as the reference's "set index out_len-1, flip, cumsum, flip" (:337-341) without an index_put, which
        # synchronises the host and cannot be captured into a hipGraph
        return torch.arange(feature_vector_length, device=attention_mask.device)[None, :] < out_len[:, None]

    @staticmethod
    def _span_mask(B, L, lens, prob, length, min_masks, dev):
        """bool [B, L]: per row n spans of `length` positions, n = max(int(prob * len / length + eps), min_masks) with ONE eps ~ U[0,1) per call,
        starts drawn without replacement from the row's valid range [0, len - length] -- HF `_compute_mask_indices` (wav2vec2:101), the
        reference's sampler (models/tav.py:283-289, :296-301), drawn with torch ops on the device (no host read: capturable).  The number of spans a
        row can take is bounded by the static L; surplus slots are switched off by comparison instead of by shape."""
        eps = torch.rand(1, device=dev).expand(B)
        n = torch.clamp((prob * lens / length + eps).floor(), min=float(min_masks))
        n = torch.minimum(n, torch.clamp((lens - (length - 1)).floor(), min=0.0))           # never more spans than start positions
        n = torch.minimum(n, torch.full_like(n, float(L // length)))
        max_spans = max(int(min_masks), int(prob * L / length + 1.0), 1)                     # static bound (eps < 1)
        pos = torch.arange(L, device=dev)[None, :]
        score = torch.rand(B, L, device=dev)
        score = torch.where(pos < (lens[:, None] - (length - 1)), score, torch.full_like(score, 2.0))   # starts outside the valid range sort last
        starts = score.argsort(dim=1)[:, :max_spans]                                          # without replacement
        live = torch.arange(max_spans, device=dev)[None, :] < n[:, None]
        cover = (pos[:, None, :] >= starts[:, :, None]) & (pos[:, None, :] < starts[:, :, None] + length) & live[:, :, None]
        return cover.any(dim=1)

    def _mask_hidden_states(self, hidden, B, T, attention_mask, training=False):
        """SpecAugment (reference models/tav.py:269-306).  Along TIME (:281-290): spans of mask_time_length frames inside each row's valid range are
        replaced by `masked_spec_embed`; along the FEATURE axis (:292-304, round 4): spans of mask_feature_length channels are zeroed for every
        frame of the row -- inactive under the Wav2Vec2Config default mask_feature_prob = 0, which is what the reference's checkpoint carries.
        The reference samples on the host with numpy; here the same distribution is drawn ON THE DEVICE (`_span_mask`), so a training step with
        train=True stays graph-capturable.  Only active when train=True, which is outside the parity / benchmark configuration."""
        ac = self.cfg["audio"] if hasattr(self, "cfg") else {}
        mask_prob, mask_len, min_masks = ac.get("mask_time_prob", 0.05), ac.get("mask_time_length", 10), ac.get("mask_time_min_masks", 2)   # Wav2Vec2Config defaults; min_masks as the reference passes it
        f_prob, f_len, f_min = ac.get("mask_feature_prob", 0.0), ac.get("mask_feature_length", 10), ac.get("mask_feature_min_masks", 0)
        if not training or T < mask_len:                                                       # (:277-278)
            return hidden
        if runtime.specaugment() != "torch":
            return self._mask_hidden_states_kernels(hidden, B, T, attention_mask)
        dev = hidden.device
        if mask_prob > 0:
            if attention_mask is not None:
                lens = attention_mask.to(dev).sum(-1).to(torch.float32)                       # frames that are not padding, per row
            else:
                lens = torch.full((B,), float(T), device=dev)
            sel = self._span_mask(B, T, lens, mask_prob, mask_len, min_masks, dev).reshape(B * T, 1)
            hidden = torch.where(sel, self.masked_spec_embed.to(hidden.dtype)[None, :], hidden)
        if f_prob > 0:
            Hh = hidden.shape[1]
            fsel = self._span_mask(B, Hh, torch.full((B,), float(Hh), device=dev), f_prob, f_len, f_min, dev)      # [B, H]: no attention mask on this axis (:296-301)
            hidden = torch.where(fsel[:, None, :].expand(B, T, Hh).reshape(B * T, Hh), torch.zeros((), dtype=hidden.dtype, device=dev), hidden)
        return hidden

    def _spec_cfg(self):
        """(time, feature) x (prob, length, min_masks): the keys and Wav2Vec2Config defaults _mask_hidden_states reads."""
        ac = self.cfg["audio"] if hasattr(self, "cfg") else {}
        return ((ac.get("mask_time_prob", 0.05), ac.get("mask_time_length", 10), ac.get("mask_time_min_masks", 2)),
                (ac.get("mask_feature_prob", 0.0), ac.get("mask_feature_length", 10), ac.get("mask_feature_min_masks", 0)))

    def reference_spec_masks(self, B, T, H, attention_mask=None):
        """The masks the reference draws (models/tav.py:283-301): HF `_compute_mask_indices` on the host, from numpy's global generator, with the
        reference's arguments in the reference's order -- the time axis first, with the frame attention mask and min_masks = mask_time_min_masks,
        then the feature axis without a mask.  -> (bool [B, T] or None, bool [B, H] or None), CPU tensors; an axis whose probability is 0 is
        None and consumes no numpy draw.  Pure host code: runs without a GPU."""
        from transformers.models.wav2vec2.modeling_wav2vec2 import _compute_mask_indices
        (t_prob, t_len, t_min), (f_prob, f_len, f_min) = self._spec_cfg()
        tmask = fmask = None
        if T < t_len:                                                                          # (:277-278)
            return None, None
        if t_prob > 0:
            am = attention_mask.detach().to("cpu", torch.long) if attention_mask is not None else None
            tmask = torch.from_numpy(_compute_mask_indices((B, T), mask_prob=t_prob, mask_length=t_len, attention_mask=am, min_masks=t_min))
        if f_prob > 0:
            fmask = torch.from_numpy(_compute_mask_indices((B, H), mask_prob=f_prob, mask_length=f_len, min_masks=f_min))
        return tmask, fmask

    def _mask_hidden_states_kernels(self, hidden, B, T, attention_mask):
        """SpecAugment through libtavhip (runtime.specaugment() "device" / "reference"): the masks come from tav_specaug_draw on this module's
        seed stream, or from the host as the reference draws them; engine.SpecAugFn applies them and owns the backward (dx, and the gradient
        of masked_spec_embed)."""
        (t_prob, t_len, t_min), (f_prob, f_len, f_min) = self._spec_cfg()
        if t_prob <= 0 and f_prob <= 0:
            return hidden
        H = hidden.shape[1]
        if runtime.specaugment() == "reference":
            if runtime.capture_active():
                raise RuntimeError('SpecAugment mode "reference" draws its masks on the host (numpy, HF _compute_mask_indices) and cannot be '
                                   'captured into a hipGraph; use runtime.set_specaugment("device") or run the step eagerly')
            tmask, fmask = self.reference_spec_masks(B, T, H, attention_mask)
            tmask = tmask.to(hidden.device) if tmask is not None else None
            fmask = fmask.to(hidden.device) if fmask is not None else None
        else:
            # one seed per forward that draws, for both axes (their tags keep the two streams apart); a device word under a capture
            seed, = runtime.dropout_seeds(self, "_spec_calls", 1)
            tmask = fmask = None
            if t_prob > 0:
                valid = attention_mask.to(hidden.device) if attention_mask is not None else None
                tmask = ops.specaug_draw(valid, B, T, t_prob, t_len, t_min, seed, ops.SPECAUG_TAG_TIME, device=hidden.device)
            if f_prob > 0:
                fmask = ops.specaug_draw(None, B, H, f_prob, f_len, f_min, seed, ops.SPECAUG_TAG_FEATURE, device=hidden.device)
        return E.SpecAugFn.apply(hidden, self.masked_spec_embed, tmask, fmask, B, T)

    def forward(self, input_ids=None, audio_features=None, video_embeds=None, text_mask=None, audio_mask=None, visual_mask=None,
                device="cpu", train=False, n_visual_true=None, visual_caps=None):
        """n_visual_true (optional): number of True entries per row of visual_mask (an int, or per row in ragged mode); passing it avoids one
        host sync.  Ragged mode with unequal rows: the video segment (last) is max_b n_true_b tokens long, padded at the end of each row
        (tav_embed 2, attention_mask 0 there).  With a bucket (runtime.set_visual_rows("ragged", bucket=g)) or explicit
        visual_caps = (cap_true, cap_keep) the segment is cap_true tokens long whatever the rows hold; nothing is read from the host when
        the capacities are given."""
        dev = _dev(device if str(device) != "cpu" else None)
        ectx = runtime.ctx()
        if audio_features.is_cuda:
            runtime.mark_inputs_ready()
        B = audio_features.shape[0]
        parts = []
        St = 0
        audio_features, video_embeds, visual_mask = audio_features.to(dev, torch.float32), video_embeds.to(dev, torch.float32), visual_mask.to(dev)
        caps = resolve_visual_caps(visual_mask, n_visual_true, visual_caps)
        nt = visual_true_counts(visual_mask, n_visual_true) if caps is None else None
        ragged = caps is not None or isinstance(nt, list)
        Sa = self.wav2vec2.conv_out_len(audio_features.shape[1])
        if audio_mask is not None:
            audio_mask = self._get_feature_vector_attention_mask(Sa, audio_mask.to(dev))     # :355 bool [B, Sa]

        def video_frontend():
            if ragged:
                xv, nv, _ = self.videomae.embed(video_embeds, ~visual_mask, caps[0] if caps is not None else max(nt), ragged=True)
            else:
                xv, nv = self.videomae.embed(video_embeds, ~visual_mask, nt)          # :368
            if hasattr(self, "vid_2_768"):
                xv = E.LinearFn.apply(xv, None, self.vid_2_768.weight, self.vid_2_768.bias, None, ectx, True)
            return xv, nv

        def audio_frontend():
            feats = self.wav2vec2.feature_extractor_fwd(audio_features)                 # :352  [B, Sa, 512]
            hidden = self.wav2vec2.feature_projection_fwd(feats)                        # :356  f32 [B*Sa, Ha]
            hidden = self._mask_hidden_states(hidden, B, Sa, audio_mask, train)         # :359
            hidden = self.wav2vec2.pos_conv_fwd(hidden, B, Sa)                          # :360
            enc = self.wav2vec2.encoder
            hidden, hidden_lp = E.layer_norm_f32(ectx, hidden, enc.layer_norm.weight, enc.layer_norm.bias, self.cfg["audio"]["eps"])   # :361
            return E.LinearFn.apply(hidden, hidden_lp if not ectx.pol.f32 else None, self.wav_2_768.weight, self.wav_2_768.bias, None, ectx, True)   # :363

        if input_ids is not None:
            input_ids = input_ids.to(dev)
            x_text, _ = self.bert.embed(input_ids)                                      # :349
            St = input_ids.shape[1]
            parts.append(x_text)
        x_audio = audio_frontend()
        x_video, Nv = video_frontend()
        parts += [x_audio, x_video]
        tav = E.ConcatSeqFn.apply(B, *parts)                                            # :372-375

        # static modality ids and masks (:378-409) -- tiny host-logic tensors
        pos = [torch.zeros((B, St), device=dev)] if input_ids is not None else []
        pos += [torch.ones((B, Sa), device=dev), torch.ones((B, Nv), device=dev) + 1]
        tav_embed = torch.concat(pos, dim=1).type(torch.long)
        masks = []
        if input_ids is not None and text_mask is not None:
            masks.append((1.0 - text_mask.to(dev)[:, None, None, :]) * FP16_MIN)        # :383
        if audio_mask is not None:
            masks.append(1.0 - audio_mask[:, None, None, :] * FP16_MIN)                 # :390 (precedence as written)
        masks.append(torch.zeros((B, 1, 1, Nv), device=dev, dtype=torch.float))         # :397
        attention_mask = torch.concat(masks, dim=-1)                                    # :409
        if self.check_shapes == 1:
            self.check_shapes += 1
            print(f"Text shape is {(B, St, 768)}\nAudio shape is {(B, Sa, 768)}\nVideo shape is {(B, Nv, 768)}\n", flush=True)
        return tav, tav_embed, attention_mask


class TAVForMAE(nn.Module):
    """Tri-modal classifier (reference models/tav.py:420-504)."""

    def __init__(self, args, config=None):
        super().__init__()
        cfg = config if config is not None else C.default_config()
        self.cfg = cfg
        self.output_dim = args["output_dim"]
        self.dropout_p = float(args["dropout"])
        self.learn_PosEmbeddings = args["learn_PosEmbeddings"]
        self.num_layers = args["num_layers"]            # stored, unused: the fusion depth is fixed (reference :430,442)
        Ha = cfg["audio"]["hidden"]
        self.test_ctr = 1
        self.train_ctr = 1
        self.embedding = nn.Embedding(3, 768)
        self.embedding.weight.requires_grad = bool(self.learn_PosEmbeddings)
        self.bert = TextEncoder(cfg["text"])
        self.bert_norm = nn.LayerNorm(768)
        self.random_mae_config = dict(cfg["fusion"])
        self.random_mae_encoder = VideoMAEEncoder(self.random_mae_config, cfg["fusion"]["layers"]).apply(self.randomize_model)
        self.rand_norm = nn.LayerNorm(768)
        self.vid_norm = nn.LayerNorm(768)
        self.aud_norm = nn.LayerNorm(768)
        self.linear1 = nn.Linear(768 * 4, self.output_dim)
        self.wav2vec2 = AudioEncoder(cfg["audio"])
        self.videomae = VideoEncoder(cfg["video"])
        self.wav_2_768_2 = nn.Linear(Ha, 768)
        nn.init.xavier_normal_(self.wav_2_768_2.weight)
        if cfg["video"]["hidden"] != 768:
            self.vid_2_768_2 = nn.Linear(cfg["video"]["hidden"], 768)
            nn.init.xavier_normal_(self.vid_2_768_2.weight)
        self._drop_calls = 0
        self._visual_status = None       # status word of the last forward at a capacity (check_visual_status)

    def randomize_model(self, model):
        """reference :461-471: xavier_uniform Linear/Embedding weights, zero biases, LayerNorm weight = 1 / bias = 0."""
        for _, m in model.named_modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.xavier_uniform_(m.weight)
            elif isinstance(m, nn.LayerNorm):
                m.bias.data.zero_()
                m.weight.data.fill_(1.0)
            if isinstance(m, nn.Linear) and m.bias is not None:
                m.bias.data.zero_()
        return model

    def check_visual_status(self):
        """The status word of the last forward at a capacity, read from the device (a host sync: call it where the step synchronises anyway,
        e.g. next to loss.item()).  Non-zero -> ValueError: a row of the batch did not fit the capacities the shapes were built for.  The
        kernels clamped every index and length, so nothing was read or written out of bounds, but that row's result is not what the model
        computes for it."""
        status, self._visual_status = getattr(self, "_visual_status", None), None
        if status is None:
            return
        word = int(status.item())
        if word:
            why = "; ".join(text for bit, text in STATUS_TEXT.items() if word & bit)
            raise ValueError(f"ragged video rows exceed the batch's capacity (status {word}): {why}")

    def forward(self, input_ids, text_attention_mask, audio_features, video_embeds, visual_mask, hidden_states, pos_embed, attention_mask,
                batch_size=2, check="train", n_visual_true=None, visual_caps=None):
        """visual_caps (optional) = (cap_true, cap_keep), as given to PreFormer.forward: the fusion rows hold cap_true video slots and the video
        encoder runs rows of cap_keep tokens; the per-row lengths come from the mask on the device (ops.ragged_lens) and a row that does
        not fit is reported by check_visual_status() at the caller's next sync."""
        dev = _dev(hidden_states.device if hidden_states.is_cuda else None)
        B, Sf, _ = hidden_states.shape
        ectx = runtime.ctx()
        audio_features, video_embeds = audio_features.to(dev, torch.float32), video_embeds.to(dev, torch.float32)
        visual_mask, input_ids, text_attention_mask = visual_mask.to(dev), input_ids.to(dev), text_attention_mask.to(dev)
        caps = resolve_visual_caps(visual_mask, n_visual_true, visual_caps)
        nt = visual_true_counts(visual_mask, n_visual_true) if caps is None else None
        ragged = caps is not None or isinstance(nt, list)     # (without a bucket, equal rows take the equal path, bit for bit)
        ntok = visual_mask.shape[1]
        vid_lens = av_lens = lens_ready = None
        self._visual_status = None
        if caps is not None:
            nkeep = caps[1]
            if Sf < caps[0]:
                raise ValueError(f"hidden_states has {Sf} tokens per row, fewer than the video segment's capacity {caps[0]}")
            visual_mask = visual_mask.contiguous()
        else:
            nkeep = None if nt is None else ntok - (min(nt) if ragged else nt)
            if ragged:
                # fusion rows: St + Sa + n_true_b valid tokens of Sf (the video segment is last); formed on the device, no copy
                av_lens = (visual_mask.sum(1) + (Sf - max(nt))).to(torch.int32)

        def row_lengths():
            # at a capacity: every length comes from the mask as it is on the device when this runs (a replay reads the mask the host
            # copied into the static buffer), clamped to the capacities; rows that do not fit set bits of the status word
            nonlocal vid_lens, av_lens
            _, vid_lens, av_lens, self._visual_status = ops.ragged_lens(visual_mask, caps[0], caps[1], Sf - caps[0])

        def video_branch():
            nonlocal vid_lens
            if caps is not None:
                v, sv, _ = self.videomae(video_embeds, visual_mask, nkeep, ragged=True, seq_lens=vid_lens)
            elif ragged:
                v, sv, vid_lens = self.videomae(video_embeds, visual_mask, nkeep, ragged=True)      # ntok - n_true_b per row
            else:
                v, sv = self.videomae(video_embeds, visual_mask, nkeep)                  # :480
            if hasattr(self, "vid_2_768_2"):
                v = E.LinearFn.apply(v, None, self.vid_2_768_2.weight, self.vid_2_768_2.bias, None, ectx, True)
            return v, sv

        def audio_branch():
            a, a_lp, sa = self.wav2vec2(audio_features)                                  # :476
            return E.LinearFn.apply(a, a_lp if not ectx.pol.f32 else None, self.wav_2_768_2.weight, self.wav_2_768_2.bias, None, ectx, True), sa   # :478

        main = torch.cuda.current_stream()
        if runtime.multistream[0]:
            ev = runtime.take_inputs_event()
            if ev is None:
                ev = torch.cuda.Event()
                ev.record(main)
            s_aud, s_vid, s_txt = runtime.branch_streams(3)
            runtime.share_with(s_aud, audio_features)
            runtime.share_with(s_vid, video_embeds, visual_mask)
            runtime.share_with(s_txt, input_ids, text_attention_mask)
            with torch.cuda.stream(s_vid):
                runtime.stream_wait(s_vid, main, ev)           # (ev was recorded on the caller's stream: here, or by PreFormer.forward)
                if caps is not None:
                    # the lengths are counted at the head of the video branch (which only waits for the inputs, not for PreFormer's
                    # kernels); the fusion stack on the caller's stream takes them over through an event
                    row_lengths()
                    lens_ready = torch.cuda.Event()
                    lens_ready.record(s_vid)
                vid, Sv = video_branch()
            with torch.cuda.stream(s_aud):
                runtime.stream_wait(s_aud, main, ev)
                aud, Sa = audio_branch()
            with torch.cuda.stream(s_txt):
                runtime.stream_wait(s_txt, main, ev)
                _, t = self.bert(input_ids, text_attention_mask)                         # :485
        else:
            if caps is not None:
                row_lengths()
            aud, Sa = audio_branch()
            vid, Sv = video_branch()
            _, t = self.bert(input_ids, text_attention_mask)
        if lens_ready is not None:
            runtime.stream_wait(main, s_vid, lens_ready)
            for ten in (av_lens, self._visual_status):
                ten.record_stream(main)
        av = E.EmbedAddFn.apply(hidden_states.to(dev).reshape(B * Sf, 768), pos_embed.to(dev).reshape(-1).contiguous(), self.embedding.weight)   # :474
        av = self.random_mae_encoder(av.view(B, Sf, 768), attention_mask.to(dev), seq_lens=av_lens)     # :487 (fusion branch stays on the caller's stream)
        if runtime.multistream[0]:
            for st, ten in ((s_aud, aud), (s_vid, vid), (s_txt, t)):
                runtime.stream_wait(main, st)
                ten.record_stream(main)
            if vid_lens is not None:
                vid_lens.record_stream(main)
        p_drop = self.dropout_p if check == "train" else 0.0
        seed, = runtime.dropout_seeds(self, "_drop_calls", draw=p_drop > 0.0)        # (a device word under a capture)
        return E.TailFn.apply(av.reshape(B * Sf, 768), t, aud, vid, B, Sf, Sa, Sv, p_drop, seed,
                              self.rand_norm.weight, self.rand_norm.bias, self.bert_norm.weight, self.bert_norm.bias,
                              self.aud_norm.weight, self.aud_norm.bias, self.vid_norm.weight, self.vid_norm.bias,
                              self.linear1.weight, self.linear1.bias, av_lens, vid_lens)   # :486-499


def remap_reference_keys(state_dict):
    """Key names of a checkpoint saved with transformers 4.2x -> this package (transformers >= 5 naming), SURVEY.md §8b:
    VideoMAE `attention.attention.q_bias / v_bias` -> `query.bias / value.bias` (+ zero key.bias) inside `videomae.*`;
    weight-norm `weight_g / weight_v` -> `parametrizations.weight.original0 / original1`."""
    out = {}
    for k, v in state_dict.items():
        if k.startswith("videomae.") and k.endswith(".attention.attention.q_bias"):
            base = k[: -len("q_bias")]
            out[base + "query.bias"] = v
            out[base + "key.bias"] = torch.zeros_like(v)
        elif k.startswith("videomae.") and k.endswith(".attention.attention.v_bias"):
            out[k[: -len("v_bias")] + "value.bias"] = v
        elif k.endswith("pos_conv_embed.conv.weight_g"):
            out[k[: -len("weight_g")] + "parametrizations.weight.original0"] = v
        elif k.endswith("pos_conv_embed.conv.weight_v"):
            out[k[: -len("weight_v")] + "parametrizations.weight.original1"] = v
        elif k.endswith("embeddings.position_ids"):
            continue
        else:
            out[k] = v
    return out


SPEAKER_CROPS = {True: (120, 2, 245, 355), False: (120, 362, 245, 355)}          # (top, left, h, w), reference :86 (IEMOCAP: left / right speaker)


def draw_clip_augmentation(speaker, check, generator=None):
    """The random draws of the reference's video Compose (models/tav.py:76-115), in its order, from torch's global generator or `generator`:
    torch.rand(1) when speaker is None (the RandomHorizontalFlip(p=0) placeholder draws although it never flips; in validation too), then,
    for check == "train", randint(256, 321, (1,)) (RandomShortSideScale), rand(1) < 0.5 (horizontal flip) and rand(1) < 0.5 (vertical flip).
    -> {"size": short-side target or None, "hflip": bool, "vflip": bool}."""
    if speaker is None:
        torch.rand(1, generator=generator)
    if check != "train":
        return {"size": None, "hflip": False, "vflip": False}
    size = int(torch.randint(256, 321, (1,), generator=generator).item())
    hflip = bool(torch.rand(1, generator=generator) < 0.5)
    vflip = bool(torch.rand(1, generator=generator) < 0.5)
    return {"size": size, "hflip": hflip, "vflip": vflip}


def subsample_indices(T, num_frames):
    """pytorchvideo's uniform_temporal_subsample, literally: an f32 linspace, truncated."""
    return torch.clamp(torch.linspace(0, T - 1, num_frames), 0, T - 1).long()


def short_side_size(h, w, size):
    """pytorchvideo's short_side_scale: the shorter side becomes `size`, the longer one floor(long / short * size)."""
    if w < h:
        return int(np.floor(float(h) / w * size)), size
    return size, int(np.floor(float(w) / h * size))


def video_features_device(frames, speaker, check, out=None, device="cuda", generator=None, num_frames=16, size=224, layout=None,
                          augmentation=None):
    """videoMAE_features (reference models/tav.py:51-121) after the decoder, on the device: frames are uint8 [T, H, W, 3] or uint8 / float32
    [3, T, H, W] holding 0..255, on the host or on the device.  Temporal subsample, /255, normalise, speaker crop (None: none; truthy /
    falsy: SPEAKER_CROPS), and for check == "train" RandomShortSideScale(256, 320), Resize((size, size)) and the two random flips, otherwise
    one Resize -- all in ONE HIP launch (ops.video_clip_transform) that writes `out` (f32 [num_frames, 3, size, size], e.g. a slab of the
    batch tensor; allocated when None).  Host frames are reduced to the selected frames first and shipped once, from pinned memory,
    non-blocking.  The draws are draw_clip_augmentation's, or `augmentation` (a dict like the one it returns; nothing is drawn then).  There is
    no host form: without a GPU this raises."""
    frames = torch.as_tensor(frames)
    lay = ops.clip_layout(frames, layout)
    tdim = 0 if lay == "THWC" else 1
    T, H, W = frames.shape[:3] if lay == "THWC" else frames.shape[1:]
    aug = draw_clip_augmentation(speaker, check, generator) if augmentation is None else augmentation
    crop = None if speaker is None else SPEAKER_CROPS[bool(speaker)]
    if crop is not None and (crop[0] + crop[2] > H or crop[1] + crop[3] > W):
        raise ValueError(f"speaker crop (top, left, h, w) = {crop} does not lie inside {H} x {W} frames")
    ch, cw = (H, W) if crop is None else crop[2:]
    mid = None if aug["size"] is None else short_side_size(ch, cw, aug["size"])
    idx = subsample_indices(T, num_frames)
    if frames.is_cuda:
        sel, which = frames, idx.tolist()
    else:
        dev = _dev(device)
        shape = list(frames.shape)
        shape[tdim] = num_frames
        staged = torch.empty(shape, dtype=frames.dtype, pin_memory=True)
        torch.index_select(frames, tdim, idx, out=staged)
        sel, which = staged.to(dev, non_blocking=True), range(num_frames)
    x = ops.clip_xform(sel, which, layout=lay, crop=crop, mid=mid, out_hw=(size, size), hflip=aug["hflip"], vflip=aug["vflip"])
    return ops.video_clip_transform(sel, out, x)


def _decoded_video(v):
    """(frames, speaker) when a collate item's video entry is decoded frames -- a uint8 tensor or {"frames": ..., "speaker": ...} -- else None."""
    if isinstance(v, dict):
        return v["frames"], v.get("speaker")
    if (isinstance(v, torch.Tensor) and v.dtype == torch.uint8) or (isinstance(v, np.ndarray) and v.dtype == np.uint8):
        return v, None
    return None


def _pcm_tensor(pcm):
    """Decoded PCM as the kernel takes it: int16 stays int16, every float type becomes float32."""
    pcm = torch.as_tensor(pcm)
    if pcm.dtype == torch.int16:
        return pcm
    if not pcm.dtype.is_floating_point:
        raise TypeError(f"decoded PCM must be int16 or floating point, got {pcm.dtype}")
    return pcm.float()


def _resampled_length_checked(pcm, sampling_rate, target_sampling_rate, layout=None):
    """L_out of one utterance, known on the host; ValueError for an empty waveform and where the reference's .squeeze() changes meaning."""
    lay = ops.pcm_layout(pcm, layout)
    nch, n = (1, pcm.shape[0]) if lay == "L" else (pcm.shape if lay == "CL" else pcm.shape[::-1])
    if n < 1 or nch < 1:
        raise ValueError(f"speech_features_device: empty waveform {tuple(pcm.shape)}")
    l_out = ops.resampled_length(n, sampling_rate, target_sampling_rate)
    if nch > 1 and l_out == 1:
        raise ValueError(f"speech_features_device: {nch} channels of one resampled sample each -- the reference's .squeeze() leaves [{nch}] and "
                         "its mean would run over the channels' place, not over them")
    return lay, l_out


def speech_features_device(pcm, sampling_rate, out=None, mask=None, device="cuda", target_sampling_rate=16000, layout=None):
    """speech_file_to_array_fn (reference models/tav.py:165-169) after the decoder, on the device: torchaudio's Resample(sampling_rate,
    16000), .squeeze() and the mean over the channels in ONE HIP launch (ops.audio_resample).  pcm: int16 or float, mono [L], planar [C, L]
    (torchaudio.load) or interleaved [L, C], on the host or on the device.  Host PCM is shipped once, from pinned memory, non-blocking --
    int16 as int16 (two bytes per sample on the link; the kernel scales by 2^-15 as torchaudio.load does); device PCM is read where it lies.
    -> a 1-D f32 tensor of L_out = ceil(16000 L / sampling_rate) samples, or `out` (a row of the batch: samples, then 0.0) and `mask` (1.0
    for the samples, then 0.0), both written in full.  There is no host form: without a GPU this raises."""
    pcm = _pcm_tensor(pcm)
    lay, _ = _resampled_length_checked(pcm, sampling_rate, target_sampling_rate, layout)
    if not pcm.is_cuda:
        dev = _dev(device)
        staged = torch.empty(pcm.shape, dtype=pcm.dtype, pin_memory=True)
        staged.copy_(pcm)
        pcm = staged.to(dev, non_blocking=True)
    table = ops.audio_resample_table(sampling_rate, target_sampling_rate, device=pcm.device)
    return ops.audio_resample(pcm, table, out=out, mask=mask, layout=lay)


def _decoded_audio(a):
    """(pcm, sampling_rate) when a collate item's audio entry is decoded PCM -- {"pcm": ..., "sampling_rate": ...} -- else None."""
    if isinstance(a, dict):
        return a["pcm"], int(a["sampling_rate"])
    return None


def _draw_visual_mask(B, ntok):
    """reference :207-209: True w.p. 1/15 per token, drawn on the host (per-row counts Binomial(ntok, 1/15), unequal)."""
    m = torch.randint(-13, 2, (B, ntok))
    m[m < 0] = 0
    return m.bool()


def collate_batch(batch, check, visual_rows="equal", bucket=None):
    """Batch assembly contract of reference models/tav.py:174-246 for ALREADY DECODED items
    ([{'input_ids','attention_mask'}, waveform 1-D tensor, video [16,3,224,224] (or [3,16,H,W])], label).
    Reproduces: random video token mask True w.p. 1/15 (:207-209) then flips so every row keeps the same number of False
    (the reference only equalises the total, which breaks batch>1 -- SURVEY.md 'Hard parts'); zero padding of audio with a
    0/1 mask (:225-228); labels as float tensor.
    visual_rows="ragged": the video mask is drawn exactly as :207-209 and left as drawn -- every row keeps its own count (train with
    runtime.set_visual_rows("ragged")).  The reference's fix-up of the batch TOTAL (:211-217) only exists to make its reshape(B, -1, C) legal
    and is not applied.  bucket: the bucket the run trains with (runtime.set_visual_rows("ragged", bucket=g)); checked like the runtime
    switch checks it and otherwise without effect -- the mask is drawn the same, the padded sizes are the step's business."""
    runtime.check_visual_rows(visual_rows, bucket)
    texts, masks, speech, vids, labels = [], [], [], [], []
    for (inp, label) in batch:
        texts.append(torch.as_tensor(inp[0]["input_ids"]).reshape(-1))
        masks.append(torch.as_tensor(inp[0]["attention_mask"]).reshape(-1).float())
        if _decoded_audio(inp[1]) is not None:
            raise ValueError("collate_batch takes finished 16 kHz waveforms: decoded PCM is resampled by the HIP kernel only "
                             "(there is no CPU fallback) -- use collate_batch_device")
        speech.append(torch.as_tensor(inp[1]).float().reshape(-1))
        if _decoded_video(inp[2]) is not None:
            raise ValueError("collate_batch takes finished float clips: decoded uint8 frames are transformed by the HIP kernel only "
                             "(there is no CPU fallback) -- use collate_batch_device")
        v = torch.as_tensor(inp[2]).float()
        vids.append(v if v.shape[1] == 3 else v.permute(1, 0, 2, 3))
        labels.append(label)
    B = len(labels)
    ntok = (vids[0].shape[0] // 2) * (vids[0].shape[2] // 16) * (vids[0].shape[3] // 16)
    vid_mask = _draw_visual_mask(B, ntok)
    target = int(vid_mask.sum(1).max().item())
    for b in range(B if visual_rows == "equal" else 0):                                   # equal per-row counts (needed for reshape(B,-1,C) semantics)
        short = target - int(vid_mask[b].sum().item())
        if short > 0:
            idx = torch.where(~vid_mask[b])[0]
            vid_mask[b, idx[torch.randperm(len(idx))[:short]]] = True
    T = max(len(s) for s in speech)
    audio = torch.zeros(B, T)
    amask = torch.zeros(B, T)
    for b, s in enumerate(speech):
        audio[b, : len(s)] = s
        amask[b, : len(s)] = 1
    text = {"input_ids": torch.stack(texts).long(), "attention_mask": torch.stack(masks)}
    audio_features = {"audio_features": audio, "attention_mask": amask}
    visual = {"visual_embeds": torch.stack(vids), "attention_mask": vid_mask}
    return [text, audio_features, visual], torch.Tensor(np.array(labels))


def sample_video_mask(B, ntok, n_true=None, device="cpu", generator=None):
    """Video token mask of collate_batch (reference :206-217) built ON THE DEVICE without a host round trip: True marks the tokens the
    fusion stack sees and the video encoder drops.  The reference draws True w.p. 1/15 per token (a Binomial(ntok, 1/15) count per row)
    and then patches the TOTAL to a multiple of the batch size; rows of unequal count make `reshape(b, -1, 768)` mix utterances, so
    -- like collate_batch above -- every row gets the same count here, n_true (default round(ntok / 15): the reference's mean),
    chosen uniformly at random: the n_true smallest of ntok i.i.d. uniforms per row."""
    k = int(round(ntok / 15)) if n_true is None else int(n_true)
    r = torch.rand(B, ntok, device=device, generator=generator)
    idx = r.topk(k, dim=1, largest=False).indices
    return torch.zeros(B, ntok, dtype=torch.bool, device=device).scatter_(1, idx, True)


def collate_batch_device(batch, check, device="cuda", n_visual_true=None, generator=None, visual_rows="equal", bucket=None,
                         clip_generator=None, num_frames=16, size=224):
    """collate_batch with the tensor work on `device`: items are decoded utterances as for collate_batch; every
    tensor is shipped once (non-blocking) and padding, the audio length mask (reference :225-228) and the video token mask are built
    there, sync-free: nothing in the step reads them back (PreFormer / TAVForMAE take `n_visual_true` instead of counting).
    visual_rows="ragged": the video mask is drawn on the HOST as in collate_batch(visual_rows="ragged") and shipped; its per-row True
    counts come back as visual["n_visual_true"] (a list), to be passed on as n_visual_true -- known without a device read (the training
    loops and graph mode pick them up from there).  bucket: as in collate_batch.
    Decoded items: the video entry may be uint8 frames ([T, H, W, 3] or [3, T, H, W]) or {"frames": ..., "speaker": ...} instead of a
    finished float clip.  The [B, num_frames, 3, size, size] batch is then allocated once and video_features_device(frames, speaker, check)
    fills each clip's slab with one launch (no stack copy), drawing its augmentation from torch's global CPU generator or clip_generator,
    item by item in batch order, before any mask is drawn.  A batch is all decoded or all float.
    Decoded audio: the audio entry may be {"pcm": tensor, "sampling_rate": int} (int16 or float; [L], [C, L] or [L, C]) instead of a finished
    16 kHz waveform.  T = max_b L_out_b is known on the host; audio [B, T] and its mask are then allocated uninitialised and
    speech_features_device fills each item's two rows with one launch (no pad_sequence, no arange mask).  It draws no random number.  A
    batch is all PCM or all finished waveforms."""
    runtime.check_visual_rows(visual_rows, bucket)
    texts, masks, speech, vids, labels = [], [], [], [], []
    decoded = [_decoded_video(inp[2]) for (inp, _) in batch]
    if any(d is not None for d in decoded) and not all(d is not None for d in decoded):
        raise ValueError("collate_batch_device: a batch holds either decoded frames or finished float clips, not both")
    pcms = [_decoded_audio(inp[1]) for (inp, _) in batch]
    if any(p is not None for p in pcms) and not all(p is not None for p in pcms):
        raise ValueError("collate_batch_device: a batch holds either decoded PCM or finished 16 kHz waveforms, not both")
    for (inp, label), d, p in zip(batch, decoded, pcms):
        texts.append(torch.as_tensor(inp[0]["input_ids"]).reshape(-1))
        masks.append(torch.as_tensor(inp[0]["attention_mask"]).reshape(-1).float())
        if p is None:
            speech.append(torch.as_tensor(inp[1]).float().reshape(-1))
        if d is None:
            v = torch.as_tensor(inp[2]).float()
            vids.append(v if v.shape[1] == 3 else v.permute(1, 0, 2, 3))
        labels.append(float(label))
    B = len(labels)
    dev = torch.device(device)
    if speech:
        lens = torch.tensor([len(s) for s in speech])
        T = int(lens.max())
        audio = torch.nn.utils.rnn.pad_sequence([s.to(dev, non_blocking=True) for s in speech], batch_first=True)      # zero padding, reference :228
        amask = (torch.arange(T, device=dev)[None, :] < lens.to(dev, non_blocking=True)[:, None]).float()
    else:
        if dev.type != "cuda":
            raise ValueError(f"collate_batch_device(device={str(dev)!r}): decoded PCM is resampled by the HIP kernel on the GPU only; "
                             "there is no CPU fallback")
        pcms = [(_pcm_tensor(p), sr) for (p, sr) in pcms]
        T = max(_resampled_length_checked(p, sr, 16000)[1] for (p, sr) in pcms)
        audio = torch.empty(B, T, dtype=torch.float32, device=_dev(dev))
        amask = torch.empty(B, T, dtype=torch.float32, device=audio.device)
        for b, (p, sr) in enumerate(pcms):
            speech_features_device(p, sr, out=audio[b], mask=amask[b], device=audio.device)
    if vids:
        video = torch.stack([v.to(dev, non_blocking=True) for v in vids])
    else:
        if dev.type != "cuda":
            raise ValueError(f"collate_batch_device(device={str(dev)!r}): decoded frames are transformed by the HIP kernel on the GPU only; "
                             "there is no CPU fallback")
        video = torch.empty(B, num_frames, 3, size, size, dtype=torch.float32, device=_dev(dev))
        for b, (frames, speaker) in enumerate(decoded):
            video_features_device(frames, speaker, check, out=video[b], device=video.device, generator=clip_generator, num_frames=num_frames,
                                  size=size)
    ntok = (video.shape[1] // 2) * (video.shape[3] // 16) * (video.shape[4] // 16)
    visual = {"visual_embeds": video}
    if visual_rows == "ragged":
        m = _draw_visual_mask(B, ntok)
        visual["attention_mask"], visual["n_visual_true"] = m.to(dev, non_blocking=True), m.sum(1).tolist()
    else:
        visual["attention_mask"] = sample_video_mask(B, ntok, n_visual_true, dev, generator)
    text = {"input_ids": torch.stack(texts).long().to(dev, non_blocking=True), "attention_mask": torch.stack(masks).to(dev, non_blocking=True)}
    return [text, {"audio_features": audio, "attention_mask": amask}, visual], \
        torch.tensor(labels, dtype=torch.float32).to(dev, non_blocking=True)

