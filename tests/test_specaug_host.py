"""CPU: the SpecAugment sampler's host model (tests/specaug_ref.py, the normative description of tav_specaug_draw) against HF
`_compute_mask_indices`; PreFormer.reference_spec_masks against the direct HF calls; argument validation of the new entry points (nothing is
launched without a GPU); the runtime mode switch, the CLI flag and what the graphed loop does with each mode."""
import ctypes as C

import numpy as np
import pytest
import torch

import specaug_ref as R
import tav_amd  # noqa: F401
from tav_amd import _lib, runtime
from tav_amd.models.tav import PreFormer
from tav_amd.train_model import graphed as G
from tav_amd.utils.global_functions import arg_parse


def _bare_preformer(audio_cfg):
    pre = PreFormer.__new__(PreFormer)                       # only the sampler is exercised: no encoder weights needed
    torch.nn.Module.__init__(pre)
    pre.cfg = {"audio": dict(audio_cfg)}
    return pre


def test_host_model_distribution_matches_hf_compute_mask_indices():
    """The settings and the acceptance condition of test_specaugment_distribution_matches_hf_compute_mask_indices: per-row mean masked count
    within rtol 0.08 of HF's, nothing masked in the padding; plus one epsilon per call (rows of equal length take the same number of spans)."""
    from transformers.models.wav2vec2.modeling_wav2vec2 import _compute_mask_indices
    B, T = 6, 249
    lens = np.array([249, 249, 200, 120, 60, 249])
    amask = np.arange(T)[None, :] < lens[:, None]
    np.random.seed(0)
    trials = 300
    ours, hf = np.zeros(B), np.zeros(B)
    counts = set()
    for k in range(trials):
        seed = (0x1234567 + runtime.GOLDEN * (k + 1)) & R.U64
        m, n, _ = R.draw(amask, B, T, 0.05, 10, 2, seed, R.TAG_TIME)
        assert not (m.astype(bool) & ~amask).any()
        assert n[0] == n[1] == n[5]
        counts.add(int(n[0]))
        ours += m.sum(1)
        ref = _compute_mask_indices((B, T), mask_prob=0.05, mask_length=10, attention_mask=torch.from_numpy(amask).long(), min_masks=2)
        assert not (ref & ~amask).any()
        hf += ref.sum(1)
    ours, hf = ours / trials, hf / trials
    print("time axis: ours", ours, "hf", hf, "rel", np.abs(ours - hf) / hf)
    assert np.allclose(ours, hf, rtol=0.08), (ours, hf)
    assert counts == {2}                                     # 0.05 * 249 / 10 + eps < 2.25: min_masks decides at full length
    H = 64
    ours_f = hf_f = 0.0
    fcounts = set()
    for k in range(200):
        seed = (0x7654321 + runtime.GOLDEN * (k + 1)) & R.U64
        m, n, _ = R.draw(None, B, H, 0.2, 4, 1, seed, R.TAG_FEATURE)
        assert len(set(n.tolist())) == 1
        fcounts.add(int(n[0]))
        ours_f += m.sum(1).mean()
        hf_f += float(_compute_mask_indices((B, H), mask_prob=0.2, mask_length=4, min_masks=1).sum(1).mean())
    print("feature axis: ours", ours_f / 200, "hf", hf_f / 200, "rel", abs(ours_f - hf_f) / hf_f)
    assert abs(ours_f - hf_f) / hf_f < 0.08, (ours_f, hf_f)
    assert fcounts == {3, 4}                                 # 0.2 * 64 / 4 = 3.2: epsilon moves the count between 3 and 4


def test_host_model_sampler_properties():
    """Spans are `length` long, start inside [0, len - length], are distinct; rows shorter than a span stay empty; the tags keep the axes apart."""
    B, L = 4, 49
    valid = np.arange(L)[None, :] < np.array([49, 10, 9, 0])[:, None]
    m, n, starts = R.draw(valid, B, L, 0.05, 10, 2, (1 << 63) + 12345, R.TAG_TIME)
    assert n.tolist() == [2, 1, 0, 0] and starts[1] == [0] and not m[2:].any()
    assert len(set(starts[0])) == 2 and all(0 <= s <= 39 for s in starts[0])
    a = R.draw(None, 2, 64, 0.2, 4, 1, 99, R.TAG_TIME)[0]
    b = R.draw(None, 2, 64, 0.2, 4, 1, 99, R.TAG_FEATURE)[0]
    assert not np.array_equal(a, b)
    # the streams stay clear of each other and of the dropout offsets (0, 1 << 40, 2 << 40 plus an element index below 2^40)
    spans = [(t, t + R.EPS_STRIDE) for t in (R.TAG_TIME, R.TAG_FEATURE)] + [(0, (3 << 40) - 1)]
    spans.sort()
    assert all(hi < lo2 for (_, hi), (lo2, _) in zip(spans, spans[1:]))


@pytest.mark.parametrize("seed", [0, 7])
def test_reference_spec_masks_are_the_direct_hf_calls(seed):
    """Under np.random.seed(s): the time axis first with the frame mask and mask_time_min_masks, then the feature axis without a mask --
    the reference's two calls (models/tav.py:283-301).  A batch with padded rows; mask_feature_prob = 0 gives None and takes no numpy draw."""
    from transformers.models.wav2vec2.modeling_wav2vec2 import _compute_mask_indices
    B, T, H = 3, 49, 64
    amask = torch.arange(T)[None, :] < torch.tensor([49, 30, 12])[:, None]
    cfg = dict(mask_time_prob=0.05, mask_time_length=10, mask_time_min_masks=2, mask_feature_prob=0.2, mask_feature_length=4, mask_feature_min_masks=1)
    pre = _bare_preformer(cfg)
    np.random.seed(seed)
    tm, fm = pre.reference_spec_masks(B, T, H, amask)
    after = np.random.random()
    np.random.seed(seed)
    want_t = _compute_mask_indices((B, T), mask_prob=0.05, mask_length=10, attention_mask=amask.long(), min_masks=2)
    want_f = _compute_mask_indices((B, H), mask_prob=0.2, mask_length=4, min_masks=1)
    assert after == np.random.random()
    assert tm.dtype == torch.bool and fm.dtype == torch.bool and tm.shape == (B, T) and fm.shape == (B, H)
    assert np.array_equal(tm.numpy(), want_t) and np.array_equal(fm.numpy(), want_f)
    assert tm.any() and fm.any() and not (tm & ~amask).any()
    # no padding, no feature axis
    pre0 = _bare_preformer(dict(cfg, mask_feature_prob=0.0))
    np.random.seed(seed)
    tm0, fm0 = pre0.reference_spec_masks(B, T, H, None)
    after0 = np.random.random()
    np.random.seed(seed)
    want0 = _compute_mask_indices((B, T), mask_prob=0.05, mask_length=10, attention_mask=None, min_masks=2)
    assert fm0 is None and np.array_equal(tm0.numpy(), want0) and after0 == np.random.random()
    # the preset's defaults when the cfg names nothing (Wav2Vec2Config: 0.05 / 10 / 2, feature axis off); rows shorter than a span: nothing
    np.random.seed(seed)
    tmd, fmd = _bare_preformer({}).reference_spec_masks(B, T, H, amask)
    assert fmd is None and np.array_equal(tmd.numpy(), want_t)
    assert pre.reference_spec_masks(B, 9, H, None) == (None, None)


def test_specaug_entry_points_validate_arguments_without_launching():
    h = _lib.lib()
    assert h.tav_version() == _lib.ABI_VERSION == 7
    for name in ("tav_specaug_draw", "tav_specaug_draw_dev", "tav_specaug_fwd", "tav_specaug_bwd", "tav_specaug_bwd_ws_bytes"):
        assert name in _lib.declared_symbols() and hasattr(h, name)
    a, b, c, d, e, w = (C.c_void_p(4096 * (i + 1)) for i in range(6))          # never dereferenced: every call below is rejected first
    draw, ddev = h.tav_specaug_draw, h.tav_specaug_draw_dev
    assert draw(a, None, c, 4, 49, 0.05, 10, 2, 1, R.TAG_TIME, None) == -1
    assert ddev(a, b, c, 4, 49, 0.05, 10, 2, None, R.TAG_TIME, None) == -1                 # the seed word is required
    assert ddev(a, None, c, 4, 49, 0.05, 10, 2, d, R.TAG_TIME, None) == -1
    for f, s in ((draw, 1), (ddev, d)):
        assert f(None, b, None, 4, 49, 0.05, 0, 2, s, R.TAG_TIME, None) == -2               # length < 1
        assert f(None, b, None, 4, 49, 0.05, -3, 2, s, R.TAG_TIME, None) == -2
        assert f(None, b, None, 4, 0, 0.05, 10, 2, s, R.TAG_TIME, None) == -2               # L < 1
        assert f(None, b, None, 0, 49, 0.05, 10, 2, s, R.TAG_TIME, None) == -2
        assert f(None, b, None, 4, 4096, 0.5, 1, 0, s, R.TAG_TIME, None) == -2              # up to 2049 spans per row
        assert f(None, b, None, 4, 4096, 0.0, 4, 129, s, R.TAG_TIME, None) == -2            # min_masks alone passes the cap
        assert f(None, b, None, 4, 1290, 1.0, 10, 0, s, R.TAG_TIME, None) == -2             # min(floor(129 + 1), 129) = 129
    assert R.span_cap(4096, 0.5, 1, 0) == 2049 and R.span_cap(4096, 0.0, 4, 129) == 129 and R.span_cap(1290, 1.0, 10, 0) == 129
    assert R.span_cap(1289, 1.0, 10, 0) == 128 and R.span_cap(16000, 0.05, 10, 2) == 81        # (legal: such calls launch, so not made here)
    fwd = h.tav_specaug_fwd
    assert fwd(None, b, c, d, e, 3, 49, 64, None) == -1
    assert fwd(a, b, c, d, None, 3, 49, 64, None) == -1
    assert fwd(a, b, c, None, e, 3, 49, 64, None) == -1                                    # a time mask needs the embedding
    assert fwd(a, b, c, d, e, 3, 49, 66, None) == -2                                       # H % 4
    assert fwd(a, b, c, d, e, 3, 0, 64, None) == -2
    assert fwd(a, b, c, d, e, 0, 49, 64, None) == -2
    bwd = h.tav_specaug_bwd
    nbytes = h.tav_specaug_bwd_ws_bytes(3 * 49, 64)
    assert nbytes == ((3 * 49 + 31) // 32) * 64 * 4 and h.tav_specaug_bwd_ws_bytes(10 ** 6, 768) == 1024 * 768 * 4
    assert bwd(None, b, c, d, e, w, nbytes, 3, 49, 64, None) == -1
    assert bwd(a, b, c, None, e, w, nbytes, 3, 49, 64, None) == -1
    assert bwd(a, b, c, d, e, None, 0, 3, 49, 64, None) == -1                              # dembed needs the workspace
    assert bwd(a, b, c, d, e, w, nbytes - 4, 3, 49, 64, None) == -2                        # ... all of it
    assert bwd(a, b, c, d, e, w, nbytes, 3, 49, 62, None) == -2
    assert bwd(a, b, c, d, None, None, 0, 3, -1, 64, None) == -2


class _Opt:
    generation = 0


class _Crit:
    epoch_switch = 2


class _Stepper:
    reducer = None

    def __init__(self):
        self.opt, self.criterion, self.model, self.pre = _Opt(), _Crit(), None, None


def _batch(B=2):
    vm = torch.zeros(B, 8, dtype=torch.bool)
    vm[:, :3] = True
    return ([{"input_ids": torch.zeros(B, 16, dtype=torch.int64), "attention_mask": torch.ones(B, 16)},
             {"audio_features": torch.zeros(B, 800), "attention_mask": torch.ones(B, 800)},
             {"visual_embeds": torch.zeros(B, 16, 3, 32, 32), "attention_mask": vm}], torch.zeros(B))


def test_specaugment_modes_flag_and_graphed_signature():
    assert runtime.specaugment() == "torch"
    with pytest.raises(ValueError, match="specaugment"):
        runtime.set_specaugment("bogus")
    assert runtime.specaugment() == "torch"
    assert arg_parse("TAV", []).specaugment == "torch"
    assert arg_parse("TAV", ["--specaugment", "device"]).specaugment == "device"
    with pytest.raises(SystemExit):
        arg_parse("TAV", ["--specaugment", "bogus"])
    prev = runtime.precision()
    runtime.set_precision("bf16")
    gs = G.GraphedSteps(_Stepper())
    sigs = {}
    try:
        for mode in runtime.SPECAUGMENT_MODES:
            assert runtime.set_specaugment(mode) == mode == runtime.specaugment()
            sigs[mode] = gs.signature(*_batch(), 0, False)
    finally:
        runtime.set_specaugment("torch")
        runtime.set_precision(prev)
    assert sigs["reference"] is None                         # host-drawn masks: every training batch runs the eager step
    assert sigs["device"] is not None and sigs["torch"] is not None and sigs["device"] != sigs["torch"] and sigs["device"][2] == 3


def test_reference_mode_refuses_a_capture_and_device_mode_counts_only_real_draws():
    """Host logic of PreFormer._mask_hidden_states under the two new modes, reached before any kernel: "reference" under a capture raises;
    with train=False, rows shorter than a span, or both probabilities 0, "device" takes no seed and returns its input."""
    cfg = dict(mask_time_prob=0.05, mask_time_length=10, mask_time_min_masks=2)
    pre = _bare_preformer(cfg)
    pre._spec_calls = 0
    pre.masked_spec_embed = torch.nn.Parameter(torch.zeros(8))
    x = torch.zeros(2 * 20, 8)
    try:
        runtime.set_specaugment("reference")
        with runtime.guard_only(object()):
            with pytest.raises(RuntimeError, match="cannot be captured"):
                pre._mask_hidden_states(x, 2, 20, None, training=True)
        runtime.set_specaugment("device")
        assert pre._mask_hidden_states(x, 2, 20, None, training=False) is x
        assert pre._mask_hidden_states(x[:2 * 9], 2, 9, None, training=True) is not None and pre._spec_calls == 0
        off = _bare_preformer(dict(cfg, mask_time_prob=0.0))
        off._spec_calls = 0
        assert off._mask_hidden_states(x, 2, 20, None, training=True) is x and off._spec_calls == 0
    finally:
        runtime.set_specaugment("torch")
