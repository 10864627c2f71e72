"""CPU: the host model of the audio waveform transform (tests/audio_resample_ref.py) -- the table facts, the restatement against analytic
sines, the f32 emulation of the kernel inside the per-element bound of the fp64 chain on every case, every mutant outside it -- and the host
side of the feature: the symbol in the header and the binding (ABI still 7), the argument checks (error codes before anything is launched),
the table ops.audio_resample_table builds, resampled_length, and what refuses to run without the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import audio_resample_ref as R
import tav_amd  # noqa: F401
from tav_amd import _lib, ops, synthetic
from tav_amd import config as cfgmod
from tav_amd.models import tav as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sr", list(R.TABLE_FACTS))
def test_table_facts(sr):
    o, n, width, taps, live_lo, live_hi = R.TABLE_FACTS[sr]
    h32, o_, n_, width_ = R.table32(sr)
    assert (o_, n_, width_, h32.shape) == (o, n, width, (n, taps)) and taps == 2 * width + o
    tab, first, live = R.compact(h32)                            # asserts that every tap it leaves out is == 0.0 in f32
    assert live == (live_lo, live_hi) and tab.shape == (n, live_hi)
    assert first.min() >= 0 and first.max() + live_hi <= taps
    full = np.zeros_like(h32)
    for p in range(n):
        full[p, first[p]:first[p] + live_hi] = tab[p]
    assert np.array_equal(full, h32)                             # the compact table is the whole table
    assert tab.nbytes <= 21760                                   # 21 KB for the two 441-sample pairs, a few hundred bytes for the others
    # the product computes the same table, bit for bit, and the same compaction
    t = ops.audio_resample_table(sr, device="cpu")
    assert (t.o, t.n, t.width, t.ntap) == (o, n, width, live_hi)
    assert np.array_equal(ops.sinc_resample_coefficients(sr)[0].view(np.int32), h32.view(np.int32))
    assert np.array_equal(t.h.view(np.int32), tab.view(np.int32)) and np.array_equal(t.first_host, first) and t.first_max == first.max()
    assert torch.equal(t.table, torch.from_numpy(tab)) and torch.equal(t.first, torch.from_numpy(first))
    assert ops.audio_resample_table(sr, device="cpu") is t       # cached per (sr, target, device)
    assert t.tile == _lib.lib().tav_audio_resample_tile(o, n, width) and t.tile % 256 == 0 and 256 <= t.tile <= 1024


def test_identity_pair_is_one_tap_and_the_sinc_table_is_no_delta():
    t = ops.audio_resample_table(16000, device="cpu")
    assert (t.o, t.n, t.width, t.ntap, t.first_max) == (1, 1, 0, 1, 0) and t.h.tolist() == [[1.0]] and t.first_host.tolist() == [0]
    h32 = R.table32(16000)[0]
    assert h32.shape == (1, 15) and np.count_nonzero(h32) == 13 and float(h32[0, 7]) == float(np.float32(0.99))      # centre tap base / o, not 1


@pytest.mark.parametrize("sr,tone", R.SINES)
def test_restatement_reproduces_a_sine_at_the_new_rate(sr, tone):
    err = R.sine_error(sr, tone)
    print(f"{sr} -> 16000, {tone:.0f} Hz: max |chain - analytic sine| = {err:.2e}")
    assert err < 1e-3                                            # the filter's passband ripple; a wrong delay, scale or phase order gives 1e-1..1


@pytest.mark.parametrize("case", list(R.CASES))
def test_emulation_stays_within_the_bound(case):
    want, bnd = R.reference(case)
    c = R.CASES[case]
    assert len(want) == R.resampled_length(c["L"], c["sr"])
    r = R.worst_ratio(R.emulate_case(case), want, bnd)
    print(f"{case}: worst |emulation - fp64| / bound = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_each_mutant_leaves_the_bound(mutant):
    left = 0
    for case in R.MUTANTS[mutant]:
        want, bnd = R.reference(case)
        ok = R.worst_ratio(R.emulate_case(case), want, bnd)
        bad = R.worst_ratio(R.emulate_case(case, mutant), want, bnd)
        print(f"{mutant} on {case}: {bad:.3g} (unmutated {ok:.3f})")
        assert ok <= 1.0
        left += bad > 1.0
    assert left >= 1


def test_length_mutant_changes_l_out():
    c = R.CASES["44k_stereo_i16"]
    assert R.resampled_length(c["L"], c["sr"]) == 545 and R.resampled_length(c["L"], c["sr"], floor=True) == 544       # 1500 * 160 / 441 = 544.2
    assert R.resampled_length(700, 48000) == 234 and R.resampled_length(700, 48000, floor=True) == 233


def test_resampled_length_agrees_with_the_chain():
    for sr in (44100, 48000, 8000, 22050, 16000, 11025, 32000, 96000):
        for L in (1, 2, 3, 5, 17, 440, 441, 442, 1000, 1499, 1500):
            x = np.zeros((1, L))
            assert ops.resampled_length(L, sr) == len(R.chain64(x, sr)) == R.resampled_length(L, sr), (sr, L)
    assert ops.resampled_length(441 * 10 ** 9, 44100) == 160 * 10 ** 9                  # integers: no float ceil
    assert ops.resample_ratio(44100) == (441, 160) and ops.resample_ratio(8000) == (1, 2) and ops.resample_ratio(16000) == (1, 1)
    assert R.seam_length(44100, 1024) == R.CASES["44k_seam"]["L"] and R.resampled_length(R.CASES["44k_seam"]["L"], 44100) == 1025
    assert ops.audio_resample_table(44100, device="cpu").tile == 1024            # the seam case sits one sample past the kernel's tile


def test_symbol_is_declared_bound_and_abi_stays_7():
    text = open(os.path.join(ROOT, "include", "tavhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\btav_audio_resample\s*\(", src) and re.search(r"\btav_audio_resample_tile\s*\(", src) and "tav_resample_args" in src
    assert "Audio waveform transform (additive to ABI v7" in text and re.search(r"TAV_I16\s*=\s*4", src)
    assert {"tav_audio_resample", "tav_audio_resample_tile"} <= set(_lib.declared_symbols())
    h = _lib.lib()
    assert hasattr(h, "tav_audio_resample") and hasattr(h, "tav_audio_resample_tile")
    assert _lib.ABI_VERSION == 7 and h.tav_version() == 7
    # the struct as the header lays it out: 2 * 4 | 3 * 8 | 4 * 4 | 2 * 4 | 8, no padding
    assert C.sizeof(_lib.ResampleArgs) == 64 and _lib.ResampleArgs.L.offset == 8 and _lib.ResampleArgs.o.offset == 32
    assert _lib.ResampleArgs.first_max.offset == 48 and _lib.ResampleArgs.T_row.offset == 56
    assert (_lib.TAV_F32, _lib.TAV_U8, _lib.TAV_I16) == (0, 3, 4)
    assert os.path.exists(os.path.join(ROOT, "multi-modal-emotion_amd", "csrc", "audio_resample.hip"))
    assert "audio_resample.hip" in open(os.path.join(ROOT, "multi-modal-emotion_amd", "csrc", "Makefile")).read()


def _good_args():
    a = _lib.ResampleArgs()
    a.src_dtype, a.C, a.L, a.sC, a.sL = _lib.TAV_I16, 2, 1500, 1, 2
    a.o, a.n, a.width, a.ntap, a.first_max = 441, 160, 17, 34, 441
    a.T_row = 545
    return a


def test_argument_checks_return_error_codes_before_any_launch():
    h = _lib.lib()
    p = 0x1000                                                   # never dereferenced: every call below is rejected on the host
    NULL, SHAPE, DTYPE = -1, -2, -3
    call = h.tav_audio_resample
    a = _good_args()
    assert call(None, p, p, p, p, C.byref(a), None) == NULL      # src
    assert call(p, None, p, p, p, C.byref(a), None) == NULL      # table
    assert call(p, p, None, p, p, C.byref(a), None) == NULL      # first
    assert call(p, p, p, None, p, C.byref(a), None) == NULL      # values
    assert call(p, p, p, p, p, None, None) == NULL               # the struct
    for code in (_lib.TAV_BF16, _lib.TAV_FP8, _lib.TAV_U8, 5, -1):
        a = _good_args()
        a.src_dtype = code
        assert call(p, p, p, p, None, C.byref(a), None) == DTYPE, code
    bad = [("C", 0), ("C", 33), ("C", -1), ("L", 0), ("L", -5), ("sC", -1), ("sL", -2), ("o", 0), ("o", -441), ("n", 0), ("n", -1),
           ("ntap", 0), ("ntap", -3), ("ntap", (1 << 24) // 160 + 1),             # n * ntap above 2^24
           ("first_max", 442), ("first_max", -1), ("first_max", 1 << 30),         # first[p] + ntap past 2 width + o = 475
           ("T_row", 544), ("T_row", 0), ("T_row", -1)]                            # below L_out = 545
    for name, v in bad:
        a = _good_args()
        setattr(a, name, v)
        assert call(p, p, p, p, p, C.byref(a), None) == SHAPE, (name, v)
    a = _good_args()                                             # n * ntap = 2^24 + 2^12 with a first_max that fits
    a.n, a.ntap, a.o, a.width, a.first_max, a.T_row = 4097, 4096, 1, 2048, 0, 1 << 30
    assert call(p, p, p, p, p, C.byref(a), None) == SHAPE
    a = _good_args()                                             # o / n = 441: not even 256 outputs' input span fits the workgroup's LDS
    a.n, a.first_max, a.T_row = 1, 0, 1 << 20
    assert h.tav_audio_resample_tile(441, 1, 17) == 0 and call(p, p, p, p, p, C.byref(a), None) == SHAPE
    assert h.tav_audio_resample_tile(441, 160, 17) == 1024 and h.tav_audio_resample_tile(0, 1, 0) == 0
    assert h.tav_error_string(DTYPE).decode() and h.tav_error_string(SHAPE).decode() == "unsupported shape"


def test_resample_args_describe_the_source_tensor():
    t = ops.audio_resample_table(44100, device="cpu")
    a = ops.resample_args(torch.zeros(1500, 2, dtype=torch.int16), t)
    assert (a.src_dtype, a.C, a.L, a.sC, a.sL, a.T_row) == (_lib.TAV_I16, 2, 1500, 1, 2, 545)
    assert (a.o, a.n, a.width, a.ntap, a.first_max) == (441, 160, 17, 34, t.first_max)
    a = ops.resample_args(torch.zeros(2, 1500), t, T_row=600)
    assert (a.src_dtype, a.C, a.L, a.sC, a.sL, a.T_row) == (_lib.TAV_F32, 2, 1500, 1500, 1, 600)
    a = ops.resample_args(torch.zeros(3000)[::2], t)
    assert (a.C, a.L, a.sC, a.sL) == (1, 1500, 0, 2)
    assert ops.pcm_layout(torch.zeros(5)) == "L" and ops.pcm_layout(torch.zeros(2, 5)) == "CL" and ops.pcm_layout(torch.zeros(5, 2)) == "LC"
    assert ops.pcm_layout(torch.zeros(2, 5), "LC") == "LC"
    with pytest.raises(ValueError, match=r"\[L\], \[C, L\] or \[L, C\]"):
        ops.pcm_layout(torch.zeros(2, 5, 1))
    with pytest.raises(TypeError, match="int16 or float32"):
        ops.resample_args(torch.zeros(2, 5, dtype=torch.float64), t)


def test_there_is_no_host_form():
    """ops.audio_resample refuses host tensors, collate_batch refuses pcm items and names collate_batch_device, a batch is all PCM or all
    finished waveforms; finished waveforms go through both collates as before."""
    t = ops.audio_resample_table(44100, device="cpu")
    with pytest.raises(ValueError, match="GPU only"):
        ops.audio_resample(torch.zeros(1500, 2, dtype=torch.int16), t)
    cfg = cfgmod.preset("B-tiny")
    items = synthetic.make_items(cfg, 2, seed=3, s_text=8, t_audio=2000, raw_audio=(44100, 2))
    floats = synthetic.make_items(cfg, 2, seed=3, s_text=8, t_audio=2000)
    for (i, _), (f, _) in zip(items, floats):
        assert i[1]["pcm"].dtype == torch.int16 and i[1]["pcm"].shape == (len(f[1]), 2) and i[1]["sampling_rate"] == 44100
    with pytest.raises(ValueError, match="collate_batch_device"):
        M.collate_batch(items, "train")
    with pytest.raises(ValueError, match="not both"):
        M.collate_batch_device([items[0], floats[1]], "train", device="cpu")
    with pytest.raises(ValueError, match="no CPU fallback"):
        M.collate_batch_device(items, "train", device="cpu")
    with pytest.raises(ValueError, match="empty waveform"):
        M.speech_features_device(torch.zeros(2, 0), 44100)
    with pytest.raises(ValueError, match="empty waveform"):
        M.speech_features_device(torch.zeros(0, dtype=torch.int16), 44100)
    with pytest.raises(ValueError, match="squeeze"):
        M.speech_features_device(torch.zeros(2, 2), 44100)                       # two channels, L_out = 1
    with pytest.raises(TypeError, match="int16 or floating point"):
        M.speech_features_device(torch.zeros(2, 50, dtype=torch.int32), 44100)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            M.speech_features_device(torch.zeros(2, 50), 44100, device="cpu")
    (t1, a1, v1), _ = M.collate_batch(floats, "train")
    (t2, a2, v2), _ = M.collate_batch_device(floats, "train", device="cpu")
    assert torch.equal(a1["audio_features"], a2["audio_features"]) and torch.equal(a1["attention_mask"], a2["attention_mask"])
