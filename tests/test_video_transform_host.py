"""CPU: the host model of the video clip transform (tests/video_transform_ref.py) -- the f32 emulation of the kernel stays inside the
per-element bound against the fp64 chain on every case, every mutant leaves it on its named case, the exact cases are exact -- and the
host side of the feature: the draws of draw_clip_augmentation, the symbol in the header and the binding (ABI still 7), the argument checks
(error codes before anything is launched), the descriptor ops.clip_xform fills, and what refuses to run without the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import tav_amd  # noqa: F401
import video_transform_ref as R
from tav_amd import _lib, ops, synthetic
from tav_amd import config as cfgmod
from tav_amd.models import tav as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", list(R.CASES) + ["real"])
def test_emulation_stays_within_the_bound(case):
    want, bnd = R.reference(case)
    combos = [(lay, dt) for lay in ("THWC", "CTHW") for dt in (np.uint8, np.float32)] if case != "real" else [("THWC", np.uint8)]
    worst = 0.0
    for hf, vf in R.FLIPS:
        for lay, dt in combos:
            got = R.emulate_case(case, hf, vf, layout=lay, dtype=dt)
            worst = max(worst, R.worst_ratio(got, R.flipped(want, hf, vf), R.flipped(bnd, hf, vf)))
    print(f"{case}: worst |emulation - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert worst <= 0.25                      # the integer-coordinate form sits at about 3 u of the 16 allowed; an f32 coordinate does not


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_each_mutant_leaves_the_bound_on_its_named_case(mutant):
    case, hf, vf = R.MUTANTS[mutant]
    want, bnd = R.reference(case)
    ok = R.worst_ratio(R.emulate_case(case, hf, vf), R.flipped(want, hf, vf), R.flipped(bnd, hf, vf))
    bad = R.worst_ratio(R.emulate_case(case, hf, vf, mutant=mutant), R.flipped(want, hf, vf), R.flipped(bnd, hf, vf))
    print(f"{mutant} on {case}: {bad:.3g} (unmutated {ok:.3f})")
    assert ok <= 1.0 < bad


def test_exact_cases_are_exact_in_the_emulation():
    for seed in range(3):
        src = R.exact_source(seed)
        for hf, vf in R.FLIPS:
            got = R.emulate(src, "THWC", np.arange(R.EXACT["nf"]), (0, 0, 8, 8), R.EXACT["mid"], R.EXACT["out"], hf, vf, scale=[1, 1, 1], shift=[0, 0, 0])
            assert np.array_equal(got.astype(np.float64), R.exact_reference(src, hf, vf).numpy()), (seed, hf, vf)


def test_plan_of_the_cases():
    assert R.plan("down_wide")[2] == (22, 31) and R.plan("down_wide", "long_side_rounded")[2] == (22, 32)            # 22 * 53 / 37 = 31.51
    assert R.plan("down_tall")[2] == (31, 22) and R.plan("down_tall", "short_side_rule_swapped")[2] == (22, 15)
    assert R.plan("up_one_level")[2] is None
    assert R.plan("crop")[1:3] == ((7, 3, 41, 55), (30, 40))
    assert R.plan("down_tall")[0].tolist() == [0, 7, 14, 22] and R.plan("down_tall", "frame_index_rounded")[0].tolist() == [0, 7, 15, 22]
    assert R.plan("identity")[0].tolist() == [0, 0, 0, 0]
    assert R.plan(R.REAL)[2] == (288, 512)
    # the product's restatements are the model's
    for T, nf in [(5, 4), (23, 4), (40, 4), (3, 4), (1, 4), (90, 16), (91, 32), (500, 16)]:
        assert torch.equal(M.subsample_indices(T, nf), R.subsample(T, nf)), (T, nf)
    for h, w in [(37, 53), (53, 37), (41, 55), (720, 1280), (245, 355), (33, 33)]:
        for size in (22, 256, 288, 320):
            assert M.short_side_size(h, w, size) == R.short_side(h, w, size), (h, w, size)


@pytest.mark.parametrize("speaker,check", [(None, "train"), (None, "val"), (True, "train"), (False, "train"), (0, "test"), (1, "val")])
def test_draw_clip_augmentation_makes_exactly_the_reference_draws(speaker, check):
    g = torch.Generator().manual_seed(99)
    replay = torch.Generator().manual_seed(99)
    for _ in range(5):
        got = M.draw_clip_augmentation(speaker, check, generator=g)
        if speaker is None:
            torch.rand(1, generator=replay)                                         # RandomHorizontalFlip(p=0)
        if check == "train":
            size = torch.randint(256, 321, (1,), generator=replay).item()           # RandomShortSideScale
            hf = bool(torch.rand(1, generator=replay) < 0.5)                        # RandomHorizontalFlip(p=0.5)
            vf = bool(torch.rand(1, generator=replay) < 0.5)                        # RandomVerticalFlip(p=0.5)
            assert got == {"size": size, "hflip": hf, "vflip": vf} and 256 <= size <= 320
        else:
            assert got == {"size": None, "hflip": False, "vflip": False}
        assert torch.equal(g.get_state(), replay.get_state())
    # without a generator argument the global one is drawn from, in the same way
    torch.manual_seed(5)
    a = M.draw_clip_augmentation(speaker, check)
    st = torch.get_rng_state()
    torch.manual_seed(5)
    b = M.draw_clip_augmentation(speaker, check, generator=torch.default_generator)
    assert a == b and torch.equal(st, torch.get_rng_state())


def test_symbol_is_declared_bound_and_abi_stays_7():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tavhip.h")).read(), flags=re.S)
    assert re.search(r"\btav_video_clip_transform\s*\(", src) and "tav_clip_xform" in src
    assert "Video clip transform (additive to ABI v7" in open(os.path.join(ROOT, "include", "tavhip.h")).read()
    assert "tav_video_clip_transform" in _lib.declared_symbols()
    h = _lib.lib()
    assert hasattr(h, "tav_video_clip_transform")
    assert _lib.ABI_VERSION == 7 and h.tav_version() == 7
    # the struct as the header lays it out: 4 + 3 * 4 | 4 * 8 | 4 + 32 * 4 | 4 * 4 | 2 * 4 | 4 * 4 | 6 * 4, no padding but the tail's
    assert C.sizeof(_lib.ClipXform) == 248 and _lib.ClipXform.sT.offset == 16 and _lib.ClipXform.frame.offset == 52
    assert _lib.ClipXform.scale.offset == 220 and (_lib.TAV_F32, _lib.TAV_U8) == (0, 3)


def _good_xform():
    x = _lib.ClipXform()
    x.src_dtype, x.T, x.H, x.W = _lib.TAV_U8, 5, 37, 53
    x.sT, x.sH, x.sW, x.sC = 37 * 53 * 3, 53 * 3, 3, 1
    x.nf = 4
    for i, f in enumerate([0, 1, 2, 4]):
        x.frame[i] = f
    x.crop_top, x.crop_left, x.crop_h, x.crop_w = 0, 0, 37, 53
    x.mid_h, x.mid_w, x.out_h, x.out_w = 22, 31, 32, 48
    return x


def test_argument_checks_return_error_codes_before_any_launch():
    h = _lib.lib()
    p = 0x1000                                                   # never dereferenced: every call below is rejected on the host
    NULL, SHAPE, DTYPE = -1, -2, -3
    call = h.tav_video_clip_transform
    x = _good_xform()
    assert call(None, p, C.byref(x), None) == NULL
    assert call(p, None, C.byref(x), None) == NULL
    assert call(p, p, None, None) == NULL
    for code in (_lib.TAV_BF16, _lib.TAV_FP8, 4, -1):
        x = _good_xform()
        x.src_dtype = code
        assert call(p, p, C.byref(x), None) == DTYPE, code
    bad = [("H", 0), ("H", -3), ("H", 16385), ("W", 0), ("W", 16385), ("T", 0), ("T", -1), ("nf", 0), ("nf", 33), ("nf", -1),
           ("out_h", 0), ("out_h", 16385), ("out_w", 0), ("out_w", -2), ("out_w", 16385),
           ("crop_h", 0), ("crop_h", 38), ("crop_w", 54), ("crop_w", -1), ("crop_top", -1), ("crop_top", 1), ("crop_left", 1), ("crop_left", -1),
           ("crop_h", 16385), ("mid_h", 0), ("mid_w", 0), ("mid_h", -1), ("mid_w", 16385), ("mid_h", 16385),
           ("sT", -1), ("sH", -1), ("sW", -1), ("sC", -1)]
    for name, v in bad:
        x = _good_xform()
        setattr(x, name, v)
        assert call(p, p, C.byref(x), None) == SHAPE, (name, v)
    for i, f in [(0, -1), (3, 5), (2, 1 << 30), (1, -(1 << 31))]:
        x = _good_xform()
        x.frame[i] = f
        assert call(p, p, C.byref(x), None) == SHAPE, (i, f)
    x = _good_xform()                                            # a crop that fits in size but not where it is put
    x.crop_top, x.crop_left, x.crop_h, x.crop_w = 7, 3, 31, 50
    assert call(p, p, C.byref(x), None) == SHAPE
    x.crop_top, x.crop_h, x.crop_left, x.crop_w = 6, 32, 4, 50
    assert call(p, p, C.byref(x), None) == SHAPE
    assert h.tav_error_string(DTYPE).decode() and h.tav_error_string(SHAPE).decode() == "unsupported shape"


def test_clip_xform_describes_the_source_tensor():
    thwc = torch.zeros(5, 37, 53, 3, dtype=torch.uint8)
    x = ops.clip_xform(thwc, [0, 1, 2, 4], crop=(7, 3, 20, 30), mid=(22, 31), out_hw=(32, 48), hflip=True)
    assert (x.src_dtype, x.T, x.H, x.W, x.nf) == (_lib.TAV_U8, 5, 37, 53, 4) and (x.sT, x.sH, x.sW, x.sC) == (37 * 53 * 3, 53 * 3, 3, 1)
    assert list(x.frame[:4]) == [0, 1, 2, 4] and (x.crop_top, x.crop_left, x.crop_h, x.crop_w) == (7, 3, 20, 30)
    assert (x.mid_h, x.mid_w, x.out_h, x.out_w, x.hflip, x.vflip) == (22, 31, 32, 48, 1, 0)
    assert [x.scale[c] for c in range(3)] == [float(np.float32(v)) for v in R.A] and [x.shift[c] for c in range(3)] == [float(np.float32(v)) for v in R.B]
    cthw = torch.zeros(3, 5, 37, 53)
    x = ops.clip_xform(cthw, range(5))
    assert (x.src_dtype, x.T, x.H, x.W) == (_lib.TAV_F32, 5, 37, 53) and (x.sT, x.sH, x.sW, x.sC) == (37 * 53, 53, 1, 5 * 37 * 53)
    assert (x.crop_top, x.crop_left, x.crop_h, x.crop_w, x.mid_h, x.mid_w, x.out_h, x.out_w) == (0, 0, 37, 53, 0, 0, 224, 224)
    assert ops.clip_layout(torch.zeros(3, 3, 20, 31, dtype=torch.uint8)) == "CTHW" and ops.clip_layout(torch.zeros(3, 20, 31, 3, dtype=torch.uint8)) == "THWC"
    x = ops.clip_xform(thwc, [0], mean=(0, 0, 0), std=(1 / 255.0,) * 3)
    assert [x.scale[c] for c in range(3)] == [1.0] * 3 and [x.shift[c] for c in range(3)] == [0.0] * 3
    with pytest.raises(ValueError, match="uint8 \\[T, H, W, 3\\]"):
        ops.clip_layout(torch.zeros(5, 37, 53, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="1..32 frames"):
        ops.clip_xform(thwc, range(33))
    with pytest.raises(TypeError, match="uint8 or float32"):
        ops.clip_xform(torch.zeros(3, 5, 37, 53, dtype=torch.float64), [0])


def test_there_is_no_host_form():
    """ops.video_clip_transform refuses host tensors, collate_batch refuses decoded frames and names collate_batch_device; float items go
    through both collates as before."""
    thwc = torch.zeros(5, 37, 53, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU only"):
        ops.video_clip_transform(thwc, None, ops.clip_xform(thwc, [0]))
    cfg = cfgmod.preset("B-tiny")
    items = synthetic.make_items(cfg, 2, raw_video=(6, 20, 24), seed=3, s_text=8, t_audio=2000)
    with pytest.raises(ValueError, match="collate_batch_device"):
        M.collate_batch(items, "train")
    wrapped = [([i[0], i[1], {"frames": i[2], "speaker": None}], lab) for (i, lab) in items]
    with pytest.raises(ValueError, match="collate_batch_device"):
        M.collate_batch(wrapped, "val")
    floats = synthetic.make_items(cfg, 2, seed=3, s_text=8, t_audio=2000)
    with pytest.raises(ValueError, match="not both"):
        M.collate_batch_device([items[0], floats[1]], "train", device="cpu")
    with pytest.raises(ValueError, match="does not lie inside"):
        M.video_features_device(items[0][0][2], True, "val")
    with pytest.raises(ValueError, match="no CPU fallback"):
        M.collate_batch_device(items, "train", device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            M.video_features_device(items[0][0][2], None, "val", device="cpu")
    (t, a, v), lab = M.collate_batch(floats, "train")
    assert torch.equal(v["visual_embeds"], torch.stack([i[2] for (i, _) in floats]))


def test_make_items_contract():
    cfg = cfgmod.preset("B-tiny")
    items = synthetic.make_items(cfg, 3, raw_video=(6, 20, 24), seed=3, s_text=8, t_audio=2000, speakers=[None, True, False])
    again = synthetic.make_items(cfg, 3, raw_video=(6, 20, 24), seed=3, s_text=8, t_audio=2000, speakers=[None, True, False])
    assert len(items) == 3
    for ((text, wave, video), label), ((_, wave2, video2), _) in zip(items, again):
        assert text["input_ids"].shape == (8,) and text["attention_mask"].shape == (8,) and wave.dim() == 1 and 0 <= label <= 6
        assert video["frames"].dtype == torch.uint8 and video["frames"].shape == (6, 20, 24, 3)
        assert torch.equal(video["frames"], video2["frames"]) and torch.equal(wave, wave2)
    assert [i[0][2]["speaker"] for i in items] == [None, True, False]
    assert len({len(i[0][1]) for i in items}) == 3                                   # unequal waveforms: the audio mask has work to do
    f = synthetic.make_items(cfg, 1, seed=3, s_text=8, t_audio=2000)[0][0][2]
    assert f.dtype == torch.float32 and f.shape == (cfg["video"]["frames"], 3, cfg["video"]["image"], cfg["video"]["image"])
