"""Host model of the video clip transform (tav_video_clip_transform, models.tav.video_features_device): the project's definition.

pytorchvideo and torchvision are not installed; what the reference's Compose (models/tav.py:76-115) does at the versions it pins is restated
here from their sources:

  UniformTemporalSubsample(n)   pytorchvideo/transforms/functional.py uniform_temporal_subsample:
                                indices = torch.linspace(0, t - 1, n); indices = torch.clamp(indices, 0, t - 1).long(); index_select(x, -3, indices)
  Lambda(x / 255.0), NormalizeVideo(mean, std)   torchvision/transforms/_functional_video.py normalize: (clip - mean[:, None, None, None]) / std[...]
  Crop((top, left, h, w))       reference utils/global_functions.py: torchvision crop = x[..., top:top + h, left:left + w]
  RandomShortSideScale(a, b)    pytorchvideo/transforms/transforms.py: size = torch.randint(a, b + 1, (1,)).item(); functional.short_side_scale:
                                if w < h: new_h = int(math.floor((float(h) / w) * size)), new_w = size
                                else:     new_h = size, new_w = int(math.floor((float(w) / h) * size))
                                torch.nn.functional.interpolate(x, size=(new_h, new_w), mode="bilinear", align_corners=False)
  Resize((224, 224))            torchvision/transforms/functional_tensor.py resize on a tensor: interpolate(..., mode="bilinear", align_corners=False),
                                antialias off for tensors  -- a SECOND resampling after the short-side scale
  RandomHorizontalFlip(p), RandomVerticalFlip(p)   torchvision/transforms/transforms.py: `if torch.rand(1) < self.p: return F.hflip(img)`; one draw
                                per call, hence per clip; the p = 0 placeholder of the speaker-less branch draws too
  bilinear, align_corners=False aten/src/ATen/native/UpSample.h area_pixel_compute_source_index: src = max(0, scale * (dst + 0.5) - 0.5),
                                scale = in / out; i0 = floor(src), i1 = i0 + (i0 < in - 1), lam = src - i0;
                                UpSampleKernel: h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11)

Three things live here:
  chain64()    the chain in fp64, literally in the reference's order (index_select, /255, normalise, slice, F.interpolate twice, flip)
  bound()      the per-element bound 16 u (v_raw a_c + |b_c|): u = 2^-24, v_raw = the same chain on un-normalised values (never negative, so
               nothing cancels), a_c = 1 / (255 std_c), b_c = mean_c / std_c; sixteen f32 roundings -- about six per interpolation level (the
               weight's division, 1 - lam twice, three products and two sums share operands), four for the affine step (the two constants, the
               product, the difference)
  emulate()    the kernel's arithmetic in numpy f32: the two levels with integer source coordinates, normalisation last -- and its mutants, each
               of which must leave the bound on a named case (MUTANTS)
"""
import functools

import numpy as np
import torch
from torch.nn import functional as F

U = 2.0 ** -24
ROUNDINGS = 16
MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
A = 1.0 / (255.0 * STD)
B = MEAN / STD

# name -> T, H, W, crop (top, left, h, w) or None, short-side size or None, out (h, w), nf
CASES = {
    "down_wide": dict(T=5, H=37, W=53, crop=None, size=22, out=(32, 48), nf=4),            # long side 22 * 53 / 37 = 31.51: floor and round differ
    "down_tall": dict(T=23, H=53, W=37, crop=None, size=22, out=(32, 32), nf=4),           # w < h: the other arm of the short-side rule
    "up_one_level": dict(T=16, H=24, W=24, crop=None, size=None, out=(32, 32), nf=4),      # validation form; upscaling: the clamp at 0 and at the edge
    "crop": dict(T=40, H=61, W=90, crop=(7, 3, 41, 55), size=30, out=(16, 48), nf=4),
    "up_two_levels": dict(T=3, H=20, W=31, crop=None, size=64, out=(32, 32), nf=4),        # up, then down; T < nf repeats frames
    "identity": dict(T=1, H=33, W=33, crop=(0, 0, 33, 33), size=33, out=(33, 33), nf=4),   # every weight 0: the normalisation alone
}
REAL = dict(T=3, H=720, W=1280, crop=None, size=288, out=(224, 224), nf=2)
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def source(case, seed=0):
    """Seeded uint8 frames [T, H, W, 3]."""
    c = CASES[case] if isinstance(case, str) else case
    rng = np.random.default_rng(seed + 1000 * c["T"] + c["H"])
    return rng.integers(0, 256, (c["T"], c["H"], c["W"], 3), dtype=np.uint8)


def subsample(T, nf, rounded=False):
    lin = torch.linspace(0, T - 1, nf)
    if rounded:
        return torch.clamp(torch.round(lin), 0, T - 1).long()
    return torch.clamp(lin, 0, T - 1).long()


def short_side(h, w, size, rounded=False, swapped=False):
    fl = (lambda v: int(np.floor(v + 0.5))) if rounded else (lambda v: int(np.floor(v)))
    if (w < h) != swapped:
        return fl(float(h) / w * size), size
    return size, fl(float(w) / h * size)


def plan(case, mutant=None):
    """-> (frame indices, crop (top, left, h, w), mid (h, w) or None, out (h, w))."""
    c = CASES[case] if isinstance(case, str) else case
    idx = subsample(c["T"], c["nf"], rounded=mutant == "frame_index_rounded")
    crop = c["crop"] if c["crop"] is not None else (0, 0, c["H"], c["W"])
    mid = None
    if c["size"] is not None:
        mid = short_side(crop[2], crop[3], c["size"], rounded=mutant == "long_side_rounded", swapped=mutant == "short_side_rule_swapped")
    return idx, crop, mid, tuple(c["out"])


# ---------------------------------------------------------------------------------------------- fp64 chain and bound
def chain64(src_thwc, idx, crop, mid, out, hflip=False, vflip=False, normalise=True):
    """fp64, the reference's order.  src_thwc: uint8 numpy [T, H, W, 3].  -> double tensor [nf, 3, out_h, out_w]."""
    x = torch.from_numpy(np.ascontiguousarray(src_thwc)).permute(3, 0, 1, 2).double()          # [3, T, H, W] as get_clip yields it
    x = torch.index_select(x, -3, idx)
    if normalise:
        x = x / 255.0
        x = (x - torch.from_numpy(MEAN)[:, None, None, None]) / torch.from_numpy(STD)[:, None, None, None]
    top, left, h, w = crop
    x = x[..., top:top + h, left:left + w]
    if mid is not None:
        x = F.interpolate(x, size=tuple(mid), mode="bilinear", align_corners=False)
    x = F.interpolate(x, size=tuple(out), mode="bilinear", align_corners=False)
    if hflip:
        x = x.flip(-1)
    if vflip:
        x = x.flip(-2)
    return x.permute(1, 0, 2, 3).contiguous()


def bound(v_raw, roundings=ROUNDINGS):
    """Per-element bound from the un-normalised chain's values [nf, 3, h, w]."""
    a = torch.from_numpy(A)[None, :, None, None]
    b = torch.from_numpy(np.abs(B))[None, :, None, None]
    return roundings * U * (v_raw * a + b)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(fp64 result, bound) of a named case (or "real") without flips; a flipped clip is the flip of both.  Computed once, shared, read-only."""
    c = REAL if case == "real" else CASES[case]
    src = source(c)
    idx, crop, mid, out = plan(c)
    want = chain64(src, idx, crop, mid, out)
    raw = chain64(src, idx, crop, mid, out, normalise=False)
    assert float(raw.min()) >= 0.0
    return want, bound(raw)


def flipped(t, hflip, vflip):
    if hflip:
        t = t.flip(-1)
    if vflip:
        t = t.flip(-2)
    return t


def worst_ratio(got, want, bnd):
    """max |got - want| / bound over the elements (inf when an element is NaN)."""
    got = torch.as_tensor(got).double()
    if torch.isnan(got).any():
        return float("inf")
    return float(((got - want).abs() / bnd).max())


# ---------------------------------------------------------------------------------------------- f32 emulation of the kernel
f32 = np.float32


def coords(n_in, n_out, mutant=None):
    """Source taps of every output coordinate, in exact integers as the kernel forms them."""
    o = np.arange(n_out, dtype=np.int64)
    if mutant == "align_corners":
        src = o * ((n_in - 1) / (n_out - 1)) if n_out > 1 else np.zeros(n_out)
        i0 = np.floor(src).astype(np.int64)
        lam = (src - i0).astype(f32)
    else:
        num = (2 * o + 1) * n_in - n_out
        assert int(np.abs(num).max()) < 2 ** 31
        if mutant != "no_clamp_at_0":
            num = np.maximum(num, 0)
        den = 2 * n_out
        i0 = np.maximum(num, 0) // den                                     # (the mutant keeps index 0 and lets the weight go negative)
        lam = (num - i0 * den).astype(f32) / f32(den)
    i1 = i0 + 1 if mutant == "i1_not_clamped" else np.minimum(i0 + 1, n_in - 1)
    return i0, i1, lam


def resize_f32(img, oh, ow, mutant=None):
    """One bilinear level on f32 [..., h, w], every operation rounded to f32 on its own, in torch's order."""
    h, w = img.shape[-2:]
    y0, y1, ly = coords(h, oh, mutant)
    x0, x1, lx = coords(w, ow, mutant)
    if mutant == "i1_not_clamped":                                         # what lies past the edge reads as 0
        img = np.pad(img, [(0, 0)] * (img.ndim - 2) + [(0, 1), (0, 1)])
    w1, h1 = lx[None, :], ly[:, None]
    w0, h0 = f32(1) - w1, f32(1) - h1
    p00, p01 = img[..., y0[:, None], x0[None, :]], img[..., y0[:, None], x1[None, :]]
    p10, p11 = img[..., y1[:, None], x0[None, :]], img[..., y1[:, None], x1[None, :]]
    out = h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11)
    assert out.dtype == np.float32
    return out


MUTANTS = {
    # mutant -> (case, hflip, vflip) on which it must leave the bound
    "one_resize": ("down_wide", False, False),
    "align_corners": ("down_wide", False, False),
    "no_clamp_at_0": ("up_one_level", False, False),
    "i1_not_clamped": ("up_one_level", False, False),
    "frame_index_rounded": ("down_tall", False, False),
    "long_side_rounded": ("down_wide", False, False),
    "short_side_rule_swapped": ("down_tall", False, False),
    "flips_swapped": ("crop", True, False),
    "hflip_ignored": ("crop", True, False),
    "vflip_ignored": ("crop", False, True),
    "channel_stats_swapped": ("identity", False, False),
    "crop_offset_dropped": ("crop", False, False),
    "thwc_read_as_cthw": ("down_wide", False, False),
}


def emulate(src, layout, idx, crop, mid, out, hflip=False, vflip=False, scale=None, shift=None, mutant=None):
    """The kernel in numpy f32.  src: uint8 or f32 numpy, [T, H, W, 3] ("THWC") or [3, T, H, W] ("CTHW").  -> f32 [nf, 3, out_h, out_w]."""
    scale = A.astype(f32) if scale is None else np.asarray(scale, f32)
    shift = B.astype(f32) if shift is None else np.asarray(shift, f32)
    if layout == "THWC":
        T, H, W, _ = src.shape
        x = np.ascontiguousarray(src).reshape(3, T, H, W) if mutant == "thwc_read_as_cthw" else src.transpose(3, 0, 1, 2)
    else:
        x = src
    x = x[:, np.asarray(idx)].astype(f32)
    top, left, h, w = crop
    if mutant == "crop_offset_dropped":
        top, left = 0, 0
    x = x[..., top:top + h, left:left + w]
    if mid is not None and mutant != "one_resize":
        x = resize_f32(x, mid[0], mid[1], mutant)
    x = resize_f32(x, out[0], out[1], mutant)
    if mutant == "flips_swapped":
        hflip, vflip = vflip, hflip
    if mutant == "hflip_ignored":
        hflip = False
    if mutant == "vflip_ignored":
        vflip = False
    if hflip:
        x = x[..., ::-1]
    if vflip:
        x = x[..., ::-1, :]
    if mutant == "channel_stats_swapped":
        scale, shift = scale[::-1], shift[::-1]
    y = x * scale[:, None, None, None] - shift[:, None, None, None]
    assert y.dtype == np.float32
    return np.ascontiguousarray(y.transpose(1, 0, 2, 3))


def emulate_case(case, hflip=False, vflip=False, mutant=None, layout="THWC", dtype=np.uint8):
    c = REAL if case == "real" else CASES[case]
    src = source(c)
    idx, crop, mid, out = plan(c, mutant)
    if layout == "CTHW":
        src = np.ascontiguousarray(src.transpose(3, 0, 1, 2))
    return emulate(src.astype(dtype), layout, idx.numpy(), crop, mid, out, hflip, vflip, mutant=mutant)


# ---------------------------------------------------------------------------------------------- exact cases
EXACT = dict(T=2, H=8, W=8, mid=(16, 16), out=(32, 32), nf=2)          # two 2x upscales: every weight is 1/4 or 3/4, every sum exact in f32


def exact_source(seed=0):
    return np.random.default_rng(77 + seed).integers(0, 256, (EXACT["T"], EXACT["H"], EXACT["W"], 3), dtype=np.uint8)


def exact_reference(src, hflip, vflip):
    """fp64 chain on raw values (scale 1, shift 0): representable in f32, so the kernel must return these bits."""
    return chain64(src, torch.arange(EXACT["nf"]), (0, 0, EXACT["H"], EXACT["W"]), EXACT["mid"], EXACT["out"], hflip, vflip, normalise=False)
