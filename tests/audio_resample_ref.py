"""Host model of the audio waveform transform (tav_audio_resample, models.tav.speech_features_device): the project's definition.

torchaudio is not installed; what the reference's speech_file_to_array_fn (models/tav.py:165-169: Resample(sr, 16000), .squeeze(), the mean
over the channels) does is restated here from torchaudio's sources:

  transforms.Resample.__init__   resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99, dtype=None;
                                 gcd = math.gcd(orig_freq, new_freq); kernel, width = _get_sinc_resample_kernel(..., dtype=None)
  functional/functional.py _get_sinc_resample_kernel
                                 orig_freq //= gcd; new_freq //= gcd; base_freq = min(orig_freq, new_freq) * rolloff
                                 width = math.ceil(lowpass_filter_width * orig_freq / base_freq)
                                 idx = torch.arange(-width, width + orig_freq, dtype=float64)[None, None] / orig_freq
                                 t = torch.arange(0, -new_freq, -1, dtype=float64)[:, None, None] / new_freq + idx
                                 t *= base_freq; t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
                                 window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
                                 t *= math.pi; scale = base_freq / orig_freq
                                 kernels = torch.where(t == 0, 1.0, t.sin() / t) * window * scale
                                 dtype is None -> kernels.to(dtype=torch.float32): fp64 arithmetic, rounded ONCE to f32
  functional/functional.py _apply_sinc_resample_kernel
                                 waveform = F.pad(waveform, (width, width + orig_freq))
                                 resampled = F.conv1d(waveform[:, None], kernel, stride=orig_freq)      # [channels, new_freq, frames]
                                 resampled = resampled.transpose(1, 2).reshape(num_wavs, -1)            # y[q * new_freq + p]
                                 target_length = ceil(new_freq * length / orig_freq); resampled[..., :target_length]
  transforms.Resample.forward    if self.orig_freq == self.new_freq: return waveform

Here: o = orig_freq / gcd, n = new_freq / gcd, K = 2 width + o taps per phase.

  table64 / table32   the coefficients in fp64 and as torchaudio stores them
  compact             the live taps of every phase: every tap outside the Hann window is exactly 0.0 in f32
  chain64             the chain in fp64 in the reference's order: every channel through the full f32 table, then the mean
  bound               per element (ntap + C + 1) u S[i], u = 2^-24, S[i] = (1 / C) sum_c sum_k |h[p][k]| |xpad_c[q o + k]|: the standard worst
                      case of ntap sequential fma plus the channel sum (C - 1 additions) and its scaling (the factor 1 / C and the product)
  emulate             the kernel's arithmetic in f32 (channel mean first, then fma over ascending k of the compact table; an fma is the exact
                      f64 product plus the accumulator, rounded to f32) and its mutants, each of which must leave the bound on a case
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
TARGET = 16000
WIDTH, ROLLOFF = 6, 0.99

# name -> sr, L, channels, dtype ("i16" | "f32"), layout ("LC" interleaved [L, C] | "CL" planar [C, L] | "L" mono [L])
CASES = {
    "44k_stereo_i16": dict(sr=44100, L=1500, C=2, dtype="i16", layout="LC"),
    "44k_mono_f32": dict(sr=44100, L=1500, C=1, dtype="f32", layout="L"),
    "48k_stereo_f32": dict(sr=48000, L=700, C=2, dtype="f32", layout="CL"),
    "8k_mono_i16": dict(sr=8000, L=300, C=1, dtype="i16", layout="L"),
    "22k_six_f32": dict(sr=22050, L=900, C=6, dtype="f32", layout="CL"),
    "16k_mono_f32": dict(sr=16000, L=1000, C=1, dtype="f32", layout="L"),
    "16k_stereo_f32": dict(sr=16000, L=1000, C=2, dtype="f32", layout="CL"),
    "44k_short": dict(sr=44100, L=5, C=2, dtype="i16", layout="LC"),                     # shorter than the filter
    "44k_seam": dict(sr=44100, L=2823, C=2, dtype="f32", layout="CL"),                  # L_out = 1025: one more than the kernel's tile of 1024
    "44k_3s_stereo_i16": dict(sr=44100, L=132300, C=2, dtype="i16", layout="LC"),        # 48 000 outputs: many workgroups
}
TABLE_FACTS = {        # sr -> o, n, width, taps, live taps per phase (least, most)
    44100: (441, 160, 17, 475, 33, 34),
    48000: (3, 1, 19, 41, 37, 37),
    8000: (1, 2, 7, 15, 12, 13),
    22050: (441, 320, 9, 459, 16, 17),
}


def ratio(sr, target=TARGET):
    g = math.gcd(int(sr), int(target))
    return int(sr) // g, int(target) // g


def resampled_length(L, sr, target=TARGET, floor=False):
    o, n = ratio(sr, target)
    return (n * L) // o if floor else (n * L + o - 1) // o


def seam_length(sr, tile, target=TARGET):
    """The shortest L whose L_out is tile + 1."""
    o, n = ratio(sr, target)
    L = (tile * o) // n + 1
    assert resampled_length(L, sr, target) == tile + 1 and resampled_length(L - 1, sr, target) <= tile
    return L


@functools.lru_cache(maxsize=None)
def table64(sr, target=TARGET, mutant=None):
    """-> (h [n][2 width + o] float64, o, n, width)."""
    o, n = ratio(sr, target)
    base = min(o, n) * (1.0 if mutant == "rolloff_one" else ROLLOFF)
    width = math.ceil(WIDTH * o / base)
    k = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    p = np.arange(0, -n, -1, dtype=np.float64)[:, None] / n
    t = ((-p if mutant == "phase_sign" else p) + k) * base
    t = np.clip(t, -WIDTH, WIDTH)
    win = np.cos(t * math.pi / WIDTH / 2)
    if mutant != "window_not_squared":
        win = win ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / t)
    h = sinc * win
    if mutant != "scale_dropped":
        h = h * (base / o)
    h.setflags(write=False)
    return h, o, n, width


def table32(sr, target=TARGET, mutant=None):
    h, o, n, width = table64(sr, target, mutant)
    return h.astype(np.float32), o, n, width


def compact(h32, strict=True):
    """-> (tab [n][ntap] f32, first [n] int32): row p holds taps first[p] .. first[p] + ntap - 1; everything left out is exactly 0.0."""
    n, K = h32.shape
    nz = h32 != 0
    lo = nz.argmax(1)
    hi = K - 1 - nz[:, ::-1].argmax(1)
    ntap = int((hi - lo + 1).max())
    first = np.minimum(lo, K - ntap).astype(np.int32)
    cols = first[:, None] + np.arange(ntap)[None, :]
    tab = np.take_along_axis(h32, cols, 1)
    keep = np.zeros_like(nz)
    np.put_along_axis(keep, cols, True, 1)
    if strict:
        assert np.all(h32[~keep] == 0.0)
    live = nz.sum(1)
    return tab, first, (int(live.min()), int(live.max()))


def kernel_table(sr, target=TARGET):
    """(tab, first, o, n, width) as the kernel takes it; the identity pair is one phase with the one tap 1.0."""
    if int(sr) == int(target):
        return np.ones((1, 1), np.float32), np.zeros(1, np.int32), 1, 1, 0
    h32, o, n, width = table32(sr, target)
    tab, first, _ = compact(h32)
    return tab, first, o, n, width


# ------------------------------------------------------------------------------------------------------ sources
def source(case, seed=0):
    """Seeded raw PCM of a case as numpy, in the case's layout and dtype (i16: the full range; f32: what torchaudio.load returns, [-1, 1))."""
    c = CASES[case] if isinstance(case, str) else case
    rng = np.random.default_rng(seed + c["sr"] + 7 * c["L"] + c["C"])
    shape = (c["L"],) if c["layout"] == "L" else ((c["L"], c["C"]) if c["layout"] == "LC" else (c["C"], c["L"]))
    if c["dtype"] == "i16":
        return rng.integers(-32768, 32768, shape, dtype=np.int16)
    return (rng.random(shape, dtype=np.float32) * 2 - 1).astype(np.float32)


def planar(raw, layout):
    """raw in its layout -> [C][L], dtype unchanged."""
    return raw[None, :] if layout == "L" else (raw.T if layout == "LC" else raw)


def to_float(x, i16_scale=2.0 ** -15):
    """What torchaudio.load hands over: int16 / 32768 (exact in f32), f32 unchanged.  -> float64 holding f32 values."""
    return x.astype(np.float64) * i16_scale if x.dtype == np.int16 else x.astype(np.float64)


# ------------------------------------------------------------------------------------------------------ the fp64 chain and the bound
def _frames(xpad, o, K, nq):
    """[C][nq][K] windows xpad[c][q * o + k] without copying."""
    s = xpad.strides
    return np.lib.stride_tricks.as_strided(xpad, (xpad.shape[0], nq, K), (s[0], s[1] * o, s[1]), writeable=False)


def _filter64(x, h, o, n, width, absolute=False):
    """Every channel of x [C][L] (float64) through the table h [n][K] (float64) -> [C][L_out]."""
    C, L = x.shape
    K = h.shape[1]
    xpad = np.zeros((C, L + 2 * width + o))
    xpad[:, width:width + L] = np.abs(x) if absolute else x
    nq = L // o + 1
    y = _frames(xpad, o, K, nq) @ (np.abs(h) if absolute else h).T          # [C][nq][n]
    return y.reshape(C, nq * n)[:, :(n * L + o - 1) // o]


def chain64(x, sr, target=TARGET):
    """Resample, squeeze, mean over the channels, in that order, in fp64 with torchaudio's f32 table.  x: [C][L] float64."""
    if int(sr) == int(target):
        return x.mean(0) if x.shape[0] > 1 else x[0].copy()
    h32, o, n, width = table32(sr, target)
    y = _filter64(x, h32.astype(np.float64), o, n, width)
    return y.sum(0) / x.shape[0] if x.shape[0] > 1 else y[0]


def bound(x, sr, target=TARGET):
    """(ntap + C + 1) u S[i] per output element; ntap is the compact table's."""
    C = x.shape[0]
    if int(sr) == int(target):
        return (1 + C + 1) * U * np.abs(x).sum(0) / C
    h32, o, n, width = table32(sr, target)
    ntap = compact(h32)[0].shape[1]
    S = _filter64(x, h32.astype(np.float64), o, n, width, absolute=True).sum(0) / C
    return (ntap + C + 1) * U * S


@functools.lru_cache(maxsize=None)
def reference(case):
    """(fp64 chain, bound) of a case; computed once, shared, read-only."""
    c = CASES[case]
    x = to_float(planar(source(case), c["layout"]))
    want, bnd = chain64(x, c["sr"]), bound(x, c["sr"])
    want.setflags(write=False)
    bnd.setflags(write=False)
    return want, bnd


def worst_ratio(got, want, bnd):
    """max |got - want| / bound; an element whose bound is 0 must be exactly equal (inf otherwise)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    if not np.all(np.isfinite(got)):
        return float("inf")
    zero = bnd == 0
    if np.any(err[zero] != 0):
        return float("inf")
    return float((err[~zero] / bnd[~zero]).max()) if np.any(~zero) else 0.0


# ------------------------------------------------------------------------------------------------------ the kernel's arithmetic in f32
def _fma32(a, b, acc):
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def emulate(raw, layout, sr, target=TARGET, mutant=None):
    """The kernel on raw PCM (numpy int16 / float32 in `layout`) -> f32 [L_out]."""
    xs = planar(raw, layout)
    C, L = xs.shape
    scale = np.float32(1.0 / 32767.0) if mutant == "i16_scale_32767" else np.float32(2.0 ** -15)
    f = xs.astype(np.float32) * scale if xs.dtype == np.int16 else xs.astype(np.float32)
    m = np.zeros(L, np.float32)
    for c in range(C):
        m = (m + f[c]).astype(np.float32)
    if mutant != "mean_not_divided":
        m = (m * (np.float32(1.0) / np.float32(C))).astype(np.float32)
    identity = int(sr) == int(target) and mutant != "identity_through_sinc"
    if identity:
        tab, first, o, n, width = kernel_table(sr, target)
    elif mutant in ("phase_sign", "scale_dropped", "window_not_squared", "rolloff_one") or int(sr) == int(target):
        h32, o, n, width = table32(sr, target, mutant if int(sr) != int(target) else None)
        tab, first = h32, np.zeros(n, np.int32)                          # a mutated table is not compacted: its dropped taps need not be 0
    else:
        tab, first, o, n, width = kernel_table(sr, target)
    if mutant == "first_off_by_one":
        first = first + 1
    lead = width - 1 if mutant == "shifted_one_sample" else width
    L_out = (n * L + o - 1) // o
    K = 2 * width + o
    xpad = np.zeros(L + 2 * width + o + 2, np.float32)
    xpad[lead:lead + L] = m
    i = np.arange(L_out)
    q, p = i // n, i % n
    start = q * o + first[p]
    acc = np.zeros(L_out, np.float32)
    for k in range(tab.shape[1]):
        acc = _fma32(tab[p, k], xpad[start + k], acc)
    return acc


def emulate_case(case, mutant=None):
    c = CASES[case]
    return emulate(source(case), c["layout"], c["sr"], mutant=mutant)


# mutant -> the cases on at least one of which it must leave the bound
MUTANTS = {
    "phase_sign": ["44k_mono_f32", "22k_six_f32"],
    "scale_dropped": ["44k_mono_f32", "48k_stereo_f32"],
    "shifted_one_sample": ["44k_mono_f32", "8k_mono_i16"],
    "window_not_squared": ["44k_mono_f32", "48k_stereo_f32"],
    "rolloff_one": ["44k_mono_f32", "22k_six_f32"],
    "first_off_by_one": ["44k_stereo_i16", "8k_mono_i16"],
    "mean_not_divided": ["44k_stereo_i16", "22k_six_f32"],
    "i16_scale_32767": ["44k_stereo_i16", "8k_mono_i16"],
    "identity_through_sinc": ["16k_mono_f32", "16k_stereo_f32"],
}


# ------------------------------------------------------------------------------------------------------ the restatement check
SINES = [(44100, 1000.0), (48000, 440.0), (8000, 1000.0), (22050, 3000.0)]        # rate, tone


def sine_error(sr, tone, target=TARGET, drop=200):
    """max |chain64(sine at sr) - the analytic sine at the new rate| for an input of sr / 4 samples, `drop` samples left out at each end."""
    L = sr // 4
    x = np.sin(2 * math.pi * tone * np.arange(L) / sr).astype(np.float32).astype(np.float64)[None, :]
    y = chain64(x, sr, target)
    t = np.arange(len(y)) / target
    return float(np.abs(y - np.sin(2 * math.pi * tone * t))[drop:-drop].max())
