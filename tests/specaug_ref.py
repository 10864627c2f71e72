"""Host model of the SpecAugment kernels (csrc/specaug.hip) -- a helper, not a test.

The sampler below is normative: tav_specaug_draw must reproduce it bit for bit (include/tavhip.h, DESIGN.md §"Dropout RNG invariant").
  mix64  splitmix64's finaliser on Python ints masked to 64 bits (the dropout kernels' mixer)
  eps    = (mix64(seed ^ mix64(tag + 2^40)) >> 40) * 2^-24, one value per call
  n0     = floor(prob * len / length + eps) in numpy.float32, one rounded operation after the other
  n      = min(max(n0, min_masks), max(len - (length - 1), 0), L // length)
  starts = the n positions s in [0, len - length] with the smallest (mix64(seed ^ mix64(tag + row * L + s)), s)
fwd / bwd are modelled in float64 (the forward and dx are selects, so the comparison with them is exact)."""
import numpy as np

U64 = (1 << 64) - 1
TAG_TIME = 0x5350010000000000
TAG_FEATURE = 0x5350030000000000
EPS_STRIDE = 1 << 40
MAX_SPANS = 128


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & U64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & U64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & U64
    return x ^ (x >> 31)


def eps_of(seed, tag):
    return np.float32(mix64((seed & U64) ^ mix64((tag + EPS_STRIDE) & U64)) >> 40) * np.float32(2.0 ** -24)


def span_count(ln, L, prob, length, min_masks, eps):
    f = np.float32
    n0 = int(np.floor(f(f(f(prob) * f(ln)) / f(length)) + f(eps)))
    return min(max(n0, int(min_masks)), max(ln - (length - 1), 0), L // length)


def span_cap(L, prob, length, min_masks):
    """The static bound the library checks before it launches (> MAX_SPANS is refused)."""
    f = np.float32
    top = int(np.floor(f(f(f(prob) * f(L)) / f(length)) + f(1.0)))
    return min(max(int(min_masks), top), L // length)


def draw(valid, B, L, prob, length, min_masks, seed, tag):
    """-> (uint8 [B, L] mask, int32 [B] span counts, list of the chosen starts per row in the order they are chosen).
    valid: None or an array [B, L] whose non-zero entries count towards the row's length."""
    seed &= U64
    eps = eps_of(seed, tag)
    mask = np.zeros((B, L), dtype=np.uint8)
    nspans = np.zeros(B, dtype=np.int32)
    chosen = []
    for row in range(B):
        ln = L if valid is None else int(np.count_nonzero(np.asarray(valid)[row]))
        n = span_count(ln, L, prob, length, min_masks, eps)
        keys = sorted((mix64(seed ^ mix64((tag + row * L + s) & U64)), s) for s in range(max(ln - (length - 1), 0)))
        starts = [s for _, s in keys[:n]]
        for s in starts:
            mask[row, s:s + length] = 1
        nspans[row] = n
        chosen.append(starts)
    return mask, nspans, chosen


def fwd(x, tmask, fmask, embed, B, T):
    """float64 [B*T, H]: fmask ? 0 : (tmask ? embed : x).  tmask [B, T] / fmask [B, H] arrays or None."""
    x = np.asarray(x, dtype=np.float64)
    H = x.shape[1]
    y = x.copy()
    if tmask is not None:
        y[np.asarray(tmask).reshape(B * T) != 0] = np.asarray(embed, dtype=np.float64)
    if fmask is not None:
        y[np.repeat(np.asarray(fmask).reshape(B, 1, H) != 0, T, axis=1).reshape(B * T, H)] = 0.0
    return y


def bwd(dy, tmask, fmask, B, T):
    """-> (dx float64 [B*T, H], dembed float64 [H], k = number of time-masked rows)."""
    dy = np.asarray(dy, dtype=np.float64)
    H = dy.shape[1]
    tm = np.zeros(B * T, dtype=bool) if tmask is None else np.asarray(tmask).reshape(B * T) != 0
    fm = np.zeros((B * T, H), dtype=bool) if fmask is None else np.repeat(np.asarray(fmask).reshape(B, 1, H) != 0, T, axis=1).reshape(B * T, H)
    kept = np.where(fm, 0.0, dy)
    dx = np.where(tm[:, None], 0.0, kept)
    dembed = kept[tm].sum(axis=0) if tm.any() else np.zeros(H)
    return dx, dembed, int(tm.sum())
