"""fp64 references, per-element bounds, inputs, exact cases and an f32 emulation for the normalisation checks (numpy only: shared by the GPU cases
of kernel_checks.py and by tests/test_norm_reference_host.py, which tests this tester on the CPU).  Kernels: csrc/norm.hip.

LayerNorm (one wave64 per row; lane l holds the float4s l, l + 64, l + 128, l + 192 of the row):

    mean = wave_sum(sum over the lane's float4s of ((v0 + v1) + v2) + v3) / W       rstd = rsqrtf(sum (x - mean)^2 / W + eps)
    z = (x - mean) rstd gamma + beta                                                y = act ? gelu(z) : z
    d = act ? dy gelu'(z) : dy      dgamma = sum_rows d xhat      dbeta = sum_rows d      g = d gamma
    dx = (g - mean_c(g) - xhat mean_c(g xhat)) rstd (+ dx_add)

Group norm over time, x [B][T][C], per (b, c), T in 32 splits of per = ceil(T / 32) rows, four row groups per split:

    pivot = mean of n = min(T, 32) rows ((2 i + 1) T) / (2 n)         s0 = sum (x - pivot)      s1 = sum (x - pivot)^2
    m = s0 / T      mean = pivot + m      rstd = rsqrtf(max(s1 / T - m^2, 0) + eps)          y = gelu((x - mean) (rstd gamma) + beta)
    dz = dy gelu'(z)      S0 = sum_t dz      S1 = sum_t dz xhat      dbeta = sum_b S0      dgamma = sum_b S1
    dx = rstd gamma (dz - S0 / T - xhat S1 / T)

Inputs have SPREAD magnitudes (ln_inputs, gn_inputs) and are rounded to the storage dtype before the reference sees them.

Bounds, u = 2^-24.  Every f32 operation on values with error bounds is charged through class V: a sum or difference carries the operands' errors
and u (|result| + error), a product |a| e_b + |b| e_a + e_a e_b and the same rounding; a sum over a chain of D additions carries the summed
term errors and D u / (1 - D u) times the summed MAGNITUDES (no cancellation assumed).  The chains, from the source:

  LayerNorm row sums      4 additions per float4 the lane holds (ceil(W / 256) of them), then the six wave_sum steps.
  variance                sum (x - m_k)^2 = W var + W (mean - m_k)^2 exactly for whatever mean m_k the kernel found (sum (x - mean) = 0 is
                          algebra, not a cancellation of roundings): E_mean enters squared; each term carries 3u (difference, square).
  dgamma / dbeta          ceil(rows / (4 blocks)) rows per wave, 3 for the four-wave add, ceil(blocks / 64) + 64 in the reduce kernel, 1 when
                          it accumulates.
  group norm sums         ceil(per / 4) rows per thread, 3 for the four row groups, 32 splits; B entries more for dgamma / dbeta.
  group norm statistics   s1 / T = var (1 + kappa), kappa = (pivot - mean)^2 / var, and |m| = sqrt(kappa var): the accumulation error of the
                          variance is (D + 4) u var (1 + kappa), that of m (D + 2) u sqrt(var (1 + kappa)) (Cauchy-Schwarz on sum |x - pivot|),
                          and m^2 returns it times 2 |m|.  kappa is that of the documented pivot and NEVER more than KAPPA_CAP = 16 -- four
                          sigma, what a typical row is allowed: an algorithm that lets an atypical row become the pivot pays for it here.
  rsqrtf                  1 ulp = 2u (HIP math API); the error of its argument through 1 / sqrt(1 - e / v) - 1.
  GELU, stores            gemm_ref's terms (GELU_D1, GELU_D2, DCDF, half a bf16 ulp at |v| + E).  The flavour follows the LOW-PRECISION OUTPUT
                          type in the LayerNorm kernels (gelu_t<TL>) and the activation type in the group norm.

A backward is bounded ISOLATED (fed the reference's mean / rstd rounded to f32: error u |value|) or CHAINED (fed the kernel's own forward: error =
the forward bounds).

Exact cases: mean = 0 and rstd = 1 fed by hand, x, dy, dx_add integers in {-7 .. 7}, gamma in {+-1, +-2, +-4}, W (T) a power of two: every sum
in any order is an integer below 2^24 and every product and difference in dx fits 24 bits (exact_ok), so dgamma, dbeta and dx have ONE right
answer.  With the activation: beta = 32 and |x gamma| <= 16, so z is in [16, 48] where both GELU flavours return exactly z and exactly 1
(gelu_saturates: the exponential underflows, the cdf is 1 - 0).
"""
import functools
import math

import numpy as np

import gemm_ref as GR
from gemm_ref import F, U, bf16_half_ulp, bf16_rne, bf16_trunc, ratio  # noqa: F401

EPS = float(F(1e-5))
RSQ = 2 * U
LN_MAX_BLOCKS = 512
GN_SPLIT = 32
GN_PIVOT_ROWS = 32
KAPPA_CAP = 16.0

LN_W = (4, 64, 252, 260, 512, 768, 1024)
LN_ROWS = (1, 5, 17, 333)
LN_ROWS_BIG = 8192 + 37
GN_C = (64, 320, 512)
GN_T = (1, 2, 31, 33, 63, 64, 65, 127, 1023, 1025, 1599, 2081)


def ln_blocks(rows):
    return max(1, min(LN_MAX_BLOCKS, (rows + 15) // 16))


def gn_workspace_floats(B, C):
    return B * GN_SPLIT * C * 2 + B * C * 2 + B * C


def gn_pivot_rows(T):
    n = min(T, GN_PIVOT_ROWS)
    return [((2 * i + 1) * T) // (2 * n) for i in range(n)]


def rnd(x, dt):
    return GR.round_to(x, dt)[0]


# ---------------------------------------------------------------------------------------------- values with error bounds
def _g(n):
    return n * U / (1.0 - n * U)


class V:
    """An fp64 value with a bound of the error of the f32 quantity that stands for it."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, dtype=np.float64), np.asarray(e, dtype=np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def _addsub(self, o, sign):
        o = V.of(o)
        v, e = self.v + sign * o.v, self.e + o.e
        free = ((self.v == 0) & (self.e == 0)) | ((o.v == 0) & (o.e == 0))          # x + 0 is exact
        return V(v, e + np.where(free, 0.0, U * (np.abs(v) + e)))

    def __add__(self, o):
        return self._addsub(o, 1.0)

    def __sub__(self, o):
        return self._addsub(o, -1.0)

    def __mul__(self, o):
        o = V.of(o)
        v = self.v * o.v
        e = np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e
        return V(v, e + U * (np.abs(v) + e))

    def __getitem__(self, k):
        return V(self.v[k], np.broadcast_to(self.e, self.v.shape)[k])


def gsum(a, axis, D, extra=None):
    """Sum along `axis` through a chain of at most D additions; extra: a V added into the same chain (an accumulated previous value)."""
    e, mag, v = np.broadcast_to(a.e, a.v.shape).sum(axis), np.abs(a.v).sum(axis), a.v.sum(axis)
    if extra is not None:
        e, mag, v = e + extra.e, mag + np.abs(extra.v), v + extra.v
    return V(v, e + _g(D) * (mag + e))


def inv(n):
    """1.f / n as the kernels form it."""
    return V(1.0 / n, 0.0 if n & (n - 1) == 0 else U / n)


def rsq(v):
    rel = 1.0 / np.sqrt(1.0 - np.minimum(v.e / v.v, 0.5)) - 1.0
    r = 1.0 / np.sqrt(v.v)
    return V(r, r * (rel + RSQ * (1.0 + rel)))


def vgelu(z, dc):
    y = GR.gelu(z.v)
    return V(y, GR.GELU_D1 * z.e + np.abs(z.v) * dc + U * np.abs(y))


def vgelu_d(z, dc):
    d = GR.gelu_d(z.v)
    return V(d, GR.GELU_D2 * z.e + dc + 3 * U + U * np.abs(d))


def lp_bound(y):
    return y.e + bf16_half_ulp(np.abs(y.v) + y.e)


def fed(v):
    """A reference value rounded to f32, as an isolated backward is fed it."""
    v32 = np.asarray(v, dtype=np.float64).astype(F).astype(np.float64)
    return V(v, np.abs(v32 - v)), v32


# ---------------------------------------------------------------------------------------------- LayerNorm: inputs, reference, bounds
@functools.lru_cache(maxsize=8)
def ln_inputs(rows, W, xdt, dydt, seed=0):
    """Row r = randn 2^(r % 7 - 3) + offset_r, offset cycling through 0, 3 scale, 64 scale; the last row all zero (rows >= 2), the one before it
    constant (rows >= 3); gamma ~ 2^(c % 5 - 2), beta randn, dy columns 2^(c % 11 - 5), dx_add randn at the scale of dx, prev_g / prev_b what
    dgamma / dbeta hold before an accumulating call."""
    rng = np.random.default_rng(seed + 13 * rows + W)
    r, c = np.arange(rows), np.arange(W)
    sc = 2.0 ** (r % 7 - 3.0)
    x = rng.standard_normal((rows, W)) * sc[:, None] + (np.array([0.0, 3.0, 64.0])[r % 3] * sc)[:, None]
    if rows >= 2:
        x[rows - 1] = 0.0
    if rows >= 3:
        x[rows - 2] = 2.5
    f = lambda a: a.astype(F).astype(np.float64)          # noqa: E731
    cs = 2.0 ** (c % 11 - 5.0)
    return dict(rows=rows, W=W, xdt=xdt, dydt=dydt, x=rnd(x, xdt), gamma=f((1.0 + 0.1 * rng.standard_normal(W)) * 2.0 ** (c % 5 - 2.0)),
                beta=f(rng.standard_normal(W)), dy=rnd(rng.standard_normal((rows, W)) * cs, dydt),
                add=f(rng.standard_normal((rows, W)) / sc[:, None]), prev_g=f(rng.standard_normal(W) * cs * math.sqrt(rows)),
                prev_b=f(rng.standard_normal(W) * cs * math.sqrt(rows)))


def ln_chain(W):
    return 4 * -(-W // 256) + 6


def ln_ref_fwd(p, act=0, lp=True):
    """-> dict: mean, rstd, y_f32, y_lp (fp64), name + "_b" their bounds, "_mean" / "_rstd" the V pairs a chained backward is fed.  lp: a bf16
    output is requested (selects the GELU flavour)."""
    x, W = V(p["x"]), p["W"]
    D = ln_chain(W)
    mean = gsum(x, 1, D) * inv(W)
    dv = p["x"] - mean.v[:, None]
    dabs2 = ((np.abs(dv) + mean.e[:, None]) ** 2).sum(1)           # >= sum (x - m_k)^2 for the kernel's own mean m_k
    v = V((dv * dv).sum(1), W * mean.e ** 2 + _g(D + 3) * dabs2) * inv(W) + V(EPS)
    rstd = rsq(v)
    z = ((x - mean[:, None]) * rstd[:, None]) * V(p["gamma"]) + V(p["beta"])
    y = vgelu(z, GR.DCDF["bf16" if lp else "f32"]) if act else z
    return dict(mean=mean.v, mean_b=mean.e, rstd=rstd.v, rstd_b=rstd.e, y_f32=y.v, y_f32_b=y.e + 0 * y.v, y_lp=y.v, y_lp_b=lp_bound(y),
                _mean=mean, _rstd=rstd)


def ln_ref_bwd(p, mean, rstd, act=0, lp=True, add=True, accumulate=False, param_scale=None):
    """mean, rstd: V pairs of what the kernel is fed.  -> dx_f32, dx_lp, dgamma, dbeta and their "_b" bounds."""
    rows, W = p["rows"], p["W"]
    nb = ln_blocks(rows)
    x, dy, gam = V(p["x"]), V(p["dy"]), V(p["gamma"])
    xh = (x - mean[:, None]) * rstd[:, None]
    d = dy
    if act:
        d = dy * vgelu_d(xh * gam + V(p["beta"]), GR.DCDF["bf16" if lp else "f32"])
    Dg = -(-rows // (4 * nb)) + 3 + -(-nb // 64) + 64 + (1 if accumulate else 0)
    dg = gsum(d * xh, 0, Dg, V(p["prev_g"]) if accumulate else None)
    db = gsum(d, 0, Dg, V(p["prev_b"]) if accumulate else None)
    g = d * gam
    D = ln_chain(W)
    m1, m2 = gsum(g, 1, D) * inv(W), gsum(g * xh, 1, D) * inv(W)
    dx = ((g - m1[:, None]) - xh * m2[:, None]) * rstd[:, None]
    if add:
        dx = dx + V(p["add"])
    return dict(dx_f32=dx.v, dx_f32_b=dx.e + 0 * dx.v, dx_lp=dx.v, dx_lp_b=lp_bound(dx), dgamma=dg.v, dgamma_b=dg.e, dbeta=db.v, dbeta_b=db.e)


# ---------------------------------------------------------------------------------------------- group norm: inputs, reference, bounds
@functools.lru_cache(maxsize=8)
def gn_inputs(B, T, C, dt, seed=0, onset=False):
    """Channel c of entry b = randn 2^(c % 7 - 3) + 2^(c % 5 - 2) over time; onset: the FIRST row sits 32 sigma (even channels) or 256 sigma
    (odd channels) off the channel's mean."""
    rng = np.random.default_rng(seed + 7 * T + C + B)
    c = np.arange(C)
    sig, mu = 2.0 ** (c % 7 - 3.0), 2.0 ** (c % 5 - 2.0)
    x = rng.standard_normal((B, T, C)) * sig + mu
    if onset:
        x[:, 0, :] = mu + np.where(c % 2 == 0, 32.0, 256.0) * sig
    f = lambda a: a.astype(F).astype(np.float64)          # noqa: E731
    cs = 2.0 ** (c % 11 - 5.0)
    return dict(B=B, T=T, C=C, dt=dt, x=rnd(x, dt), gamma=f((1.0 + 0.1 * rng.standard_normal(C)) * 2.0 ** (c % 3 - 1.0)),
                beta=f(0.5 * rng.standard_normal(C)), dy=rnd(rng.standard_normal((B, T, C)) * cs, dt),
                prev_g=f(rng.standard_normal(C) * cs * math.sqrt(B * T)), prev_b=f(rng.standard_normal(C) * cs * math.sqrt(B * T)))


def gn_chain(T):
    per = -(-T // GN_SPLIT)
    return -(-per // 4) + 3 + GN_SPLIT


def gn_kappa(x):
    """kappa of the documented pivot per (b, c), capped."""
    T = x.shape[1]
    mu, var = x.mean(1), x.var(1)
    piv = x[:, gn_pivot_rows(T), :].mean(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(var > 0, (piv - mu) ** 2 / var, 0.0)
    return np.minimum(k, KAPPA_CAP)


def gn_ref_fwd(p):
    """-> mean, rstd [B][C], y [B][T][C] and "_b" bounds, "_mean" / "_rstd" V pairs."""
    x, T = p["x"], p["T"]
    D = gn_chain(T)
    mu, var = x.mean(1), x.var(1)
    kap = gn_kappa(x)
    Q = var * (1.0 + kap)
    m_abs = np.sqrt(kap * var)
    Em = _g(D + 2) * np.sqrt(Q)
    mean = V(mu, Em + U * (np.abs(mu) + Em))
    Ev = _g(D + 4) * Q + 2 * m_abs * Em + Em ** 2 + U * m_abs ** 2 + U * (Q + m_abs ** 2)
    rstd = rsq(V(var, Ev) + V(EPS))
    dc = GR.DCDF[p["dt"]]
    y = vgelu((V(x) - mean[:, None, :]) * (rstd * V(p["gamma"]))[:, None, :] + V(p["beta"]), dc)
    return dict(mean=mean.v, mean_b=mean.e, rstd=rstd.v, rstd_b=rstd.e, y=y.v, y_b=lp_bound(y) if p["dt"] == "bf16" else y.e + 0 * y.v,
                _mean=mean, _rstd=rstd)


def gn_ref_bwd(p, mean, rstd, accumulate=False):
    x, T, B = V(p["x"]), p["T"], p["B"]
    D = gn_chain(T)
    dc = GR.DCDF[p["dt"]]
    gam = V(p["gamma"])
    xh = (x - mean[:, None, :]) * rstd[:, None, :]
    dz = V(p["dy"]) * vgelu_d(xh * gam + V(p["beta"]), dc)
    S0, S1 = gsum(dz, 1, D), gsum(dz * xh, 1, D)
    db = gsum(S0, 0, B + (1 if accumulate else 0), V(p["prev_b"]) if accumulate else None)
    dg = gsum(S1, 0, B + (1 if accumulate else 0), V(p["prev_g"]) if accumulate else None)
    k0, k1 = S0 * inv(T), S1 * inv(T)
    dx = (rstd * gam)[:, None, :] * ((dz - k0[:, None, :]) - xh * k1[:, None, :])
    return dict(dx=dx.v, dx_b=lp_bound(dx) if p["dt"] == "bf16" else dx.e + 0 * dx.v, dgamma=dg.v, dgamma_b=dg.e, dbeta=db.v, dbeta_b=db.e)


# ---------------------------------------------------------------------------------------------- exact cases
def _ints(rng, shape, lo=-7, hi=7):
    a = rng.integers(lo, hi + 1, size=shape).astype(np.float64)
    a.flat[0], a.flat[-1] = hi, lo
    return a


def exact_ok(rows, W, T=1024, B=3):
    """The bit budget of the largest exact case: every intermediate of the integer construction below fits a 24-bit significand."""
    ln = (rows * 49 + 7 * 64 < 2 ** 24                     # dgamma: sum d xhat (+ an integer previous value), any order
          and W * 28 * 7 < 2 ** 24                         # sum_c g xhat, g = d gamma <= 28
          and (28 + 28 + 7 * 196) * W < 2 ** 24            # g - m1 - xhat m2 in units of 1 / W
          and W & (W - 1) == 0)
    gn = B * T * 28 + 7 * 64 < 2 ** 24 and (7 + 7 + 4 * 28) * T < 2 ** 24 and T & (T - 1) == 0
    return ln and gn


def ln_exact_case(rows, W, xdt, dydt, act, seed=0):
    """Integer operands for a backward fed mean = 0, rstd = 1; act: beta = 32 and |x gamma| <= 16 (saturated GELU).  -> inputs and the one right
    answer (dx, dgamma, dbeta with accumulation onto prev_g / prev_b)."""
    rng = np.random.default_rng(seed + rows + W)
    x = _ints(rng, (rows, W), -4, 4) if act else _ints(rng, (rows, W))
    gam = rng.choice([1.0, -1.0, 2.0, -2.0, 4.0, -4.0], size=W)
    p = dict(rows=rows, W=W, xdt=xdt, dydt=dydt, x=x, gamma=gam, beta=np.full(W, 32.0) if act else np.zeros(W), dy=_ints(rng, (rows, W)),
             add=_ints(rng, (rows, W)), prev_g=_ints(rng, (W,)) * 64, prev_b=_ints(rng, (W,)) * 64)
    g = p["dy"] * gam
    dx = g - g.mean(1, keepdims=True) - x * (g * x).mean(1, keepdims=True) + p["add"]
    p.update(want_dx=dx, want_dg=(p["dy"] * x).sum(0), want_db=p["dy"].sum(0))
    return p


def gn_exact_case(B, T, C, dt, seed=0):
    """Integer operands for the group norm: backward fed stats = (0, 1) with beta = 32, |x gamma| <= 16."""
    rng = np.random.default_rng(seed + T + C)
    x = _ints(rng, (B, T, C), -4, 4)
    gam = rng.choice([1.0, -1.0, 2.0, -2.0, 4.0, -4.0], size=C)
    p = dict(B=B, T=T, C=C, dt=dt, x=x, gamma=gam, beta=np.full(C, 32.0), dy=_ints(rng, (B, T, C)), prev_g=_ints(rng, (C,)) * 64,
             prev_b=_ints(rng, (C,)) * 64)
    dz = p["dy"]
    p.update(want_dx=gam * (dz - dz.mean(1, keepdims=True) - x * (dz * x).mean(1, keepdims=True)), want_dg=(dz * x).sum((0, 1)), want_db=dz.sum((0, 1)),
             want_mean=x.mean(1))
    return p


def ln_stats_case(rows, W, seed=0):
    """Forward rows with one right mean: even rows +-a in equal number in a shuffled column order, a = 2^(r % 9 - 4) -> mean 0; odd rows the
    constant integer r % 15 - 7 -> mean = it and y = beta.  W a power of two."""
    rng = np.random.default_rng(seed + rows + W)
    x = np.empty((rows, W))
    for r in range(rows):
        x[r] = rng.permutation(np.repeat([1.0, -1.0], W // 2)) * 2.0 ** (r % 9 - 4) if r % 2 == 0 else float(r % 15 - 7)
    return dict(rows=rows, W=W, x=x, gamma=rng.choice([1.0, -2.0, 0.5], size=W), beta=rng.standard_normal(W).astype(F).astype(np.float64),
                want_mean=np.where(np.arange(rows) % 2 == 0, 0.0, np.arange(rows) % 15 - 7.0))


def gelu_saturates(flavour):
    """Both GELU forms of this flavour ("f32": erff / __expf, "bf16": gelu_parts_fast) return exactly z and exactly 1 on [16, 48]."""
    z = np.concatenate([np.arange(16, 49, dtype=np.float64), np.linspace(16, 48, 4097)]).astype(F)
    y, d = GR._emu_gelu_both(z, flavour)
    return bool(np.array_equal(y, z) and np.all(d == F(1.0)))


# ---------------------------------------------------------------------------------------------- f32 emulation
LN_MUTANTS = {1: "raw_moment_variance", 2: "variance_over_w_minus_1", 3: "eps_outside_sqrt", 4: "last_float4_not_in_mean", 5: "w_for_pitch",
              6: "dx_without_m2", 7: "dx_add_before_rstd", 8: "next_rows_stats", 9: "dgamma_first_pass_only", 10: "dgamma_from_dy_gamma",
              11: "gelu_grad_at_xhat", 12: "bf16_store_truncates", 13: "accumulate_overwrites", 14: "reduce_drops_rows_ge_64"}
GN_MUTANTS = {15: "raw_moment_variance", 16: "stats_pass_uses_entry_0_pivot", 17: "boundary_row_twice", 18: "ragged_split_dropped", 19: "unbiased_variance",
              20: "dgamma_dbeta_exchanged", 21: "sums_not_over_t", 22: "stats_of_neighbour_channel"}
_IDX = np.arange(64)


def _f(a):
    return np.asarray(a, dtype=np.float64).astype(F)


def _lanes(a):
    """[rows][W] f32 -> [rows][4][64][4]: float4 c = lane + 64 j of a row zero-padded to 1024."""
    rows, W = a.shape
    out = np.zeros((rows, 1024), dtype=F)
    out[:, :W] = a
    return out.reshape(rows, 4, 64, 4)


def _wave_sum(s, rev):
    for o in ((1, 2, 4, 8, 16, 32) if rev else (32, 16, 8, 4, 2, 1)):
        s = s + s[:, _IDX ^ o]
    return s[:, 0]


def _row_sum(a, rev=False):
    t = _lanes(a)
    s = np.zeros((a.shape[0], 64), dtype=F)
    for j in ((3, 2, 1, 0) if rev else (0, 1, 2, 3)):
        s = s + (((t[:, j, :, 0] + t[:, j, :, 1]) + t[:, j, :, 2]) + t[:, j, :, 3])
    return _wave_sum(s, rev)


def _rsqrt(v):
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(F)


def _store_lp(v, mut=None):
    return (bf16_trunc if mut == "bf16_store_truncates" else bf16_rne)(v)


def emu_ln_fwd(p, act=0, lp=True, rev=False, mut=None, pitch=0):
    """-> dict mean, rstd, y_f32, y_lp (float64 of what the f32 / bf16 outputs hold).  pitch: extra elements between rows (only mutant 5 notices)."""
    x, W = _f(p["x"]), p["W"]
    rows = x.shape[0]
    if mut == "w_for_pitch" and pitch:
        wide = np.full((rows, W + pitch), np.nan, dtype=F)
        wide[:, :W] = x
        x = wide.reshape(-1)[:rows * W].reshape(rows, W)
    invW = F(1.0) / F(W)
    xs = x
    if mut == "last_float4_not_in_mean":
        xs = x.copy()
        xs[:, W - 4:] = 0
    mean = _row_sum(xs, rev) * invW
    if mut == "raw_moment_variance":
        var = _row_sum(x * x, rev) * invW - mean * mean
    else:
        d = x - mean[:, None]
        var = _row_sum(d * d, rev) * (F(1.0) / F(W - 1) if mut == "variance_over_w_minus_1" else invW)
    eps = F(EPS)
    rstd = (F(1.0) / (np.sqrt(var) + eps)).astype(F) if mut == "eps_outside_sqrt" else _rsqrt(var + eps)
    y = ((x - mean[:, None]) * rstd[:, None]) * _f(p["gamma"]) + _f(p["beta"])
    if act:
        y = GR._emu_gelu_both(y, "bf16" if lp else "f32")[0]
    return dict(mean=mean.astype(np.float64), rstd=rstd.astype(np.float64), y_f32=y.astype(np.float64), y_lp=_store_lp(y, mut))


def emu_ln_bwd(p, mean, rstd, act=0, lp=True, add=True, accumulate=False, rev=False, mut=None):
    """The backward with its real summation structure: per-wave row chains at a stride of 4 blocks, the four-wave add, the two-stage reduce of
    ln_param_reduce(_multi)_kernel.  mean, rstd: what the kernel is fed.  -> dx_f32, dx_lp, dgamma, dbeta (float64)."""
    x, dy, gam = _f(p["x"]), _f(p["dy"]), _f(p["gamma"])
    rows, W = x.shape
    nb = ln_blocks(rows)
    stride = 4 * nb
    mean, rstd = _f(mean), _f(rstd)
    if mut == "next_rows_stats":
        nxt = np.where(np.arange(rows) + stride < rows, np.arange(rows) + stride, np.arange(rows))       # the wave's next row
        mean, rstd = mean[nxt], rstd[nxt]
    invW = F(1.0) / F(W)
    xh = (x - mean[:, None]) * rstd[:, None]
    d = dy
    if act:
        z = xh if mut == "gelu_grad_at_xhat" else xh * gam + _f(p["beta"])
        d = dy * GR._emu_gelu_both(z, "bf16" if lp else "f32")[1]
    g = d * gam
    m1, m2 = _row_sum(g, rev) * invW, _row_sum(g * xh, rev) * invW
    a = _f(p["add"]) if add else None
    if mut == "dx_without_m2":
        dx = (g - m1[:, None]) * rstd[:, None]
    elif mut == "dx_add_before_rstd" and add:
        dx = (((g - m1[:, None]) - xh * m2[:, None]) + a) * rstd[:, None]
    else:
        dx = ((g - m1[:, None]) - xh * m2[:, None]) * rstd[:, None]
    if add and mut != "dx_add_before_rstd":
        dx = dx + a
    out = dict(dx_f32=dx.astype(np.float64), dx_lp=_store_lp(dx, mut))
    for name, term, prev in (("dgamma", (g if mut == "dgamma_from_dy_gamma" else d) * xh, p["prev_g"]), ("dbeta", d, p["prev_b"])):
        acc = np.zeros((stride, W), dtype=F)
        K = -(-rows // stride)
        for k in (range(K - 1, -1, -1) if rev else range(K)):
            if mut == "dgamma_first_pass_only" and name == "dgamma" and k > 0:
                continue
            n = min(stride, rows - k * stride)
            acc[:n] = acc[:n] + term[k * stride:k * stride + n]
        w4 = acc.reshape(nb, 4, W)
        part = ((w4[:, 0] + w4[:, 1]) + w4[:, 2]) + w4[:, 3]
        red = np.zeros((64, W), dtype=F)
        for i in range(-(-nb // 64)):
            if mut == "reduce_drops_rows_ge_64" and i > 0:
                break
            n = min(64, nb - 64 * i)
            red[:n] = red[:n] + part[64 * i:64 * i + n]
        s = np.zeros(W, dtype=F)
        for k in (range(63, -1, -1) if rev else range(64)):
            s = s + red[k]
        if accumulate and mut != "accumulate_overwrites":
            s = _f(prev) + s
        out[name] = s.astype(np.float64)
    return out


def emu_gn_pivot(x, old=False):
    """[B][C] f32: the pivot of the forward statistics; old: the entry's first row (the kernel before the sampled pivot)."""
    if old:
        return x[:, 0, :].copy()
    rows = gn_pivot_rows(x.shape[1])
    s = np.zeros_like(x[:, 0, :])
    for t in rows:
        s = s + x[:, t, :]
    return s * (F(1.0) / F(len(rows)))


def _gn_split_sums(t0, t1, T, rev, mut):
    """Per-split sums of the [B][T][C] f32 term arrays t0, t1 in the kernel's structure -> two [B][32][C] arrays of partials."""
    B, _, C = t0.shape
    per = -(-T // GN_SPLIT)
    parts = [np.zeros((B, GN_SPLIT, C), dtype=F) for _ in range(2)]
    for sp in range(GN_SPLIT):
        lo, hi = sp * per, min(sp * per + per, T)
        if mut == "boundary_row_twice" and lo < hi < T:
            hi += 1
        if mut == "ragged_split_dropped" and lo < T and sp * per + per > T:
            hi = lo
        for which, t in enumerate((t0, t1)):
            acc = np.zeros((B, 4, C), dtype=F)
            starts = range(lo, hi, 4)
            for s in (reversed(starts) if rev else starts):
                n = min(4, hi - s)
                acc[:, :n] = acc[:, :n] + t[:, s:s + n]
            parts[which][:, sp] = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    return parts


def _chain(parts, rev):
    s = np.zeros_like(parts[:, 0])
    n = parts.shape[1]
    for k in (range(n - 1, -1, -1) if rev else range(n)):
        s = s + parts[:, k]
    return s


def emu_gn_fwd(p, rev=False, mut=None, old_pivot=False):
    """-> mean, rstd [B][C], y [B][T][C] as float64 of what the outputs hold."""
    x, T = _f(p["x"]), p["T"]
    piv = emu_gn_pivot(x, old_pivot)
    if mut == "raw_moment_variance":
        piv = np.zeros_like(piv)
    ps = np.broadcast_to(piv[:1], piv.shape) if mut == "stats_pass_uses_entry_0_pivot" else piv          # (the statistics pass alone: finalize adds the entry's own)
    d = x - ps[:, None, :]
    p0, p1 = _gn_split_sums(d, d * d, T, rev, mut)
    s0, s1 = _chain(p0, rev), _chain(p1, rev)
    Tf = F(T)
    m = s0 / Tf
    var = s1 / Tf - m * m
    if mut == "unbiased_variance" and T > 1:
        var = var * (Tf / F(T - 1))
    var = np.maximum(var, F(0.0))
    mean, rstd = piv + m, _rsqrt(var + F(EPS))
    am, ar = mean, rstd
    if mut == "stats_of_neighbour_channel":
        nb = np.arange(x.shape[2]) ^ 1
        am, ar = mean[:, nb], rstd[:, nb]
    y = (x - am[:, None, :]) * (ar * _f(p["gamma"]))[:, None, :] + _f(p["beta"])
    y = GR._emu_gelu_both(y, p["dt"])[0]
    return dict(mean=mean.astype(np.float64), rstd=rstd.astype(np.float64), y=bf16_rne(y) if p["dt"] == "bf16" else y.astype(np.float64))


def emu_gn_bwd(p, mean, rstd, accumulate=False, rev=False, mut=None):
    x, T, B = _f(p["x"]), p["T"], p["B"]
    mean, rstd, gam, bet = _f(mean), _f(rstd), _f(p["gamma"]), _f(p["beta"])
    if mut == "stats_of_neighbour_channel":
        nb = np.arange(x.shape[2]) ^ 1
        mean, rstd = mean[:, nb], rstd[:, nb]
    xh = (x - mean[:, None, :]) * rstd[:, None, :]
    dz = _f(p["dy"]) * GR._emu_gelu_both(xh * gam + bet, p["dt"])[1]
    p0, p1 = _gn_split_sums(dz, dz * xh, T, rev, None)
    S0, S1 = _chain(p0, rev), _chain(p1, rev)
    db, dg = _chain(S0[None], rev)[0], _chain(S1[None], rev)[0]
    if accumulate:
        dg, db = _f(p["prev_g"]) + dg, _f(p["prev_b"]) + db
    if mut == "dgamma_dbeta_exchanged":
        dg, db = db, dg
    invT = F(1.0) if mut == "sums_not_over_t" else F(1.0) / F(T)
    k0, k1 = S0 * invT, S1 * invT
    dx = (rstd * gam)[:, None, :] * ((dz - k0[:, None, :]) - xh * k1[:, None, :])
    return dict(dx=bf16_rne(dx) if p["dt"] == "bf16" else dx.astype(np.float64), dgamma=dg.astype(np.float64), dbeta=db.astype(np.float64))


# ---------------------------------------------------------------------------------------------- ratios
def ratios(got, ref, names, sfx="_b"):
    return {n: ratio(got[n], ref[n], ref[n + sfx]) for n in names if n in got and got[n] is not None}


LN_FWD_OUT = ("mean", "rstd", "y_f32", "y_lp")
LN_BWD_OUT = ("dx_f32", "dx_lp", "dgamma", "dbeta")
GN_FWD_OUT = ("mean", "rstd", "y")
GN_BWD_OUT = ("dx", "dgamma", "dbeta")
