"""fp64 reference, per-element bounds, inputs and an f32 emulation for the GEMM checks (numpy only: shared by the GPU cases of kernel_checks.py and
by tests/test_gemm_reference_host.py, which tests this tester on the CPU).

The epilogue, in the order include/tavhip.h documents and csrc/gemm.hip runs it:

    v = alpha * sum_k a[m][k] b[n][k] + bias[n]          C_pre = (act & 2) ? gelu'(v) : v
    if act & 1:  v = gelu_erf(v)
    if gelu_in:  v *= (act & 4) ? gelu_in[m][n] : gelu'(gelu_in[m][n])
    v += resid[m][n];  v += C[m][n] (accumulate);  C = v

Inputs have SPREAD magnitudes: a[m][k] = randn * 2^(m % 13 - 6), b[n][k] = 0.1 * randn * 2^(n % 11 - 5), both periods coprime to every tile edge,
rounded to the operand dtype before the reference sees them; bias follows the column scale, the f32 residual the product of both.  Row m of the
output is 2^(m % 13 - 6) times as large as row 0: a value that belongs into a large row is grossly wrong in a small one, and in the small rows the
bias dominates the product, so the epilogue is checked almost free of accumulation error.  For the weight gradients (TN) the scales sit on the N1
and N2 columns and the token axis stays randn.

Bounds per output element, u = 2^-24.  S = sum_k |a||b| in fp64.

  accumulation     E_acc = D * 2u * |alpha| * S.  2u, not u, because nothing documents that the matrix unit rounds its internal additions to
                   nearest: 2u |x| >= one ulp of x covers a truncating adder.  D is the longest chain of additions a product goes through, from
                   the source: one MFMA takes KM products (bf16 16x16x32: 32, f32 16x16x4: 4, e4m3 16x16x128: 128) and the running accumulator, so
                   in whatever order and at whatever alignment it adds them a product passes at most KM + 1 additions inside it, then one per later
                   MFMA of the chain, ceil(L / KM) of them for a reduction of length L, then one per slab of a split reduction: D = KM + 1 +
                   ceil(L / KM) + nsplit (+ 1 for f32 operands, whose products are not exact in f32).  It depends on no order, tile, ring depth or
                   split, only on L and an upper limit of the split count.
  alpha, bias      v = acc * alpha + bias is at most two roundings: u |alpha| S + u (|alpha| S + |bias|).  fp8: alpha = alpha * sa * sb, two more
                   f32 multiplies, 2u |alpha| S.
  GELU             E' = 1.13 E + |x| dcdf + u |y|  (|gelu'| <= 1.13);  gelu': E' = 0.8 E + dcdf + 3u + u |d|  (|gelu''| <= 0.8).  dcdf, the absolute
                   error of the normal cdf the kernel evaluates:
                     bf16 / fp8 operands (gelu_parts_fast, common.h): half of the documented |erf error| <= 1.5e-7 of Abramowitz-Stegun 7.1.26, plus
                       the f32 evaluation: v_rcp_f32 and v_exp_f32 are 1 ulp = 2u each (ISA guide), t = rcp(1 + p z) then carries 4u, the quintic
                       in t in [0, 1] has slope <= 3.5 (14u) and five Horner steps on partial sums <= 1.5 (8u), the exponent -z^2 log2(e) carries
                       3u of itself and e * |exponent| <= 0.54 (1.2u), the product and the subtraction 2u more: 0.5 * (1.5e-7 + 28u) + u = 15u + 7.5e-8;
                     f32 operands (erff): 4 ulp = 8u (HIP math API), its argument x / sqrt(2) 2u * max x erf'(x/sqrt 2)/sqrt 2 <= u, 1 + erf u:
                       0.5 * 10u + u = 6u.
                   The exponential of gelu' (exp2 / __expf: 2u relative plus 3u of the exponent, times x e^(-x^2/2) <= 0.61 and x^3 e^(-x^2/2) <= 1.16,
                   times 0.4) stays below 3u.
  gelu_in, resid,  each f32 multiply or add: u times the magnitudes entering it; a differentiated gelu_in (an exact input) carries dcdf + 3u + u |g|.
  accumulate
  store            f32: u |v|.  bf16: HALF AN ULP of bf16 at |v| + E, that is 2^-9 times the power of two above |v| + E.  (2^-9 |v| itself is below
                   what round-to-nearest-even may err by -- half an ulp is between 2^-9 |v| and 2^-8 |v| -- and 2^-8 |v| would let a truncating store,
                   which errs by up to one ulp, pass at large significands.)
  dbias            (rows + 2) * 2u * |scale| * sum |a|  (+ u (|v| + |previous|) when it accumulates): rows >= every chain the column sums take.

Exact integer operands: values in {-7 .. 7}, integer bias, alpha = 1, no activation.  Every product and every partial sum in any order is an
integer below 2^24 (int_exact_ok), so an f32 output equals the fp64 reference bit for bit and a bf16 output its round-to-nearest-even; with
amax = 7 the fp8 scales 448 / 7 = 64 and 7 / 448 = 2^-6 are powers of two and 64 x is exact in e4m3, so the fp8 GEMM is exact as well.
"""
import math

import numpy as np

from step_end_ref import ratio  # noqa: F401  (worst |got - ref| / bound; a zero bound demands equality, non-finite is infinitely wrong)

U = 2.0 ** -24
UB = 2.0 ** -9                                            # half a bf16 ulp relative to the power of two ABOVE the value
F = np.float32
MFMA_K = {"bf16": 32, "f32": 4, "fp8": 128}               # products one MFMA adds into the accumulator
CHUNK = {"bf16": 8, "f32": 4, "fp8": 16}                  # elements per 16-byte chunk
KTILE = {"bf16": 64, "f32": 32, "fp8": 128}               # elements per 128-byte K-tile row of the NT kernels
ERF_FAST_ERR = 1.5e-7                                     # common.h, gelu_parts_fast
DCDF = {"bf16": 0.5 * (ERF_FAST_ERR + 28 * U) + U, "fp8": 0.5 * (ERF_FAST_ERR + 28 * U) + U, "f32": 6 * U}
GELU_D1, GELU_D2 = 1.13, 0.8                              # sup |gelu'|, sup |gelu''|

try:                                                      # (the same function either way; scipy's is merely vectorised)
    from scipy.special import erf as _erf
except Exception:                                         # pragma: no cover
    _erf = np.frompyfunc(math.erf, 1, 1)


def erf(x):
    return np.asarray(_erf(np.asarray(x, dtype=np.float64)), dtype=np.float64)


def gelu(x):
    return 0.5 * x * (1.0 + erf(x / math.sqrt(2.0)))


def gelu_d(x):
    return 0.5 * (1.0 + erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ---------------------------------------------------------------------------------------------- number formats
def bf16_rne(x):
    """x rounded to bfloat16 (nearest even), returned as float64."""
    b = np.ascontiguousarray(np.asarray(x, dtype=F)).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(F).astype(np.float64).reshape(np.shape(x))


def bf16_trunc(x):
    b = np.ascontiguousarray(np.asarray(x, dtype=F)).view(np.uint32) & np.uint32(0xFFFF0000)
    return b.view(F).astype(np.float64).reshape(np.shape(x))


def bf16_half_ulp(mag):
    """Half an ulp of bfloat16 at magnitude `mag` (> 0): 2^-9 times the power of two above it."""
    mag = np.maximum(np.asarray(mag, dtype=np.float64), 2.0 ** -126)
    return UB * 2.0 ** (np.floor(np.log2(mag)) + 1.0)


def e4m3_rne(x):
    """x (|x| <= 448) rounded to OCP e4m3 (nearest even, subnormals below 2^-6), as float64."""
    x = np.asarray(x, dtype=np.float64)
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -40)))
    step = 2.0 ** (np.maximum(e, -6.0) - 3.0)
    return np.clip(np.rint(x / step) * step, -448.0, 448.0)


def round_to(x, dtype):
    """x as the operand dtype holds it -> (float64 values, dequantisation factor).  fp8: per-tensor scaling as tav_fp8_amax / tav_fp8_quantize do
    it (q = e4m3(x * f32(448 / amax)), the GEMM multiplies by f32(amax / 448)); the values returned are the q themselves."""
    x = np.asarray(x, dtype=np.float64)
    if dtype == "bf16":
        return bf16_rne(x), 1.0
    if dtype == "f32":
        return x.astype(F).astype(np.float64), 1.0
    amax = F(np.abs(x.astype(F)).max())
    return e4m3_rne(x.astype(F).astype(np.float64) * float(F(448.0) / amax)), float(amax / F(448.0))


def side_dtype(dtype):
    return "f32" if dtype == "f32" else "bf16"


# ---------------------------------------------------------------------------------------------- inputs
def row_scale(n):
    return 2.0 ** ((np.arange(n) % 13) - 6.0)


def col_scale(n):
    return 2.0 ** ((np.arange(n) % 11) - 5.0)


def nt_inputs(M, N, K, dtype, seed):
    """Operands and every side tensor of one NT problem.  a, b: float64 arrays of the values the operand dtype holds (fp8: the e4m3 values q, with
    sa / sb the dequantisation factors; else sa = sb = 1); bias, resid f32; gin (a pre-activation) and gin_d (a stored derivative) in the side dtype;
    cprev_f32 / cprev_bf16 what C holds before an accumulating call."""
    rng = np.random.default_rng(seed)
    rs, cs = row_scale(M)[:, None], col_scale(N)[:, None]
    a, sa = round_to(rng.standard_normal((M, K)) * rs, dtype)
    b, sb = round_to(0.1 * rng.standard_normal((N, K)) * cs, dtype)
    out_scale = rs * cs.T * 0.1 * math.sqrt(K)
    sd = side_dtype(dtype)
    cprev = rng.standard_normal((M, N)) * out_scale
    return dict(a=a, b=b, sa=sa, sb=sb, dtype=dtype,
                bias=(rng.standard_normal(N) * cs[:, 0]).astype(F).astype(np.float64),
                resid=(rng.standard_normal((M, N)) * rs * cs.T).astype(F).astype(np.float64),
                gin=round_to(rng.standard_normal((M, N)) * 1.5, sd)[0],
                gin_d=round_to(gelu_d(rng.standard_normal((M, N)) * 1.5), sd)[0],
                cprev_f32=cprev.astype(F).astype(np.float64), cprev_bf16=bf16_rne(cprev))


def tn_inputs(T, N1, N2, dtype, seed):
    """A [T][N1] = randn * 2^(n1 % 13 - 6), B [T][N2] = 0.1 randn * 2^(n2 % 11 - 5), rounded to the operand dtype; prev / prev_b: what out / dbias
    hold before an accumulating call."""
    rng = np.random.default_rng(seed)
    a = round_to(rng.standard_normal((T, N1)) * row_scale(N1)[None, :], dtype)[0]
    b = round_to(0.1 * rng.standard_normal((T, N2)) * col_scale(N2)[None, :], dtype)[0]
    prev = (rng.standard_normal((N1, N2)) * row_scale(N1)[:, None] * col_scale(N2)[None, :] * 0.1 * math.sqrt(T)).astype(F).astype(np.float64)
    prev_b = (rng.standard_normal(N1) * row_scale(N1) * math.sqrt(T)).astype(F).astype(np.float64)
    return dict(a=a, b=b, prev=prev, prev_b=prev_b, dtype=dtype)


def int_tensor(shape, seed):
    """Integers in {-7 .. 7} as float64, at least one +7 and one -7 (so amax = 7 exactly)."""
    x = np.random.default_rng(seed).integers(-7, 8, size=shape).astype(np.float64)
    x.flat[0], x.flat[-1] = 7.0, -7.0
    return x


def int_exact_ok(L):
    """A reduction of L products of values in {-7 .. 7} (times 64 each on the fp8 path) plus an integer bias of the same range never needs more than
    24 bits of significand: L * 49 * 64^2 + 7 * 64^2 < 2^24 * 64^2."""
    return (L * 49 + 7) * 64 ** 2 < 2 ** 24 * 64 ** 2


# ---------------------------------------------------------------------------------------------- reference and bounds
def chain_len(L, dtype, nsplit=0):
    """D of the module docstring: the longest chain of additions between a product and the stored sum."""
    km = MFMA_K[dtype]
    return km + 1 + -(-L // km) + nsplit + (1 if dtype == "f32" else 0)


def _rnd(val, err):
    """err after one more f32 rounding of a result whose true value is val."""
    return err + U * (np.abs(val) + err)


def _store(val, err, out_dtype):
    if out_dtype == "bf16":
        return err + bf16_half_ulp(np.abs(val) + err)
    return _rnd(val, err)


def nt_ref(x, *, alpha=1.0, bias=False, act=0, want_pre=False, gelu_in=None, resid=False, accumulate=False, out_dtype=None, L=None):
    """x = nt_inputs(...).  gelu_in: None, "gin" (differentiated unless act & 4) or "gin_d".  -> dict(out, out_bound[, pre, pre_bound]), fp64.
    L: the reduction length the bound assumes (default K)."""
    dtype = x["dtype"]
    out_dtype = out_dtype or side_dtype(dtype)
    a, b = x["a"], x["b"]
    alpha_k = float(F(alpha))                                   # the ABI takes alpha as f32
    al = alpha_k * x["sa"] * x["sb"]
    dot, S = a @ b.T, np.abs(a) @ np.abs(b).T
    aS = abs(al) * S
    err = chain_len(L or a.shape[1], dtype) * 2 * U * aS + (2 * U * aS if dtype == "fp8" else 0.0)
    v = al * dot
    err = err + U * aS                                          # acc * alpha
    if bias:
        v = v + x["bias"][None, :]
        err = err + U * (aS + np.abs(x["bias"])[None, :] + err)
    res = {}
    dc = DCDF[dtype]
    if want_pre:
        if act & 2:
            d = gelu_d(v)
            res["pre"], res["pre_bound"] = d, _store(d, GELU_D2 * err + dc + 3 * U + U * np.abs(d), out_dtype)
        else:
            res["pre"], res["pre_bound"] = v, _store(v, err, out_dtype)
    if act & 1:
        y = gelu(v)
        err = GELU_D1 * err + np.abs(v) * dc + U * np.abs(y)
        v = y
    if gelu_in is not None:
        g = x[gelu_in]
        if act & 4:
            gv, ge = g, 0.0
        else:
            gv = gelu_d(g)
            ge = dc + 3 * U + U * np.abs(gv)
        err = _rnd(v * gv, err * (np.abs(gv) + ge) + np.abs(v) * ge)
        v = v * gv
    if resid:
        err = err + U * (np.abs(v) + np.abs(x["resid"]) + err)          # (the residual is exact; the sum rounds once)
        v = v + x["resid"]
    if accumulate:
        c = x["cprev_" + out_dtype]
        err = err + U * (np.abs(v) + np.abs(c) + err)
        v = v + c
    res["out"], res["out_bound"] = v, _store(v, err, out_dtype)
    return res


def tn_perm(N2, inner, outer):
    """Column n2 of the product lands in column (n2 % inner) * outer + n2 // inner of out (outer <= 1: identity)."""
    n2 = np.arange(N2)
    return n2 if outer <= 1 else (n2 % inner) * outer + n2 // inner


def tn_ref(x, *, scale=1.0, accumulate=False, perm=(0, 0), nsplit=1, rows=None):
    """x = tn_inputs(...).  -> dict(out, out_bound, dbias, dbias_bound).  nsplit: an upper limit of the slabs summed; rows: tokens (default all)."""
    a, b, dtype = x["a"], x["b"], x["dtype"]
    T = rows or a.shape[0]
    sc = float(F(scale))
    dot, S = a.T @ b, np.abs(a).T @ np.abs(b)
    v = sc * dot
    err = chain_len(T, dtype, nsplit) * 2 * U * abs(sc) * S + U * abs(sc) * S
    col, colS = sc * a.sum(0), abs(sc) * np.abs(a).sum(0)
    berr = (T + 2) * 2 * U * colS
    p = tn_perm(b.shape[1], *perm)
    out, bound = np.empty_like(v), np.empty_like(v)
    out[:, p], bound[:, p] = v, err
    if accumulate:
        bound = bound + U * (np.abs(out) + np.abs(x["prev"]) + bound)
        out = out + x["prev"]
        berr = berr + U * (np.abs(col) + np.abs(x["prev_b"]) + berr)
        col = col + x["prev_b"]
    return dict(out=out, out_bound=_rnd(out, bound), dbias=col, dbias_bound=_rnd(col, berr))


# ---------------------------------------------------------------------------------------------- f32 emulation (host test of the tester)
ORDERS = ("forward", "reversed", "pairwise")


def _add32(x, y):
    return (x.astype(np.float64) + y).astype(F)


def _block_sum(terms, order):
    """f32 sum of a list of float64 arrays (each exact or rounded once): a chain in the given order, or a pairwise tree."""
    if order == "pairwise":
        t = [p.astype(F) for p in terms]
        while len(t) > 1:
            t = [_add32(t[i], t[i + 1].astype(np.float64)) if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        return t[0]
    s = np.zeros_like(terms[0], dtype=F)
    for p in (terms if order == "forward" else terms[::-1]):
        s = _add32(s, p)
    return s


def emu_acc(a, b, dtype, order="forward", acc=None):
    """sum_k a[m][k] b[n][k] as the kernels add it: MFMA_K products per step into an f32 accumulator, steps in K order (reversed: from the end)."""
    km = MFMA_K[dtype]
    K = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=F) if acc is None else acc
    steps = list(range(0, K, km))
    for k0 in (steps[::-1] if order == "reversed" else steps):
        terms = [a[:, k, None] * b[None, :, k] for k in range(k0, min(k0 + km, K))]          # exact in fp64 (<= 48 bits)
        acc = _add32(acc, _block_sum(terms, order).astype(np.float64))
    return acc


def _cdf_fast(x):
    """gelu_parts_fast of common.h in f32 -> (cdf, exp(-x^2 / 2))."""
    z = np.abs(x) * F(0.70710678118654752440)
    t = F(1.0) / (F(0.3275911) * z + F(1.0))
    e = np.exp2(-z * z * F(1.4426950408889634)).astype(F)
    poly = t * (F(0.254829592) + t * (F(-0.284496736) + t * (F(1.421413741) + t * (F(-1.453152027) + t * F(1.061405429)))))
    return F(0.5) + F(0.5) * np.copysign(F(1.0) - poly * e, x), e


def _emu_gelu_both(x, dtype, tanh=False):
    """(gelu(x), gelu'(x)) in f32 as the kernels of this operand dtype evaluate them; tanh: the tanh form (a mutant)."""
    x = x.astype(F)
    if tanh:
        x64 = x.astype(np.float64)
        inner = math.sqrt(2.0 / math.pi) * (x64 + 0.044715 * x64 ** 3)
        th = np.tanh(inner)
        y = 0.5 * x64 * (1.0 + th)
        d = 0.5 * (1.0 + th) + 0.5 * x64 * (1.0 - th * th) * math.sqrt(2.0 / math.pi) * (1.0 + 3 * 0.044715 * x64 * x64)
        return y.astype(F), d.astype(F)
    if dtype == "f32":
        cdf = (F(0.5) * (F(1.0) + erf(x * F(0.70710678118654752440)).astype(F))).astype(F)
        e = np.exp(-0.5 * x.astype(np.float64) ** 2).astype(F)
    else:
        cdf, e = _cdf_fast(x)
    return (x * cdf).astype(F), (cdf + x * F(0.39894228040143267794) * e).astype(F)


def emu_epilogue(acc, x, *, alpha=1.0, bias=False, act=0, want_pre=False, gelu_in=None, resid=False, accumulate=False, out_dtype=None, mutant=None):
    """The epilogue of gemm_nt_kernel in f32 on an accumulator tile, one rounding at the store.  -> (out, pre | None) as float64 arrays of what
    the output dtype holds.  mutant: None or one of EPILOGUE_MUTANTS."""
    dtype = x["dtype"]
    out_dtype = out_dtype or side_dtype(dtype)
    al = F(F(alpha) * F(x["sa"]) * F(x["sb"]))
    bv = x["bias"].astype(F)[None, :] if bias else F(0.0)
    store = (lambda t: t.astype(F).astype(np.float64)) if out_dtype == "f32" else (bf16_trunc if mutant == "bf16_store_truncates" else bf16_rne)
    if mutant == "alpha_after_bias":
        v = ((acc + bv) * al).astype(F)
    elif mutant == "bias_after_gelu":
        v = (acc * al).astype(F)
    else:
        v = (acc * al + bv).astype(F)
    if mutant == "resid_before_gelu" and resid:
        v = (v + x["resid"].astype(F)).astype(F)
    if mutant == "pre_rounded_to_bf16":
        v = bf16_rne(v).astype(F)
    pre = None
    y, d = _emu_gelu_both(v, dtype, tanh=mutant in ("tanh_gelu", "tanh_gelu_grad"))
    if mutant == "tanh_gelu":
        d = _emu_gelu_both(v, dtype)[1]
    if mutant == "tanh_gelu_grad":
        y = _emu_gelu_both(v, dtype)[0]
    if want_pre:
        pre = store(d if act & 2 else v)
    if act & 1:
        v = y
    if mutant == "bias_after_gelu":
        v = (v + bv).astype(F)
    if gelu_in is not None:
        g = x[gelu_in].astype(F)
        if (act & 4) and mutant != "gelu_in_differentiated_twice":
            v = (v * g).astype(F)
        else:
            v = (v * _emu_gelu_both(g, dtype, tanh=mutant == "tanh_gelu_grad")[1]).astype(F)
    if resid and mutant != "resid_before_gelu":
        v = (v + x["resid"].astype(F)).astype(F)
    if accumulate:
        c = x["cprev_" + out_dtype].astype(F)
        v = (v + c).astype(F)
        if mutant == "accumulate_twice":
            v = (v + c).astype(F)
    return store(v), pre


# The wrong kernels the bounds must reject (tests/test_gemm_reference_host.py), by the number they carry in DESIGN.md.
MAINLOOP_MUTANTS = {1: "one_product_dropped", 2: "last_chunk_of_last_ktile_dropped", 3: "two_k_chunks_of_a_swapped"}
EPILOGUE_MUTANTS = {4: "bias_after_gelu", 5: "alpha_after_bias", 6: "tanh_gelu", 7: "pre_rounded_to_bf16", 8: "bf16_store_truncates",
                    9: "resid_before_gelu", 10: "accumulate_twice", 11: "gelu_in_differentiated_twice"}
TN_MUTANTS = {12: "last_row_of_split_skipped", 13: "first_row_of_next_split_twice", 14: "perm_wrong_way_round", 15: "dbias_misses_ragged_tail",
              16: "grouped_dbias_from_previous_problem"}


def mutate_operands(a, b, dtype, mutant, m0=3, n0=5):
    """-> (a', b', rows, cols): operands that make an honest kernel compute what the main-loop mutant computes, and the output region it touches."""
    a = a.copy()
    K = a.shape[1]
    ch = CHUNK[dtype]
    if mutant == "one_product_dropped":                       # in ONE element: the caller recomputes (m0, n0) only.  A median-sized product.
        p = np.abs(a[m0] * b[n0])
        k0 = int(np.argsort(p)[len(p) // 2]) if np.median(p) > 0 else int(np.flatnonzero(p)[0])
        a[m0, k0] = 0.0
        return a, b, slice(m0, m0 + 1), slice(n0, n0 + 1)
    if mutant == "last_chunk_of_last_ktile_dropped":          # for one tile row: every column of row m0
        a[m0, K - ch:] = 0.0
        return a, b, slice(m0, m0 + 1), slice(None)
    if mutant == "two_k_chunks_of_a_swapped":
        a[m0, :ch], a[m0, ch:2 * ch] = a[m0, ch:2 * ch].copy(), a[m0, :ch].copy()
        return a, b, slice(m0, m0 + 1), slice(None)
    raise KeyError(mutant)


def emu_tn(x, *, chunk_rows, scale=1.0, accumulate=False, perm=(0, 0), order="forward", batches=1, mutant=None, prev_problem=None):
    """out / dbias of the weight-gradient kernels in f32: per batch entry the token axis in splits of chunk_rows (a multiple of 64), one f32 slab per
    split, slabs summed in order, times scale, (+ previous), columns permuted.  -> (out, dbias) float64.  mutant: None or one of TN_MUTANTS;
    prev_problem: the inputs of problem k - 1 of a grouped launch (mutant 16)."""
    a, b, dtype = x["a"], x["b"], x["dtype"]
    T, N1 = a.shape
    rpb = T // batches
    assert rpb * batches == T and chunk_rows % 64 == 0
    ones = np.ones((1, T))
    out, col = np.zeros((N1, b.shape[1]), dtype=F), np.zeros((N1, 1), dtype=F)
    splits = [(z * rpb + r0, z * rpb + min(r0 + chunk_rows, rpb)) for z in range(batches) for r0 in range(0, rpb, chunk_rows)]
    for s, (lo, hi) in enumerate(splits):
        rows = list(range(lo, hi))
        rows_b = list(rows)
        if mutant == "last_row_of_split_skipped" and s == 0:
            rows = rows[:-1]
        if mutant == "first_row_of_next_split_twice" and s == 0 and len(splits) > 1:
            rows = rows + [hi]
        if mutant == "dbias_misses_ragged_tail":
            rows_b = rows_b[:len(rows_b) // 64 * 64]
        out = _add32(out, emu_acc(a[rows].T, b[rows].T, dtype, order).astype(np.float64))
        src = prev_problem["a"] if mutant == "grouped_dbias_from_previous_problem" else a
        cols = np.arange(N1) % src.shape[1]
        if rows_b:
            col = _add32(col, emu_acc(src[rows_b][:, cols].T, ones[:, :len(rows_b)], dtype, order).astype(np.float64))
    sc = F(scale)
    out, col = (out * sc).astype(F), (col[:, 0] * sc).astype(F)
    inner, outer = perm
    p = tn_perm(b.shape[1], inner, outer)
    if mutant == "perm_wrong_way_round" and outer > 1:
        n2 = np.arange(b.shape[1])
        p = (n2 % outer) * inner + n2 // outer
    res = np.empty_like(out)
    res[:, p] = out
    if accumulate:
        res, col = (res + x["prev"].astype(F)).astype(F), (col + x["prev_b"].astype(F)).astype(F)
    return res.astype(np.float64), col.astype(np.float64)


# ---------------------------------------------------------------------------------------------- the epilogue flavours the GPU cases run
# name -> keyword arguments of nt_ref / emu_epilogue ("->f32": f32 output from low-precision operands; f32 operands always store f32)
FLAVOURS = {
    "plain": dict(),
    "bias": dict(bias=True),
    "bias+resid->f32": dict(bias=True, resid=True, out_dtype="f32"),
    "bias+resid": dict(bias=True, resid=True),
    "act1+pre": dict(bias=True, act=1, want_pre=True),
    "act1+pre->f32": dict(bias=True, act=1, want_pre=True, out_dtype="f32"),
    "act1+resid->f32": dict(bias=True, act=1, resid=True, out_dtype="f32"),
    "act3": dict(bias=True, act=3, want_pre=True),
    "act3->f32": dict(bias=True, act=3, want_pre=True, out_dtype="f32"),
    "gelu_in.act0": dict(gelu_in="gin", act=0),
    "gelu_in.act0->f32": dict(gelu_in="gin", act=0, out_dtype="f32"),
    "gelu_in.act4": dict(gelu_in="gin_d", act=4),
    "gelu_in.act4->f32": dict(bias=True, gelu_in="gin_d", act=4, out_dtype="f32"),
    "accumulate": dict(bias=True, accumulate=True),
    "accumulate->f32": dict(bias=True, accumulate=True, out_dtype="f32"),
    "alpha": dict(bias=True, alpha=0.37),
    "alpha->f32": dict(bias=True, alpha=-1.7, out_dtype="f32"),
}
