"""Non-finite values through the kernels: poison patterns, the three-set rule and its verdict (numpy only: shared by nonfinite_checks() in
kernel_checks.py and by tests/test_nonfinite_reference_host.py, which tests this tester on the CPU).

The fp64 models of the other *_ref modules already say what a NaN or an Inf in an operand must do: numpy propagates both by IEEE rules.  A case
computes its reference twice, from the clean operands and from the same operands with ONE element replaced by a poison pattern, and classify()
splits every output tensor into three disjoint sets:

    N   the poisoned reference is non-finite                      -> the kernel's output is non-finite (the class is compared: NaN for Inf passes)
    U   the poisoned reference equals the clean one exactly       -> the kernel's output is BIT-EQUAL to its own clean launch (and finite)
    C   finite but changed                                        -> the kernel is within the family's existing per-element bound

verdict() checks a kernel's two launches against those sets.  The sets are equal, not nested: a kernel that is non-finite outside N (it
spreads) fails as much as one that is finite inside N (it launders).  widen() is the only exception there is: it ADDS a stated set to N.

Poison patterns are written through integer views, so the payloads are exact: a quiet NaN, all ones (what the guard allocator of tests/guarded.py
fills with: a negative quiet NaN with every payload bit set), a signalling NaN, +Inf and -Inf.

Where an existing reference cannot take a poisoned input this module handles it, the other modules stay as they are:
  - gemm_ref.e4m3_rne is for |x| <= 448: e4m3_quantize() below clamps the finite elements first and sets the elements whose INPUT is non-finite
    to NaN afterwards (the rule of csrc/fp8.hip: the class of the input decides, not the scaled value).
  - the bound arithmetic of the references turns a poisoned operand into a NaN or Inf bound: usable_bound() takes the clean problem's bound for
    such an element (the same element with the same other operands).
"""
import numpy as np

import gemm_ref as GR

F = np.float32
NAMES = ("qnan", "ones", "snan", "+inf", "-inf")
BITS = {"f32": (0x7FC00000, 0xFFFFFFFF, 0x7F800001, 0x7F800000, 0xFF800000), "bf16": (0x7FC0, 0xFFFF, 0x7F81, 0x7F80, 0xFF80)}
NPAT = len(NAMES)


def bits(i, dtype):
    """Pattern i (mod 5) of the dtype ("f32" / "bf16") as an unsigned integer."""
    return BITS[dtype][i % NPAT]


def signed_bits(i, dtype):
    """The same word as the signed integer of its width (what an int32 / int16 view of a tensor takes)."""
    b, w = bits(i, dtype), 32 if dtype == "f32" else 16
    return b - (1 << w) if b >> (w - 1) else b


def value(i, dtype="f32"):
    """Pattern i as the float64 the references see (through an integer view: NaN, +Inf or -Inf)."""
    word = np.array([bits(i, dtype) << (0 if dtype == "f32" else 16)], dtype=np.uint32)
    return float(word.view(F)[0])


def plant(a, index, i, dtype="f32"):
    """A float64 copy of `a` with pattern i at `index` (any numpy index: an element, a row, a slice)."""
    out = np.array(a, dtype=np.float64, copy=True)
    out[index] = value(i, dtype)
    return out


# ---------------------------------------------------------------------------------------------- the three sets
def classify(ref_clean, ref_poisoned):
    """-> dict(N, U, C) of boolean masks over the output tensor, disjoint, together everything."""
    c, p = np.asarray(ref_clean, dtype=np.float64), np.asarray(ref_poisoned, dtype=np.float64)
    assert c.shape == p.shape and np.isfinite(c).all(), "the clean reference must be finite"
    n = ~np.isfinite(p)
    with np.errstate(invalid="ignore"):
        u = ~n & (p == c)
    return dict(N=n, U=u, C=~n & ~u)


def widen(sets, extra, why):
    """The sets with `extra` (a mask) moved into N.  `why` names the stated set; an exception can only add to N."""
    assert isinstance(why, str) and why
    extra = np.asarray(extra, dtype=bool)
    n = sets["N"] | extra
    return dict(N=n, U=sets["U"] & ~n, C=sets["C"] & ~n)


def counts(sets):
    return tuple(int(sets[k].sum()) for k in "NUC")


def usable_bound(bound_poisoned, bound_clean):
    """The poisoned problem's bound where it is a number, the clean problem's bound of the same element where the bound arithmetic itself met
    the poison (u * |inf|)."""
    bp = np.asarray(bound_poisoned, dtype=np.float64)
    return np.where(np.isfinite(bp), bp, np.broadcast_to(np.asarray(bound_clean, dtype=np.float64), bp.shape))


def _same_bits(a, b):
    """Finite and equal including the sign of zero: for finite values of one dtype that is bit equality."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(a) & np.isfinite(b) & (a == b) & (np.signbit(a) == np.signbit(b))


def verdict(name, got_clean, got_poisoned, ref_poisoned, bound, sets):
    """The kernel's clean and poisoned launch (arrays of the values its output dtype holds) against the sets of classify().
    -> [(name, err, tol, ok)]: offenders in N (finite there), offenders in U (not bit-equal to the clean launch, or non-finite), and the worst
    |got - ref| / bound over C.  bound may be None when C is empty."""
    gc, gp = np.asarray(got_clean, dtype=np.float64), np.asarray(got_poisoned, dtype=np.float64)
    n, u, c = sets["N"], sets["U"], sets["C"]
    assert gc.shape == gp.shape == n.shape, (gc.shape, gp.shape, n.shape)
    assert not (n & u).any() and not (n & c).any() and not (u & c).any() and (n | u | c).all()
    size = "|N|=%d |U|=%d |C|=%d" % counts(sets)
    bad_n = int((n & np.isfinite(gp)).sum())
    bad_u = int((u & ~_same_bits(gc, gp)).sum())
    rows = [(f"{name}: finite inside N ({size})", float(bad_n), 0.0, bad_n == 0),
            (f"{name}: differs from the clean launch inside U ({size})", float(bad_u), 0.0, bad_u == 0)]
    if c.any():
        assert bound is not None
        b = np.broadcast_to(np.asarray(bound, dtype=np.float64), gp.shape)
        assert np.isfinite(b[c]).all(), "a bound on C must be a number (usable_bound)"
        r = GR.ratio(gp[c], np.asarray(ref_poisoned, dtype=np.float64)[c], b[c])
        rows.append((f"{name}: worst error / bound inside C ({size})", r, 1.0, bool(r <= 1.0)))
    return rows


def accepted(rows):
    return all(ok for _, _, _, ok in rows)


# the two wrong kernels every case's verdict must reject (tests/test_nonfinite_reference_host.py)
def launder(got_poisoned, sets, limit=448.0):
    """What v_med3(x, -limit, limit) makes of the poisoned launch: every element of N replaced by a clamped finite value."""
    g = np.array(got_poisoned, dtype=np.float64, copy=True)
    with np.errstate(invalid="ignore"):
        g[sets["N"]] = np.where(g[sets["N"]] > 0, limit, -limit)          # (NaN compares false: -limit, the min3 a NaN operand yields)
    return g


def spread(got_poisoned, sets):
    """One more row (the last axis) of U set to NaN: the row of the first element of U."""
    g = np.array(got_poisoned, dtype=np.float64, copy=True).reshape(-1, np.shape(got_poisoned)[-1] if np.ndim(got_poisoned) else 1)
    u = sets["U"].reshape(g.shape)
    r = int(np.flatnonzero(u.any(1))[0])
    g[r, :] = np.nan
    return g.reshape(np.shape(got_poisoned))


# ---------------------------------------------------------------------------------------------- e4m3 (csrc/fp8.hip)
def e4m3_decode(b):
    """OCP e4m3fn bytes -> float64 (0x7f / 0xff: NaN; the format has no Inf)."""
    b = np.asarray(b, dtype=np.uint8).astype(np.int64)
    e, m = (b >> 3) & 0xF, b & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))
    mag = np.where((b & 0x7F) == 0x7F, np.nan, mag)
    return np.where(b & 0x80, -mag, mag)


def e4m3_quantize(x, scale):
    """tav_fp8_quantize's documented result as float64 e4m3 values: e4m3(clamp(f32(x) * f32(scale), +-448)) for a finite x -- a product that
    overflows f32 saturates -- and NaN for a NaN or +-Inf x."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    with np.errstate(over="ignore", invalid="ignore"):
        v = (np.where(fin, x, 0.0).astype(F) * F(scale)).astype(np.float64)
    assert not np.isnan(v).any(), "0 * inf: a scale the states never hold"
    out = GR.e4m3_rne(np.clip(v, -448.0, 448.0))
    out[~fin] = np.nan
    return out


def finite_amax(x):
    """The maximum of |x| over the finite elements as f32 (0 when there is none): what state[3] gathers."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    return F(np.abs(x[fin]).max()) if fin.any() else F(0.0)


def amax_scales(x):
    """tav_fp8_amax: (448 / m, m / 448, m) in f32, m the maximum of |x| over the finite elements; an all-zero tensor or one that holds an Inf
    falls back to (1, 1, 0) (csrc/fp8.hip, fp8_amax_final_kernel).  A NaN is simply not counted."""
    x = np.asarray(x, dtype=np.float64)
    m = finite_amax(x)
    if np.isinf(x).any() or not m > 0:
        return np.array([1.0, 1.0, 0.0], dtype=F)
    return np.array([F(448.0) / m, m / F(448.0), m], dtype=F)


FP8_SHAPES = ((33, 136), (129, 1032))


def fp8_sites(rows, cols):
    """Five elements, one per pattern: the corners, the 64 x 64 tile boundary (or the last row before it), an odd interior element and the last
    group of four of row 1."""
    return [(0, 0), (rows - 1, cols - 1), (min(64, rows - 1), 64), (rows // 2, 7), (1, cols - 4)]


def fp8_inputs(rows, cols, dtype, seed=0):
    """randn rounded to the operand dtype, float64."""
    x = np.random.default_rng(1800 + rows + cols + seed).standard_normal((rows, cols))
    return GR.round_to(x, dtype)[0]


def fp8_quantize_case(rows, cols, dtype, site, pat, scale):
    """-> (x_poisoned, clean reference, poisoned reference, sets, expected N) of one quantiser launch."""
    x = fp8_inputs(rows, cols, dtype)
    xp = plant(x, site, pat, dtype)
    rc, rp = e4m3_quantize(x, scale), e4m3_quantize(xp, scale)
    want = np.zeros((rows, cols), dtype=bool)
    want[site] = True
    return xp, rc, rp, classify(rc, rp), want


# ---------------------------------------------------------------------------------------------- GEMM NT (tests/gemm_ref.py)
NT_SHAPE = (333, 384, 256)
NT_FLAVOURS = ("plain", "bias", "bias+resid->f32", "act3", "gelu_in.act4", "accumulate->f32", "act1+pre->f32")


def nt_tile(dname, hint):
    """(rows, cols) of the output tile a hint selects at NT_SHAPE, for the placement on a tile boundary (csrc/gemm_plan.h: hint 16 the 256 x 256
    tile, 8 the 256 x 128 one, 0 the default 128 x 128)."""
    return {16: (256, 256), 8: (256, 128)}.get(hint, (128, 128))


def nt_sites(dname, hint, flavour):
    """[(tensor, index, structural kind)] of one flavour: A and B at the first, the last (ragged tail tile) and a tile-boundary row with k = 0,
    k = K - 1 and a k of a middle K-tile; the side tensors the flavour has at the same rows / columns."""
    M, N, K = NT_SHAPE
    tm, tn = nt_tile(dname, hint)
    kmid = 2 * GR.KTILE[dname] + 3
    kw = GR.FLAVOURS[flavour]
    rows, cols, ks = (0, M - 1, tm), (0, N - 1, tn), (0, K - 1, kmid)
    sites = [("a", (rows[i], ks[i]), "row") for i in range(3)] + [("b", (cols[i], ks[(i + 1) % 3]), "col") for i in range(3)]
    if kw.get("bias"):
        sites += [("bias", (c,), "col") for c in cols]
    for key, tensor in (("resid", "resid"), ("gelu_in", kw.get("gelu_in")), ("accumulate", "cprev_" + (kw.get("out_dtype") or GR.side_dtype(dname)))):
        if kw.get(key):
            sites += [(tensor, (rows[i], cols[(i + 2) % 3]), "elem") for i in range(3)]
    return sites


def nt_side_dtype(dname, tensor):
    """The dtype a tensor of nt_inputs is uploaded in (the pattern's width)."""
    if tensor in ("a", "b", "gin", "gin_d"):
        return GR.side_dtype(dname)
    return "bf16" if tensor == "cprev_bf16" else "f32"


def nt_expect(tensor, index, kind):
    M, N, _ = NT_SHAPE
    want = np.zeros((M, N), dtype=bool)
    if kind == "row":
        want[index[0], :] = True
    elif kind == "col":
        want[:, index[0]] = True
    else:
        want[index] = True
    return want


def nt_case(x, ref_clean, flavour, tensor, index, pat):
    """x = gemm_ref.nt_inputs(...), ref_clean = gemm_ref.nt_ref(x, flavour).  -> (poisoned reference with usable bounds, sets of out, sets of pre
    or None)."""
    dname = x["dtype"]
    xp = dict(x)
    xp[tensor] = plant(x[tensor], index, pat, nt_side_dtype(dname, tensor))
    with np.errstate(all="ignore"):
        rp = GR.nt_ref(xp, **GR.FLAVOURS[flavour])
    rp["out_bound"] = usable_bound(rp["out_bound"], ref_clean["out_bound"])
    sets = classify(ref_clean["out"], rp["out"])
    pre = None
    if "pre" in rp:
        rp["pre_bound"] = usable_bound(rp["pre_bound"], ref_clean["pre_bound"])
        pre = classify(ref_clean["pre"], rp["pre"])
    return rp, sets, pre


def nt_flavours(dname):
    """NT_FLAVOURS for bf16 operands; f32 operands store f32 only, so their "->f32" names run as the twins without the suffix."""
    names = [n[:-5] if dname == "f32" and n.endswith("->f32") else n for n in NT_FLAVOURS]
    return tuple(dict.fromkeys(names))


# ---------------------------------------------------------------------------------------------- fp8 GEMMs: a NaN byte in a q operand
E4M3_NAN = (0x7F, 0xFF)


def fp8_nt_sites(M, N, K, hint):
    """[(tensor, (row, k), kind)]: first, last and tile-boundary row of A and of B, k = 0, K - 1 and one of a middle 16-byte chunk."""
    t = 256 if hint == 16 else 128
    rows, cols, ks = (0, M - 1, min(t, M - 1)), (0, N - 1, min(t, N - 1)), (0, K - 1, K // 2 + 17)
    return [("a", (rows[i], ks[i]), "row") for i in range(3)] + [("b", (cols[i], ks[(i + 1) % 3]), "col") for i in range(3)]


def fp8_nt_case(x, ref_clean, tensor, index):
    """x = gemm_ref.nt_inputs(..., "fp8"), ref_clean = nt_ref(x, bias=True, out_dtype="f32") -> (poisoned reference, sets)."""
    xp = dict(x)
    xp[tensor] = plant(x[tensor], index, 0)
    with np.errstate(all="ignore"):
        rp = GR.nt_ref(xp, bias=True, out_dtype="f32")
    rp["out_bound"] = usable_bound(rp["out_bound"], ref_clean["out_bound"])
    return rp, classify(ref_clean["out"], rp["out"])


def fp8_expect(shape, tensor, index):
    want = np.zeros(shape, dtype=bool)
    if tensor in ("a", "at"):
        want[index[0], :] = True
    else:
        want[:, index[0]] = True
    return want


def fp8_wgrad_problem(T, N1, N2, kpad=1024):
    """dY^T [N1, Kp] and X^T [N2, Kp] as e4m3 values with the token axis zero padded to a multiple of kpad, and their dequantisation factors."""
    rng = np.random.default_rng(9300 + T + N1 + N2)
    kp = -(-T // kpad) * kpad
    at, bt = np.zeros((N1, kp)), np.zeros((N2, kp))
    at[:, :T], sa = GR.round_to(rng.standard_normal((N1, T)) * GR.row_scale(N1)[:, None], "fp8")
    bt[:, :T], sb = GR.round_to(0.1 * rng.standard_normal((N2, T)) * GR.col_scale(N2)[:, None], "fp8")
    return dict(at=at, bt=bt, sa=sa, sb=sb, T=T)


def fp8_wgrad_ref(p, nsplit=8):
    """dW = sa sb dY^T X in fp64 and its bound: the accumulation chain of gemm_ref's docstring over the padded token axis and nsplit slabs, the
    two dequantisation multiplies, alpha, the store."""
    with np.errstate(all="ignore"):
        al = float(F(p["sa"])) * float(F(p["sb"]))
        out, aS = al * (p["at"] @ p["bt"].T), abs(al) * (np.abs(p["at"]) @ np.abs(p["bt"]).T)
        err = (GR.chain_len(p["at"].shape[1], "fp8", nsplit) * 2 + 3) * GR.U * aS
        return dict(out=out, out_bound=err + GR.U * (np.abs(out) + err))


def fp8_wgrad_sites(T, N1, N2):
    ts = (0, T - 1, T // 2 + 5)
    return [("at", (r, ts[i])) for i, r in enumerate((0, N1 - 1, 128))] + [("bt", (r, ts[(i + 1) % 3])) for i, r in enumerate((0, N2 - 1, 128))]


def fp8_wgrad_case(p, ref_clean, tensor, index):
    pp = dict(p)
    pp[tensor] = plant(p[tensor], index, 0)
    rp = fp8_wgrad_ref(pp)
    rp["out_bound"] = usable_bound(rp["out_bound"], ref_clean["out_bound"])
    return rp, classify(ref_clean["out"], rp["out"])


# ---------------------------------------------------------------------------------------------- GEMM TN (weight gradients): dW = A^T B, dbias = colsum(A)
TN_WIDTHS = (136, 264)


def tn_sites(T, N1, N2):
    """[(tensor, (token, column))]: the first token, the last one (the ragged last K-tile) and one of a middle K-tile; the first column, the last
    one (the ragged tail tile) and one on the 128-wide tile boundary."""
    ts = (0, T - 1, 64 + T // 3)
    return [("a", (ts[i], c)) for i, c in enumerate((0, N1 - 1, 128))] + [("b", (ts[(i + 1) % 3], c)) for i, c in enumerate((0, N2 - 1, 128))]


def tn_expect(N1, N2, tensor, index, perm=(0, 0)):
    """(dW, dbias) masks: an A element poisons row n1 of dW and dbias[n1] (dbias is the column sum of A: include/tavhip.h, tav_gemm_tn); a B
    element poisons one dW column (where the permutation puts it) and nothing of dbias."""
    out, db = np.zeros((N1, N2), dtype=bool), np.zeros(N1, dtype=bool)
    if tensor == "a":
        out[index[1], :] = True
        db[index[1]] = True
    else:
        out[:, GR.tn_perm(N2, *perm)[index[1]]] = True
    return out, db


def tn_case(x, ref_clean, tensor, index, pat, **kw):
    """x = gemm_ref.tn_inputs(...), ref_clean = tn_ref(x, **kw) -> (poisoned reference with usable bounds, sets of dW, sets of dbias)."""
    xp = dict(x)
    xp[tensor] = plant(x[tensor], index, pat, GR.side_dtype(x["dtype"]))
    with np.errstate(all="ignore"):
        rp = GR.tn_ref(xp, **kw)
    for k in ("out", "dbias"):
        rp[k + "_bound"] = usable_bound(rp[k + "_bound"], ref_clean[k + "_bound"])
    return rp, classify(ref_clean["out"], rp["out"]), classify(ref_clean["dbias"], rp["dbias"])


# ---------------------------------------------------------------------------------------------- step end and the loss link
STEP_SIZES = "nt2"                                        # step_end_ref.SIZE_LISTS: a 5-element tensor and one of two chunks + 7


def sumsq_ref(x):
    """sum x^2 in fp64: one NaN gives NaN, one +-Inf gives +Inf."""
    with np.errstate(all="ignore"):
        return float(np.sum(np.asarray(x, dtype=np.float64) ** 2))


def step_sites(sizes, chunk=16384):
    """Flat indices over the concatenated tensors: the very first element, the first element of the second tensor's second chunk, the last
    element of all (the tail of a chunk)."""
    n = sum(sizes)
    return [0, sizes[0] + chunk, n - 1]


def adamw_state(SR):
    """SR = step_end_ref -> (p, g, m, v) f32 of the AdamW cases: step_end_ref's parameters and gradients, non-zero moments of the gradients' scale."""
    n = sum(SR.SIZE_LISTS[STEP_SIZES])
    p0, g0 = SR.make_inputs(n, seed=4242)
    rng = np.random.default_rng(4243)
    m0 = (0.1 * g0 * rng.uniform(0.5, 1.5, n)).astype(F)
    v0 = (1e-3 * g0.astype(np.float64) ** 2 * rng.uniform(0.5, 1.5, n)).astype(F)
    return p0, g0, m0, v0


def adamw_case(p, g, m, v, step, lr, wd, cc, site, pat, ref_step):
    """ref_step = step_end_ref.ref_step.  site None: pattern `pat` is the clip coefficient itself.  -> (clean, poisoned, {k: sets}) over p / m / v."""
    rc = ref_step(p, g, m, v, step, lr, wd, cc)
    with np.errstate(all="ignore"):
        rp = ref_step(p, plant(g, site, pat), m, v, step, lr, wd, cc) if site is not None else ref_step(p, g, m, v, step, lr, wd, value(pat))
    for k in "pmv":
        rp[k + "_bound"] = usable_bound(rp[k + "_bound"], rc[k + "_bound"])
    return rc, rp, {k: classify(rc[k], rp[k]) for k in "pmv"}


def ce_sites(p):
    """[(row, column, where)] of a front_ref.ce_inputs problem: the target class and another one, in the first row, a row past 256 when there
    is one, and the last row."""
    B, C = p["B"], p["C"]
    rows = sorted({0, min(B - 1, 256), B - 1})
    return [(r, int(p["t"][r]), "target") for r in rows] + [(r, (int(p["t"][r]) + 1 + r) % C, "off") for r in rows if C > 1]


def ce_case(p, ref_clean, ce_ref, weighted, gs, row, col, pat):
    """ce_ref = front_ref.ce_ref -> (poisoned reference with usable bounds, sets of the loss, sets of dlogits)."""
    q = dict(p)
    q["z"] = plant(p["z"], (row, col), pat)
    with np.errstate(all="ignore"):
        rp = ce_ref(q, weighted, gs)
    rp["loss_b"] = usable_bound(rp["loss_b"], ref_clean["loss_b"])
    rp["dlogits_b"] = usable_bound(rp["dlogits_b"], ref_clean["dlogits_b"])
    return rp, classify(ref_clean["loss"], rp["loss"]), classify(ref_clean["dlogits"], rp["dlogits"])


# ---------------------------------------------------------------------------------------------- LayerNorm (tests/norm_ref.py)
LN_SHAPE = (5, 768)          # norm_ref.LN_ROWS' smallest count that leaves rows the poison does not reach (1 would make every case all N)


def ln_sites(rows, W):
    """[(tensor, index)]: x and dy at the first row, the all-zero last row and a middle one, first / last column and one on the 256-element
    boundary of the row loop; gamma at those columns; dx_add at two of the elements."""
    rc = [(0, 0), (rows - 1, W - 1), (rows // 2, 256)]
    return [("x", i) for i in rc] + [("dy", i) for i in rc] + [("gamma", (c,)) for _, c in rc] + [("add", i) for i in rc[:2]]


def _ln_poisoned(p, tensor, index, pat):
    q = dict(p)
    dt = {"x": p["xdt"], "dy": p["dydt"]}.get(tensor, "f32")
    q[tensor] = plant(p[tensor], index, pat, dt)
    return q


def _with_usable_bounds(rp, rc, names):
    for n in names:
        rp[n + "_b"] = usable_bound(rp[n + "_b"], rc[n + "_b"])
    return rp


def ln_case(NR, p, tensor, index, pat, act, lp):
    """NR = norm_ref.  One poisoned LayerNorm problem, forward and isolated backward (fed the poisoned forward's own mean / rstd, rounded to
    f32, as norm_ref.fed does).  -> dict(q, fwd_clean, fwd, fwd_sets, bwd_clean, bwd, bwd_sets, fed_clean, fed)."""
    q = _ln_poisoned(p, tensor, index, pat)
    out = dict(q=q)
    with np.errstate(all="ignore"):
        fc, fp = NR.ln_ref_fwd(p, act, lp), NR.ln_ref_fwd(q, act, lp)
        out.update(fwd_clean=fc, fwd=_with_usable_bounds(fp, fc, NR.LN_FWD_OUT), fwd_sets={n: classify(fc[n], fp[n]) for n in NR.LN_FWD_OUT})
        feds = []
        for f in (fc, fp):
            (mv, m32), (rv, r32) = NR.fed(f["mean"]), NR.fed(f["rstd"])
            feds.append((mv, rv, m32, r32))
        bc = NR.ln_ref_bwd(p, feds[0][0], feds[0][1], act=act, lp=lp, add=True)
        bp = NR.ln_ref_bwd(q, feds[1][0], feds[1][1], act=act, lp=lp, add=True)
    out.update(bwd_clean=bc, bwd=_with_usable_bounds(bp, bc, NR.LN_BWD_OUT), bwd_sets={n: classify(bc[n], bp[n]) for n in NR.LN_BWD_OUT},
               fed_clean=feds[0][2:], fed=feds[1][2:])
    return out


def ln_expect(rows, W, tensor, index, act):
    """Structural N of every output.  Forward: an x element its row (y, mean, rstd), a gamma element its column of y.  Backward: an x element
    its row of dx and ALL of dgamma (x-hat of the row enters every column), and all of dbeta only under the fused GELU (act: gelu' of the row);
    a dy element its row of dx (the row means) and ITS COLUMN of dgamma / dbeta; a gamma element all of dx (g = d gamma enters every row mean),
    and under act its column of dgamma / dbeta; a dx_add element that element."""
    z2, z1r, z1c = (lambda: np.zeros((rows, W), dtype=bool)), (lambda: np.zeros(rows, dtype=bool)), (lambda: np.zeros(W, dtype=bool))
    y, mean, dx, dg, db = z2(), z1r(), z2(), z1c(), z1c()
    if tensor == "x":
        y[index[0]] = mean[index[0]] = dx[index[0]] = True
        dg[:] = True
        db[:] = bool(act)
    elif tensor == "dy":
        dx[index[0]] = True
        dg[index[1]] = db[index[1]] = True
    elif tensor == "gamma":
        y[:, index[0]] = True
        dx[:] = True
        dg[index[0]] = db[index[0]] = bool(act)
    else:
        dx[index] = True
    return dict(y_f32=y, y_lp=y, mean=mean, rstd=mean, dx_f32=dx, dx_lp=dx, dgamma=dg, dbeta=db)


# ---------------------------------------------------------------------------------------------- attention (tests/attn_ref.py)
# attn_ref._slice_ref asserts on its own bound arithmetic (rl < 0.25) and clamps a -inf additive mask to -1e300, so it takes a -Inf element of a
# pre-softmax mask as it stands (the one case with a C set) and nothing else poisoned.  attn_plain() below is the same forward and backward
# in plain fp64 without bounds: IEEE rules then say where the NaN goes.  Its sets carry no C, so no bound is needed.
ATTN_S = (65, 129)
ATTN_SITES = ("q", "k", "v", "mask", "do")


def attn_plain(AR, x):
    """AR = attn_ref; x = AR.make_inputs(...) at full lengths -> the outputs of AR.attn_ref in the same layouts, values only."""
    B, S, nh, mode, pre = x["B"], x["S"], x["nh"], x["mode"], x["pre"]
    r = {n: np.zeros((B, S, nh, 64)) for n in AR.OUT4}
    r.update(lse=np.zeros((B, nh, S)), delta=np.zeros((B, nh, S)), corr=np.zeros((B, nh, 64)))
    c, kq = (1.0 if pre else AR.C2), ((AR.SCALE / AR.C2) if pre else AR.SCALE)
    with np.errstate(all="ignore"):
        for b in range(B):
            mask = None if mode == 0 else x["mask"][b]
            for h in range(nh):
                q, k, v, do = (x[n][b, :, h] for n in ("q", "k", "v", "do"))
                t = (q @ k.T) * c + (mask * AR.LOG2E if mode == 1 else 0.0)
                tm = t.max(1, keepdims=True)
                p = np.exp2(t - tm)
                lsum = p.sum(1, keepdims=True)
                P = p / lsum
                o_soft = P @ v
                dP, delta = do @ v.T, (do * o_soft).sum(1)
                dS = P * (dP - delta[:, None])
                dv = P.T @ do
                o = o_soft
                if mode == 2:
                    r["corr"][b, h] = mask @ v
                    o = o_soft + r["corr"][b, h][None, :]
                    dv = dv + mask[:, None] * do.sum(0)[None, :]
                r["o"][b, :, h], r["o_soft"][b, :, h], r["dv"][b, :, h] = o, o_soft, dv
                r["dk"][b, :, h], r["dq"][b, :, h] = kq * (dS.T @ q), AR.SCALE * (dS @ k)
                r["lse"][b, h], r["delta"][b, h] = (tm + np.log2(lsum))[:, 0] * AR.LN2, delta
    return r


def attn_site(S, mode, cfg, i):
    """(tensor, index) of site i of configuration number cfg: the row rotates through the first one, the last one (the ragged tail tile) and 64
    (the tile boundary), the batch entry, head and channel move with it."""
    name = ATTN_SITES[i]
    if name == "mask" and mode == 0:
        return None
    k = i + cfg
    s, b, h, d = (0, S - 1, 64)[k % 3], k % 2, (k // 2) % 3, (7 * i + 13 * cfg) % 64
    return (name, (b, s)) if name == "mask" else (name, (b, s, h, d))


def attn_pattern(tensor, k, mode=0, pre=False):
    """Pattern number of a site (k = site + configuration number).  Q and K take the three NaN patterns only: an Inf there gives scores of +Inf
    or -Inf by the sign of the other operand's element, and a -Inf score is a legitimate zero of the softmax -- a data-dependent mix of N and C
    whose bound attn_ref cannot compute.  V and dO take all five.  A pre-softmax mask (mode 1) takes -Inf with a raw q -- the one non-finite
    value a caller passes on purpose, the key gets probability 0 and the case a C set -- and +Inf with a pre-scaled q; the post-softmax mask
    (mode 2) rotates through all five like V."""
    if tensor == "mask" and mode == 1:
        return 3 if pre else 4
    return k % 3 if tensor in ("q", "k") else k % NPAT


def attn_case(AR, x, tensor, index, pat):
    """-> (poisoned problem, clean reference, poisoned reference, {name: sets}); the references carry name + "_bound" only for a -Inf element
    of a pre-softmax mask (attn_ref takes that one itself)."""
    xp = dict(x)
    xp[tensor] = plant(x[tensor], index, pat, "f32" if tensor == "mask" else x["dtype"])
    if tensor == "mask" and x["mode"] == 1 and value(pat) == -np.inf:
        rc, rp = AR.attn_ref(x), AR.attn_ref(xp)
    else:
        rc, rp = attn_plain(AR, x), attn_plain(AR, xp)
    names = AR.FWD_OUT + AR.BWD_OUT
    return xp, rc, rp, {n: classify(rc[n], rp[n]) for n in names}


def attn_expect(x, tensor, index):
    """Structural N of every output for a NaN / +Inf poison (and -Inf outside a pre-softmax mask).  A Q element: its query's o / o_soft / lse /
    delta / dq, and dk, dv of every key of that head (dS row).  A K element: everything of that (batch, head).  A V element: channel d of o /
    o_soft of every query, hence every delta, dq, dk of the head; dv does not read V.  A dO element: delta and dq of its query, dk of every
    key, channel d of dv.  A mask element, mode 1 (added before the softmax): everything of the batch entry, all heads; mode 2 (added after, as
    corr = mask V): corr and o of the entry, dv of that key; o_soft, lse, delta, dq, dk do not read it."""
    B, S, nh, mode = x["B"], x["S"], x["nh"], x["mode"]
    w = {n: np.zeros((B, S, nh, 64), dtype=bool) for n in ("o", "o_soft", "dq", "dk", "dv")}
    w.update(lse=np.zeros((B, nh, S), dtype=bool), delta=np.zeros((B, nh, S), dtype=bool), corr=np.zeros((B, nh, 64), dtype=bool))
    b, s = index[0], index[1]
    if tensor == "mask":
        if mode == 1:
            for n in w:
                if n != "corr":
                    w[n][b] = True
        else:
            w["corr"][b] = w["o"][b] = True
            w["dv"][b, s] = True
        return w
    h, d = index[2], index[3]
    if tensor == "q":
        w["o"][b, s, h] = w["o_soft"][b, s, h] = w["dq"][b, s, h] = True
        w["lse"][b, h, s] = w["delta"][b, h, s] = True
        w["dk"][b, :, h] = w["dv"][b, :, h] = True
    elif tensor == "k":
        for n in ("o", "o_soft", "dq", "dk", "dv"):
            w[n][b, :, h] = True
        w["lse"][b, h] = w["delta"][b, h] = True
    elif tensor == "v":
        w["o"][b, :, h, d] = w["o_soft"][b, :, h, d] = True
        w["delta"][b, h] = True
        w["dq"][b, :, h] = w["dk"][b, :, h] = True
        if mode == 2:
            w["corr"][b, h, d] = True
    else:
        w["delta"][b, h, s] = True
        w["dq"][b, s, h] = True
        w["dk"][b, :, h] = True
        w["dv"][b, :, h, d] = True
    return w


# ---------------------------------------------------------------------------------------------- casts and dropout
def cast_ref(x, dname, scale=None):
    """x (f32 values, possibly poisoned), optionally times an f32 scale in f32, rounded to the dtype: float64.  gemm_ref.bf16_rne works on the
    bits and is for numbers only, so the non-finite elements are put back after it."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        v = x if scale is None else (x.astype(F) * F(scale)).astype(np.float64)
        fin = np.isfinite(v)
        out = GR.round_to(np.where(fin, v, 0.0), dname)[0]
    return np.where(fin, out, v)


def dropout_ref(x, keep, p):
    """keep ? x / (1 - p) : 0, divided in f32 -- a select (include/tavhip.h, tav_dropout_fwd: "y = keep ? x / (1-p) : 0"; the kernel's
    `keep ? x[i] / (1.f - p) : 0.f`): a dropped NaN or Inf is exactly 0.  The backward is the same formula on dy."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.asarray(keep, dtype=bool), (x.astype(F) / (F(1.0) - F(p))).astype(np.float64), 0.0)
