"""CPU test of the tester behind the GEMM checks (tests/gemm_ref.py): an f32 emulation of the kernels' arithmetic -- MFMA-sized partial sums into an
f32 accumulator, one slab per token split summed in order, the epilogue in f32, one rounding at the store -- stays inside the per-element bounds of the
fp64 reference for bf16, f32 and dequantised fp8 operands, at the smallest and the largest reduction length the GPU cases use and in three summation
orders; sixteen wrong kernels leave the bounds at the largest length; the exact-integer cases come out exact and catch the eight mutants that change
a sum."""
import numpy as np
import pytest

import gemm_ref as R

M, N = 28, 24                                      # two periods of the row scales, two of the column scales
L_NT = {"bf16": (64, 1536), "f32": (32, 1536), "fp8": (128, 1536)}      # smallest / largest K of the GPU cases (K-tile = 128 bytes)
L_TN = (64, 777)
DTYPES = ("bf16", "f32", "fp8")


def _flavours(dtype):
    """The flavours this operand dtype can run: f32 operands store f32 only (their "->f32" twins are the same launch)."""
    return {k: v for k, v in R.FLAVOURS.items() if dtype != "f32" or not k.endswith("->f32")}


@pytest.fixture(scope="module")
def nt():
    """(dtype, K) -> (inputs, {order: accumulator}) of the clean emulation, computed once."""
    out = {}
    for dtype in DTYPES:
        for K in L_NT[dtype]:
            x = R.nt_inputs(M, N, K, dtype, seed=K)
            out[(dtype, K)] = (x, {o: R.emu_acc(x["a"], x["b"], dtype, o) for o in R.ORDERS})
    return out


def _worst(x, acc, kw, mutant=None):
    ref = R.nt_ref(x, **kw)
    got, pre = R.emu_epilogue(acc, x, mutant=mutant, **kw)
    r = R.ratio(got, ref["out"], ref["out_bound"])
    return max(r, R.ratio(pre, ref["pre"], ref["pre_bound"])) if pre is not None else r


def test_number_formats():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -7 + 2.0 ** -9), 3.0e-5, 447.0])
    assert list(R.bf16_rne(x)[:4]) == [1.0, 1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7)]                  # ties to even, both ways; nearest otherwise
    assert list(R.bf16_trunc(x)[:4]) == [1.0, 1.0, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7)]
    assert np.all(np.abs(R.bf16_rne(x) - x) <= R.bf16_half_ulp(np.abs(x)))
    assert R.bf16_half_ulp(1.0) == 2.0 ** -8 and R.bf16_half_ulp(1.99) == 2.0 ** -8 and R.bf16_half_ulp(2.0) == 2.0 ** -7
    assert list(R.e4m3_rne(np.array([448.0, 17.0, 18.0, 19.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 1e9]))) == \
        [448.0, 16.0, 18.0, 20.0, 2.0 ** -9, 0.0, 2.0 ** -8, 448.0]
    i = np.arange(-7, 8, dtype=np.float64)
    assert np.array_equal(R.e4m3_rne(64.0 * i), 64.0 * i)                                             # 64 x is exact in e4m3
    q, s = R.round_to(R.int_tensor((5, 16), 1), "fp8")
    assert s == 2.0 ** -6 and np.array_equal(q * s * s * 64.0, R.int_tensor((5, 16), 1))


def test_inputs_are_what_the_checks_promise():
    x = R.nt_inputs(130, 132, 256, "bf16", seed=3)
    rms_a, rms_b = np.sqrt((x["a"] ** 2).mean(1)), np.sqrt((x["b"] ** 2).mean(1))
    assert np.allclose(rms_a / R.row_scale(130), 1.0, rtol=0.25) and np.allclose(rms_b / (0.1 * R.col_scale(132)), 1.0, rtol=0.25)
    assert rms_a.max() / rms_a.min() > 2.0 ** 11 and rms_b.max() / rms_b.min() > 2.0 ** 9
    assert np.array_equal(x["a"], R.bf16_rne(x["a"])) and np.array_equal(x["gin"], R.bf16_rne(x["gin"]))
    assert all(np.gcd(p, t) == 1 for p in (13, 11) for t in (64, 96, 128, 256))
    t = R.tn_inputs(200, 26, 24, "f32", seed=4)
    assert np.allclose(np.sqrt((t["a"] ** 2).mean(0)) / R.row_scale(26), 1.0, rtol=0.3)               # scales on the columns, tokens plain randn
    for shape in ((3, 5), (1, 2)):
        i = R.int_tensor(shape, 9)
        assert i.max() == 7 and i.min() == -7 and np.array_equal(i, np.rint(i))


def test_integer_products_fit_the_significand():
    """The largest K and the largest row count of the exact-integer GPU cases (and well beyond)."""
    assert R.int_exact_ok(3072) and R.int_exact_ok(5000) and R.int_exact_ok(46848 + 37)
    assert 3072 * 49 * 64 ** 2 < 2 ** 24 * 64 ** 2 and 5000 * 49 * 64 ** 2 < 2 ** 24 * 64 ** 2
    assert not R.int_exact_ok(2 ** 24 // 49 + 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1])
def test_clean_emulation_passes(nt, dtype, which):
    K = L_NT[dtype][which]
    x, accs = nt[(dtype, K)]
    for name, kw in _flavours(dtype).items():
        for order in R.ORDERS:
            r = _worst(x, accs[order], kw)
            print(f"{dtype} K={K} {name} {order}: worst err/bound {r:.3f}")
            assert r <= 1.0, (name, order, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant", sorted(R.MAINLOOP_MUTANTS))
def test_mainloop_mutant_is_rejected(nt, dtype, mutant):
    K = L_NT[dtype][1]
    x, accs = nt[(dtype, K)]
    a2, b2, rows, cols = R.mutate_operands(x["a"], x["b"], dtype, R.MAINLOOP_MUTANTS[mutant])
    acc = accs["forward"].copy()
    acc[rows, cols] = R.emu_acc(a2[rows], b2[cols], dtype)
    for name in ("plain", "bias+resid"):
        r = _worst(x, acc, R.FLAVOURS[name])
        print(f"mutant {mutant} {dtype} K={K} {name}: worst err/bound {r:.3g}")
        assert r > 1.0, f"mutant {mutant} passes the bounds"


# mutant -> (flavour that shows it, operand dtypes it must fail for)
_EPI = {4: ("act1+pre->f32", DTYPES), 5: ("alpha->f32", DTYPES), 6: ("act1+pre->f32", DTYPES), 7: ("act1+pre->f32", ("bf16",)),
        8: ("bias", ("bf16", "fp8")), 9: ("act1+resid->f32", DTYPES), 10: ("accumulate->f32", DTYPES), 11: ("gelu_in.act4->f32", DTYPES)}


@pytest.mark.parametrize("mutant", sorted(_EPI))
def test_epilogue_mutant_is_rejected(nt, mutant):
    name, dtypes = _EPI[mutant]
    for dtype in dtypes:
        flav = name if dtype != "f32" else name.replace("->f32", "")
        kw = R.FLAVOURS[flav] if flav in R.FLAVOURS else {k: v for k, v in R.FLAVOURS[name].items() if k != "out_dtype"}
        x, accs = nt[(dtype, L_NT[dtype][1])]
        r = _worst(x, accs["forward"], kw, mutant=R.EPILOGUE_MUTANTS[mutant])
        print(f"mutant {mutant} {R.EPILOGUE_MUTANTS[mutant]} {dtype} {flav}: worst err/bound {r:.3g}")
        assert r > 1.0, f"mutant {mutant} passes the bounds ({dtype})"


@pytest.mark.parametrize("dtype", DTYPES)
def test_tanh_derivative_is_rejected(nt, dtype):
    """Mutant 6, second half: the tanh form's derivative, where it is stored (act 3) and where gelu_in is differentiated."""
    x, accs = nt[(dtype, L_NT[dtype][1])]
    for name in ("act3->f32", "gelu_in.act0->f32"):
        kw = {k: v for k, v in R.FLAVOURS[name].items() if dtype != "f32" or k != "out_dtype"}
        r = _worst(x, accs["forward"], kw, mutant="tanh_gelu_grad")
        print(f"mutant 6' {dtype} {name}: worst err/bound {r:.3g}")
        assert r > 1.0


def test_bf16_store_hides_the_tanh_form_but_not_truncation(nt):
    """Why mutant 6 is asked of the f32 output only, and that the store term is still tight: truncation fails for every bf16-output flavour."""
    x, accs = nt[("bf16", 1536)]
    for name, kw in _flavours("bf16").items():
        if kw.get("out_dtype") != "f32":
            assert _worst(x, accs["forward"], kw, mutant="bf16_store_truncates") > 1.0, name


# ------------------------------------------------------------------------------------------------ weight gradients
N1, N2 = 26, 24
_TN = [dict(), dict(scale=0.37), dict(accumulate=True), dict(scale=-1.7, accumulate=True), dict(perm=(8, 3))]


@pytest.fixture(scope="module")
def tn():
    return {(d, T): R.tn_inputs(T, N1, N2, d, seed=T) for d in ("bf16", "f32") for T in L_TN + (249 * 3,)}


def _tn_worst(x, kw, emu_kw, nsplit):
    ref = R.tn_ref(x, nsplit=nsplit, **kw)
    out, db = R.emu_tn(x, **kw, **emu_kw)
    return R.ratio(out, ref["out"], ref["out_bound"]), R.ratio(db, ref["dbias"], ref["dbias_bound"])


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_clean_tn_emulation_passes(tn, dtype):
    for T, batches in ((64, 1), (777, 1), (747, 3)):
        x = tn[(dtype, T)]
        for chunk in (64, 256, 832):
            nsplit = batches * -(-(T // batches) // chunk)
            for kw in _TN:
                for order in R.ORDERS:
                    r = _tn_worst(x, kw, dict(chunk_rows=chunk, order=order, batches=batches), nsplit)
                    print(f"tn {dtype} T={T}x{batches} chunk={chunk} {kw} {order}: out {r[0]:.3f} dbias {r[1]:.3f}")
                    assert max(r) <= 1.0, (T, chunk, kw, order, r)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("mutant", sorted(R.TN_MUTANTS))
def test_tn_mutant_is_rejected(tn, dtype, mutant):
    x = tn[(dtype, 777)]
    name = R.TN_MUTANTS[mutant]
    kw = dict(perm=(8, 3)) if mutant == 14 else dict()
    prev = R.tn_inputs(777, N1 + 13, N2, dtype, seed=5)
    r = _tn_worst(x, kw, dict(chunk_rows=256, mutant=name, prev_problem=prev), nsplit=4)
    print(f"mutant {mutant} {name} {dtype}: out {r[0]:.3g} dbias {r[1]:.3g}")
    assert (r[1] if mutant in (15, 16) else r[0]) > 1.0, f"mutant {mutant} passes the bounds"


# ------------------------------------------------------------------------------------------------ exact integer operands
def _int_nt(dtype, K, seed=11):
    a, b = R.int_tensor((M, K), seed), R.int_tensor((N, K), seed + 1)
    bias = R.int_tensor((N,), seed + 2)
    x = dict(a=a, b=b, sa=1.0, sb=1.0, dtype=dtype, bias=bias)
    if dtype == "fp8":
        (x["a"], x["sa"]), (x["b"], x["sb"]) = R.round_to(a, "fp8"), R.round_to(b, "fp8")
    return x, a @ b.T + bias[None, :]


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_nt_is_exact_and_catches_the_sum_mutants(dtype):
    K = 3072
    x, want = _int_nt(dtype, K)
    for order in R.ORDERS:
        acc = R.emu_acc(x["a"], x["b"], dtype, order)
        for out_dtype in ("f32",) if dtype == "f32" else ("f32", "bf16"):
            got, _ = R.emu_epilogue(acc, x, bias=True, out_dtype=out_dtype)
            assert np.array_equal(got, want if out_dtype == "f32" else R.bf16_rne(want)), (order, out_dtype)
    acc0 = R.emu_acc(x["a"], x["b"], dtype)
    for mutant in sorted(R.MAINLOOP_MUTANTS):
        a2, b2, rows, cols = R.mutate_operands(x["a"], x["b"], dtype, R.MAINLOOP_MUTANTS[mutant])
        acc = acc0.copy()
        acc[rows, cols] = R.emu_acc(a2[rows], b2[cols], dtype)
        got, _ = R.emu_epilogue(acc, x, bias=True, out_dtype="f32")
        assert not np.array_equal(got, want), f"mutant {mutant} is invisible to the integer case"


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_integer_tn_is_exact_and_catches_the_sum_mutants(dtype):
    T = 777
    x = dict(a=R.int_tensor((T, N1), 21), b=R.int_tensor((T, N2), 22), dtype=dtype)
    prev = dict(a=R.int_tensor((T, N1 + 13), 23))
    want, want_b = x["a"].T @ x["b"], x["a"].sum(0)
    for order in R.ORDERS:
        out, db = R.emu_tn(x, chunk_rows=256, order=order)
        assert np.array_equal(out, want) and np.array_equal(db, want_b)
    p = R.tn_perm(N2, 8, 3)
    out, _ = R.emu_tn(x, chunk_rows=256, perm=(8, 3))
    assert np.array_equal(out[:, p], want)
    for mutant, name in sorted(R.TN_MUTANTS.items()):
        out, db = R.emu_tn(x, chunk_rows=256, perm=(8, 3) if mutant == 14 else (0, 0), mutant=name, prev_problem=prev)
        same = np.array_equal(db, want_b) if mutant in (15, 16) else np.array_equal(out[:, p] if mutant == 14 else out, want)
        assert not same, f"mutant {mutant} is invisible to the integer case"
