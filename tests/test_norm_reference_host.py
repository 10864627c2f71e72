"""CPU test of the tester behind the normalisation checks (tests/norm_ref.py): an f32 emulation of the kernels' arithmetic with their real
summation structure -- lanes and wave_sum, per-wave row chains and the two-stage parameter reduce, row groups and splits of the group norm --
stays inside every per-element bound of the fp64 reference at the smallest and the largest shape of the GPU cases, in both dtypes, with and
without the activation, in forward and reversed order, isolated and chained; it equals every exact case bit for bit; twenty-two wrong kernels,
each a one-line mutation of it, are rejected in both dtypes; and the first-row pivot of the group norm fails the capped statistics bound on an
atypical first row where the sampled pivot passes.  Run with -s to see every ratio."""
import numpy as np
import pytest

import norm_ref as R

DTYPES = ("bf16", "f32")


def _worst(into, rs):
    for k, v in rs.items():
        into[k] = max(into.get(k, 0.0), v)


def _fed_stats(ref):
    (m, m32), (r, r32) = R.fed(ref["mean"]), R.fed(ref["rstd"])
    return m, r, m32, r32


def _ln_all(p, act, lp, rev, worst, mut_f=None, mut_b=None, add=True, accumulate=True):
    """Forward, isolated backward and chained backward of one problem -> the ratios in `worst`."""
    ref = R.ln_ref_fwd(p, act, lp)
    e = R.emu_ln_fwd(p, act, lp, rev, mut_f, pitch=8)
    _worst(worst, R.ratios(e, ref, R.LN_FWD_OUT))
    m, r, m32, r32 = _fed_stats(ref)
    kw = dict(act=act, lp=lp, add=add, accumulate=accumulate)
    _worst(worst, R.ratios(R.emu_ln_bwd(p, m32, r32, rev=rev, mut=mut_b, **kw), R.ln_ref_bwd(p, m, r, **kw), R.LN_BWD_OUT))
    if mut_f is None and mut_b is None:
        ch = R.ratios(R.emu_ln_bwd(p, e["mean"], e["rstd"], rev=rev, **kw), R.ln_ref_bwd(p, ref["_mean"], ref["_rstd"], **kw), R.LN_BWD_OUT)
        _worst(worst, {k + ".chained": v for k, v in ch.items()})


def _gn_all(p, rev, worst, mut=None, old_pivot=False, accumulate=True):
    ref = R.gn_ref_fwd(p)
    e = R.emu_gn_fwd(p, rev, mut, old_pivot)
    _worst(worst, R.ratios(e, ref, R.GN_FWD_OUT))
    m, r, m32, r32 = _fed_stats(ref)
    _worst(worst, R.ratios(R.emu_gn_bwd(p, m32, r32, accumulate, rev, mut), R.gn_ref_bwd(p, m, r, accumulate), R.GN_BWD_OUT))
    if mut is None and not old_pivot:
        ch = R.ratios(R.emu_gn_bwd(p, e["mean"], e["rstd"], accumulate, rev), R.gn_ref_bwd(p, ref["_mean"], ref["_rstd"], accumulate), R.GN_BWD_OUT)
        _worst(worst, {k + ".chained": v for k, v in ch.items()})


def test_inputs_and_constructions_are_what_the_checks_promise():
    p = R.ln_inputs(333, 260, "bf16", "bf16")
    assert np.array_equal(p["x"], R.bf16_rne(p["x"])) and np.array_equal(p["dy"], R.bf16_rne(p["dy"]))
    ref = R.ln_ref_fwd(p)
    sd = 1.0 / ref["rstd"][:300]
    assert (np.abs(ref["mean"][:300]) / sd).max() > 60 and sd.max() / sd.min() > 32          # rows whose mean dwarfs their spread
    assert not p["x"][332].any() and np.ptp(p["x"][331]) == 0 and p["x"][331, 0] != 0
    assert np.array_equal(ref["y_f32"][332], p["beta"]) and not ref["y_f32_b"][332].any()       # the zero row: y = beta, bound 0
    g = R.gn_inputs(2, 1599, 64, "f32")
    assert R.gn_kappa(g["x"]).max() < 1.0
    a = R.gn_inputs(2, 1599, 64, "f32", onset=True)
    k = (a["x"][:, 0] - a["x"].mean(1)) ** 2 / a["x"].var(1)
    assert k[:, 0::2].min() > 500 and k[:, 1::2].min() > 1500                                   # first rows ~ 32 and ~ 256 sigma off (of the inflated sigma)
    assert R.exact_ok(R.LN_ROWS_BIG, 1024, 1024, 3)
    assert R.gn_pivot_rows(1) == [0] and R.gn_pivot_rows(2) == [0, 1] and R.gn_pivot_rows(31) == list(range(31))
    assert all(len(set(R.gn_pivot_rows(T))) == min(T, 32) and max(R.gn_pivot_rows(T)) < T for T in R.GN_T + (31999,))
    assert R.gn_pivot_rows(1599)[0] > 0                                                         # the first row is not among the sampled ones


@pytest.mark.parametrize("flavour", DTYPES)
def test_both_gelu_flavours_saturate_exactly(flavour):
    assert R.gelu_saturates(flavour)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("act", [0, 1])
def test_layernorm_emulation_is_inside_every_bound(dt, act):
    worst = {}
    for rows, W in ((1, 4), (333, 260), (R.LN_ROWS_BIG, 1024)):
        p = R.ln_inputs(rows, W, dt, dt)
        for rev in (False, True):
            for lp in (True, False):
                if rows > 1000 and (lp != (dt == "bf16") or (rev and act)):                    # the largest shape: one output flavour per dtype
                    continue
                _ln_all(p, act, lp, rev, worst)
    print(f"ln emulation[{dt},act{act}] worst err / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("dt", DTYPES)
def test_group_norm_emulation_is_inside_every_bound(dt):
    worst = {}
    for B, T, C in ((1, 1, 64), (3, 33, 320), (3, 2081, 512)):
        p = R.gn_inputs(B, T, C, dt)
        for rev in (False, True):
            _gn_all(p, rev, worst)
    print(f"gn emulation[{dt}] worst err / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def _store(want, lp):
    return R.bf16_rne(want) if lp else want


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("act", [0, 1])
def test_emulation_equals_the_exact_layernorm_cases(dt, act):
    for rows, W in ((333, 64), (17, 512), (R.LN_ROWS_BIG, 1024)):
        p = R.ln_exact_case(rows, W, dt, dt, act)
        for rev in (False, True):
            e = R.emu_ln_bwd(p, np.zeros(rows), np.ones(rows), act=act, lp=dt == "bf16", add=True, accumulate=True, rev=rev)
            assert np.array_equal(e["dx_f32"], p["want_dx"]) and np.array_equal(e["dx_lp"], R.bf16_rne(p["want_dx"]))
            assert np.array_equal(e["dgamma"], p["want_dg"] + p["prev_g"]) and np.array_equal(e["dbeta"], p["want_db"] + p["prev_b"])


def test_emulation_equals_the_exact_forward_statistics():
    p = R.ln_stats_case(33, 512)
    for rev in (False, True):
        e = R.emu_ln_fwd(p, 0, False, rev)
        assert np.array_equal(e["mean"], p["want_mean"])
        assert np.array_equal(e["y_f32"][1::2], np.broadcast_to(p["beta"], (16, 512)))


@pytest.mark.parametrize("dt", DTYPES)
def test_emulation_equals_the_exact_group_norm_cases(dt):
    for T in (1, 64, 1024):
        p = R.gn_exact_case(3, T, 64, dt)
        for rev in (False, True):
            e = R.emu_gn_bwd(p, np.zeros((3, 64)), np.ones((3, 64)), True, rev)
            assert np.array_equal(e["dx"], _store(p["want_dx"], dt == "bf16"))
            assert np.array_equal(e["dgamma"], p["want_dg"] + p["prev_g"]) and np.array_equal(e["dbeta"], p["want_db"] + p["prev_b"])
            assert np.array_equal(R.emu_gn_fwd(p, rev)["mean"], p["want_mean"])


# ------------------------------------------------------------------------------------------------ wrong kernels
# number -> (where it acts, the bounded problem that must reject it: rows, W, act | B, T, C).  X: the exact cases see it as well.
LN_AT = {1: ("f", 333, 260, 0), 2: ("f", 333, 260, 0), 3: ("f", 333, 260, 0), 4: ("f", 333, 260, 0), 5: ("f", 333, 260, 0), 6: ("b", 333, 260, 0),
         7: ("b", 333, 260, 0), 8: ("b", 333, 260, 0), 9: ("b", 333, 260, 0), 10: ("b", 333, 260, 0), 11: ("b", 333, 260, 1), 12: ("fb", 333, 260, 0),
         13: ("b", 333, 260, 0), 14: ("b", R.LN_ROWS_BIG, 64, 0)}
LN_EXACT_SEES = {6, 9, 10, 11, 12, 13, 14}
GN_EXACT_SEES = {16, 17, 20, 21}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("num", sorted(R.LN_MUTANTS))
def test_wrong_layernorm_kernels_are_rejected(dt, num):
    side, rows, W, act = LN_AT[num]
    mut = R.LN_MUTANTS[num]
    p = R.ln_inputs(rows, W, dt, dt)
    worst = {}
    _ln_all(p, act, True, False, worst, mut if "f" in side else None, mut if "b" in side else None)
    if num == 12:
        worst = {k: v for k, v in worst.items() if k.endswith("_lp")}
    name, r = max(worst.items(), key=lambda kv: kv[1])
    exact = None
    if num in LN_EXACT_SEES:
        er = R.LN_ROWS_BIG if num == 14 else 333
        q = R.ln_exact_case(er, 64, dt, dt, 1 if num == 11 else 0)
        e = R.emu_ln_bwd(q, np.zeros(er), np.ones(er), act=1 if num == 11 else 0, add=True, accumulate=True, mut=mut)
        exact = not (np.array_equal(e["dx_f32"], q["want_dx"]) and np.array_equal(e["dx_lp"], R.bf16_rne(q["want_dx"]))
                     and np.array_equal(e["dgamma"], q["want_dg"] + q["prev_g"]) and np.array_equal(e["dbeta"], q["want_db"] + q["prev_b"]))
        assert exact, f"mutant {num} ({mut}) equals the exact case"
    print(f"mutant {num:2d} {mut:28s} [{dt}] bound: {name} {r:.3g}" + ("" if exact is None else "  exact: rejected"))
    assert r > 1.0, f"mutant {num} ({mut}) passes the bounds: {worst}"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("num", sorted(R.GN_MUTANTS))
def test_wrong_group_norm_kernels_are_rejected(dt, num):
    mut = R.GN_MUTANTS[num]
    p = R.gn_inputs(2, 1025, 64, dt)
    worst = {}
    _gn_all(p, False, worst, mut)
    name, r = max(worst.items(), key=lambda kv: kv[1])
    exact = None
    if num in GN_EXACT_SEES:
        q = R.gn_exact_case(3, 1024, 64, dt)
        e = R.emu_gn_bwd(q, np.zeros((3, 64)), np.ones((3, 64)), True, False, mut)
        exact = not (np.array_equal(e["dx"], _store(q["want_dx"], dt == "bf16")) and np.array_equal(e["dgamma"], q["want_dg"] + q["prev_g"])
                     and np.array_equal(e["dbeta"], q["want_db"] + q["prev_b"]) and np.array_equal(R.emu_gn_fwd(q, mut=mut)["mean"], q["want_mean"]))
        assert exact, f"mutant {num} ({mut}) equals the exact case"
    print(f"mutant {num:2d} {mut:28s} [{dt}] bound: {name} {r:.3g}" + ("" if exact is None else "  exact: rejected"))
    assert r > 1.0, f"mutant {num} ({mut}) passes the bounds: {worst}"


# ------------------------------------------------------------------------------------------------ the pivot
@pytest.mark.parametrize("dt", DTYPES)
def test_first_row_pivot_fails_the_capped_bound_and_the_sampled_pivot_passes(dt):
    p = R.gn_inputs(2, 1599, 64, dt, onset=True)
    ref = R.gn_ref_fwd(p)
    old = R.ratios(R.emu_gn_fwd(p, old_pivot=True), ref, R.GN_FWD_OUT)
    new = {}
    for rev in (False, True):
        _worst(new, R.ratios(R.emu_gn_fwd(p, rev), ref, R.GN_FWD_OUT))
    print(f"onset T=1599 [{dt}] first-row pivot {old}  sampled pivot {new}")
    assert old["rstd"] > 1.0 and max(new.values()) <= 1.0


def test_sampled_pivot_passes_at_ten_seconds_of_audio():
    p = R.gn_inputs(1, 31999, 64, "f32", onset=True)
    ref = R.gn_ref_fwd(p)
    old = R.ratios(R.emu_gn_fwd(p, old_pivot=True), ref, ("mean", "rstd"))
    new = R.ratios(R.emu_gn_fwd(p), ref, ("mean", "rstd"))
    print(f"onset T=31999 [f32] first-row pivot {old}  sampled pivot {new}")
    assert old["rstd"] > 1.0 and max(new.values()) <= 1.0
