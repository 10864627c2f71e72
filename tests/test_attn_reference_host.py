"""CPU test of the tester behind the attention checks (tests/attn_ref.py): an f32 emulation of the kernels' arithmetic -- 64-key tiles, a running
maximum with and without the lazy threshold, P rounded to bf16 and l summed from the rounded P, f32 accumulation, lse formed as the kernel forms
it, the backward from lse and delta as accumulator starts -- stays inside every per-element bound of the fp64 reference in three summation orders,
both dtypes, all mask modes, pre-scaled and not, with lengths, at the largest S the GPU cases use; it equals the exact selections bit for bit;
and twenty-one wrong kernels, each a one-line mutation of it, are rejected at the GPU cases' own shapes by the instrument named in INSTRUMENT."""
import functools

import numpy as np
import pytest

import attn_ref as R

DTYPES = ("bf16", "f32")
S_MAX = max(R.BOUND_S)
LENS_BOUND = (257, list(R.LEN_CASES[257][0]))             # S, lengths of the length-aware bounded case the mutants run at
LENS_EXACT = (129, list(R.LEN_CASES[129][1]))             # ... and of the exact one (65: a ragged tile; 1; 128)


@functools.lru_cache(maxsize=None)
def _problem(dtype, S, mode, pre, lens=None, B=2):
    x = R.make_inputs(len(lens) if lens else B, S, 1, dtype, seed=3, **R.bound_config(S, mode, pre, list(lens) if lens else None))
    ref = R.attn_ref(x)
    return x, ref, R.fed(ref, x)


def _eq(got, want, dtype):
    return np.array_equal(got, want if dtype == "f32" else R.bf16_rne(want))


def test_inputs_are_what_the_checks_promise():
    assert all(np.gcd(7, t) == 1 and np.gcd(5, t) == 1 for t in (16, 64))
    x = R.make_inputs(2, 321, 2, "bf16", 1, False, spike=True)
    assert all(np.array_equal(x[n], R.bf16_rne(x[n])) for n in ("q", "k", "v", "do"))
    rms = np.sqrt((x["q"] ** 2).mean((0, 2, 3)))
    assert np.allclose(rms / R.temperatures(321), 1.0, rtol=0.3) and rms.max() / rms.min() > 32
    m = x["mask"]
    assert (m == R.FMIN).any() and (m == -65504.0).any() and (m[:, 0] == 0).all()
    P = R.attn_ref(R.make_inputs(1, 321, 1, "f32", 0, False))["probs"][0, 0]
    assert P.max(1).max() > 0.99 and P.max(1).min() < 0.02                                         # nearly one-hot rows and nearly flat ones
    xp = R.make_inputs(1, 321, 1, "f32", 0, True, spike=True)
    t = xp["q"][0, :, 0] @ xp["k"][0, :, 0].T
    assert (t[:, 321 - 7] - t[:, :256].max(1)).max() > 10 * R.LAZY_THR                             # the late spike passes the lazy threshold by far
    assert set(np.unique(R.make_mask(2, 200, 2, "ref"))) == {0.0, -65504.0, 65505.0, 1.0}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("pre", [False, True])
def test_clean_emulation_is_inside_every_bound(dtype, mode, pre):
    worst = {}
    for S, lens in ((S_MAX, None), LENS_BOUND):
        x, ref, fd = _problem(dtype, S, mode, pre, tuple(lens) if lens else None)
        for order in R.ORDERS:
            e = R.emu_fwd(x, order)
            rs = R.fwd_ratios(x, ref, e)
            rs.update(R.bwd_ratios(x, ref, R.emu_bwd(x, fd["o_soft"], fd["lse"], order)))
            rs.update({k + ".chained": v for k, v in R.bwd_ratios(x, ref, R.emu_bwd(x, e["o_soft"], e["lse"], order), chained=True).items()})
            for k, v in rs.items():
                worst[k] = max(worst.get(k, 0.0), v)
            for b, L in enumerate(x["lens"]):                                                      # rows past a length: exactly zero
                assert not e["o"][b, L:].any() and not e["lse"][b, :, L:].any()
    print(f"{dtype} mode {mode} pre {int(pre)}: worst err/bound " + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))
    assert max(worst.values()) < 1.0, worst


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_shapes_and_helpers_inside_bounds(dtype):
    for S in (1, 63, 65):
        for mode, pre in ((0, True), (1, False), (2, True)):
            x, ref, fd = _problem(dtype, S, mode, pre)
            rs = R.fwd_ratios(x, ref, R.emu_fwd(x))
            rs.update(R.bwd_ratios(x, ref, R.emu_bwd(x, fd["o_soft"], fd["lse"])))
            want, bound = R.probs_ref(x, ref)
            rs["probs"] = R.ratio(R.emu_probs(x, fd["lse"]), want, bound)
            print(f"{dtype} S={S} mode {mode} pre {int(pre)}: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(rs.items())))
            assert max(rs.values()) < 1.0, (S, mode, rs)
            if mode == 1:
                masked = x["mask"][0] < -60000.0
                assert not R.emu_probs(x, fd["lse"])[0, :, :, masked].any() and not want[0, :, :, masked].any() and not bound[0, :, :, masked].any()
    rng = np.random.default_rng(1)
    a, b = (R.round_to(rng.standard_normal((37, 3, 64)), dtype)[0] for _ in range(2))
    f = (R.F(-1.0) + (rng.standard_normal((37, 3)) * 2.0 ** np.arange(-1, 2)).astype(R.F)).astype(np.float64)
    want, bound = R.head_scale_ref(a, b, f, dtype)
    got = (a.astype(R.F) + (b.astype(R.F) * f[:, :, None].astype(R.F)).astype(R.F)).astype(R.F)
    assert R.ratio(R.round_to(got, dtype)[0], want, bound) < 1.0
    assert R.ratio(R.round_to(got * R.F(1.0 + 2.0 ** -7), dtype)[0], want, bound) > 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_emulation_equals_the_exact_selections(dtype, mode):
    for S, lens in ((257, None), (65, None), LENS_EXACT, (257, list(R.LEN_CASES[257][0]))):
        for pre in (False, True):
            for single in (False, True):
                x = R.exact_case(len(lens) if lens else 2, S, 2, dtype, mode, pre, lens=lens, single=single)
                assert R.exact_ok(x)
                w = R.exact_want(x)
                ref = R.attn_ref(x)
                for n in ("o", "o_soft", "corr") + (("probs",) if mode != 2 else ()):         # the fp64 reference agrees with the construction
                    assert np.allclose(ref[n], w[n], rtol=1e-12, atol=1e-12), n
                assert {1.0, 2.0, 4.0} >= set(np.unique(x["sel"].sum(2))) - {0.0}
                for order in R.ORDERS:
                    e = R.emu_fwd(x, order)
                    assert _eq(e["o"], w["o"], dtype) and _eq(e["o_soft"], w["o_soft"], dtype) and np.array_equal(e["corr"], w["corr"]), (S, pre, order)
                    l1 = ~np.isnan(w["lse"])
                    assert not e["lse"][l1].any() and R.ratio(e["lse"], w["lse_full"], ref["lse_bound"]) < 1.0
                    if single:
                        eb = R.emu_bwd(x, R.round_to(w["o_soft"], dtype)[0], np.zeros_like(w["lse"]), order)
                        assert all(_eq(eb[n], w[n], dtype) for n in ("dq", "dk", "dv")), (S, pre, order)
                        assert all(np.array_equal(eb["delta"][b, :, :L], w["delta"][b, :, :L]) for b, L in enumerate(x["lens"]))
                if single and lens is None:
                    assert np.array_equal(R.emu_probs(x, np.zeros_like(w["lse"])), w["probs"])


# mutant -> (mask mode, pre-scaled, with lengths) of the case that shows it, and the instruments that must reject it in BOTH dtype flavours:
# "bound" = a per-element bound of the spread-magnitude case, "exact" = the exact selections.  (7 and 8 in the f32 flavour: a P / an o that went
# through a bf16 truncation.  13, 14, 17, 18 leave the exact cases alone: lse = 0 and dK = dQ = 0 there; 7 too: P is 0 or 1.)
INSTRUMENT = {1: ((0, True, False), ("bound", "exact")), 2: ((0, False, False), ("bound", "exact")), 3: ((0, True, True), ("bound", "exact")),
              4: ((0, False, True), ("bound", "exact")), 5: ((0, True, False), ("bound", "exact")), 6: ((0, False, False), ("bound", "exact")),
              7: ((0, True, False), ("bound",)), 8: ((2, True, False), ("bound", "exact")), 9: ((1, False, False), ("bound", "exact")),
              10: ((2, False, True), ("bound", "exact")), 11: ((2, False, False), ("bound", "exact")), 12: ((2, False, False), ("bound", "exact")),
              13: ((0, True, False), ("bound",)), 14: ((0, False, False), ("bound",)), 15: ((2, True, False), ("bound", "exact")),
              16: ((0, False, False), ("bound", "exact")), 17: ((0, True, False), ("bound",)), 18: ((0, False, False), ("bound",)),
              19: ((2, True, False), ("bound", "exact")), 20: ((2, False, True), ("bound", "exact")), 21: ((0, True, True), ("bound", "exact"))}


def _bound_rejects(dtype, mu):
    (mode, pre, with_len), _ = INSTRUMENT[mu]
    S, lens = LENS_BOUND if with_len else (S_MAX, None)
    x, ref, fd = _problem(dtype, S, mode, pre, tuple(lens) if lens else None)
    name = R.MUTANTS[mu]
    if mu in R.FWD_MUTANTS:
        top = int(np.argmax(ref["probs"][0, 0].max(0)))                                        # mutant 1 drops a key that leads some row
        rs = R.fwd_ratios(x, ref, R.emu_fwd(x, mutant=name, drop_key=top))
    else:
        rs = R.bwd_ratios(x, ref, R.emu_bwd(x, fd["o"] if mu == 15 else fd["o_soft"], fd["lse"], mutant=name))
    return rs


def _exact_rejects(dtype, mu):
    (mode, pre, with_len), _ = INSTRUMENT[mu]
    S, lens = LENS_EXACT if with_len else (129, None)
    x = R.exact_case(3, S, 1, dtype, mode, pre, lens=lens, single=mu in R.BWD_MUTANTS)
    w = R.exact_want(x)
    name = R.MUTANTS[mu]
    if mu in R.FWD_MUTANTS:
        e = R.emu_fwd(x, mutant=name, drop_key=64)
        same = _eq(e["o"], w["o"], dtype) and _eq(e["o_soft"], w["o_soft"], dtype) and np.array_equal(e["corr"], w["corr"]) \
            and not e["lse"][~np.isnan(w["lse"])].any()
    else:
        e = R.emu_bwd(x, R.round_to(w["o"] if mu == 15 else w["o_soft"], dtype)[0], np.zeros_like(w["lse"]), mutant=name)
        same = all(_eq(e[n], w[n], dtype) for n in ("dq", "dk", "dv")) and all(
            np.array_equal(e["delta"][b, :, :L], w["delta"][b, :, :L]) for b, L in enumerate(x["lens"]))
    return not same


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mu", sorted(R.MUTANTS))
def test_mutant_is_rejected(dtype, mu):
    _, instruments = INSTRUMENT[mu]
    rs = _bound_rejects(dtype, mu)
    ex = _exact_rejects(dtype, mu)
    print(f"mutant {mu} {R.MUTANTS[mu]} {dtype}: bound " + " ".join(f"{k}={v:.3g}" for k, v in rs.items()) + f" | exact rejects: {ex}")
    if "bound" in instruments:
        assert max(rs.values()) > 1.0, f"mutant {mu} passes the bounds"
    if "exact" in instruments:
        assert ex, f"mutant {mu} is invisible to the exact selections"


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_key_in_a_flat_row_and_a_truncating_store(dtype):
    """What the max-relative instrument could not see: ANY key dropped (not only a leading one) leaves the f32 bounds, and the exact case sees it in
    both dtypes (test_mutant_is_rejected); a truncating bf16 store leaves the bound of o wherever the rank-1 term dominates."""
    x, ref, _ = _problem(dtype, S_MAX, 0, False)
    r = R.fwd_ratios(x, ref, R.emu_fwd(x, mutant="one_key_dropped", drop_key=200))
    print(f"{dtype}: key 200 of {S_MAX} dropped: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert max(r.values()) > 1.0
    if dtype == "bf16":
        x, ref, _ = _problem(dtype, S_MAX, 2, True)
        assert R.fwd_ratios(x, ref, R.emu_fwd(x, mutant="o_store_truncates"))["o"] > 1.0
