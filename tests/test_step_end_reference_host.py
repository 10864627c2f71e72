"""CPU test of the tester behind check_optimizer_step (tests/step_end_ref.py): an f32 emulation of the kernels' formula stays inside the per-element
bounds of the fp64 reference over the check's own inputs, and every plausible wrong formula leaves them at the step where it first differs."""
import numpy as np
import pytest

import step_end_ref as R

N = 200_000


def _trajectory(form, wd):
    """[(plan entry, state before the step, reference of the step, state after)] of the CORRECT emulation, three steps from zero moments."""
    p, g = R.make_inputs(N, seed=7)
    m, v = np.zeros(N, np.float32), np.zeros(N, np.float32)
    out = []
    for plan in R.step_plan():
        step, lr, cc, _ = plan
        ref = R.ref_step(p, g, m, v, step, lr, wd, cc)
        new = R.emulate_step(p, g, m, v, step, lr, wd, cc, form=form)
        out.append((plan, (p, g, m, v), ref, new))
        p, m, v = new
    return out


@pytest.fixture(scope="module")
def runs():
    return {(form, wd): _trajectory(form, wd) for form in ("chunked", "multi") for wd in (R.WD, 0.0)}


def test_inputs_are_what_the_check_promises():
    p, g = R.make_inputs(N, seed=7)
    mag = np.abs(g[g != 0])
    assert 0.04 < np.mean(g == 0) < 0.06
    assert mag.min() >= 0.99e-10 and mag.max() <= 1.01e2
    assert np.mean(mag < 1e-8) > 0.1 and np.mean(mag > 1.0) > 0.1          # eps-dominated and eps-free elements both present
    assert 0.45 < np.mean(g < 0) / np.mean(g != 0) < 0.55
    assert abs(p.mean()) < 0.02 and abs(p.std() - 1) < 0.02
    pre, n = R.chunk_prefix(R.SIZE_LISTS["many"])
    assert len(pre) == 67 and n == 67 + 1 + 2 and pre[24] - pre[23] == 2 and pre[51] - pre[50] == 3
    assert all(1 <= s <= 29 for i, s in enumerate(R.SIZE_LISTS["many"]) if i not in (23, 50))


@pytest.mark.parametrize("form", ["chunked", "multi"])
@pytest.mark.parametrize("wd", [R.WD, 0.0])
def test_correct_formula_passes(runs, form, wd):
    for (step, _, _, _), _, ref, (p, m, v) in runs[(form, wd)]:
        r = R.ratios(ref, p, m, v)
        print(f"{form} wd={wd} step {step}: worst ratio p {r['p']:.3f} exp_avg {r['m']:.3f} exp_avg_sq {r['v']:.3f}")
        assert max(r.values()) <= 1.0, (step, r)


def test_forms_agree_within_the_sum_of_their_bounds(runs):
    for a, b in zip(runs[("chunked", R.WD)], runs[("multi", R.WD)]):
        (plan, (p, g, m, v), ref, got_a) = a
        got_b = R.emulate_step(p, g, m, v, plan[0], plan[1], R.WD, plan[2], form="multi")      # from the chunked form's own state
        for k, x, y in zip("pmv", got_a, got_b):
            assert R.ratio(x, y.astype(np.float64), 2 * ref[k + "_bound"]) <= 1.0


@pytest.mark.parametrize("form", ["chunked", "multi"])
@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_mutant_is_rejected(runs, form, mutant):
    at = R.MUTANTS[mutant]
    traj = runs[(form, R.WD)]
    (step, lr, cc, _), (p, g, m, v), ref, _ = traj[at - 1]
    assert step == at
    lr_prev = traj[at - 2][0][1] if at > 1 else lr
    got = R.emulate_step(p, g, m, v, step, lr, R.WD, cc, form=form, mutant=mutant, lr_prev=lr_prev)
    r = R.ratios(ref, *got)
    print(f"{mutant} ({form}) at step {at}: worst ratio p {r['p']:.3g} exp_avg {r['m']:.3g} exp_avg_sq {r['v']:.3g}")
    assert max(r.values()) > 1.0, f"{mutant} passes the bounds: inputs or bounds too weak"


def test_ratio_edge_cases():
    ref, bound = np.array([1.0, 0.0, 2.0]), np.array([0.5, 0.0, 0.5])
    assert R.ratio(np.array([1.25, 0.0, 2.0]), ref, bound) == 0.5
    assert R.ratio(np.array([1.0, 1e-30, 2.0]), ref, bound) == np.inf           # a zero bound demands equality
    assert R.ratio(np.array([1.0, 0.0, np.nan]), ref, bound) == np.inf
    assert R.ratio(np.array([]), np.array([]), np.array([])) == 0.0
