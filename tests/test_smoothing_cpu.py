"""Host-only checks of the Savitzky-Golay finish's test material (smoothing_cases.py,
smoothing_reference.py): the exact weights against the oracle's, the oracle against the exact filter
chain on every case, and proof that the chain sees the errors the GPU tests exist for.

E_cpu (smoothing_cases.E_CPU) is measured here: the largest |U* - chain U*| and |uu - chain uu| over
every case and update, the oracle fed seeded injected noise and the chain fed the oracle's gradient.
It is the spread between two fp64 evaluations of the same sums (the oracle's left-to-right products
and additions against the exactly rounded sum, fed back through the window).  Measured: 3.109e-15,
recorded as 3.2e-15; test_oracle_against_exact_chain prints it and holds the constant against it.
"""
import os
import re

import numpy as np
import pytest

from oracle import oracle as O

import smoothing_cases as SC
from helpers import CONTROL_ATOL
from smoothing_reference import BackInTime, FilterChain, MUTANTS, exact_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}


def oracle_run(case):
    """The oracle driven through the case's times with seeded injected noise, once per case: a list
    of records (time, raised, gradient, U*, (uu, tt, start)) and the configuration."""
    if case.name not in _RUNS:
        conf, orc, x, sd = SC.oracle_for(case)
        rng = np.random.default_rng(case.seed)
        recs = []
        for j, t in enumerate(case.times):
            n = orc.noise_draws(t)
            orc.inject_noise(rng.standard_normal((n, len(sd))) * sd)
            raised = False
            try:
                orc.update(x, t)
            except RuntimeError as e:
                assert "MPPI_ERR_SMOOTHING" in str(e), str(e)
                raised = True
            recs.append(dict(t=t, raised=raised, gradient=orc.gradient(), U=orc.optimal_control(),
                             windows=orc.smoothing_windows(case.w)))
        orc.close()
        _RUNS[case.name] = (conf, recs)
    return _RUNS[case.name]


def chain_run(case, conf, recs, mutant=None, w=None, order=None):
    """The chain fed the records' gradients: [(raised, U*, (uu, tt, start))] per update."""
    if w is None:
        chain = SC.chain_for(case, conf, mutant)
    else:
        chain = FilterChain(case.H, len(conf.control_min), w, order, conf.time_step, conf.gradient_step,
                            list(conf.control_min), list(conf.control_max), mutant=mutant)
    out = []
    for r in recs:
        raised = False
        try:
            chain.update(r["t"], r["gradient"])
        except BackInTime:
            raised = True
        uu, tt, st = chain.window_arrays()
        out.append((raised, np.array(chain.U), (np.array(uu), np.array(tt), np.array(st))))
    return out


def test_engine_constants():
    """The thresholds the case table derives its shapes from are the engine's."""
    text = open(os.path.join(REPO, "assistedmanipulation_amd", "csrc", "kernels.hip")).read()
    assert int(re.search(r"constexpr int SGK_MAXW = (\d+);", text).group(1)) == SC.SGK_MAXW
    assert int(re.search(r"constexpr int SGK_ZM = (\d+);", text).group(1)) == SC.SGK_ZM
    for c in SC.CASES:
        assert SC.expected_path(c.H, c.w, 12 if c.model == "fr" else 3) == c.path, c.name
        assert c.S <= 32
    z, lit = SC.by_name("zm_edge"), SC.by_name("literal")
    assert z.w - 1 == SC.SGK_ZM and lit.w - 1 == SC.SGK_ZM + 1
    assert SC.by_name("maxw").H + 2 * 2 + 1 == SC.SGK_MAXW and SC.by_name("fallback").H + 2 * 2 + 1 == SC.SGK_MAXW + 1


@pytest.mark.parametrize("w,order", sorted({(c.w, c.order) for c in SC.CASES}) + SC.UNIFORM)
def test_exact_weights(w, order):
    ex = exact_weights(w, order)
    assert sum(ex) == 1 and ex == ex[::-1]
    # the Gram recursion in fp64: a few ulp of the largest weight per term
    np.testing.assert_allclose(O.sg_weights(w, 0, order, 0), [float(v) for v in ex], rtol=0, atol=1e-13)
    if (w, order) in SC.UNIFORM:
        assert all(v == ex[0] for v in ex)
    else:
        assert len(set(ex)) > 1


def test_step_times_collide():
    """colliding_times: fewer distinct step times than steps, so some lower_bound(t_k) != w + k."""
    c = SC.by_name("colliding_times")
    conf, recs = oracle_run(c)
    for r in recs:
        tt = r["windows"][1][0][c.w:c.w + c.H]   # the H step times
        assert len(set(tt.tolist())) <= c.H // 2, len(set(tt.tolist()))
    assert int((c.times[0] - 0.0) / SC.TIME_STEP) > 2 ** 50   # the first update's shift count


def test_oracle_against_exact_chain():
    worst = 0.0
    for case in SC.CASES:
        conf, recs = oracle_run(case)
        got = chain_run(case, conf, recs)
        for j, (r, (raised, U, (uu, tt, st))) in enumerate(zip(recs, got)):
            tag = "%s update %d" % (case.name, j)
            assert r["raised"] == raised == (j in case.raises), tag
            ou, ot, os_ = r["windows"]
            np.testing.assert_array_equal(ot, tt, err_msg=tag + " tt")
            np.testing.assert_array_equal(os_, st, err_msg=tag + " start")
            e = max(float(np.max(np.abs(r["U"] - U))), float(np.max(np.abs(ou - uu))))
            worst = max(worst, e)
    print("E_cpu = %.3e" % worst)
    assert 0.0 < worst <= SC.E_CPU, worst
    assert SC.E_CPU <= 2.0 * worst, "the recorded E_cpu is looser than the measured spread: %.3e" % worst


def gpu_bar(U):
    return SC.FILTER_BAR_FACTOR * SC.E_CPU * max(1.0, float(np.max(np.abs(U))))


@pytest.mark.parametrize("name", SC.MUTANT_CASES)
@pytest.mark.parametrize("mutant", MUTANTS)
def test_chain_sees_the_mutants(name, mutant):
    """Each error the GPU tests exist for moves U* or the window by more than 1000 x the GPU bar."""
    case = SC.by_name(name)
    conf, recs = oracle_run(case)
    true, bad = chain_run(case, conf, recs), chain_run(case, conf, recs, mutant)
    margin = 0.0
    for (_, U, (uu, tt, _)), (_, Ub, (uub, ttb, _)) in zip(true, bad):
        d = max(float(np.max(np.abs(U - Ub))), float(np.max(np.abs(uu - uub))))
        margin = max(margin, d / gpu_bar(U))
    print("%s %s: %.3e x the GPU bar" % (name, mutant, margin))
    assert margin > 1000.0, margin


def test_back_in_time_sees_a_clip_on_the_failed_update():
    """The failed update leaves U*_shifted outside the bounds somewhere, so a finish that clips it on
    the way out (sg_finish_kernel and finish_kernel did) shows in the next update, which does not
    shift: by more than CONTROL_ATOL against the oracle and 1000 x the filter bar against the chain."""
    case = SC.by_name("back_in_time")
    conf, recs = oracle_run(case)
    true, bad = chain_run(case, conf, recs), chain_run(case, conf, recs, "clamp_failed")
    j = case.raises[0]
    for k in range(j + 1):   # nothing differs up to and including the failure: U* and the windows stay
        np.testing.assert_array_equal(true[k][1], bad[k][1])
        np.testing.assert_array_equal(true[k][2][0], bad[k][2][0])
    U, Ub = true[j + 1][1], bad[j + 1][1]
    d = float(np.max(np.abs(U - Ub)))
    print("back_in_time clamp_failed: |dU*| %.3e, %.3e x the GPU bar" % (d, d / gpu_bar(U)))
    assert d > 1000.0 * gpu_bar(U) and d > 1000.0 * CONTROL_ATOL


@pytest.mark.parametrize("w,order", SC.UNIFORM)
def test_rotated_weights_are_invisible_at_order_one(w, order):
    """The gap: with the order-1 filters of every other smoothing run, rotated weights change nothing."""
    case = SC.by_name("nonuniform")
    conf, recs = oracle_run(case)
    true, bad = chain_run(case, conf, recs, None, w, order), chain_run(case, conf, recs, "rotate", w, order)
    for (_, U, (uu, tt, st)), (_, Ub, (uub, ttb, stb)) in zip(true, bad):
        np.testing.assert_array_equal(U, Ub)
        np.testing.assert_array_equal(uu, uub)


@pytest.mark.parametrize("case", SC.CASES, ids=[c.name for c in SC.CASES])
def test_most_outputs_are_off_the_bounds(case):
    """The bars mean little on clamped outputs: fewer than half of U* sits on a bound, every update."""
    conf, recs = oracle_run(case)
    lo, hi = np.asarray(conf.control_min), np.asarray(conf.control_max)
    for j, r in enumerate(recs):
        on = (r["U"] == lo) | (r["U"] == hi)
        assert on.mean() < 0.5, (case.name, j, float(on.mean()))
    assert any(np.any(r["U"] != 0.0) for r in recs)
