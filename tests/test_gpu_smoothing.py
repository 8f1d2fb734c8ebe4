"""The Savitzky-Golay finish on the device, on every path launch_finish can take, with weights that
are not all equal and update times that are not a steady 0.05 s from 0 (smoothing_cases.py).

Every update of every case is held against two references:
  * the oracle, with the suite's usual bars (helpers.assert_update_parity), and its windows: tt and
    start bit-equal, uu within CONTROL_ATOL;
  * the exact filter chain (smoothing_reference.FilterChain) fed the device's own gradient, so that
    what is compared depends on the finish kernel alone: tt and start equal, U* and uu within the
    filter bar 16 x E_cpu x max(1, max |U*|) (smoothing_cases.py: E_cpu is measured on the CPU
    between the oracle and the exact chain; the bar is not tuned against the device).
update_info()["finish_path"] must be the kernel the case was written for.
"""
import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi

import smoothing_cases as SC
from helpers import CONTROL_ATOL, assert_update_parity
from smoothing_reference import BackInTime

pytestmark = pytest.mark.gpu


def _setup(case):
    conf, orc, x, sd = SC.oracle_for(case)
    _, dyn, cost, _ = SC.parts(case)
    dev = am.Trajectory.create(conf, dyn, cost)
    assert dev is not None and dev.H == case.H
    dev.set_noise_source(abi.MPPI_NOISE_HOST_INJECTED)
    if case.model == "fr":
        dev.set_forecast(am.constant_forecast(dev.H))
    return conf, dev, orc, SC.chain_for(case, conf), x, sd


def _inject(dev, orc, t, rng, sd):
    n = orc.noise_draws(t)
    assert dev.noise_draws(t) == n
    eps = rng.standard_normal((n, len(sd))) * sd
    dev.inject_noise(eps)
    orc.inject_noise(eps)


def _check_windows(case, dev, orc, chain, tag):
    """The device's windows against the oracle's and the chain's; returns the worst chain error
    over the filter bar."""
    U = dev.get_optimal_rollout()
    ud, td, sdv = dev.smoothing_windows()
    uo, to, so = orc.smoothing_windows(case.w)
    np.testing.assert_array_equal(td, to, err_msg=tag + " tt against the oracle")
    np.testing.assert_array_equal(sdv, so, err_msg=tag + " start against the oracle")
    np.testing.assert_allclose(ud, uo, rtol=0, atol=CONTROL_ATOL, err_msg=tag + " uu against the oracle")
    uc, tc, sc = chain.window_arrays()
    np.testing.assert_array_equal(td, np.array(tc), err_msg=tag + " tt against the chain")
    np.testing.assert_array_equal(sdv, np.array(sc), err_msg=tag + " start against the chain")
    bar = SC.FILTER_BAR_FACTOR * SC.E_CPU * max(1.0, float(np.max(np.abs(U))))
    eu = float(np.max(np.abs(U - np.array(chain.U))))
    ew = float(np.max(np.abs(ud - np.array(uc))))
    print("%s: |U* - chain| %.3e, |uu - chain| %.3e, bar %.3e" % (tag, eu, ew, bar))
    assert eu <= bar, "%s U* against the exact chain: %.3e > %.3e" % (tag, eu, bar)
    assert ew <= bar, "%s uu against the exact chain: %.3e > %.3e" % (tag, ew, bar)


def _run(case):
    conf, dev, orc, chain, x, sd = _setup(case)
    rng = np.random.default_rng(case.seed)
    for j, t in enumerate(case.times):
        tag = "%s update %d (t = %r)" % (case.name, j, t)
        _inject(dev, orc, t, rng, sd)
        if j in case.raises:
            U0, w0 = dev.get_optimal_rollout(), dev.smoothing_windows()
            with pytest.raises(RuntimeError, match="MPPI_ERR_SMOOTHING"):
                orc.update(x, t)
            with pytest.raises(am.EngineError) as ei:
                dev.update(x, t)
            assert ei.value.status == abi.MPPI_ERR_SMOOTHING, tag
            with pytest.raises(BackInTime):
                chain.update(t, dev.get_gradient())
            # U*, the windows and start are what they were; the plan still answers
            np.testing.assert_array_equal(dev.get_optimal_rollout(), U0, err_msg=tag + " U* after the failure")
            for a, b in zip(dev.smoothing_windows(), w0):
                np.testing.assert_array_equal(a, b, err_msg=tag + " windows after the failure")
            np.testing.assert_array_equal(dev.unfiltered_control(), U0, err_msg=tag + " unfiltered_control")
            t_last = case.times[j - 1]
            for tq in (t_last, t_last + 0.013):
                np.testing.assert_allclose(dev.get(tq), orc.get(tq), rtol=0, atol=CONTROL_ATOL, err_msg=tag + " get")
            np.testing.assert_allclose(dev.get_gradient(), orc.gradient(), rtol=0, atol=CONTROL_ATOL, err_msg=tag + " gradient")
        else:
            orc.update(x, t)
            dev.update(x, t)
            chain.update(t, dev.get_gradient())
            assert_update_parity(dev, orc, tag)
        info = dev.update_info()
        assert info["finish_path"] == case.path, (tag, info)
        assert info["wait_timeouts"] == 0, (tag, info)
        _check_windows(case, dev, orc, chain, tag)
    on = (dev.get_optimal_rollout() == conf.control_min) | (dev.get_optimal_rollout() == conf.control_max)
    assert on.mean() < 0.5, case.name


@pytest.mark.parametrize("case", [c for c in SC.CASES if c.name != "colliding_times"],
                         ids=[c.name for c in SC.CASES if c.name != "colliding_times"])
def test_smoothing_case(case):
    _run(case)


def test_colliding_times():
    """Times near 2^47, where ulp(t) > dt: step times repeat, so sg_finish_kernel leaves its
    recurrence for the literal loop at w = 5.  The first update's shift count is ~1.4e16: every use
    of SampleParams::shift_by as an index (sample_device.hpp, fr_coop.hip, pm_fused.hip, kernels.hip)
    sits behind k < shifted with shifted = max(0, H - shift_by) = 0, and the engine narrows only
    min(shift_by, H)."""
    _run(SC.by_name("colliding_times"))
