"""The Savitzky-Golay finish's cases, as plain data shared by the host-only checks
(test_smoothing_cpu.py) and the GPU tests (test_gpu_smoothing.py).

launch_finish (kernels.hip) takes one of three kernels, and sg_finish_kernel one of two modes:
  finish_flat_kernel        no filter                                         finish_path 0
  sg_finish_kernel, mode 2  P_k summed ahead + the order-(w - 1) recurrence   finish_path 1
  sg_finish_kernel, mode 1  the literal loop in LDS: w - 1 > SGK_ZM, or some
                            lower_bound(t_k) != w + k                         finish_path 1
  finish_kernel             W = H + 2w + 1 > SGK_MAXW (or the LDS need)       finish_path 2
The mode cannot be observed from outside; `zm_edge` / `literal` and `nonuniform` / `colliding_times`
sit on either side of its rule by construction (w - 1 = SGK_ZM against SGK_ZM + 1; step times that
are distinct against step times that repeat).  H and w of the threshold cases are derived from the
two constants below, which test_smoothing_cpu.py holds against kernels.hip.

Every case: time step 0.01, S <= 32 rollouts.  "fr": FrankaRidgeback, the default objective, a
constant forecast, the huddled state; "pm": the point mass at rest in the origin.  Noise is injected
(seeded), as helpers.step_both does.  A time in `raises` goes backwards: that update must fail with
MPPI_ERR_SMOOTHING on every side and leave U* and the windows alone.
"""
from collections import namedtuple

SGK_MAXW = 384   # kernels.hip: the largest window sg_finish_kernel stages
SGK_ZM = 15      # kernels.hip: the recurrence's register slots (w - 1 <= SGK_ZM)
TIME_STEP = 0.01
FINISH_FLAT, FINISH_SG, FINISH_SG_GLOBAL = 0, 1, 2   # update_info()["finish_path"]

# E_cpu: the largest |U* - chain U*| and |uu - chain uu| between the oracle and the exact chain over
# every case here (test_smoothing_cpu.py::test_oracle_against_exact_chain measures and prints it):
# the spread between the oracle's left-to-right fp64 sums and the exactly rounded ones.
E_CPU = 3.2e-15   # measured 3.109e-15
# The device against the exact chain: one more association of the same sums (fma, four partial
# sums, P_k formed first), of the kind E_cpu measures; 16 covers the 15-deep feedback.  Times
# max(1, max |U*|) of the case.  Not tuned against the device.
FILTER_BAR_FACTOR = 16.0

Case = namedtuple("Case", "name model H w order times raises S keep seed path")

BIG = 2.0 ** 47   # ulp(2^47) = 1/32 > the time step: step times t + k dt repeat

CASES = [
    # mode 2 with unequal weights
    Case("nonuniform", "fr", 16, 5, 2, (0.0, 0.05, 0.10, 0.15), (), 24, 6, 101, FINISH_SG),
    # every trim case: a first update at t > 0, a repeated time (offset 0), a sub-step advance (no
    # shift, offset 1), a 7-step shift, a shift of exactly H, a jump far past the horizon
    Case("cubic_short", "fr", 8, 3, 3, (0.3, 0.3, 0.304, 0.37, 0.45, 5.0), (), 16, 4, 102, FINISH_SG),
    # w - 1 = SGK_ZM: mode 2 with all the recurrence's slots live
    Case("zm_edge", "fr", 24, SGK_ZM + 1, 3, (0.0, 0.05, 0.05, 0.073, 0.5), (), 20, 5, 103, FINISH_SG),
    # w - 1 = SGK_ZM + 1: mode 1
    Case("literal", "fr", 24, SGK_ZM + 2, 3, (0.0, 0.05, 0.05, 0.073, 0.5), (), 20, 5, 104, FINISH_SG),
    # W = 35 >> H = 2: the window is mostly the repeated tail
    Case("window_over_horizon", "fr", 2, 16, 2, (0.0, 0.01, 0.02, 0.05), (), 16, 4, 105, FINISH_SG),
    # C = 3: a 256-thread block whose fourth wave has no dimension
    Case("pm_mode2", "pm", 16, 4, 2, (0.0, 0.05, 0.10), (), 32, 8, 106, FINISH_SG),
    # W = SGK_MAXW: every slot of the rotation's register gather
    Case("maxw", "pm", SGK_MAXW - 2 * 2 - 1, 2, 2, (0.0, 0.05, 0.10), (), 32, 8, 107, FINISH_SG),
    # W = SGK_MAXW + 1: finish_kernel
    Case("fallback", "pm", SGK_MAXW - 2 * 2, 2, 2, (0.0, 0.05, 0.10), (), 32, 8, 108, FINISH_SG_GLOBAL),
    # 0.2 goes backwards and must raise; 0.352 then shifts by 0 steps, so the failed update's
    # gradient step, left in U*_shifted, carries over
    Case("back_in_time", "fr", 16, 4, 3, (0.3, 0.35, 0.2, 0.352, 0.4), (2,), 24, 6, 109, FINISH_SG),
    # ulp(t) > dt: step times repeat, lower_bound(t_k) != w + k: mode 1 at a small w; the first
    # update shifts by ~1.4e16 steps
    Case("colliding_times", "fr", 16, 5, 2, (BIG, BIG + 0.0625, BIG + 1.0), (), 24, 6, 110, FINISH_SG),
]

# the configurations every other smoothing run of the suite uses: order 1, where the weights are equal
UNIFORM = [(10, 1), (4, 1)]
# the cases whose weights the mutants are run on
MUTANT_CASES = ("nonuniform", "zm_edge", "literal")


def by_name(name):
    return next(c for c in CASES if c.name == name)


def horizon(H):
    """A horizon of H steps: H = ceil(horison / time_step); half a step short of H, since
    H * 0.01 / 0.01 rounds up for some H."""
    return (H - 0.5) * TIME_STEP


def expected_path(H, w, C):
    """launch_finish's rule."""
    if w <= 0:
        return FINISH_FLAT
    W = H + 2 * w + 1
    lds = (C * (2 * W + H) + 2 * w + 1) * 8
    return FINISH_SG if (W <= SGK_MAXW and C <= 16 and lds <= 65536) else FINISH_SG_GLOBAL


def parts(case):
    """(configuration, dynamics, cost, state) of a case."""
    import numpy as np

    import assistedmanipulation_amd as am

    if case.model == "fr":
        conf = am.frankaridgeback_configuration(rollouts=case.S, horison=horizon(case.H), keep_best_rollouts=case.keep,
                                                smoothing=am.Smoothing(case.w, case.order), threads=4)
        return conf, am.FrankaRidgebackDynamics(), am.AssistedManipulation(), am.huddled_state()
    conf = am.point_mass_configuration(rollouts=case.S, horison=horizon(case.H), keep_best_rollouts=case.keep)
    conf.smoothing = am.Smoothing(case.w, case.order)   # (point_mass_configuration itself has none)
    return conf, am.PointMassDynamics(), am.QuadraticCost(), np.zeros(6)


def oracle_for(case):
    """(configuration, OracleTrajectory, state, noise standard deviations)."""
    import numpy as np

    import assistedmanipulation_amd as am
    from oracle import oracle as O

    conf, dyn, cost, x = parts(case)
    cc, keep = conf.to_c()
    orc = O.OracleTrajectory(cc, dyn.descriptor(), cost.descriptor())
    assert orc.H == case.H
    if case.model == "fr":
        orc.set_forecast(am.constant_forecast(orc.H))
    return conf, orc, x, np.sqrt(np.diag(conf.covariance))


def chain_for(case, conf, mutant=None):
    from smoothing_reference import FilterChain

    C = len(conf.control_min)
    bound = bool(conf.control_bound)
    return FilterChain(case.H, C, case.w, case.order, conf.time_step, conf.gradient_step,
                       list(conf.control_min) if bound else None, list(conf.control_max) if bound else None, mutant=mutant)
