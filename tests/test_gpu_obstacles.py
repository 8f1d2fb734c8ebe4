"""Obstacle avoidance (mppi_set_obstacle_avoidance / mppi_set_obstacles) on the device against the
numpy composition of obstacle_reference.py: the obstacle term in every launch plan of the rollouts
(the x kernel with its relay and folded filter(), the four-wave and one-wave kernels, the separate
cost kernel), both objectives, the tank, the simulated wrench, the full table, the graph path,
sharding, the device object, the refusals and the C++ surface.

The pattern is test_gpu_link_positions.py's: three updates at time 0 from its three states with its
noise scaling, host-injected noise, U*_shifted the previous get_optimal_rollout(), helpers.py's bars.
The obstacle set changes between the updates (obstacle_sets.py): "clear", "breach", then empty.  The
reference keeps books on every clearance it evaluates, and each run asserts from them that nothing
sat within 1e-6 of the barrier's branch discontinuity and that set A stayed 0.02 m clear.

The objective's arm radii are 0.04 (obstacle_sets.ARM_RADIUS), so no self-collision pair saturates.
The rollout costs still reach 1e11 where the injected noise drives a joint or the workspace barrier
into saturation, so beside the bars on the costs every run checks the optimal rollout's obstacle
total against the reference's sum, relative to the term itself.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi
from assistedmanipulation_amd.trajectory import EngineError

import link_reference as LR
import obstacle_reference as OR
import obstacle_sets as SETS
import wrench_reference as WR
from helpers import COST_RTOL
from launch_shapes import TIME_STEP, by_name, horizon
from test_gpu_link_positions import SHAPES, _assert_bars, _hip, _noise_scale, _record, _set_env as _lp_env, _states

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-6      # least |v - bound| the reference may see
CLEAR_A = 0.02     # least v of set A


def _set_env(monkeypatch, req=0, sw=""):
    monkeypatch.delenv("MPPI_SIMULATED_WRENCH", raising=False)
    _lp_env(monkeypatch, req, sw)


def _abc():
    return [(SETS.set_a(), SETS.T_REF_A), (SETS.set_b(), 0.0), ([], 0.0)]


def _close(got, want, tag):
    assert abs(got - want) <= COST_RTOL * max(abs(want), 1.0), (tag, got, want)


def _check_books(term, j, H, tag):
    """The guards on the reference's own bookkeeping for the sets of _abc()."""
    if not term.obstacles:
        assert term.evaluated == 0
        return
    assert term.least_margin >= MARGIN, (tag, j, term.least_margin)
    if j == 0:
        assert term.least_v >= CLEAR_A and all(b == {"inverse"} for b in term.branches), (tag, term.least_v, term.branches)
    if j == 1:   # the sphere on the grasp frame: the end effector inside, PANDA_LINK7 outside, at every shape;
        assert term.branches[0] == {"inverse", "saturated"}, (tag, term.branches)
        if H >= 20:   # the flying sphere needs about 15 steps to reach PANDA_LINK5
            assert term.branches[1] == {"inverse", "saturated"}, (tag, term.branches)


def _handle(conf, cost, config=None, avoidance=True, wrench=None):
    dyn = am.FrankaRidgebackDynamics(link_positions=True, simulated_wrench=wrench)
    dev = am.Trajectory.create(conf, dyn, cost)
    assert dev is not None and dev.link_positions
    if avoidance:
        assert dev.obstacle_avoidance is None
        dev.set_obstacle_avoidance(config)
        assert dev.obstacle_avoidance == (config or am.ObstacleAvoidance())
    dev.set_noise_source(abi.MPPI_NOISE_HOST_INJECTED)
    return dyn, dev


def _run(name, cost, sets, monkeypatch, plans=True, config=None, books=True):
    """Three updates against the composition.  plans: the launch plan of every update is the shape's
    (launch_shapes.py) and nothing reads the optimal rollout before the end, so the filter() row is
    folded where the shape folds it; otherwise get_optimal_obstacle_cost() is read after every update."""
    _, S, H, keep, req, sw, first, pend = by_name(name)
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    table = am.constant_forecast(H)
    dyn, dev = _handle(conf, cost, config)
    assert dev.H == H and dev.R == S + 2
    dev.set_forecast(table)
    comp = OR.Composition(conf, dyn.model, cost, table, config)
    states, scale = _states(), _noise_scale(H)
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance)) * scale
    U = np.zeros((H, dev.C))
    prev = None
    for j, (x, (obstacles, t_ref)) in enumerate(zip(states, sets)):
        tag = "%s upd %d" % (name, j)
        dev.set_obstacles(obstacles, t_ref)
        got_set, got_time = dev.obstacles()
        assert len(got_set) == len(obstacles) and got_time == t_ref
        term = comp.set_obstacles(obstacles, t_ref)
        dev.inject_noise(rng.standard_normal((dev.noise_draws(0.0), dev.C)) * sd)
        dev.update(x, 0.0)
        info = dev.update_info()
        assert info["wait_timeouts"] == 0 and info["cooperative"] == 1, (tag, info)
        if plans:
            want = first if j == 0 else pend
            assert info["folded_filter"] == want[5] and info["objective_in_launch"] == want[6], (tag, info)
        if info["folded_filter"]:   # the previous update's filter() row: its own set, before any optimal-cost read
            comp.term = prev
            ref = comp.rollout(states[j - 1], U)[0]
            comp.term = term
            _close(dev.debug_folded_cost(), ref, tag + " folded filter()")
        eps = dev.noise()
        J = comp.costs(x, U, eps)
        w, g, Un = LR.mppi_update(conf, J, eps, U)
        _assert_bars(tag, dev.costs(), J, dev.get_weights(), w, dev.get_optimal_rollout(), Un, H)
        U = dev.get_optimal_rollout()   # U*_prev of the next update (nothing shifts at one time)
        if books:
            _check_books(term, j, H, tag)
        if not plans:
            ref, _, ob = comp.rollout(x, U)
            _close(dev.get_optimal_obstacle_cost(), ob.sum(), tag + " optimal obstacle cost")
            _close(dev.get_optimal_total_cost(), ref, tag + " optimal total")
        prev = term
    ref, sc, ob = comp.rollout(states[len(sets) - 1], U)
    _close(dev.get_optimal_total_cost(), ref, name + " optimal total")
    _close(dev.get_optimal_obstacle_cost(), ob.sum(), name + " optimal obstacle cost")
    if cost.descriptor().kind == abi.MPPI_COST_ASSISTED_MANIPULATION:   # the seven terms keep their meaning
        _close(dev.get_optimal_terms()[1], sc.sum(), name + " self-collision total")
    return dev, comp


# ---- 1. parity against the composition, every launch plan ---------------------------------------

@pytest.mark.parametrize("name", SHAPES)
def test_update_against_the_composition(name, monkeypatch):
    _run(name, SETS.objective(), _abc(), monkeypatch)


def test_optimal_obstacle_cost_after_every_update(monkeypatch):
    """The same three sets with the optimal rollout read after each update (so filter() runs by
    itself): the obstacle total of a non-empty set against the reference's sum."""
    dev, comp = _run("r19_h33", SETS.objective(), _abc(), monkeypatch, plans=False)
    assert [len(t.obstacles) for t in comp.history] == [3, 2, 0]


# ---- 2. other objectives and modes --------------------------------------------------------------

def test_track_point(monkeypatch):
    """TrackPoint with its default switches (no self-collision term of its own): the link FK runs for
    the obstacles alone."""
    _run("r19_h33", SETS.objective("track_point"), _abc(), monkeypatch)


def test_energy_tank(monkeypatch):
    _run("r19_h33", SETS.objective(energy=True), _abc(), monkeypatch)


def test_track_point_with_its_self_collision_term(monkeypatch):
    """TrackPoint's own self-collision term and the obstacle term on one link FK (the barrier's
    maximum lowered: obstacle_sets.objective says why), the optimal rollout read after every update."""
    _run("r19_h33", SETS.objective("track_point", tp_self=True), _abc(), monkeypatch, plans=False)


def test_simulated_wrench_forecast(monkeypatch):
    """The pushed robot (simulated_wrench="forecast") with the obstacle term, against the wrench
    composition plus the term at that class's states: test_gpu_simulated_wrench.py's update pattern
    (three times, so U* shifts and t0 - t_ref changes) and its bars."""
    from test_gpu_simulated_wrench import TIMES, _assert_update, _state
    _, S, H, keep, req, sw, _, _ = by_name("r19_h33")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = SETS.objective()
    table = WR.forecast_table(H)
    dyn, dev = _handle(conf, cost, wrench="forecast")
    dev.set_forecast(table)
    ref = OR.WrenchComposition(conf, dyn.model, cost, "forecast", table)
    sd = np.sqrt(np.diag(conf.covariance))
    rng, shift, dt = np.random.default_rng(11), WR.Shift(), dev.get_time_step()
    prev = None
    for j, (t, (obstacles, t_ref)) in enumerate(zip(TIMES, _abc())):
        tag = "wrench upd %d" % j
        x0 = _state(j)
        U_prev = dev.get_optimal_rollout()
        U_shift = WR.shifted(U_prev, shift(t, dt))
        dev.set_obstacles(obstacles, t_ref)
        term = ref.set_obstacles(obstacles, t_ref)
        dev.inject_noise(rng.standard_normal((dev.noise_draws(t), 12)) * sd)
        dev.update(x0, t)
        info = dev.update_info()
        assert info["wait_timeouts"] == 0, (tag, info)
        if info["folded_filter"]:
            ref.term = prev[0]
            want = ref.rollout(prev[1], U_prev, prev[2])[0]
            ref.term = term
            _close(dev.debug_folded_cost(), want, tag + " folded filter()")
        eps = dev.noise()
        J = ref.costs(x0, U_shift, eps, t)
        w, g, Un = LR.mppi_update(conf, J, eps, U_shift)
        _assert_update(tag, dev, J, w, g, Un, H)
        if term.obstacles:
            assert term.least_margin >= MARGIN, (tag, term.least_margin)
        prev = (term, x0, t)
    want, _, ob = ref.rollout(x0, dev.get_optimal_rollout(), TIMES[-1])
    _close(dev.get_optimal_total_cost(), want, "wrench optimal total")
    _close(dev.get_optimal_obstacle_cost(), ob.sum(), "wrench optimal obstacle cost")


# ---- 3. capacity ---------------------------------------------------------------------------------

def test_sixteen_obstacles(monkeypatch):
    """The full table, mixed kinds and masks, with a configuration of its own (a nonzero bound and
    point radii that differ), given at three reference times."""
    config = am.ObstacleAvoidance(limit=(0.01, 2.0, 1e8), radii=(0.7, 0.11, 0.12, 0.13, 0.1, 0.09, 0.08, 0.07, 0.06))
    sets = [(SETS.set_16(), 0.0), (SETS.set_16(), -0.5), (SETS.set_16()[::-1], 0.25)]
    dev, comp = _run("r19_h33", SETS.objective(), sets, monkeypatch, plans=False, config=config, books=False)
    for term in comp.history:
        assert term.least_margin >= MARGIN and all(term.branches), (term.least_margin, term.branches)


def test_empty_set_equals_the_kinematic_mode(monkeypatch):
    """count = 0 on an enabled handle against a kinematic-mode handle that never enabled avoidance, the
    same injected noise, at the bars."""
    _, S, H, keep, req, sw, _, _ = by_name("r19_h33")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = SETS.objective()
    on, off = _handle(conf, cost)[1], _handle(conf, cost, avoidance=False)[1]
    assert off.obstacle_avoidance is None
    on.set_obstacles([], 3.0)
    rng = np.random.default_rng(3)
    sd = np.sqrt(np.diag(conf.covariance))
    for j, x in enumerate(_states()):
        eps = rng.standard_normal((on.noise_draws(0.0), on.C)) * sd
        for t in (on, off):
            t.set_forecast(am.constant_forecast(H))
            t.inject_noise(eps)
            t.update(x, 0.0)
            assert t.update_info()["wait_timeouts"] == 0
        _assert_bars("empty set upd %d" % j, on.costs(), off.costs(), on.get_weights(), off.get_weights(), on.get_optimal_rollout(),
                     off.get_optimal_rollout(), H)
    _close(on.get_optimal_total_cost(), off.get_optimal_total_cost(), "empty set optimal total")
    assert on.get_optimal_obstacle_cost() == 0.0


# ---- 4. paths ------------------------------------------------------------------------------------

def test_in_launch_objective_against_the_cost_kernel(monkeypatch):
    """The same inputs through the launch's own objective and through fr_step_cost_kernel
    (MPPI_COSTS_IN_LAUNCH=0), r147_h64: at the bars; whether they agree bit for bit is printed."""
    _, S, H, keep, req, sw, _, _ = by_name("r147_h64")
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = SETS.objective()
    _set_env(monkeypatch, req, "")
    a = _handle(conf, cost)[1]
    _set_env(monkeypatch, req, "c")
    b = _handle(conf, cost)[1]
    rng = np.random.default_rng(4)
    sd = np.sqrt(np.diag(conf.covariance)) * _noise_scale(H)
    same = True
    for j, (x, (obstacles, t_ref)) in enumerate(zip(_states(), _abc())):
        eps = rng.standard_normal((a.noise_draws(0.0), a.C)) * sd
        for t in (a, b):
            t.set_forecast(am.constant_forecast(H))
            t.set_obstacles(obstacles, t_ref)
            t.inject_noise(eps)
            t.update(x, 0.0)
            assert t.update_info()["wait_timeouts"] == 0
        assert a.update_info()["objective_in_launch"] == 1 and b.update_info()["objective_in_launch"] == 0
        same = same and np.array_equal(a.costs(), b.costs())
        _assert_bars("in-launch vs cost kernel upd %d" % j, a.costs(), b.costs(), a.get_weights(), b.get_weights(),
                     a.get_optimal_rollout(), b.get_optimal_rollout(), H)
    print("in-launch objective and cost kernel bit for bit: %s" % same)


def _philox(conf, graph=0, avoidance=True):
    t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=True), am.AssistedManipulation())
    assert t is not None
    if avoidance:
        t.set_obstacle_avoidance()
    t.set_graph(graph)
    t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
    t.set_forecast(am.constant_forecast(t.H))
    return t


GRAPH_SETS = [(SETS.set_a(), SETS.T_REF_A), (SETS.set_b(), 0.0), (SETS.set_a()[:2], 0.06), (SETS.set_b(), 0.1)]


def test_graph_path(monkeypatch):
    """test_graph_path_kinematic's structure with the set replaced and the time advancing between the
    replays: the graph's rollout nodes see the current set and time (the eager launches' bits), and
    all three updates after the first are graph updates."""
    _set_env(monkeypatch, 0, "")
    conf = am.frankaridgeback_configuration(rollouts=1000, horison=0.64, keep_best_rollouts=20, threads=8)
    out = {}
    for graph in (0, 1):
        t = _philox(conf, graph)
        x = am.huddled_state()
        rec = []
        for j, tm in enumerate([0.0, 0.05, 0.07, 0.12]):
            if j == 2:
                x = x.copy()
                x[12 + 4] = 0.3
            t.set_obstacles(*GRAPH_SETS[j])
            t.update(x, tm)
            assert t.update_info()["wait_timeouts"] == 0
            rec.append(_record(t))
        out[graph] = (rec, t.graph_updates(), t.get_optimal_total_cost(), t.get_optimal_obstacle_cost())
    assert out[0][1] == 0 and out[1][1] == 3, (out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3] and out[0][3] > 0.0
    for j, (a, b) in enumerate(zip(out[0][0], out[1][0])):
        for what, u, v in zip(("noise", "costs", "optimal", "weights"), a, b):
            np.testing.assert_array_equal(u, v, err_msg="update %d %s" % (j, what))
    # the term is live, and the time matters: the same sets a second late give other costs
    plain = _philox(conf, 0, avoidance=False)
    plain.update(am.huddled_state(), 0.0)
    assert not np.array_equal(plain.costs(), out[0][0][0][1])
    late = _philox(conf, 0)
    late.set_obstacles(GRAPH_SETS[0][0], GRAPH_SETS[0][1] - 1.0)
    late.update(am.huddled_state(), 0.0)
    assert not np.array_equal(late.costs(), out[0][0][0][1])


def test_two_shards_equal_one_handle(monkeypatch):
    """test_two_shards_kinematic_equal_one_handle's structure and bars with avoidance on: every rank
    enables it and sets the same set."""
    _, S, H, keep, req, sw, _, _ = by_name("r147_h20")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    world = 2
    single, shards = _philox(conf), [_philox(conf) for _ in range(world)]
    for r, sh in enumerate(shards):
        sh.set_shard(world, r)
    hip = _hip()
    R, HC = single.R, single.H * single.C
    x = am.huddled_state()

    def allreduce(ptrs, n):
        bufs = [np.zeros(n) for _ in ptrs]
        for p, b in zip(ptrs, bufs):
            assert hip.hipMemcpy(b.ctypes.data, p, n * 8, 2) == 0   # D2H
        s = bufs[0].copy()
        for b in bufs[1:]:
            s += b
        for p in ptrs:
            assert hip.hipMemcpy(p, s.ctypes.data, n * 8, 1) == 0   # H2D

    for j in range(3):
        t = 0.05 * j
        for h in [single] + shards:
            h.set_obstacles(*GRAPH_SETS[j])
        single.update(x, t)
        for sh in shards:
            sh.update_phase1(x, t)
        hip.hipDeviceSynchronize()
        allreduce([sh.device_costs_ptr() for sh in shards], R + 1)   # + slot R: wait timeouts
        for sh in shards:
            sh.update_phase2()
        hip.hipDeviceSynchronize()
        allreduce([sh.device_gradient_ptr() for sh in shards], HC)
        for sh in shards:
            sh.update_phase3(t)
        cu = single.costs()
        delta = np.nanmax(cu) - np.nanmin(cu)
        assert single.update_info()["wait_timeouts"] == 0
        for sh in shards:
            cs = sh.costs()
            if j == 0:
                np.testing.assert_array_equal(cs, cu)
            assert np.all(np.abs(cs - cu) <= 1e-11 * (delta + np.abs(cu)))
            assert np.max(np.abs(sh.get_optimal_rollout() - single.get_optimal_rollout())) <= 1e-12
            assert np.max(np.abs(sh.get_weights() - single.get_weights())) <= 3e-15
            assert sh.argmin() == single.argmin() and sh.update_info()["wait_timeouts"] == 0


def test_device_object_obstacle_cost(monkeypatch):
    """PinocchioDynamicsObject.obstacle_cost after set_state and after a step (the cached positions
    lag the state by that step) against the numpy term, 1e-12 relative."""
    monkeypatch.delenv("MPPI_LINK_POSITIONS", raising=False)
    model = am.FrankaRidgebackDynamics().model
    x = am.huddled_state()
    obj = am.PinocchioDynamicsObject.create(x, link_positions=True)
    config = am.ObstacleAvoidance(limit=(0.01, 2.0, 1e8), radii=(0.7, 0.11, 0.12, 0.13, 0.1, 0.09, 0.08, 0.07, 0.06))
    cases = [(None, SETS.set_a(), 0.07), (None, SETS.set_b(), 0.0), (None, SETS.set_b(), 0.2), (config, SETS.set_16(), 0.5),
             (config, SETS.set_16(), -0.5), (None, [], 1.0)]

    def check(q, tag):
        for conf, obstacles, elapsed in cases:
            want = OR.Term(conf or am.ObstacleAvoidance(), obstacles, 0.0).at(OR.robot_points(model, q), elapsed)
            got = obj.obstacle_cost(conf, obstacles, elapsed)
            assert abs(got - want) <= 1e-12 * max(abs(want), 1.0), (tag, len(obstacles), elapsed, got, want)

    obj.set_state(x, 0.0)
    check(x[:12], "set_state")
    u = np.array([0.2, -0.1, 0.3, 5.0, -4.0, 3.0, -2.0, 1.0, 2.0, -3.0, 0.0, 0.0])
    xn = obj.step(u, 0.01)
    assert np.abs(xn[:12] - x[:12]).max() > 1e-4
    check(x[:12], "after a step")   # the calculate() of the step ran at the old configuration
    x2 = xn.copy()
    x2[3:10] += 0.2
    obj.set_state(x2, 0.0)
    check(x2[:12], "moved")
    zero = am.PinocchioDynamicsObject.create(x)
    with pytest.raises(EngineError) as e:
        zero.obstacle_cost(None, SETS.set_a(), 0.0)
    assert e.value.status == abi.MPPI_ERR_INVALID and "kinematic" in str(e.value)
    with pytest.raises(EngineError) as e:
        obj.obstacle_cost(None, [am.SphereObstacle((0, 0, 0), -1.0)], 0.0)
    assert e.value.status == abi.MPPI_ERR_INVALID


# ---- 5. validation -------------------------------------------------------------------------------

def _invalid(fn, status=abi.MPPI_ERR_INVALID, word=None):
    with pytest.raises(EngineError) as e:
        fn()
    assert e.value.status == status, (e.value.status, str(e.value))
    if word:
        assert word in str(e.value), str(e.value)


def test_validation(monkeypatch):
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=17, horison=0.05, keep_best_rollouts=5)
    mk = lambda lp: am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=lp), am.AssistedManipulation())
    ok = am.SphereObstacle((2, 2, 1), 0.1)

    # a handle that never enables it
    plain = mk(True)
    assert plain.obstacle_avoidance is None
    _invalid(lambda: plain.set_obstacles([ok], 0.0), word="not enabled")
    _invalid(lambda: plain.obstacles(), word="not enabled")
    _invalid(lambda: plain.get_optimal_obstacle_cost(), abi.MPPI_ERR_UNSUPPORTED)
    # enabling in the zero link mode, and after the first update
    _invalid(lambda: mk(False).set_obstacle_avoidance(), word="kinematic")
    _invalid(lambda: mk(None).set_obstacle_avoidance(), word="kinematic")
    plain.update(am.huddled_state(), 0.0)
    _invalid(lambda: plain.set_obstacle_avoidance(), word="before the first update")
    # a point-mass handle
    pm = am.Trajectory.create(am.point_mass_configuration(rollouts=64), am.PointMassDynamics(), am.QuadraticCost())
    _invalid(lambda: pm.set_obstacle_avoidance(), abi.MPPI_ERR_UNSUPPORTED)
    assert pm.obstacle_avoidance is None
    # the configuration
    t = mk(True)
    for bad in (am.ObstacleAvoidance(limit=(np.nan, 1.0, 1e10)), am.ObstacleAvoidance(limit=(0.0, np.inf, 1e10)),
                am.ObstacleAvoidance(limit=(0.0, 1.0, np.inf)), am.ObstacleAvoidance(radii=(0.75,) + (0.1,) * 7 + (-0.1,)),
                am.ObstacleAvoidance(radii=(np.nan,) + (0.1,) * 8)):
        _invalid(lambda: t.set_obstacle_avoidance(bad))
        assert t.obstacle_avoidance is None
    t.set_obstacle_avoidance()
    _invalid(lambda: t.set_link_positions(abi.MPPI_LINK_POSITIONS_ZERO), word="obstacle avoidance")
    assert t.obstacles() == ([], 0.0) and t.get_optimal_obstacle_cost() == 0.0
    # the set
    t.set_obstacles([ok] * 16, 1.5)
    assert len(t.obstacles()[0]) == 16 and t.obstacles()[1] == 1.5
    _invalid(lambda: t.set_obstacles([ok] * 17, 0.0), word="count")
    L = am._lib.load()
    arr = (abi.mppi_obstacle * 16)()
    assert L.mppi_set_obstacles(t._h, arr, -1, 0.0) == abi.MPPI_ERR_INVALID
    unknown = am.SphereObstacle((2, 2, 1), 0.1)
    unknown.kind = 2
    _invalid(lambda: t.set_obstacles([unknown], 0.0), word="kind")
    _invalid(lambda: t.set_obstacles([am.SphereObstacle((2, 2, 1), 0.1, mask=0x200)], 0.0), word="mask")
    _invalid(lambda: t.set_obstacles([am.SphereObstacle((2, np.nan, 1), 0.1)], 0.0), word="finite")
    _invalid(lambda: t.set_obstacles([am.SphereObstacle((2, 2, 1), 0.1, velocity=(np.inf, 0, 0))], 0.0), word="finite")
    _invalid(lambda: t.set_obstacles([ok], np.nan), word="finite")
    _invalid(lambda: t.set_obstacles([am.SphereObstacle((2, 2, 1), -0.1)], 0.0), word="radius")
    _invalid(lambda: t.set_obstacles([am.HalfSpaceObstacle((0, 0, 0), (0, 0, 1.0 + 1e-8))], 0.0), word="unit")
    _invalid(lambda: t.set_obstacles([am.HalfSpaceObstacle((0, 0, 0), (0, 0, 0))], 0.0), word="unit")
    t.set_obstacles([am.HalfSpaceObstacle((0, 0, 0), (0, 0, 1.0 + 5e-10)), am.SphereObstacle((2, 2, 1), 0.0, mask=0)], 0.0)
    assert len(t.obstacles()[0]) == 2   # a refused call left the previous set in place until this one
    # a set may be replaced after updates have run; enabling may not
    t.update(am.huddled_state(), 0.0)
    t.set_obstacles([ok], 0.0)
    t.update(am.huddled_state(), 0.01)
    assert t.update_info()["wait_timeouts"] == 0
    _invalid(lambda: t.set_obstacle_avoidance(), word="before the first update")


# ---- 6. the C++ surface --------------------------------------------------------------------------

def test_cpp_obstacle_surface_on_the_device(monkeypatch):
    _set_env(monkeypatch)
    cpp = os.path.join(REPO, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "obstacles.mk"])
    out = subprocess.check_output([os.path.join(cpp, "build", "obstacles"), "gpu"], timeout=300).decode()
    lines = [json.loads(l) for l in out.strip().split("\n")]
    assert lines[0] == {"cpu": "ok"}
    assert lines[1] == {"zero_mode_enabled": False, "reports": False, "set_obstacles": False}
    assert lines[2] == {"enabled": True, "ee_radius": 0.12, "empty": 0}
    assert lines[3] == {"count": 2, "time": -0.25, "kind1": abi.MPPI_OBSTACLE_HALF_SPACE, "vx0": -0.5}
    assert lines[4]["with_set"] > 0.0 and lines[4]["cleared"] == 0.0 and lines[4]["late_enable"] is False
    # the object's cost: the same program's inputs through the Python object
    config = am.ObstacleAvoidance(radii=(0.75,) + (0.1,) * 7 + (0.12,))
    obstacles = [am.SphereObstacle((2.2, 0.9, 1.0), 0.3, velocity=(-0.5, 0, 0)), am.HalfSpaceObstacle((0, 0, -0.3), (0, 0, 1), mask=0x1FE)]
    d = am.PinocchioDynamicsObject.create(am.huddled_state(), link_positions=True)
    d.set_state(am.huddled_state(), 0.0)
    d.step(np.array([(5.0 - i) if 3 <= i < 10 else 0.1 for i in range(12)]), 0.01)
    assert lines[5]["same"] and lines[5]["object_cost"] == d.obstacle_cost(config, obstacles, 0.3)
