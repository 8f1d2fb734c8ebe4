"""Target tracking (mppi_set_target_tracking / mppi_set_target_path) on the device against the numpy
composition of target_reference.py: the timed pose target in every launch plan of the rollouts (the x
kernel with its relay and folded filter(), the four-wave and one-wave kernels, the separate cost
kernel), the path replaced between updates, time advancing, bit-identity with a plain TrackPoint
handle, the zero link mode, the tables' coexistence with the capsule term and the simulated wrench,
TrackPoint's own self-collision term, the graph path, sharding, the device object, the refusals and
the C++ surface.

The pattern is test_gpu_obstacles.py's: host-injected noise, U*_shifted the previous
get_optimal_rollout() (shifted on the host where the time advances), helpers.py's bars.  The
reference keeps books on the sampling regime of every step; the placement of the first path is
asserted from them (and on the CPU, test_target_path_cpu.py).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi

import capsule_reference as CR
import capsule_sets as CS
import link_reference as LR
import state_space as SS
import target_paths as TP
import target_reference as TR
import wrench_reference as WR
from helpers import COST_RTOL, WEIGHT_ATOL
from launch_shapes import TIME_STEP, by_name, horizon
from test_gpu_link_positions import _assert_bars, _hip, _noise_scale, _record, _states
from test_gpu_obstacles import _close, _invalid, _set_env

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["r147_h33", "r48_h33", "r10_h33", "r20_h33", "r19_h1", "r19_h129"]
POSE = am.TargetTracking(10.0, True)
# the times of the advancing tests and the shifts they assume: int((t_j - t_{j-1}) / dt)
TIMES, SHIFTS = (0.0, 0.055, 0.128), (0, 5, 7)


def _objective(self_collision=True):
    """TrackPoint at TP.POINT.  The parity tests carry its self-collision term with the barrier's
    maximum lowered to 100 (obstacle_sets.objective says why it cannot stay 1e10): 2000 a step.  Without
    it the cheapest rollouts' J is the two smooth target terms alone, about 8e2 over 33 steps, and
    helpers.py's COST_RTOL, which is relative to J, then measures the rollout kernel's dynamics and not
    the objective: device and oracle joint positions differ by 3e-12 to 5e-12 after 33 steps at the
    full noise and by 1.4e-11 after 64 (test_gpu_simulated_wrench.py MEASURED), so the grasp frame's
    angle and position by about 1e-11 rad and m at 33 steps and ten times that at 129; the terms'
    slopes, 2 w sin(theta) = 20 and 200 d = 30 a step, turn that into 1.6e-8 over 33 steps and 3e-7
    over 129.  Measured on an MI355X: 1.0e-11 of J = 8e2 at r147_h33 without the term, and with a
    maximum of 10 (J = 2.6e4) 1.2e-11 at r19_h129 without a path, which is the plain TrackPoint
    objective.  A tenth of COST_RTOL at the longest horizon needs J >= 3e5: 2000 a step over 129.
    The tests that compare device with device keep the term off."""
    cost = am.TrackPoint(point=TP.POINT)
    if self_collision:
        cost.configuration.enable_self_collision_avoidance = 1
        cost.configuration.self_collision_limit.maximum_cost = 100.0
        for i in range(1, 8):
            cost.configuration.self_collision_radii[i] = 0.04
    return cost


def _handle(conf, cost, tracking=POSE, links=True, wrench=None, enable=True):
    dyn = am.FrankaRidgebackDynamics(link_positions=links, simulated_wrench=wrench)
    dev = am.Trajectory.create(conf, dyn, cost)
    assert dev is not None and bool(dev.link_positions) == bool(links)
    if enable:
        assert dev.target_tracking is None
        dev.set_target_tracking(tracking)
        assert dev.target_tracking == (tracking or am.TargetTracking())
        assert dev.target_path() is None
    dev.set_noise_source(abi.MPPI_NOISE_HOST_INJECTED)
    return dyn, dev


def _set_path(dev, comp, path):
    dev.set_target_path(path)
    comp.set_path(path)
    back = dev.target_path()
    if path is None:
        assert back is None
        return
    assert np.array_equal(back.times, path.times) and np.array_equal(back.positions, path.positions)
    if path.has_orientation:   # stored as the host class stores them: normalised, sign-fixed
        np.testing.assert_allclose(back.orientations, path.orientations, rtol=0, atol=2e-16)
        assert np.all(np.sum(back.orientations[1:] * back.orientations[:-1], axis=1) >= 0.0)


def _run(name, monkeypatch, paths, cost=None, tracking=POSE, links=True, plans=True, times=(0.0, 0.0, 0.0)):
    """Three updates against the composition, the path replaced before each.  plans: the launch plan
    of every update is the shape's and nothing reads the optimal rollout before the end, so the
    filter() row is folded where the shape folds it (and compared against the previous update's path);
    otherwise get_optimal_target_cost() is read after every update."""
    _, S, H, keep, req, sw, first, pend = by_name(name)
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = cost or _objective()
    dyn, dev = _handle(conf, cost, tracking, links)
    assert dev.H == H and dev.R == S + 2
    comp = TR.Composition(conf, dyn.model, cost, tracking, "kinematic" if links else "zero")
    states, scale = _states(), _noise_scale(H)
    rng, shift, dt = np.random.default_rng(11), WR.Shift(), dev.get_time_step()
    sd = np.sqrt(np.diag(conf.covariance)) * scale
    prev = None
    for j, (x, path, t) in enumerate(zip(states, paths, times)):
        tag = "%s upd %d" % (name, j)
        U_prev = dev.get_optimal_rollout()
        n = shift(t, dt)
        if times == TIMES:
            assert n == SHIFTS[j] == (int((t - TIMES[j - 1]) / dt) if j else 0), (tag, n)
        U = WR.shifted(U_prev, n)
        _set_path(dev, comp, path)
        dev.inject_noise(rng.standard_normal((dev.noise_draws(t), dev.C)) * sd)
        dev.update(x, t)
        info = dev.update_info()
        assert info["wait_timeouts"] == 0 and info["cooperative"] == 1, (tag, info)
        if plans:
            want = first if j == 0 else pend
            assert info["folded_filter"] == want[5] and info["objective_in_launch"] == want[6], (tag, info)
        if info["folded_filter"]:   # the previous update's filter() row: its own path and time, before any optimal-cost read
            comp.set_path(prev[0])
            ref = comp.rollout(prev[1], U_prev, prev[2])[0]
            comp.set_path(path)
            _close(dev.debug_folded_cost(), ref, tag + " folded filter()")
        eps = dev.noise()
        J = comp.costs(x, U, eps, t)
        w, g, Un = LR.mppi_update(conf, J, eps, U)
        _assert_bars(tag, dev.costs(), J, dev.get_weights(), w, dev.get_optimal_rollout(), Un, H)
        books = comp.targets.books
        if path is None:
            assert books["none"] == H * dev.R and books["inside"] == 0, (tag, books)
        elif path.times.tolist() == list(TP.A_TIMES) and t == 0.0 and H >= 33:
            # one horizon holds steps before the first waypoint, in every segment, and past the last
            assert books["before"] and books["after"] and books["segments"] == {0, 1, 2} and not books["none"], (tag, books)
        if not plans:
            ref, pos, ori = comp.rollout(x, dev.get_optimal_rollout(), t)
            got = dev.get_optimal_target_cost()
            _close(got[0], pos.sum(), tag + " optimal position total")
            _close(got[1], ori.sum(), tag + " optimal orientation total")
            assert (ori.sum() > 0.0) == (path is not None and path.has_orientation and tracking.track_orientation), (tag, ori.sum())
            _close(dev.get_optimal_total_cost(), ref, tag + " optimal total")
        prev = (path, x, t)
    ref, pos, ori = comp.rollout(prev[1], dev.get_optimal_rollout(), prev[2])
    _close(dev.get_optimal_total_cost(), ref, name + " optimal total")
    got = dev.get_optimal_target_cost()
    _close(got[0], pos.sum(), name + " optimal position total")
    _close(got[1], ori.sum(), name + " optimal orientation total")
    return dev, comp


# ---- 1. parity against the composition, every launch plan ---------------------------------------

@pytest.mark.parametrize("name", SHAPES)
def test_update_against_the_composition(name, monkeypatch):
    """Position and orientation, then another path, then none."""
    _run(name, monkeypatch, [TP.path_a(), TP.path_b(), None])


# ---- 2. time advances ----------------------------------------------------------------------------

def test_time_advances_with_the_path_kept(monkeypatch):
    """Updates at three increasing times with one path: the targets move along it with the update's
    time, U* shifts on the host, and the read-out matches the reference's two sums after every update."""
    path = TP.path_c()
    _run("r19_h33", monkeypatch, [path, path, path], plans=False, times=TIMES)


# ---- 3. bit-identity -------------------------------------------------------------------------------

@pytest.mark.parametrize("links", [False, True])
def test_constant_target_is_bit_identical_to_plain_track_point(links, monkeypatch):
    """A tracking handle with a one-waypoint path at the objective's point, and one with no path,
    against a plain TrackPoint handle: the same noise, the times advancing; costs, weights, gradient,
    U* and optimal cost bit for bit.  (links: the kinematic mode with orientation tracking on - the
    targets carry no orientation, so the term contributes nothing.)"""
    _, S, H, keep, req, sw, _, _ = by_name("r147_h33")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    tracking = POSE if links else am.TargetTracking()
    plain = _handle(conf, _objective(False), links=links, enable=False)[1]
    one = _handle(conf, _objective(False), tracking, links)[1]
    none = _handle(conf, _objective(False), tracking, links)[1]
    assert plain.target_tracking is None
    one.set_target_path(TP.constant_path())
    rng = np.random.default_rng(3)
    sd = np.sqrt(np.diag(conf.covariance))
    for j, (x, t) in enumerate(zip(_states(), TIMES)):
        eps = rng.standard_normal((plain.noise_draws(t), plain.C)) * sd
        for h in (plain, one, none):
            assert h.noise_draws(t) == len(eps)
            h.inject_noise(eps)
            h.update(x, t)
            assert h.update_info()["wait_timeouts"] == 0
        for h, what in ((one, "constant path"), (none, "no path")):
            tag = "%s upd %d " % (what, j)
            np.testing.assert_array_equal(h.costs(), plain.costs(), err_msg=tag + "costs")
            np.testing.assert_array_equal(h.get_weights(), plain.get_weights(), err_msg=tag + "weights")
            np.testing.assert_array_equal(h.get_gradient(), plain.get_gradient(), err_msg=tag + "gradient")
            np.testing.assert_array_equal(h.get_optimal_rollout(), plain.get_optimal_rollout(), err_msg=tag + "U*")
    for h in (one, none):
        assert h.get_optimal_total_cost() == plain.get_optimal_total_cost()
        assert h.get_optimal_target_cost()[1] == 0.0 and h.get_optimal_target_cost()[0] > 0.0
    assert one.get_optimal_target_cost() == none.get_optimal_target_cost()


# ---- 4. the zero link mode -------------------------------------------------------------------------

def test_position_only_in_the_zero_link_mode(monkeypatch):
    """Position tracking needs no link positions; orientation tracking is refused there."""
    dev, _ = _run("r19_h33", monkeypatch, [TP.path_a(), TP.path_b(False), None], tracking=am.TargetTracking(), links=False)
    conf = am.frankaridgeback_configuration(rollouts=17, horison=0.05, keep_best_rollouts=5)
    zero = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(), _objective())
    _invalid(lambda: zero.set_target_tracking(POSE), word="kinematic")
    assert zero.target_tracking is None
    zero.set_target_tracking()
    assert zero.target_tracking == am.TargetTracking()


# ---- 5. together with the capsule term and the simulated wrench ------------------------------------

def test_with_capsule_avoidance_and_the_simulated_wrench(monkeypatch):
    """r19_h33 with capsule obstacle avoidance and the pushed robot (simulated_wrench="state"): the
    targets in the step constants, the wrench rows and the obstacle table of one update side by side,
    alternating together.  The sets and the paths change between the updates, the time advances."""
    from test_gpu_simulated_wrench import _assert_update, _state
    _, S, H, keep, req, sw, _, _ = by_name("r19_h33")
    _set_env(monkeypatch, req, sw)
    monkeypatch.delenv("MPPI_SIMULATED_WRENCH", raising=False)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = _objective()
    dyn, dev = _handle(conf, cost, POSE, True, wrench="state")
    dev.set_obstacle_avoidance()
    dev.set_obstacle_capsules(CS.capsules())
    ref = TR.WrenchObstacleComposition(conf, dyn.model, cost, "state", POSE)
    sd = np.sqrt(np.diag(conf.covariance))
    rng, shift, dt = np.random.default_rng(11), WR.Shift(), dev.get_time_step()
    prev = None
    for j, (t, (obstacles, t_ref), path) in enumerate(zip(TIMES, CS.cde(), [TP.path_c(), TP.path_a(), None])):
        tag = "combined upd %d" % j
        x0 = _state(j)
        U_prev = dev.get_optimal_rollout()
        U_shift = WR.shifted(U_prev, shift(t, dt))
        dev.set_obstacles(obstacles, t_ref)
        term = CR.Term(am.ObstacleAvoidance(), CS.capsules(), obstacles, t_ref)
        _set_path(dev, ref, path)
        ref.term = term
        dev.inject_noise(rng.standard_normal((dev.noise_draws(t), 12)) * sd)
        dev.update(x0, t)
        info = dev.update_info()
        assert info["wait_timeouts"] == 0, (tag, info)
        if info["folded_filter"]:
            ref.term = prev[0]
            ref.set_path(prev[3])
            want = ref.rollout(prev[1], U_prev, prev[2])[0]
            ref.term = term
            ref.set_path(path)
            _close(dev.debug_folded_cost(), want, tag + " folded filter()")
        eps = dev.noise()
        J = ref.costs(x0, U_shift, eps, t)
        w, g, Un = LR.mppi_update(conf, J, eps, U_shift)
        _assert_update(tag, dev, J, w, g, Un, H)
        prev = (term, x0, t, path)
    want = ref.rollout(x0, dev.get_optimal_rollout(), TIMES[-1])[0]
    _close(dev.get_optimal_total_cost(), want, "combined optimal total")


# ---- 6. TrackPoint's own self-collision term ---------------------------------------------------------

def test_with_the_self_collision_term(monkeypatch):
    """The self-collision term's link FK beside the orientation term's, the read-out after every
    update (so filter() runs by itself)."""
    _run("r19_h33", monkeypatch, [TP.path_a(), TP.path_b(), None], cost=_objective(self_collision=True), plans=False)


# ---- 7. paths through the engine ---------------------------------------------------------------------

def test_in_launch_objective_against_the_cost_kernel(monkeypatch):
    """The same inputs through the launch's own objective and through fr_step_cost_kernel
    (MPPI_COSTS_IN_LAUNCH=0), r147_h33: equal costs at the bars, as test_gpu_obstacles.py's test of the
    same name holds them; whether they agree bit for bit is printed."""
    _, S, H, keep, req, sw, _, _ = by_name("r147_h33")
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    _set_env(monkeypatch, req, "")
    a = _handle(conf, _objective(False))[1]
    _set_env(monkeypatch, req, "c")
    b = _handle(conf, _objective(False))[1]
    rng = np.random.default_rng(4)
    sd = np.sqrt(np.diag(conf.covariance))
    same = True
    for j, (x, path, t) in enumerate(zip(_states(), [TP.path_a(), TP.path_c(), None], TIMES)):
        eps = rng.standard_normal((a.noise_draws(t), a.C)) * sd
        for h in (a, b):
            h.set_target_path(path)
            h.inject_noise(eps)
            h.update(x, t)
            assert h.update_info()["wait_timeouts"] == 0
        assert a.update_info()["objective_in_launch"] == 1 and b.update_info()["objective_in_launch"] == 0
        same = same and np.array_equal(a.costs(), b.costs())
        _assert_bars("in-launch vs cost kernel upd %d" % j, a.costs(), b.costs(), a.get_weights(), b.get_weights(),
                     a.get_optimal_rollout(), b.get_optimal_rollout(), H)
    print("in-launch objective and cost kernel bit for bit: %s" % same)
    for u, v in zip(a.get_optimal_target_cost(), b.get_optimal_target_cost()):
        _close(u, v, "in-launch vs cost kernel read-out")


def _philox(conf, graph=0, tracking=POSE):
    t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=True), _objective(False))
    assert t is not None
    if tracking is not None:
        t.set_target_tracking(tracking)
    t.set_graph(graph)
    t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
    return t


GRAPH_PATHS = [TP.path_a(), TP.path_c(), None, TP.path_b()]


def test_graph_path(monkeypatch):
    """test_gpu_obstacles.py::test_graph_path's structure with the path replaced and the time advancing
    between the replays: the targets' launch stays ahead of the graph, whose rollout nodes see the
    current path and time (the eager launches' bits), and all three updates after the first are graph
    updates."""
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
            t.set_target_path(GRAPH_PATHS[j])
            t.update(x, tm)
            assert t.update_info()["wait_timeouts"] == 0
            rec.append(_record(t))
        out[graph] = (rec, t.graph_updates(), t.get_optimal_total_cost(), t.get_optimal_target_cost())
    assert out[0][1] == 0 and out[1][1] == 3, (out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3] and out[0][3][1] > 0.0
    for j, (a, b) in enumerate(zip(out[0][0], out[1][0])):
        for what, u, v in zip(("noise", "costs", "optimal", "weights"), a, b):
            np.testing.assert_array_equal(u, v, err_msg="update %d %s" % (j, what))
    # the target is live, and the time matters: the same path a second late gives other costs
    plain = _philox(conf, 0, tracking=None)
    plain.update(am.huddled_state(), 0.0)
    assert not np.array_equal(plain.costs(), out[0][0][0][1])
    late = _philox(conf, 0)
    late.set_target_path(am.TargetPath(np.asarray(TP.A_TIMES) - 1.0, TP.A_POSITIONS, TP.A_QUATERNIONS))
    late.update(am.huddled_state(), 0.0)
    assert not np.array_equal(late.costs(), out[0][0][0][1])


def test_two_shards_equal_one_handle(monkeypatch):
    """test_gpu_obstacles.py::test_two_shards_equal_one_handle's structure and bars with tracking on:
    every rank enables it and sets the same path."""
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
            h.set_target_path(GRAPH_PATHS[j])
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
            # (helpers.py's bar: the weights follow the costs through exp(-10 (J - Jmin) / Delta), and this
            # objective's Delta is of J's own size, where test_gpu_obstacles.py's 1e11 left them 3e-15 apart)
            assert np.max(np.abs(sh.get_weights() - single.get_weights())) <= WEIGHT_ATOL
            assert sh.argmin() == single.argmin() and sh.update_info()["wait_timeouts"] == 0


# ---- 8. the device object ----------------------------------------------------------------------------

def test_device_object_target_cost(monkeypatch):
    """PinocchioDynamicsObject.target_cost at state_space.py's states against the reference's terms on
    the numpy grasp frame, 1e-12 relative (test_gpu_obstacles.py's bar for the object's obstacle cost)."""
    monkeypatch.delenv("MPPI_LINK_POSITIONS", raising=False)
    model = am.FrankaRidgebackDynamics().model
    obj = am.PinocchioDynamicsObject.create(am.huddled_state())
    config = am.TargetTracking(3.5, True)
    quats = [None, TP.A_QUATERNIONS[1], TP.A_QUATERNIONS[2], (0.0, 0.0, 0.0, 1.0)]
    entries = SS.using("a")
    assert len(entries) > 40
    for n, entry in enumerate(entries):
        x = SS.state(entry)
        obj.set_state(x, 0.0)
        ee, Ree = TR.grasp_rotation(model, x[:12])
        point, quat = TP.A_POSITIONS[n % 4], quats[n % 4]
        d = ee - np.asarray(point)
        want_p = 100.0 * (np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) ** 2)
        want_o = 0.0 if quat is None else TR.orientation_term(3.5, np.asarray(quat) / np.linalg.norm(quat), Ree)
        got = obj.target_cost(point, quat, config)
        bar = 1e-12   # (both sides take the sine of the same double, also at the far yaws)
        assert abs(got[0] - want_p) <= bar * max(abs(want_p), 1.0), (entry[0], got, want_p)
        assert abs(got[1] - want_o) <= bar * max(abs(want_o), 1.0), (entry[0], got, want_o)
    # after a step the cached pose lags the state by that step
    x = am.huddled_state()
    obj.set_state(x, 0.0)
    before = obj.target_cost(TP.POINT, TP.A_QUATERNIONS[1])
    obj.step(np.array([0.2, -0.1, 0.3, 5.0, -4.0, 3.0, -2.0, 1.0, 2.0, -3.0, 0.0, 0.0]), 0.01)
    assert obj.target_cost(TP.POINT, TP.A_QUATERNIONS[1]) == before
    assert obj.target_cost(TP.POINT)[1] == 0.0
    _invalid(lambda: obj.target_cost(TP.POINT, (0, 0, 0, 0.4)), word="norm")
    _invalid(lambda: obj.target_cost(TP.POINT, (0, 0, np.nan, 1)), word="finite")
    _invalid(lambda: obj.target_cost((0, np.inf, 0)), word="finite")
    _invalid(lambda: obj.target_cost(TP.POINT, None, am.TargetTracking(-1.0)), word="orientation_weight")


# ---- 9. validation -----------------------------------------------------------------------------------

def _raw(times, positions=None, quaternions=None, count=None):
    n = len(times)
    c = abi.mppi_target_path()
    c.count = n if count is None else count
    c.has_orientation = 1 if quaternions is not None else 0
    for i in range(min(n, abi.MPPI_TARGET_WAYPOINTS_MAX)):
        c.waypoints[i].time = times[i]
        for k in range(3):
            c.waypoints[i].position[k] = 0.5 if positions is None else positions[i][k]
        for k in range(4):
            c.waypoints[i].quaternion[k] = 0.0 if quaternions is None else quaternions[i][k]
    return c


def test_validation(monkeypatch):
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=17, horison=0.05, keep_best_rollouts=5)
    mk = lambda lp=True, cost=None: am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=lp), cost or _objective())
    x = am.huddled_state()

    # a handle that never enables it
    plain = mk()
    assert plain.target_tracking is None
    _invalid(lambda: plain.set_target_path(TP.path_a()), word="not enabled")
    _invalid(lambda: plain.set_target_path(None), word="not enabled")
    _invalid(lambda: plain.target_path(), word="not enabled")
    _invalid(lambda: plain.get_optimal_target_cost(), abi.MPPI_ERR_UNSUPPORTED)
    # enabling after an update
    plain.update(x, 0.0)
    _invalid(lambda: plain.set_target_tracking(), word="before the first update")
    # an AssistedManipulation handle, a point-mass handle
    _invalid(lambda: mk(cost=am.AssistedManipulation()).set_target_tracking(), abi.MPPI_ERR_UNSUPPORTED)
    pm = am.Trajectory.create(am.point_mass_configuration(rollouts=64), am.PointMassDynamics(), am.QuadraticCost())
    _invalid(lambda: pm.set_target_tracking(), abi.MPPI_ERR_UNSUPPORTED)
    assert pm.target_tracking is None
    # the configuration
    t = mk()
    for bad in (am.TargetTracking(-0.1), am.TargetTracking(np.nan), am.TargetTracking(np.inf, True)):
        _invalid(lambda: t.set_target_tracking(bad), word="orientation_weight")
        assert t.target_tracking is None
    _invalid(lambda: mk(False).set_target_tracking(POSE), word="kinematic")
    t.set_target_tracking(am.TargetTracking(0.0, True))
    assert t.target_tracking == am.TargetTracking(0.0, True)
    _invalid(lambda: t.set_link_positions(abi.MPPI_LINK_POSITIONS_ZERO), word="orientation tracking")
    _invalid(lambda: t.attach_forecast(am.locf_forecast_configuration(horison=1.0)), word="target tracking")
    assert t.target_path() is None and t.get_optimal_target_cost() == (0.0, 0.0)
    # the path
    t.set_target_path(TP.path_b())
    for bad, word in ((_raw((0.0, 0.2, 0.1)), "increasing"), (_raw((0.0, 0.1, 0.1)), "increasing"),
                      (_raw((0.0, np.nan)), "finite"), (_raw((np.inf,)), "finite"),
                      (_raw((), count=0), "count"), (_raw((0.0,), count=-1), "count"),
                      (_raw(np.arange(32.0), count=33), "count"),
                      (_raw((0.0,), [(0.0, np.nan, 0.0)]), "position"),
                      (_raw((0.0,), None, [(0, 0, 0, 0.49)]), "norm"), (_raw((0.0,), None, [(0, 0, 0, 2.01)]), "norm"),
                      (_raw((0.0,), None, [(0, 0, 0, 0)]), "norm"), (_raw((0.0,), None, [(0, np.nan, 0, 1)]), "finite")):
        _invalid(lambda: t.set_target_path(bad), word=word)
    assert len(t.target_path()) == 2   # a refused call left the previous path in place
    t.set_target_path(_raw(np.arange(32.0)))
    assert len(t.target_path()) == 32 and not t.target_path().has_orientation
    t.set_target_path(_raw((0.0,), None, [(0, 0, 0, 0.5)]))
    assert t.target_path().orientations[0, 3] == 1.0
    t.set_target_path(_raw((0.0, 1.0), None, [(0, 0, 0, 2.0), (0, 0, 0.1, -1.0)]))
    assert np.all(t.target_path().orientations[:, 3] > 0.0)   # normalised, then sign-fixed
    # a path may be replaced and cleared after updates have run; enabling may not
    t.update(x, 0.0)
    t.set_target_path(TP.path_a())
    t.update(x, 0.01)
    t.set_target_path(None)
    t.update(x, 0.02)
    assert t.update_info()["wait_timeouts"] == 0 and t.target_path() is None
    _invalid(lambda: t.set_target_tracking(), word="before the first update")


# ---- 10. the C++ surface -----------------------------------------------------------------------------

def test_cpp_target_surface_on_the_device(monkeypatch):
    """tests/cpp/target_path.cpp writes the numbers the Python API gives for the same inputs (the same
    Philox seed), in the manner of test_cpp_dropin.py."""
    _set_env(monkeypatch)
    cpp = os.path.join(REPO, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "target_path.mk"])
    out = subprocess.check_output([os.path.join(cpp, "build", "target_path"), "gpu"], timeout=300).decode()
    lines = [json.loads(l) for l in out.strip().split("\n")]
    assert lines[0] == {"cpu": "ok"}
    assert lines[1] == {"assisted_manipulation": False, "zero_mode_orientation": False, "zero_mode_position": True,
                        "path_without_tracking": False}
    assert lines[2] == {"enabled": True, "weight": 4.0, "orientation": 1}
    conf = am.frankaridgeback_configuration(rollouts=64, horison=0.16)
    t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=True), am.TrackPoint())
    t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
    pose = am.TargetTracking(4.0, True)
    t.set_target_tracking(pose)
    path = am.TargetPath((0.015, 0.085, 0.145), ((0.88, 0.86, 0.90), (0.80, 0.95, 0.95), (0.75, 0.80, 1.00)),
                         ((0.1, 0.0, 0.0, 1.0), (0.2, 0.1, -0.1, 0.9), (-0.3, -0.3, 0.2, -0.7)))
    x = am.huddled_state()
    for j in range(3):
        if j == 1:
            t.set_target_path(path)
        if j == 2:
            t.set_target_path(None)
        t.update(x, 0.03 * j)
        pos, ori = t.get_optimal_target_cost()
        assert lines[3 + j] == {"update": j, "optimal_cost": t.get_optimal_total_cost(), "position": pos, "orientation": ori}
    assert lines[4]["orientation"] > 0.0 and lines[3]["orientation"] == 0.0 and lines[5]["orientation"] == 0.0
    assert lines[6] == {"late_enable": False}
    d = am.PinocchioDynamicsObject.create(x)
    d.set_state(x, 0.0)
    d.step(np.array([(5.0 - i) if 3 <= i < 10 else 0.1 for i in range(12)]), 0.01)
    pos, ori = d.target_cost(path.positions[1], path.raw_orientations[1], pose)
    assert lines[7] == {"object_position": pos, "object_orientation": ori, "same": True}
