"""Obstacle avoidance with a held object (mppi_set_held_object_avoidance) on the device against the Python
composition of held_object_reference.py: the held term in every launch plan of the rollouts, both
objectives, the tank, the simulated wrench, the separate cost kernel, the graph path and the two new rollout
units, sharding, the handles it must equal bit for bit, the rotation, the device object, the predicted held
paths, the refusals and the C++ surface.

The pattern is test_gpu_distance_field.py's: three updates at time 0 from test_gpu_link_positions.py's three
states with its noise scaling, host-injected noise, helpers.py's bars.  The object is replaced between the
updates (held_object_sets.py): a beam, a tray of four points and three segments, then a tool tip, with
primitives and fields beside them; the folded filter() row of an update is checked against the object of that
update, which by then has been replaced.  The reference keeps books on every held clearance it evaluates, and
each run asserts from them (test_held_object_cpu.check_books), on the device's own noise, that nothing sat
within 1e-6 of the barrier's branch point or, in grid units, of the grid's boundary, that the beam stayed
0.02 m clear on the inverse branch, that the tray took both branches, and that the held term moved every
rollout's cost in the first two updates.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi

import capsule_sets as CS
import field_sets as FS
import held_object_reference as HR
import held_object_sets as HS
import link_reference as LR
import obstacle_sets as OS
import test_gpu_rollout_units as UNITS
import wrench_reference as WR
from launch_shapes import X, by_name, horizon
from test_gpu_link_positions import SHAPES, _assert_bars, _hip, _noise_scale, _record, _states
from test_gpu_obstacles import _close, _invalid, _set_env
from test_gpu_predicted import FK_BAR
from test_held_object_cpu import check_books

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _handle(conf, cost, wrench=None, held=True, config=None):
    dyn = am.FrankaRidgebackDynamics(link_positions=True, simulated_wrench=wrench)
    dev = am.Trajectory.create(conf, dyn, cost)
    assert dev is not None and dev.link_positions
    dev.set_obstacle_avoidance(config)
    dev.set_obstacle_capsules(CS.capsules())
    dev.set_distance_field_avoidance()
    if held:
        assert not dev.held_object_avoidance
        dev.set_held_object_avoidance()
        assert dev.held_object_avoidance and dev.held_object is None
    dev.set_noise_source(abi.MPPI_NOISE_HOST_INJECTED)
    return dyn, dev


def _print_books(tag, term):
    b = term.hbooks
    print("%s held books: least margin %.3e, least v %.4f, %s, evaluated %d, inside %d, outside %d, least distance to the grid's edge %.3e"
          % (tag, b.least_margin, b.least_v, sorted(b.branches), b.evaluated, b.inside, b.outside, b.edge))


def _costs(comp, x, U, eps, t0=0.0):
    """comp.costs, and per rollout the discounted sum of its held terms."""
    J, held = np.zeros(eps.shape[0]), np.zeros(eps.shape[0])
    for r in range(eps.shape[0]):
        J[r] = comp.rollout(x, U + eps[r], t0)[0]
        held[r] = sum(comp.gamma ** k * t for k, t in enumerate(comp.term.held_steps))
    return J, held


def _assert_moved(tag, J, held):
    """The held term moved every rollout's cost: its discounted sum is positive and shows in the cost's bits."""
    assert np.all(held > 0.0) and np.all(J - held != J), (tag, float(held.min()))


def _run(name, cost, monkeypatch, plans=True):
    """test_gpu_distance_field.py::_run on a held handle: before update j the set, the field and the object
    of held_object_sets are put in place."""
    _, S, H, keep, req, sw, first, pend = by_name(name)
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    table = am.constant_forecast(H)
    dyn, dev = _handle(conf, cost)
    assert dev.H == H and dev.R == S + 2
    dev.set_forecast(table)
    comp = HR.Composition(conf, dyn.model, cost, table, capsules=CS.capsules())
    states, scale = _states(), _noise_scale(H)
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance)) * scale
    U = np.zeros((H, dev.C))
    prev = None
    for j, (x, held, field, (obstacles, t_ref)) in enumerate(zip(states, HS.objects(), HS.fields(), HS.sets())):
        tag = "%s upd %d" % (name, j)
        dev.set_obstacles(obstacles, t_ref)
        dev.set_distance_field(field)
        dev.set_held_object(held)
        assert dev.held_object == held
        comp.field, comp.held = field, held
        term = comp.set_obstacles(obstacles, t_ref)
        dev.inject_noise(rng.standard_normal((dev.noise_draws(0.0), dev.C)) * sd)
        dev.update(x, 0.0)
        info = dev.update_info()
        assert info["wait_timeouts"] == 0 and info["cooperative"] == 1, (tag, info)
        if plans:
            want = first if j == 0 else pend
            assert info["folded_filter"] == want[5] and info["objective_in_launch"] == want[6], (tag, info)
        if info["folded_filter"]:   # the previous update's filter() row: its own object, replaced since
            comp.term = prev
            ref = comp.rollout(states[j - 1], U)[0]
            comp.term = term
            _close(dev.debug_folded_cost(), ref, tag + " folded filter()")
        eps = dev.noise()
        J, moved = _costs(comp, x, U, eps)
        w, g, Un = LR.mppi_update(conf, J, eps, U)
        _assert_bars(tag, dev.costs(), J, dev.get_weights(), w, dev.get_optimal_rollout(), Un, H)
        U = dev.get_optimal_rollout()
        _print_books(tag, term)
        check_books(term, j, tag)
        if j < 2:
            _assert_moved(tag, J, moved)
        if not plans:
            ref, _, ob = comp.rollout(x, U)
            _close(dev.get_optimal_held_cost(), term.held_steps.sum(), tag + " optimal held cost")
            _close(dev.get_optimal_field_cost(), term.field_steps.sum(), tag + " optimal field cost")
            _close(dev.get_optimal_obstacle_cost(), ob.sum(), tag + " optimal obstacle cost")
            _close(dev.get_optimal_total_cost(), ref, tag + " optimal total")
        prev = term
    ref, sc, ob = comp.rollout(states[2], U)
    _close(dev.get_optimal_total_cost(), ref, name + " optimal total")
    _close(dev.get_optimal_obstacle_cost(), ob.sum(), name + " optimal obstacle cost")
    _close(dev.get_optimal_held_cost(), comp.term.held_steps.sum(), name + " optimal held cost")
    _close(dev.get_optimal_field_cost(), comp.term.field_steps.sum(), name + " optimal field cost")
    return dev, comp


# ---- 1. parity against the composition, every launch plan ---------------------------------------

@pytest.mark.parametrize("name", SHAPES)
def test_update_against_the_composition(name, monkeypatch):
    _run(name, HS.objective(), monkeypatch)


def test_optimal_held_cost_after_every_update(monkeypatch):
    """The optimal rollout read after each update (filter() runs by itself): the held, field, obstacle and total
    costs against the reference's sums; the obstacle cost holds all three parts."""
    dev, comp = _run("r19_h33", HS.objective(), monkeypatch, plans=False)
    assert dev.get_optimal_obstacle_cost() > dev.get_optimal_held_cost() > 0.0


# ---- 2. other objectives and modes --------------------------------------------------------------

def test_track_point(monkeypatch):
    _run("r19_h33", HS.objective("track_point"), monkeypatch)


def test_energy_tank(monkeypatch):
    _run("r19_h33", HS.objective(energy=True), monkeypatch)


def test_simulated_wrench_forecast(monkeypatch):
    """The pushed robot with the held term: test_gpu_distance_field.py's wrench test on a held handle."""
    from test_gpu_simulated_wrench import TIMES, _assert_update, _state
    _, S, H, keep, req, sw, _, _ = by_name("r19_h33")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = HS.objective()
    table = WR.forecast_table(H)
    dyn, dev = _handle(conf, cost, wrench="forecast")
    dev.set_forecast(table)
    ref = HR.WrenchComposition(conf, dyn.model, cost, "forecast", table, capsules=CS.capsules())
    sd = np.sqrt(np.diag(conf.covariance))
    rng, shift, dt = np.random.default_rng(11), WR.Shift(), dev.get_time_step()
    prev = None
    for j, (t, held, field, (obstacles, t_ref)) in enumerate(zip(TIMES, HS.objects(), HS.fields(), HS.sets())):
        tag = "wrench upd %d" % j
        x0 = _state(j)
        U_prev = dev.get_optimal_rollout()
        U_shift = WR.shifted(U_prev, shift(t, dt))
        dev.set_obstacles(obstacles, t_ref)
        dev.set_distance_field(field)
        dev.set_held_object(held)
        ref.field, ref.held = field, held
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
        J, moved = _costs(ref, x0, U_shift, eps, t)
        w, g, Un = LR.mppi_update(conf, J, eps, U_shift)
        _assert_update(tag, dev, J, w, g, Un, H)
        _print_books(tag, term)
        check_books(term, j, tag)
        if j < 2:
            _assert_moved(tag, J, moved)
        prev = (term, x0, t)
    want, _, ob = ref.rollout(x0, dev.get_optimal_rollout(), TIMES[-1])
    _close(dev.get_optimal_total_cost(), want, "wrench optimal total")
    _close(dev.get_optimal_held_cost(), ref.term.held_steps.sum(), "wrench optimal held cost")


# ---- 3. paths ------------------------------------------------------------------------------------

def test_in_launch_objective_against_the_cost_kernel(monkeypatch):
    """The same inputs through the launch's own objective and through fr_step_cost_links_kernel<OB_TERM_HELD>
    (MPPI_COSTS_IN_LAUNCH=0), r147_h64: costs and U* bit for bit."""
    _, S, H, keep, req, sw, _, _ = by_name("r147_h64")
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = HS.objective()
    _set_env(monkeypatch, req, "")
    a = _handle(conf, cost)[1]
    _set_env(monkeypatch, req, "c")
    b = _handle(conf, cost)[1]
    rng = np.random.default_rng(4)
    sd = np.sqrt(np.diag(conf.covariance)) * _noise_scale(H)
    for j, (x, held, field, (obstacles, t_ref)) in enumerate(zip(_states(), HS.objects(), HS.fields(), HS.sets())):
        eps = rng.standard_normal((a.noise_draws(0.0), a.C)) * sd
        for t in (a, b):
            t.set_forecast(am.constant_forecast(H))
            t.set_obstacles(obstacles, t_ref)
            t.set_distance_field(field)
            t.set_held_object(held)
            t.inject_noise(eps)
            t.update(x, 0.0)
            assert t.update_info()["wait_timeouts"] == 0
        assert a.update_info()["objective_in_launch"] == 1 and b.update_info()["objective_in_launch"] == 0
        np.testing.assert_array_equal(a.costs(), b.costs(), err_msg="update %d costs" % j)
        np.testing.assert_array_equal(a.get_optimal_rollout(), b.get_optimal_rollout(), err_msg="update %d U*" % j)
        assert a.get_optimal_held_cost() == b.get_optimal_held_cost() > 0.0


def _philox(conf, graph=0, held=True, wrench=False, cost=None):
    dyn = am.FrankaRidgebackDynamics(link_positions=True, simulated_wrench="state" if wrench else False)
    t = am.Trajectory.create(conf, dyn, cost or am.AssistedManipulation())
    assert t is not None
    t.set_obstacle_avoidance()
    t.set_obstacle_capsules(CS.capsules())
    t.set_distance_field_avoidance()
    if held:
        t.set_held_object_avoidance()
    t.set_graph(graph)
    t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
    t.set_forecast(am.constant_forecast(t.H))
    return t


def _held_bits(obstacles, which=(2,)):
    """The set with the held bits added to the masks of the obstacles `which`."""
    out = list(obstacles)
    for i in which:
        o = out[i].to_c()
        o.mask |= am.MASK_HELD
        out[i] = am.obstacle_from_c(o)
    return out


def _unit_run(name, wrench, graph):
    """test_gpu_rollout_units.run for the held cell: that module's field cell - its objective, set C, field F,
    its states and times - with the held bits in one obstacle's mask and in the field's, and an object that is
    a beam, then put down, then a tray.  ([(costs, weights, optimal rollout)], graph updates, the last update's
    optimal held cost)."""
    _, S, H, keep = by_name(name)[:4]
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    t = _philox(conf, graph, wrench=wrench, cost=OS.objective())
    assert t.H == H and t.R == S + 2
    f = FS.field_f()
    t.set_distance_field(am.DistanceField(f.values, f.origin, f.voxel, mask=f.mask | am.MASK_HELD, segment_samples=f.segment_samples))
    t.set_obstacles(_held_bits(CS.set_c()), CS.T_REF_C)
    x = am.huddled_state()
    x[24:30] = WR.W0
    rec = []
    for j, (tm, held) in enumerate(zip(UNITS.TIMES, [HS.beam(), None, HS.tray()])):
        if j == 2:
            x = x.copy()
            x[12 + 4] = 0.3
        t.set_held_object(held)
        t.update(x, tm)
        assert t.update_info()["wait_timeouts"] == 0
        rec.append((t.costs().copy(), t.get_weights().copy(), t.get_optimal_rollout().copy()))
    # (the optimal rollout's costs are read once, at the end: reading them runs the pending filter() by itself, and an
    # update without a folded filter() row is not a graph update)
    return rec, t.graph_updates(), t.get_optimal_held_cost()


@pytest.mark.parametrize("wrench", (0, 1))
@pytest.mark.parametrize("name", UNITS.SHAPES)
def test_graph_equals_eager_and_the_new_cells_differ(name, wrench, monkeypatch):
    """What test_gpu_rollout_units.py holds the ten cells to, for the two new ones: the graph path gives the
    eager launches' bits, with the object replaced and put down between the replays, and the first update's
    costs differ from every other cell's (two cells with the same costs ran the same unit)."""
    for v in UNITS.ENV:
        monkeypatch.delenv(v, raising=False)
    eager, eager_graphs, eager_held = _unit_run(name, wrench, 0)
    graph, graphs, graph_held = _unit_run(name, wrench, 1)
    pend = by_name(name)[7]
    want = len(UNITS.TIMES) - 1 if pend[0] == X and pend[5] else 0
    assert eager_graphs == 0 and graphs == want, (eager_graphs, graphs, want)
    for j, (a, b) in enumerate(zip(eager, graph)):
        for what, u, v in zip(("costs", "weights", "optimal"), a, b):
            np.testing.assert_array_equal(u, v, err_msg="update %d %s" % (j, what))
    assert eager_held == graph_held > 0.0      # the tray's
    assert np.all(np.isfinite(eager[0][0]))
    for c in UNITS.CELLS:
        other = UNITS._eager(name, c[0], c[1], monkeypatch)[0][0][0]
        assert not np.array_equal(eager[0][0], other), (name, wrench, c)


def test_two_shards_equal_one_handle(monkeypatch):
    """Two phase-split shards against one handle at 128 x 32, every rank with the same object:
    test_gpu_distance_field.py's structure and bars."""
    _set_env(monkeypatch, 0, "")
    conf = am.frankaridgeback_configuration(rollouts=128, horison=horizon(32), keep_best_rollouts=20, threads=8)
    world = 2
    single, shards = _philox(conf), [_philox(conf) for _ in range(world)]
    assert single.H == 32
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

    for j, (held, field, (obstacles, t_ref)) in enumerate(zip(HS.objects(), HS.fields(), HS.sets())):
        t = 0.05 * j
        for h in [single] + shards:
            h.set_obstacles(obstacles, t_ref)
            h.set_distance_field(field)
            h.set_held_object(held)
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
        assert single.update_info()["wait_timeouts"] == 0 and single.get_optimal_held_cost() > 0.0
        for sh in shards:
            cs = sh.costs()
            if j == 0:
                np.testing.assert_array_equal(cs, cu)
            assert np.all(np.abs(cs - cu) <= 1e-11 * (delta + np.abs(cu)))
            assert np.max(np.abs(sh.get_optimal_rollout() - single.get_optimal_rollout())) <= 1e-12
            assert np.max(np.abs(sh.get_weights() - single.get_weights())) <= 3e-15
            assert sh.argmin() == single.argmin() and sh.update_info()["wait_timeouts"] == 0


# ---- 4. the handles it must equal bit for bit ------------------------------------------------------

def test_no_object_equals_a_field_handle(monkeypatch):
    """A held handle without an object against a field handle, three updates on set C, D and the empty set with
    the fields of field_sets behind them: costs, weights and U* bit for bit (the term is skipped by a uniform
    branch on the object's count).  Handle c has held bits in every obstacle's mask and in the field's, which
    name nothing while nothing is held; handle d carries a beam through the first update and puts it down: from
    the second update on it gives the field handle's bits for the same inputs."""
    _set_env(monkeypatch, 0, "")
    conf = am.frankaridgeback_configuration(rollouts=147, horison=horizon(20), keep_best_rollouts=20, threads=8)
    a, b, c = _philox(conf), _philox(conf, held=False), _philox(conf)
    assert a.held_object_avoidance and not b.held_object_avoidance
    for j, (x, (obstacles, t_ref), field) in enumerate(zip(_states(), CS.cde(), FS.fgh())):
        for t in (a, b):
            t.set_obstacles(obstacles, t_ref)
            t.set_distance_field(field)
        c.set_obstacles(_held_bits(obstacles, range(len(obstacles))), t_ref)
        c.set_distance_field(am.DistanceField(field.values, field.origin, field.voxel, mask=field.mask | am.MASK_HELD,
                                              segment_samples=field.segment_samples))
        for t in (a, b, c):
            t.update(x, 0.03 * j)
            assert t.update_info()["wait_timeouts"] == 0
        for t in (a, c):
            for u, v in zip(_record(t), _record(b)):
                np.testing.assert_array_equal(u, v, err_msg="update %d" % j)
            assert t.get_optimal_obstacle_cost() == b.get_optimal_obstacle_cost() and t.get_optimal_held_cost() == 0.0
            assert t.get_optimal_field_cost() == b.get_optimal_field_cost()
    assert a.get_optimal_total_cost() == b.get_optimal_total_cost() == c.get_optimal_total_cost()
    # put down mid-run, at one step a horizon (r19_h1): every rollout's cost is x0's, so the first update leaves U*
    # alone whatever it cost, and the updates after the put-down have the field handle's inputs: the first
    # update's costs differ (the beam), every later record is the field handle's bit for bit, held bits in place
    conf1 = am.frankaridgeback_configuration(rollouts=19, horison=horizon(1), keep_best_rollouts=5, threads=8)
    d, e = _philox(conf1), _philox(conf1, held=False)
    assert d.H == 1
    for j, (x, field, (obstacles, t_ref)) in enumerate(zip(_states(), HS.fields(), HS.sets())):
        plain = []
        for o in obstacles:
            c_o = o.to_c()
            c_o.mask &= ~am.MASK_HELD
            plain.append(am.obstacle_from_c(c_o))
        d.set_obstacles(obstacles, t_ref)
        d.set_distance_field(field)
        e.set_obstacles(plain, t_ref)
        e.set_distance_field(am.DistanceField(field.values, field.origin, field.voxel, mask=field.mask & ~am.MASK_HELD,
                                              segment_samples=field.segment_samples))
        d.set_held_object(HS.beam() if j == 0 else None)
        for t in (d, e):
            t.update(x, 0.03 * j)
            assert t.update_info()["wait_timeouts"] == 0
        if j == 0:
            assert np.all(d.costs() != e.costs()) and d.get_optimal_held_cost() > 0.0
            np.testing.assert_array_equal(d.get_optimal_rollout(), e.get_optimal_rollout())
        else:
            for u, v in zip(_record(d), _record(e)):
                np.testing.assert_array_equal(u, v, err_msg="put down, update %d" % j)
            assert d.get_optimal_held_cost() == 0.0 and d.get_optimal_obstacle_cost() == e.get_optimal_obstacle_cost()


def test_an_identity_by_construction(monkeypatch):
    """A one-point object at the grasp origin with radius radii[8] and one obstacle masked HELD_POINT(0) only, no
    field: p_ee + Ree 0 is p_ee exactly and both sums have one term, so the costs are bit for bit those of a
    field handle with the same obstacle masked bit 8."""
    _set_env(monkeypatch, 0, "")
    conf = am.frankaridgeback_configuration(rollouts=147, horison=horizon(20), keep_best_rollouts=20, threads=8)
    a, b = _philox(conf), _philox(conf, held=False)
    radius = am.ObstacleAvoidance().radii[8]
    a.set_held_object(am.HeldObject([(0.0, 0.0, 0.0)], (radius,)))
    for kind in ("sphere", "half-space", "capsule"):
        for j, x in enumerate(_states()):
            for t, mask in ((a, am.mask_held_point(0)), (b, 1 << 8)):
                if kind == "sphere":   # set B's: on the huddled grasp position, both branches
                    ob = am.SphereObstacle((0.8703, 0.8774, 0.8908), 0.05, velocity=(0.1, 0.0, 0.0), mask=mask)
                elif kind == "half-space":
                    ob = am.HalfSpaceObstacle((1.0, 0.0, 0.0), (-0.8, 0.0, 0.6), mask=mask)
                else:
                    ob = am.CapsuleObstacle((0.9, 0.6, 0.9), (0.0, 0.5, 0.1), 0.05, mask=mask)
                t.set_obstacles([ob], -0.07)
                t.update(x, 0.03 * j)
                assert t.update_info()["wait_timeouts"] == 0
            for what, u, v in zip(("noise", "costs", "optimal", "weights"), _record(a), _record(b)):
                np.testing.assert_array_equal(u, v, err_msg="%s update %d %s" % (kind, j, what))
            assert a.get_optimal_held_cost() == a.get_optimal_obstacle_cost() == b.get_optimal_obstacle_cost() > 0.0
            assert a.get_optimal_total_cost() == b.get_optimal_total_cost()


def test_the_rotation_is_used(monkeypatch):
    """A sphere at the tip of a 0.3 m offset along the grasp's x axis (just past it, so that it keeps 0.3 m from
    all nine robot points at all three states), seen only through the held bit: every cost differs from the
    field handle's and agrees with the reference - with the offset turned by any other rotation the point
    would sit elsewhere."""
    _, S, H, keep, req, sw, _, _ = by_name("r19_h33")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = HS.objective()
    table = am.constant_forecast(H)
    dyn, dev = _handle(conf, cost)
    _, plain = _handle(conf, cost, held=False)
    states = _states()
    p0, R0 = HR.grasp_pose(dyn.model, states[0][:12])
    held = am.HeldObject([(0.3, 0.0, 0.0)], (0.03,))
    centre = p0 + 0.34 * R0[:, 0]
    import obstacle_reference as OR
    for x in states:
        assert np.linalg.norm(OR.robot_points(dyn.model, x[:12]) - centre, axis=1).min() >= 0.3
    ob = [am.SphereObstacle(centre, 0.05, mask=am.mask_held_point(0))]
    comp = HR.Composition(conf, dyn.model, cost, table, capsules=CS.capsules())
    comp.held = held
    term = comp.set_obstacles(ob, 0.0)
    dev.set_held_object(held)
    dev.set_obstacles(ob, 0.0)
    plain.set_obstacles([am.SphereObstacle(centre, 0.05, mask=0)], 0.0)
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance)) * _noise_scale(H)
    U = np.zeros((H, dev.C))
    for j, x in enumerate(states):
        eps_in = rng.standard_normal((dev.noise_draws(0.0), dev.C)) * sd
        for t in (dev, plain):
            t.set_forecast(table)
            t.inject_noise(eps_in)
            t.update(x, 0.0)
            assert t.update_info()["wait_timeouts"] == 0
        eps = dev.noise()
        J, moved = _costs(comp, x, U, eps)
        w, g, Un = LR.mppi_update(conf, J, eps, U)
        _assert_bars("rotation upd %d" % j, dev.costs(), J, dev.get_weights(), w, dev.get_optimal_rollout(), Un, H)
        _assert_moved("rotation upd %d" % j, J, moved)
        assert term.hbooks.least_margin >= 1e-6
        if j == 0:   # (later the two handles' plans, and so their rollouts, have parted)
            assert np.all(dev.costs() != plain.costs())
            assert term.hbooks.branches == {"inverse", "saturated"}
        U = dev.get_optimal_rollout()


# ---- 5. the device object --------------------------------------------------------------------------

def test_device_object_held_cost(monkeypatch):
    """PinocchioDynamicsObject.held_object_cost at huddled_state() against the scalar reference, 1e-12 relative:
    the objects, sets and fields of the tests, unit by unit (each held point and segment alone against each
    kind and against a smooth field), and by hand: a sphere on a held point is -(r + r_o) whatever the pose, an
    absent unit is exactly 0, nothing held is 0, a NaN pose is NaN; the refusals."""
    monkeypatch.delenv("MPPI_LINK_POSITIONS", raising=False)
    model = am.FrankaRidgebackDynamics().model
    x = am.huddled_state()
    p, R = HR.grasp_pose(model, x[:12])
    for link_positions in (True, False):   # the object caches the grasp pose in both models
        obj = am.PinocchioDynamicsObject.create(x, link_positions=link_positions)
        obj.set_state(x, 0.0)
        config = am.ObstacleAvoidance(limit=(0.01, 2.0, 1e8))

        def check(held, obstacles, elapsed, field, conf=None, what=""):
            term = HR.Term(conf or am.ObstacleAvoidance(), am.ObstacleCapsules(), obstacles, 0.0, field, held)
            want = term.held_at(p, R, elapsed)
            got = obj.held_object_cost(conf, obstacles, elapsed, field, held)
            assert abs(got - want) <= 1e-12 * max(abs(want), 1.0), (what, got, want)
            return term, got

        for held, field, (obstacles, t_ref) in zip(HS.objects(), HS.fields(), HS.sets()):
            term, got = check(held, obstacles, 0.07, field, None, "the tests' sets")
            assert got > 0.0 and term.hbooks.evaluated > 0
            check(held, obstacles, 0.4, field, config, "the tests' sets, another limit and time")
        tray = HS.tray()
        smooth = am.DistanceField.from_function(lambda x, y, z: 0.3 * x - 0.2 * y + 0.1 * z + 0.5, mask=am.MASK_HELD, segment_samples=5, **FS.ROOM)
        kinds = [am.SphereObstacle((1.3, 0.6, 0.7), 0.1), am.HalfSpaceObstacle((0.0, 0.0, 0.2), (0.0, 0.6, 0.8)),
                 am.CapsuleObstacle((1.2, 0.4, 0.5), (0.1, 0.7, 0.3), 0.05, velocity=(0.0, 0.5, 0.0))]
        for u in range(7):
            mask = am.mask_held_point(u) if u < 4 else am.mask_held_segment(u - 4)
            for ob in kinds:
                o = ob.to_c()
                o.mask = mask
                term, got = check(tray, [am.obstacle_from_c(o)], 0.1, None, config, "unit %d" % u)
                assert term.hbooks.evaluated == 1 and got > 0.0
            term, got = check(tray, [], 0.0, am.DistanceField(smooth.values, smooth.origin, smooth.voxel, mask=mask, segment_samples=5), config, "unit %d field" % u)
            assert term.hbooks.inside == (1 if u < 4 else 5)
        # by hand
        ee = obj.get_end_effector_state_row()[abi.MPPI_EE_POSITION:abi.MPPI_EE_POSITION + 3]
        origin = am.HeldObject([(0.0, 0.0, 0.0)], (0.125,))
        on_it = am.SphereObstacle(ee, 0.5, mask=am.mask_held_point(0))
        assert obj.held_object_cost(None, [on_it], 0.0, None, origin) == 1e10 + 0.625 ** 2     # |p - c| = 0: v = -(r + r_o)
        assert obj.held_object_cost(None, [on_it], 0.0, None, HS.beam()) > 0.0
        absent = am.SphereObstacle(ee, 0.5, mask=am.mask_held_point(1) | am.mask_held_segment(0) | am.MASK_ALL | am.MASK_SEGMENTS)
        assert obj.held_object_cost(None, [absent], 0.0, None, origin) == 0.0
        assert obj.held_object_cost(None, [on_it], 0.0, None, None) == 0.0
        assert obj.held_object_cost(None, [on_it], 0.0, None, am.HeldObject(np.zeros((0, 3)), ())) == 0.0
        assert obj.held_object_cost(None, [], 0.0, None, origin) == 0.0
        away = am.DistanceField.from_function(lambda x, y, z: x - 100.0, (5.0, 5.0, 5.0), 0.5, (3, 4, 5), mask=am.MASK_HELD)
        assert obj.held_object_cost(None, [], 0.0, away, HS.tray()) == 0.0                   # a grid that holds nothing of the object
        far = am.SphereObstacle(ee + np.array([3.0, 0.0, 4.0]), 0.5, mask=am.MASK_HELD)
        got = obj.held_object_cost(None, [far], 0.0, None, origin)
        assert abs(got - 1.0 / (5.0 - 0.625)) <= 1e-12
        bad = x.copy()
        bad[5] = np.nan
        obj.set_state(bad, 0.0)
        assert np.isnan(obj.held_object_cost(None, [on_it], 0.0, None, origin))
        assert obj.held_object_cost(None, [absent], 0.0, None, origin) == 0.0              # nothing masked: +0.0 whatever the pose
        obj.set_state(x, 0.0)
        five = abi.mppi_held_object()
        five.count = 5
        v = C.c_double(0.0)
        assert obj._L.mppi_dynamics_held_object_cost(obj._h, None, None, 0, 0.0, None, None, C.byref(five), C.byref(v)) == abi.MPPI_ERR_INVALID
        neg = origin.to_c()
        neg.radii[0] = -0.1
        assert obj._L.mppi_dynamics_held_object_cost(obj._h, None, None, 0, 0.0, None, None, C.byref(neg), C.byref(v)) == abi.MPPI_ERR_INVALID
        _invalid(lambda: obj.held_object_cost(None, [am.SphereObstacle(ee, 0.5, mask=1 << 13)], 0.0, None, origin), word="mask")


# ---- 6. the predicted held paths -------------------------------------------------------------------

def _numpy_paths(model, Q, held):
    """The held points at a stack of configurations (..., 12): (..., 4, 3), NaN rows for absent points."""
    out = np.full(Q.shape[:-1] + (4, 3), np.nan)
    for idx in np.ndindex(*Q.shape[:-1]):
        if np.isfinite(Q[idx]).all():
            p, R = HR.grasp_pose(model, Q[idx])
            out[idx][:held.count] = HR.world_points(held, p, R)
    return out


def test_predicted_held_paths(monkeypatch):
    """predicted_held_rollouts / predicted_held_optimal against numpy forward kinematics at the predicted q_k
    themselves (not lagged), to the bar test_gpu_predicted.py holds the link positions to; the rows of points
    the object does not have are NaN; a rollout that goes NaN is NaN from that step on; held_object_clearance
    runs on what they return; the error rules."""
    _, S, H, keep, req, sw, _, _ = by_name("r19_h33")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    dyn, dev = _handle(conf, HS.objective())
    dev.set_forecast(am.constant_forecast(H))
    for call in (dev.predicted_held_optimal, lambda: dev.predicted_held_rollouts([0])):
        with pytest.raises(am.EngineError) as ei:
            call()
        assert ei.value.status == abi.MPPI_ERR_INVALID and "yet" in str(ei.value)
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance))
    rows = np.arange(dev.R)
    for j, (x, held, field, (obstacles, t_ref)) in enumerate(zip(_states(), HS.objects(), HS.fields(), HS.sets())):
        dev.set_obstacles(obstacles, t_ref)
        dev.set_distance_field(field)
        dev.set_held_object(held)
        eps = rng.standard_normal((dev.noise_draws(0.0), dev.C)) * sd
        dev.inject_noise(eps)
        dev.update(x, 0.0)
        assert dev.update_info()["wait_timeouts"] == 0
        pred = dev.predicted_rollouts(rows)
        paths = dev.predicted_held_rollouts(rows)
        assert paths.shape == (dev.R, H, 4, 3)
        q = pred.raw[..., :12]
        want = _numpy_paths(dyn.model, q, held)
        assert np.array_equal(np.isnan(paths), np.isnan(want)), "update %d NaN pattern" % j
        assert np.isnan(paths[:, :, held.count:]).all() and np.isfinite(paths[np.isfinite(q).all(axis=-1)][:, :held.count]).all()
        err = np.nanmax(np.abs(paths - want))
        print("update %d: held paths differ from the numpy chain at q_k by %.3e m" % (j, err))
        assert err <= FK_BAR
        assert np.array_equal(paths[:, 0], np.broadcast_to(paths[0, 0], paths[:, 0].shape), equal_nan=True)      # step 0 is x0's pose
        opt, popt = dev.predicted_held_optimal(), dev.predicted_optimal()
        assert opt.shape == (H, 4, 3)
        wopt = _numpy_paths(dyn.model, popt.raw[:, :12], held)
        assert np.array_equal(np.isnan(opt), np.isnan(wopt)) and np.nanmax(np.abs(opt - wopt)) <= FK_BAR
        np.testing.assert_array_equal(dev.predicted_held_rollouts(rows[3:5]), paths[3:5])
        # the clearance helper on the device's paths against the same helper on the numpy paths
        got = am.held_object_clearance(paths, pred.time, None, obstacles, t_ref, held, field)
        ref = am.held_object_clearance(want, pred.time, None, obstacles, t_ref, held, field)
        fin = np.isfinite(ref) & np.isfinite(got)
        assert got.shape == (dev.R, H) and fin.any() and np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.abs(got[fin] - ref[fin]).max() <= 1e-9      # (clearances are 1-Lipschitz in the points; a thresholded field's are 400 times steeper)
    dev.set_held_object(None)
    assert np.isfinite(dev.predicted_held_optimal()[:, 0]).all()       # the last update's object, not the next one's
    dev.inject_noise(rng.standard_normal((dev.noise_draws(0.0), dev.C)) * sd)
    dev.update(_states()[0], 0.0)
    assert np.isnan(dev.predicted_held_optimal()).all() and np.isnan(dev.predicted_held_rollouts([0, 1])).all()
    assert dev.predicted_held_rollouts([]).shape == (0, H, 4, 3)
    for bad in (-1, dev.R):
        with pytest.raises(am.EngineError) as ei:
            dev.predicted_held_rollouts([0, bad])
        assert ei.value.status == abi.MPPI_ERR_INVALID and "outside" in str(ei.value)
    # the NaN rule, on a handle of its own (a NaN rollout's noise makes the next update's U* NaN): one NaN in the noise
    # of one rollout at step 5 makes its rows from step 6 on NaN, and no other row
    _, nd = _handle(conf, HS.objective())
    nd.set_forecast(am.constant_forecast(H))
    nd.set_held_object(HS.beam())
    eps = rng.standard_normal((nd.noise_draws(0.0), nd.C)) * sd
    eps[7 * H + 5, 4] = np.nan
    nd.inject_noise(eps)
    nd.update(_states()[0], 0.0)
    q = nd.predicted_rollouts(rows).raw[..., :12]
    paths = nd.predicted_held_rollouts(rows)
    bad = np.argwhere(np.isnan(q).any(axis=(1, 2))).ravel()
    assert bad.size == 1 and np.isnan(paths[bad[0], 6:]).all() and np.isfinite(paths[bad[0], :6, :2]).all()
    assert np.isfinite(np.delete(paths, bad[0], axis=0)[:, :, :2]).all() and np.isnan(paths[:, :, 2:]).all()
    _, plain = _handle(conf, HS.objective(), held=False)
    plain.inject_noise(rng.standard_normal((plain.noise_draws(0.0), plain.C)) * sd)
    plain.update(_states()[0], 0.0)
    for call in (plain.predicted_held_optimal, lambda: plain.predicted_held_rollouts([0])):
        _invalid(call, word="not enabled")


# ---- 7. validation ---------------------------------------------------------------------------------

def test_validation(monkeypatch):
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=17, horison=0.05, keep_best_rollouts=5)
    mk = lambda: am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=True), am.AssistedManipulation())   # noqa: E731
    beam = HS.beam()
    held_sphere = am.SphereObstacle((2.0, 0.0, 0.0), 0.1, mask=am.MASK_ALL | am.mask_held_point(0))
    held_field = am.DistanceField(np.ones((2, 2, 2)), (5.0, 5.0, 5.0), 0.1, mask=am.MASK_HELD)

    # the wrong order of the enabling calls, held bits on a handle without the mode, calls after the first update
    t = mk()
    assert not t.held_object_avoidance
    _invalid(lambda: t.set_held_object_avoidance(), word="distance field avoidance")
    t.set_obstacle_avoidance()
    _invalid(lambda: t.set_held_object_avoidance(), word="distance field avoidance")
    t.set_obstacle_capsules()
    _invalid(lambda: t.set_held_object_avoidance(), word="distance field avoidance")
    _invalid(lambda: t.set_obstacles([held_sphere], 0.0), word="mask")
    t.set_distance_field_avoidance()
    _invalid(lambda: t.set_held_object(beam), word="not enabled")
    _invalid(lambda: t.held_object, word="not enabled")
    _invalid(lambda: t.set_obstacles([held_sphere], 0.0), word="mask")
    _invalid(lambda: t.set_distance_field(held_field), word="mask")
    with pytest.raises(am.EngineError) as ei:
        t.get_optimal_held_cost()
    assert ei.value.status == abi.MPPI_ERR_UNSUPPORTED
    t.update(am.huddled_state(), 0.0)
    _invalid(lambda: t.set_held_object_avoidance(), word="before the first update")
    assert not t.held_object_avoidance

    f = mk()
    f.set_obstacle_avoidance()
    f.set_obstacle_capsules()
    f.set_distance_field_avoidance()
    f.set_held_object_avoidance()
    assert f.held_object is None and f.get_optimal_held_cost() == 0.0
    f.set_obstacles([held_sphere], 0.0)
    f.set_distance_field(held_field)
    for bit in (13, 14, 15, 27, 28, 29, 30, 31):
        _invalid(lambda: f.set_obstacles([am.SphereObstacle((2.0, 0.0, 0.0), 0.1, mask=1 << bit)], 0.0), word="mask")
        _invalid(lambda: f.set_distance_field(am.DistanceField(np.ones((2, 2, 2)), (5.0, 5.0, 5.0), 0.1, mask=1 << bit)), word="mask")
    f.set_held_object(beam)
    assert f.held_object == beam
    L, h = f._L, f._h

    def refused(o, word):
        assert L.mppi_set_held_object(h, C.byref(o)) == abi.MPPI_ERR_INVALID
        assert word in L.mppi_last_error(h).decode(), (word, L.mppi_last_error(h).decode())
        assert f.held_object == beam        # a refused call leaves the object in place

    for count in (5, -1):
        o = beam.to_c()
        o.count = count
        refused(o, "count")
    for value in (-0.1, np.nan, np.inf):
        o = beam.to_c()
        o.radii[1] = value
        refused(o, "radii")
        o = beam.to_c()
        o.segment_radii[0] = value
        refused(o, "segment_radii")
    for value in (np.nan, np.inf, -np.inf):
        o = beam.to_c()
        o.centres[0][2] = value
        refused(o, "centres")
    o = beam.to_c()
    o.radii[3] = np.nan              # what the object does not have is not read
    o.segment_radii[2] = -1.0
    assert L.mppi_set_held_object(h, C.byref(o)) == abi.MPPI_OK and f.held_object == beam
    f.update(am.huddled_state(), 0.0)
    assert f.update_info()["wait_timeouts"] == 0 and f.get_optimal_held_cost() > 0.0
    f.set_held_object(HS.tip())      # replaced between updates, also after the first
    f.set_held_object(None)
    assert f.held_object is None
    f.update(am.huddled_state(), 0.01)
    assert f.get_optimal_held_cost() == 0.0
    zero = beam.to_c()
    zero.count = 0
    assert L.mppi_set_held_object(h, C.byref(zero)) == abi.MPPI_OK and f.held_object is None     # count = 0: put down
    _invalid(lambda: f.set_held_object_avoidance(), word="before the first update")
    assert f.held_object_avoidance

    # a point-mass handle
    pm = am.Trajectory.create(am.point_mass_configuration(rollouts=64, horison=0.08, keep_best_rollouts=20), am.PointMassDynamics(), am.QuadraticCost())
    with pytest.raises(am.EngineError):
        pm.set_held_object_avoidance()
    assert not pm.held_object_avoidance
    with pytest.raises(am.EngineError):
        pm.set_held_object(beam)
    with pytest.raises(am.EngineError) as ei:
        pm.predicted_held_optimal()
    assert ei.value.status in (abi.MPPI_ERR_UNSUPPORTED, abi.MPPI_ERR_INVALID)


# ---- 8. the C++ surface ----------------------------------------------------------------------------

def test_cpp_held_object_surface_on_the_device(monkeypatch):
    _set_env(monkeypatch)
    cpp = os.path.join(REPO, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "held_object.mk"])
    out = subprocess.check_output([os.path.join(cpp, "build", "held_object"), "gpu"], timeout=300).decode()
    lines = [json.loads(l) for l in out.strip().split("\n")]
    assert lines[0] == {"cpu": "ok"}
    assert lines[1] == {"before_field": False, "object_before_avoidance": False}
    assert lines[2]["with_beam"] > 0.0 and lines[2]["obstacle_cost"] == lines[2]["with_beam"] and lines[2]["put_down"] == 0.0
    assert lines[2]["with_tip"] > 0.0 and lines[2]["rows"] is True and lines[2]["count5"] is False and lines[2]["late_enable"] is False
    # the object's cost: the same program's sphere and beam through the Python object
    d = am.PinocchioDynamicsObject.create(am.huddled_state(), link_positions=True)
    d.set_state(am.huddled_state(), 0.0)
    sphere = am.SphereObstacle((1.08, 0.66, 0.84), 0.05, mask=am.MASK_HELD)
    assert lines[3]["same"] and lines[3]["object_cost"] == d.held_object_cost(None, [sphere], 0.0, None, HS.beam())
