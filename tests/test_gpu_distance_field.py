"""Obstacle avoidance with a distance field (mppi_set_distance_field_avoidance) on the device against
the Python composition of field_reference.py: the field term in every launch plan of the rollouts, both
objectives, the tank, the simulated wrench, the separate cost kernel, the graph path, sharding, the two
device grids' alternation, a grid near the size limit, the device object, the refusals and the C++
surface.

The pattern is test_gpu_capsules.py's: three updates at time 0 from test_gpu_link_positions.py's three
states with its noise scaling, host-injected noise, helpers.py's bars.  The field is replaced between the
updates (field_sets.py): "clear" (F), "breach" (G), then "partial" (H); the folded filter() row of an
update is checked against the field of that update, which by then has been replaced - the two device
grids.  The reference keeps books on every sample it evaluates, and each run asserts from them
(test_distance_field_cpu.check_books) that nothing sat within 1e-6 of the barrier's branch discontinuity
or, in grid units, of the grid's boundary, that F stayed 0.02 m clear on the inverse branch, that G and H
took both branches, and that H had samples inside and outside its grid.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi

import capsule_sets as CS
import field_reference as FR
import field_sets as FS
import link_reference as LR
import obstacle_reference as OR
import wrench_reference as WR
from launch_shapes import by_name, horizon
from test_distance_field_cpu import MARGIN, check_books
from test_gpu_capsules import _check_books as _check_capsule_books
from test_gpu_link_positions import SHAPES, _assert_bars, _hip, _noise_scale, _record, _states
from test_gpu_obstacles import _close, _invalid, _set_env

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _handle(conf, cost, wrench=None, enable=True, config=None):
    dyn = am.FrankaRidgebackDynamics(link_positions=True, simulated_wrench=wrench)
    dev = am.Trajectory.create(conf, dyn, cost)
    assert dev is not None and dev.link_positions
    dev.set_obstacle_avoidance(config)
    dev.set_obstacle_capsules(CS.capsules())
    if enable:
        assert not dev.distance_field_avoidance
        dev.set_distance_field_avoidance()
        assert dev.distance_field_avoidance and dev.distance_field is None
    dev.set_noise_source(abi.MPPI_NOISE_HOST_INJECTED)
    return dyn, dev


def _print_books(tag, term):
    b = term.fbooks
    print("%s books: least margin %.3e, least v %.4f, %s, inside %d, outside %d, least distance to the grid's edge %.3e"
          % (tag, b.least_margin, b.least_v, sorted(b.branches), b.inside, b.outside, b.edge))


def _run(name, cost, fields, monkeypatch, plans=True, primitives=None, books=True):
    """test_gpu_capsules.py::_run on a field handle: fields[j] is set before update j, primitives[j]
    (a set and its reference time; none unless given) beside it."""
    _, S, H, keep, req, sw, first, pend = by_name(name)
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    table = am.constant_forecast(H)
    dyn, dev = _handle(conf, cost)
    assert dev.H == H and dev.R == S + 2
    dev.set_forecast(table)
    comp = FR.Composition(conf, dyn.model, cost, table, capsules=CS.capsules())
    states, scale = _states(), _noise_scale(H)
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance)) * scale
    U = np.zeros((H, dev.C))
    prev = None
    for j, (x, field) in enumerate(zip(states, fields)):
        tag = "%s upd %d" % (name, j)
        obstacles, t_ref = primitives[j] if primitives else ([], 0.0)
        dev.set_obstacles(obstacles, t_ref)
        dev.set_distance_field(field)
        assert dev.distance_field == field
        comp.field = field
        term = comp.set_obstacles(obstacles, t_ref)
        dev.inject_noise(rng.standard_normal((dev.noise_draws(0.0), dev.C)) * sd)
        dev.update(x, 0.0)
        info = dev.update_info()
        assert info["wait_timeouts"] == 0 and info["cooperative"] == 1, (tag, info)
        if plans:
            want = first if j == 0 else pend
            assert info["folded_filter"] == want[5] and info["objective_in_launch"] == want[6], (tag, info)
        if info["folded_filter"]:   # the previous update's filter() row: its own field, replaced since
            comp.term = prev
            ref = comp.rollout(states[j - 1], U)[0]
            comp.term = term
            _close(dev.debug_folded_cost(), ref, tag + " folded filter()")
        eps = dev.noise()
        J = comp.costs(x, U, eps)
        w, g, Un = LR.mppi_update(conf, J, eps, U)
        _assert_bars(tag, dev.costs(), J, dev.get_weights(), w, dev.get_optimal_rollout(), Un, H)
        U = dev.get_optimal_rollout()
        if books and field is not None:
            _print_books(tag, term)
            check_books(term, j, tag)
        if primitives and obstacles:   # set C: nothing near the branch discontinuity; clear on the inverse branch at the first state, as its own tests assert
            assert term.least_margin >= MARGIN, (tag, term.least_margin)
            if j == 0:
                _check_capsule_books(term, 0, H, tag)
        if not plans:
            ref, _, ob = comp.rollout(x, U)
            _close(dev.get_optimal_field_cost(), term.field_steps.sum(), tag + " optimal field cost")
            _close(dev.get_optimal_obstacle_cost(), ob.sum(), tag + " optimal obstacle cost")
            _close(dev.get_optimal_total_cost(), ref, tag + " optimal total")
        prev = term
    ref, sc, ob = comp.rollout(states[len(fields) - 1], U)
    _close(dev.get_optimal_total_cost(), ref, name + " optimal total")
    _close(dev.get_optimal_obstacle_cost(), ob.sum(), name + " optimal obstacle cost")
    _close(dev.get_optimal_field_cost(), comp.term.field_steps.sum(), name + " optimal field cost")
    if cost.descriptor().kind == abi.MPPI_COST_ASSISTED_MANIPULATION:
        _close(dev.get_optimal_terms()[1], sc.sum(), name + " self-collision total")
    return dev, comp


# ---- 1. parity against the composition, every launch plan ---------------------------------------

@pytest.mark.parametrize("name", SHAPES)
def test_update_against_the_composition(name, monkeypatch):
    _run(name, FS.objective(), FS.fgh(), monkeypatch)


def test_optimal_field_cost_after_every_update(monkeypatch):
    """The optimal rollout read after each update (filter() runs by itself): the field total against the
    reference's sum, and the obstacle cost, which on a field handle holds it too."""
    dev, comp = _run("r19_h33", FS.objective(), FS.fgh(), monkeypatch, plans=False)
    assert dev.get_optimal_field_cost() > 0.0 and dev.get_optimal_obstacle_cost() == dev.get_optimal_field_cost()   # no primitives


def test_primitives_beside_the_field(monkeypatch):
    """Set C's capsules, sphere and wall with the fields behind them: the term is the capsule term plus
    the field's."""
    c = (CS.set_c(), CS.T_REF_C)
    dev, comp = _run("r19_h33", FS.objective(), FS.fgh(), monkeypatch, plans=False, primitives=[c, c, c])
    assert dev.get_optimal_obstacle_cost() > dev.get_optimal_field_cost() > 0.0


# ---- 2. other objectives and modes --------------------------------------------------------------

def test_track_point(monkeypatch):
    _run("r19_h33", FS.objective("track_point"), FS.fgh(), monkeypatch)


def test_energy_tank(monkeypatch):
    _run("r19_h33", FS.objective(energy=True), FS.fgh(), monkeypatch)


def test_simulated_wrench_forecast(monkeypatch):
    """The pushed robot with the field term: test_gpu_capsules.py's wrench test on a field handle."""
    from test_gpu_simulated_wrench import TIMES, _assert_update, _state
    _, S, H, keep, req, sw, _, _ = by_name("r19_h33")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = FS.objective()
    table = WR.forecast_table(H)
    dyn, dev = _handle(conf, cost, wrench="forecast")
    dev.set_forecast(table)
    ref = FR.WrenchComposition(conf, dyn.model, cost, "forecast", table, capsules=CS.capsules())
    sd = np.sqrt(np.diag(conf.covariance))
    rng, shift, dt = np.random.default_rng(11), WR.Shift(), dev.get_time_step()
    prev = None
    for j, (t, field) in enumerate(zip(TIMES, FS.fgh_wrench())):   # (F with more room: these states push the arm 0.0003 m inside F's 0.02)
        tag = "wrench upd %d" % j
        x0 = _state(j)
        U_prev = dev.get_optimal_rollout()
        U_shift = WR.shifted(U_prev, shift(t, dt))
        dev.set_distance_field(field)
        term = ref.set_field(field)
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
        _print_books(tag, term)
        check_books(term, j, tag)
        prev = (term, x0, t)
    want, _, ob = ref.rollout(x0, dev.get_optimal_rollout(), TIMES[-1])
    _close(dev.get_optimal_total_cost(), want, "wrench optimal total")
    _close(dev.get_optimal_field_cost(), ref.term.field_steps.sum(), "wrench optimal field cost")


# ---- 3. paths ------------------------------------------------------------------------------------

def test_in_launch_objective_against_the_cost_kernel(monkeypatch):
    """The same inputs through the launch's own objective and through fr_step_cost_links_kernel<OB_TERM_FIELD>
    (MPPI_COSTS_IN_LAUNCH=0), r147_h64, test_gpu_capsules.py's structure: bit for bit (the two inline
    the same text of the term, whose arithmetic is rounded operation by operation)."""
    _, S, H, keep, req, sw, _, _ = by_name("r147_h64")
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = FS.objective()
    _set_env(monkeypatch, req, "")
    a = _handle(conf, cost)[1]
    _set_env(monkeypatch, req, "c")
    b = _handle(conf, cost)[1]
    rng = np.random.default_rng(4)
    sd = np.sqrt(np.diag(conf.covariance)) * _noise_scale(H)
    same = True
    for j, (x, field) in enumerate(zip(_states(), FS.fgh())):
        eps = rng.standard_normal((a.noise_draws(0.0), a.C)) * sd
        for t in (a, b):
            t.set_forecast(am.constant_forecast(H))
            t.set_distance_field(field)
            t.inject_noise(eps)
            t.update(x, 0.0)
            assert t.update_info()["wait_timeouts"] == 0
        assert a.update_info()["objective_in_launch"] == 1 and b.update_info()["objective_in_launch"] == 0
        same = same and np.array_equal(a.costs(), b.costs()) and np.array_equal(a.get_optimal_rollout(), b.get_optimal_rollout())
        _assert_bars("in-launch vs cost kernel upd %d" % j, a.costs(), b.costs(), a.get_weights(), b.get_weights(),
                     a.get_optimal_rollout(), b.get_optimal_rollout(), H)
    assert same, "the in-launch field objective and the cost kernel differ in some bit"


def _philox(conf, graph=0, field=True):
    t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=True), am.AssistedManipulation())
    assert t is not None
    t.set_obstacle_avoidance()
    t.set_obstacle_capsules(CS.capsules())
    if field:
        t.set_distance_field_avoidance()
    t.set_graph(graph)
    t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
    t.set_forecast(am.constant_forecast(t.H))
    return t


def _graph_fields():
    f, g, h = FS.fgh()
    return [f, g, h, g]


def test_graph_path(monkeypatch):
    """test_gpu_capsules.py::test_graph_path on a field handle: the field replaced and the time advancing
    between the replays, the graph's rollout nodes give the eager launches' bits - a replay sees the
    current grid through the table, which is launched ahead of the graph."""
    _set_env(monkeypatch, 0, "")
    conf = am.frankaridgeback_configuration(rollouts=1000, horison=0.64, keep_best_rollouts=20, threads=8)
    out = {}
    fields = _graph_fields()
    for graph in (0, 1):
        t = _philox(conf, graph)
        x = am.huddled_state()
        rec = []
        for j, tm in enumerate([0.0, 0.05, 0.07, 0.12]):
            if j == 2:
                x = x.copy()
                x[12 + 4] = 0.3
            t.set_distance_field(fields[j])
            t.update(x, tm)
            assert t.update_info()["wait_timeouts"] == 0
            rec.append(_record(t))
        out[graph] = (rec, t.graph_updates(), t.get_optimal_total_cost(), t.get_optimal_field_cost())
    assert out[0][1] == 0 and out[1][1] == 3, (out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3] and out[0][3] > 0.0
    for j, (a, b) in enumerate(zip(out[0][0], out[1][0])):
        for what, u, v in zip(("noise", "costs", "optimal", "weights"), a, b):
            np.testing.assert_array_equal(u, v, err_msg="update %d %s" % (j, what))
    # the field is live: the same handle without one gives other costs
    none = _philox(conf, 0)
    none.update(am.huddled_state(), 0.0)
    assert not np.array_equal(none.costs(), out[0][0][0][1])


def test_two_shards_equal_one_handle(monkeypatch):
    """Two phase-split shards against one handle at 128 x 32, every rank with the same field:
    test_gpu_capsules.py's structure and bars."""
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
    fields = _graph_fields()

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
            h.set_distance_field(fields[j])
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


# ---- 4. the two device grids ---------------------------------------------------------------------

def _pair(conf):
    a, b = _philox(conf), _philox(conf)
    return a, b


def test_buffer_alternation(monkeypatch):
    """Two sets between two updates (the second one counts, and both land in the grid that the last
    update's table does not name), and a clear followed by a set: handle `a` goes the long way, handle `b`
    sets each update's field once; every update gives the same bits, and so does the filter() row of
    every update, read after the field was replaced again."""
    _set_env(monkeypatch, 0, "")
    conf = am.frankaridgeback_configuration(rollouts=19, horison=horizon(33), keep_best_rollouts=5, threads=8)
    f, g, h = FS.fgh()
    a, b = _pair(conf)
    x = am.huddled_state()
    plan = [([f], f), ([h, g], g), ([None, h], h), ([g, f, None], None), ([f, None, g], g)]
    for j, (sets, last) in enumerate(plan):
        for s in sets:
            a.set_distance_field(s)
        b.set_distance_field(last)
        assert a.distance_field == last and b.distance_field == last
        for t in (a, b):
            t.update(x, 0.02 * j)
            assert t.update_info()["wait_timeouts"] == 0
        np.testing.assert_array_equal(a.costs(), b.costs(), err_msg="update %d" % j)
        np.testing.assert_array_equal(a.get_optimal_rollout(), b.get_optimal_rollout(), err_msg="update %d" % j)
        # the next field is in place before this update's filter() row is read
        a.set_distance_field(h if last is not h else f)
        a.set_distance_field(g if last is not g else f)
        assert a.get_optimal_field_cost() == b.get_optimal_field_cost() and a.get_optimal_total_cost() == b.get_optimal_total_cost()
        assert (b.get_optimal_field_cost() > 0.0) == (last is not None), j


def test_no_field_equals_a_capsule_handle(monkeypatch):
    """A field handle that never gets a field against a capsule handle on set C, D and the empty set, three
    updates: bit for bit (the term is skipped by a uniform branch on the table's grid pointer)."""
    _set_env(monkeypatch, 0, "")
    conf = am.frankaridgeback_configuration(rollouts=147, horison=horizon(20), keep_best_rollouts=20, threads=8)
    a, b = _philox(conf, field=True), _philox(conf, field=False)
    assert a.distance_field_avoidance and not b.distance_field_avoidance
    for j, (x, (obstacles, t_ref)) in enumerate(zip(_states(), CS.cde())):
        for t in (a, b):
            t.set_obstacles(obstacles, t_ref)
            t.update(x, 0.03 * j)
            assert t.update_info()["wait_timeouts"] == 0
        for u, v in zip(_record(a), _record(b)):
            np.testing.assert_array_equal(u, v, err_msg="update %d" % j)
        assert a.get_optimal_obstacle_cost() == b.get_optimal_obstacle_cost() and a.get_optimal_field_cost() == 0.0
    assert a.get_optimal_total_cost() == b.get_optimal_total_cost()


def test_large_awkward_grid(monkeypatch):
    """(255, 257, 250) samples of 0.01 m, 16.4 million values just under the 2^24 limit, filled from a
    plane: one update at r19_h33 against the composition, and the optimal field cost.  A transposed or
    overflowing index reads another value of the plane."""
    _, S, H, keep, req, sw, _, _ = by_name("r19_h33")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = FS.objective()
    dyn, dev = _handle(conf, cost)
    dev.set_forecast(am.constant_forecast(H))
    field = FS.plane()
    assert field.values.size == 255 * 257 * 250 <= abi.MPPI_DISTANCE_FIELD_MAX_VALUES
    dev.set_distance_field(field)
    comp = FR.Composition(conf, dyn.model, cost, am.constant_forecast(H), capsules=CS.capsules())
    term = comp.set_field(field)
    x = _states()[0]
    rng = np.random.default_rng(11)
    dev.inject_noise(rng.standard_normal((dev.noise_draws(0.0), dev.C)) * np.sqrt(np.diag(conf.covariance)))
    dev.update(x, 0.0)
    assert dev.update_info()["wait_timeouts"] == 0
    U = np.zeros((H, dev.C))
    eps = dev.noise()
    J = comp.costs(x, U, eps)
    w, g, Un = LR.mppi_update(conf, J, eps, U)
    _assert_bars("large grid", dev.costs(), J, dev.get_weights(), w, dev.get_optimal_rollout(), Un, H)
    _print_books("large grid", term)
    assert term.fbooks.least_margin >= MARGIN and term.fbooks.edge >= MARGIN and term.fbooks.inside > 0
    comp.rollout(x, dev.get_optimal_rollout())
    _close(dev.get_optimal_field_cost(), comp.term.field_steps.sum(), "large grid optimal field cost")


# ---- 5. the device object ------------------------------------------------------------------------

def test_device_object_field_cost(monkeypatch):
    """PinocchioDynamicsObject.distance_field_cost at huddled_state() against the scalar reference, 1e-12
    relative: a linear and a multilinear field on dyadic grids around the robot, unit by unit (each of the
    nine points and eight segments alone: the loop's choice of end points), every sample count, the
    fields of the tests, a grid that holds nothing of the robot (exactly 0), and the refusals."""
    monkeypatch.delenv("MPPI_LINK_POSITIONS", raising=False)
    model = am.FrankaRidgebackDynamics().model
    x = am.huddled_state()
    p = OR.robot_points(model, x[:12])
    obj = am.PinocchioDynamicsObject.create(x, link_positions=True)
    obj.set_state(x, 0.0)
    config = am.ObstacleAvoidance(limit=(0.01, 2.0, 1e8), radii=(0.7, 0.11, 0.12, 0.13, 0.1, 0.09, 0.08, 0.07, 0.06))
    caps = am.ObstacleCapsules((0.1, 0.05, 0.06, 0.07, 0.04, 0.05, 0.06, 0.03))

    def check(field, conf=None, cc=None, what=""):
        term = FR.Term(conf or am.ObstacleAvoidance(), cc or am.ObstacleCapsules(), [], 0.0, field)
        want = term.field_at(p)
        got = obj.distance_field_cost(conf, cc, field)
        assert abs(got - want) <= 1e-12 * max(abs(want), 1.0), (what, got, want)
        return term, got

    room = dict(origin=(-0.5, -0.25, -0.5), voxel=0.125, dims=(17, 13, 19))
    for fn in (lambda x, y, z: 2.0 * x - 3.0 * y + 0.5 * z + 1.0, lambda x, y, z: x * y * z + 0.25):
        values = am.DistanceField.from_function(fn, **room).values
        for u in range(17):
            mask = (1 << u) if u < 9 else am.mask_segment(u - 9)
            term, got = check(am.DistanceField(values, room["origin"], room["voxel"], mask=mask, segment_samples=3), config, caps, "unit %d" % u)
            assert term.fbooks.inside == (1 if u < 9 else 3) and term.fbooks.outside == 0 and term.fbooks.least_margin >= MARGIN
        for m in range(9):
            term, got = check(am.DistanceField(values, room["origin"], room["voxel"], segment_samples=m), config, caps, "m = %d" % m)
            assert term.fbooks.inside == 9 + 8 * m
    for field in FS.fgh():
        term, got = check(field, None, CS.capsules(), "the tests' field")
        assert got > 0.0 and term.fbooks.least_margin >= MARGIN and term.fbooks.edge >= MARGIN
    # a smooth field that reaches the saturated branch: true distances to a 0.12 m ball on the forearm's axis, so
    # the saturated samples' cells have eight different corners (G's and H's thresholded maps have eight equal ones)
    ball = am.DistanceField.from_function(lambda x, y, z: np.sqrt((x - 0.7106) ** 2 + (y - 0.7176) ** 2 + (z - 1.1857) ** 2) - 0.12,
                                          segment_samples=7, **FS.ROOM)
    for mask, want in ((FS.EVERYTHING, {"inverse", "saturated"}), (am.mask_segment(4), {"saturated"}), (am.mask_segment(3), {"inverse"})):
        term, got = check(am.DistanceField(ball.values, ball.origin, ball.voxel, mask=mask, segment_samples=7), None, CS.capsules(), "ball")
        assert term.fbooks.branches == want and term.fbooks.least_margin >= MARGIN, (mask, term.fbooks)   # (the forearm's seven samples are all inside the matter)
    away = am.DistanceField.from_function(lambda x, y, z: x - 100.0, (5.0, 5.0, 5.0), 0.5, (3, 4, 5))
    assert obj.distance_field_cost(None, None, away) == 0.0
    assert obj.distance_field_cost(None, None, am.DistanceField(FS.field_g().values, FS.ROOM["origin"], 0.05, mask=0)) == 0.0
    _invalid(lambda: obj.distance_field_cost(None, None, am.DistanceField(np.zeros((2, 2, 2)), (0, 0, 0), 0.0)), word="voxel")
    _invalid(lambda: obj.distance_field_cost(None, None, am.DistanceField(np.zeros((2, 2, 2)), (0, 0, 0), 0.1, segment_samples=9)), word="segment_samples")
    zero = am.PinocchioDynamicsObject.create(x)
    _invalid(lambda: zero.distance_field_cost(None, None, away), word="kinematic")


def _object_points(obj):
    """The nine points as the object holds them (what fr_object_term_kernel<OB_TERM_FIELD> reads), bit for bit."""
    return np.concatenate([obj.link_positions()[abi.MPPI_LINK_PIVOT:abi.MPPI_LINK_PIVOT + 8],
                           obj.get_end_effector_state_row()[None, abi.MPPI_EE_POSITION:abi.MPPI_EE_POSITION + 3]])


def _exact_origin(p, g, voxel):
    """An origin with (p_a - origin_a) * (1 / voxel) == g_a exactly on every axis (voxel a power of two), or None."""
    o = [float(p[a]) - g[a] * voxel for a in range(3)]
    return o if all((float(p[a]) - o[a]) * (1.0 / voxel) == g[a] for a in range(3)) else None


def test_device_object_by_hand_cases(monkeypatch):
    """test_distance_field_cpu.py's by-hand cases on the device, built around a point as the object holds it:
    the bottom faces, the top faces and the corner (n - 1, n - 1, n - 1), which are inside (the inclusive
    test, the last cell with f = 1), one ulp of g outside each face, which is exactly 0, and NaN.  The grid
    is linear in x, y and z with dyadic values that differ at every node, so on a face or the corner D is a
    node's or an edge's value and a cell taken one off shows.  Compared with == where the arithmetic is
    exact (0.0 outside, NaN), and at 1e-12 with the scalar reference, which decides inside and outside from
    the same two rounded operations, where the barrier's quotient follows."""
    monkeypatch.delenv("MPPI_LINK_POSITIONS", raising=False)
    x = am.huddled_state()
    obj = am.PinocchioDynamicsObject.create(x, link_positions=True)
    obj.set_state(x, 0.0)
    pts = _object_points(obj)
    dims, top = (5, 4, 3), (4, 3, 2)
    values = am.DistanceField.from_function(lambda x, y, z: 0.5 * x + 2.0 * y + 16.0 * z + 0.25, (0.0, 0.0, 0.0), 1.0, dims).values
    config = am.ObstacleAvoidance(limit=(0.0, 1.0, 1e10), radii=(0.125,) * 9)

    def cost(i, origin, voxel):
        field = am.DistanceField(values, origin, voxel, mask=1 << i, segment_samples=0)
        term = FR.Term(config, am.ObstacleCapsules(), [], 0.0, field)
        return obj.distance_field_cost(config, None, field), term.field_at(pts), term.fbooks

    seen = 0
    for i in (0, 4, 8):
        p = pts[i]
        inside_cases = [(0.0, 0.0, 0.0), tuple(float(t) for t in top)]                       # the first node, the last corner
        for a in range(3):
            lo, hi = [1.5, 1.25, 0.5], [1.5, 1.25, 0.5]
            lo[a], hi[a] = 0.0, float(top[a])
            inside_cases += [tuple(lo), tuple(hi)]                                          # each bottom face, each top face
        for g in inside_cases:
            found = [(v, o) for v in (0.5, 0.25, 0.125, 0.0625) for o in [_exact_origin(p, g, v)] if o]
            assert found, ("no exact origin", i, g)
            voxel, origin = found[0]
            got, want, books = cost(i, origin, voxel)
            assert books.inside == 1 and books.edge == 0.0, (i, g, books)                   # on the boundary, inside
            D = 0.5 * g[0] + 2.0 * g[1] + 16.0 * g[2] + 0.25                                # exact: the interpolant of a linear dyadic field
            assert want == 1.0 / (D - 0.125) and got != 0.0 and abs(got - want) <= 1e-12 * want, (i, g, got, want)
            seen += 1
            # the least step outside that face: move the origin by ulps of the subtraction until the reference's g leaves [0, n - 1]
            for a in range(3):
                if g[a] not in (0.0, float(top[a])):
                    continue
                o, out = list(origin), False
                ulp = float(np.spacing(max(abs(float(p[a])), abs(origin[a]))))               # (a smaller step is lost in p - origin)
                for k in range(1, 9):
                    o[a] = origin[a] + (k * ulp if g[a] == 0.0 else -k * ulp)
                    D1, edge = FR.sample(am.DistanceField(values, o, voxel), p)
                    if D1 is None:
                        out = True
                        break
                assert out and edge < 1e-9, (i, g, a, edge)
                got, want, books = cost(i, o, voxel)
                assert want == 0.0 and books.outside == 1 and got == 0.0, (i, g, a, got)      # exactly 0
    assert seen == 3 * 8
    # NaN: a NaN arm joint makes the links behind it NaN; their contribution, and the sum, is NaN
    bad = x.copy()
    bad[5] = np.nan
    obj.set_state(bad, 0.0)
    nanpts = _object_points(obj)
    assert np.isnan(nanpts[8]).any() and not np.isnan(nanpts[0]).any()
    field = am.DistanceField(values, (-1.0, -1.0, -1.0), 1.0, mask=1 << 8, segment_samples=0)
    assert np.isnan(obj.distance_field_cost(config, None, field))
    base = am.DistanceField(values, [float(nanpts[0][a]) - 0.5 for a in range(3)], 1.0, mask=1, segment_samples=0)
    got = obj.distance_field_cost(config, None, base)                                       # the base point is finite and inside
    assert got == got and got > 0.0
    assert np.isnan(obj.distance_field_cost(config, None, am.DistanceField(values, base.origin, 1.0, mask=0x101, segment_samples=0)))
    # a grid 1e308 m away: g overflows nothing and is outside, exactly 0
    far = am.DistanceField(values, (1e308, 0.0, 0.0), 1.0, mask=1, segment_samples=0)
    assert obj.distance_field_cost(config, None, far) == 0.0


# ---- 6. validation -------------------------------------------------------------------------------

def test_validation(monkeypatch):
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=17, horison=0.05, keep_best_rollouts=5)
    mk = lambda: am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=True), am.AssistedManipulation())   # noqa: E731
    ok = FS.field_h()

    # before capsules are enabled, without field avoidance, and after the first update
    t = mk()
    assert not t.distance_field_avoidance
    _invalid(lambda: t.set_distance_field_avoidance(), word="capsules")
    t.set_obstacle_avoidance()
    _invalid(lambda: t.set_distance_field_avoidance(), word="capsules")
    t.set_obstacle_capsules()
    _invalid(lambda: t.set_distance_field(ok), word="not enabled")
    _invalid(lambda: t.distance_field, word="not enabled")
    with pytest.raises(am.EngineError):
        t.get_optimal_field_cost()
    t.update(am.huddled_state(), 0.0)
    _invalid(lambda: t.set_distance_field_avoidance(), word="before the first update")
    assert not t.distance_field_avoidance

    f = mk()
    f.set_obstacle_avoidance()
    f.set_obstacle_capsules()
    f.set_distance_field_avoidance()
    assert f.distance_field is None and f.get_optimal_field_cost() == 0.0
    f.set_distance_field(ok)
    assert f.distance_field == ok
    v = ok.values
    mkf = lambda values=v, origin=(0.5, 0.5, 0.9), voxel=0.05, **kw: am.DistanceField(values, origin, voxel, **kw)   # noqa: E731
    for bad, word in ((mkf(np.zeros((1, 4, 4))), "dims"), (mkf(np.zeros((4, 513, 2))), "dims"), (mkf(np.zeros((4, 2, 1))), "dims"),
                      (mkf(np.zeros((512, 512, 65), dtype=np.float32)), "2^24"),
                      (mkf(voxel=0.0), "voxel"), (mkf(voxel=-0.05), "voxel"), (mkf(voxel=np.nan), "voxel"), (mkf(voxel=np.inf), "voxel"),
                      (mkf(origin=(0.0, np.nan, 0.0)), "origin"), (mkf(origin=(np.inf, 0.0, 0.0)), "origin"),
                      (mkf(segment_samples=9), "segment_samples"), (mkf(segment_samples=-1), "segment_samples")):
        _invalid(lambda: f.set_distance_field(bad), word=word)
    for bit in list(range(9, 16)) + list(range(24, 32)):
        _invalid(lambda: f.set_distance_field(mkf(mask=(1 << bit) | 1)), word="mask")
    for value in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[12, 10, 8] = value     # the last one
        _invalid(lambda: f.set_distance_field(mkf(w)), word="finite")
    assert f.distance_field == ok   # the refused calls left the field in place
    f.set_distance_field(mkf(np.full((512, 512, 64), 1.0, dtype=np.float32), origin=(-10.0, -10.0, -1.0), voxel=0.04, segment_samples=0, mask=0))   # 2^24 exactly
    f.update(am.huddled_state(), 0.0)
    assert f.update_info()["wait_timeouts"] == 0 and f.get_optimal_field_cost() == 0.0
    f.set_distance_field(FS.field_g())
    f.update(am.huddled_state(), 0.01)
    assert f.update_info()["wait_timeouts"] == 0 and f.get_optimal_field_cost() > 0.0
    f.set_distance_field(None)
    assert f.distance_field is None
    f.update(am.huddled_state(), 0.02)
    assert f.get_optimal_field_cost() == 0.0
    _invalid(lambda: f.set_distance_field_avoidance(), word="before the first update")
    assert f.distance_field_avoidance


# ---- 7. the C++ surface --------------------------------------------------------------------------

def test_cpp_distance_field_surface_on_the_device(monkeypatch):
    _set_env(monkeypatch)
    cpp = os.path.join(REPO, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "distance_field.mk"])
    out = subprocess.check_output([os.path.join(cpp, "build", "distance_field"), "gpu"], timeout=300).decode()
    lines = [json.loads(l) for l in out.strip().split("\n")]
    assert lines[0] == {"cpu": "ok"}
    assert lines[1] == {"before_capsules": False, "field_before_avoidance": False}
    assert lines[2]["with_field"] > 0.0 and lines[2]["obstacle_cost"] == lines[2]["with_field"] and lines[2]["cleared"] == 0.0
    assert lines[2]["late_enable"] is False
    # the object's cost: the same program's field through the Python object
    field = am.DistanceField.from_function(lambda x, y, z: np.sqrt((x - 0.7106) ** 2 + (y - 0.7176) ** 2 + (z - 1.1857) ** 2) - 0.03,
                                           mask=CS.ARM, segment_samples=3, **FS.ROOM)
    d = am.PinocchioDynamicsObject.create(am.huddled_state(), link_positions=True)
    d.set_state(am.huddled_state(), 0.0)
    assert lines[3]["same"] and lines[3]["object_cost"] == d.distance_field_cost(None, None, field)
