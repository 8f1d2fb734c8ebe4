"""The kinematic link-position model (mppi_set_link_positions) on the device against the CPU
composition of link_reference.py: the live self-collision term in every launch plan of the rollouts
(the x kernel with its relay and folded filter(), the four-wave and one-wave kernels, the separate
cost kernel), the filter() rows, the per-term totals, the device object and get_cost, the graph
path and sharding - and the zero mode left bit for bit as it was.

The oracle knows only the reference's stub, so every update check first runs the scaffold: the
composition with the stub's constant against an OracleTrajectory that has the constant on, at
helpers.py's bars.  Only then is the same composition, with the term on the numpy forward kinematics
(pinned by the oracle in test_link_positions_cpu.py), the reference of the kinematic mode - at the
same bars: COST_RTOL and the COST_DFRAC allowance on the costs, WEIGHT_ATOL, CONTROL_ATOL.

All three updates of a handle run at time 0, so nothing shifts: U*_shifted is the previous
get_optimal_rollout() and eps is noise() read after the update.  The state changes between updates.
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
from oracle import oracle as O

import link_reference as LR
from helpers import CONTROL_ATOL, COST_RTOL, WEIGHT_ATOL, cost_errors
from launch_shapes import by_name, horizon
from test_link_positions_cpu import configurations

pytestmark = pytest.mark.gpu

SHAPES = ["r19_h33", "r147_h20", "r48_h33", "r10_h33", "r20_h33", "r19_h129", "r19_h1", "r147_h64_c"]
ARM_RADII = {"default": None, "arm004": 0.04}
SWITCH_ENV = {"c": "MPPI_COSTS_IN_LAUNCH", "h": "MPPI_HANDOVER", "s": "MPPI_SPLIT"}
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise_scale(H):
    """Injected noise as a fraction of the configured deviations: small enough over the longer
    horizons that the arm's spheres stay clear with the 0.04 m radii (three numpy updates of the
    composition: the least clearance stays the fixed 0.008 m of PANDA_LINK5 - PANDA_LINK7)."""
    return 1.0 if H <= 33 else (0.3 if H <= 64 else 0.1)


def _set_env(monkeypatch, req, sw):
    for v in ("MPPI_RELAY_K", "MPPI_TAIL_DRAWS", "MPPI_DRAW_AHEAD", "MPPI_LINK_POSITIONS", "MPPI_GRAPH") + tuple(SWITCH_ENV.values()):
        monkeypatch.delenv(v, raising=False)
    if req:
        monkeypatch.setenv("MPPI_RELAY_K", str(req))
    for s in sw:
        monkeypatch.setenv(SWITCH_ENV[s], "0")


def _cost(objective, arm_radius=None):
    if objective == "track_point":
        cost = am.TrackPoint()
        cost.configuration.enable_self_collision_avoidance = 1
    else:
        cost = am.AssistedManipulation()
    if arm_radius is not None:
        for i in range(1, 8):
            cost.configuration.self_collision_radii[i] = arm_radius
    return cost


def _states(n=3):
    out, x = [], am.huddled_state()
    for j in range(n):
        x = x.copy()
        x[3 + j] += 0.03
        x[12 + 4 + j] = 0.1 * (j + 1)
        out.append(x)
    return out


def _assert_bars(tag, Jd, Jr, wd, wr, Ud, Ur, H):
    assert np.array_equal(np.isnan(Jd), np.isnan(Jr)), tag + " NaN pattern"
    rel, dfrac, sfrac, worst = cost_errors(Jd, Jr, H)
    print("%s: cost rel err %.3e, err / Delta %.3e, (J - Jmin) err / Delta %.3e, %.3f of the allowance" % (tag, rel, dfrac, sfrac, worst))
    assert rel <= COST_RTOL, "%s cost rel err %.3e" % (tag, rel)
    ok = ~np.isnan(Jr)
    if ok.sum() > 1 and Jr[ok].max() - Jr[ok].min() >= 1e-6:
        assert worst <= 1.0, "%s cost err / Delta %.3e, (J - Jmin) err / Delta %.3e: %.2f x the allowance" % (tag, dfrac, sfrac, worst)
    assert int(np.nanargmin(Jd)) == int(np.nanargmin(Jr)), tag + " argmin"
    if wd is not None and wr is not None:   # (None: mppi_update's early return, max - min < 1e-6 - one step: every cost is x0's)
        np.testing.assert_allclose(wd, wr, rtol=0, atol=WEIGHT_ATOL, err_msg=tag + " weights")
    np.testing.assert_allclose(Ud, Ur, rtol=0, atol=CONTROL_ATOL, err_msg=tag + " U*")


def _scaffold(conf, dyn, cost, table, states, scale, tag):
    """Zero mode, CPU against CPU: the composition with the stub's constant reproduces the oracle."""
    cc, keepalive = conf.to_c()
    orc = O.OracleTrajectory(cc, dyn.descriptor(), cost.descriptor(), scalar=0, mode=0)
    orc.set_forecast(table)
    comp = LR.Composition(conf, dyn.model, cost, "zero", table)
    rng = np.random.default_rng(7)
    sd = np.sqrt(np.diag(conf.covariance)) * scale
    U = np.zeros((orc.H, orc.C))
    for j, x in enumerate(states):
        orc.inject_noise(rng.standard_normal((orc.noise_draws(0.0), orc.C)) * sd)
        orc.update(x, 0.0)
        eps = orc.noise()
        J = comp.costs(x, U, eps)
        w, g, Un = LR.mppi_update(conf, J, eps, U)
        _assert_bars("%s scaffold upd %d" % (tag, j), J, orc.costs(), w, orc.weights(), Un, orc.optimal_control(), orc.H)
        oc = orc.optimal_cost()
        assert abs(comp.rollout(x, orc.optimal_control())[0] - oc) <= COST_RTOL * max(abs(oc), 1.0), tag
        U = orc.optimal_control()


def _kinematic_run(name, objective, arm_radius, monkeypatch):
    _, S, H, keep, req, sw, first, pend = by_name(name)
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost = _cost(objective, arm_radius)
    table = am.constant_forecast(H)
    states, scale = _states(), _noise_scale(H)
    tag = "%s %s %s" % (name, objective, "default" if arm_radius is None else "arm %.2f" % arm_radius)
    _scaffold(conf, am.FrankaRidgebackDynamics(), cost, table, states, scale, tag)

    dyn = am.FrankaRidgebackDynamics(link_positions=True)
    dev = am.Trajectory.create(conf, dyn, cost)
    assert dev is not None and dev.H == H and dev.R == S + 2 and dev.link_positions
    dev.set_noise_source(abi.MPPI_NOISE_HOST_INJECTED)
    dev.set_forecast(table)
    comp = LR.Composition(conf, dyn.model, cost, "kinematic", table)
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance)) * scale
    U = np.zeros((H, dev.C))
    for j, x in enumerate(states):
        dev.inject_noise(rng.standard_normal((dev.noise_draws(0.0), dev.C)) * sd)
        dev.update(x, 0.0)
        info = dev.update_info()
        want = first if j == 0 else pend
        assert info["wait_timeouts"] == 0 and info["cooperative"] == 1, (tag, info)
        assert info["folded_filter"] == want[5] and info["objective_in_launch"] == want[6], (tag, j, info)
        if info["folded_filter"]:   # the previous update's filter() row, before any optimal-cost read
            ref = comp.rollout(states[j - 1], U)[0]
            got = dev.debug_folded_cost()
            assert abs(got - ref) <= COST_RTOL * max(abs(ref), 1.0), (tag, j, got, ref)
        eps = dev.noise()
        J = comp.costs(x, U, eps)
        w, g, Un = LR.mppi_update(conf, J, eps, U)
        _assert_bars("%s upd %d" % (tag, j), dev.costs(), J, dev.get_weights(), w, dev.get_optimal_rollout(), Un, H)
        U = dev.get_optimal_rollout()   # U*_prev of the next update (nothing shifts at one time)
    ref, terms = comp.rollout(states[-1], U)
    got = dev.get_optimal_total_cost()
    assert abs(got - ref) <= COST_RTOL * max(abs(ref), 1.0), (tag, got, ref)
    if objective == "am":   # the optimal rollout's real self-collision total
        t1 = dev.get_optimal_terms()[1]
        assert abs(t1 - terms.sum()) <= COST_RTOL * max(abs(terms.sum()), 1.0), (tag, t1, terms.sum())
    if arm_radius is not None:   # the barrier's inverse branch carried the whole term
        assert comp.least_clearance > 0.0, (tag, comp.least_clearance)
    else:                        # PANDA_LINK5 - PANDA_LINK7 sit inside their radii: the saturated branch
        assert comp.least_clearance < 0.0, (tag, comp.least_clearance)


@pytest.mark.parametrize("radii", list(ARM_RADII))
@pytest.mark.parametrize("name", SHAPES)
def test_kinematic_update_against_the_composition(name, radii, monkeypatch):
    _kinematic_run(name, "am", ARM_RADII[radii], monkeypatch)


def test_track_point_kinematic_update(monkeypatch):
    _kinematic_run("r19_h33", "track_point", None, monkeypatch)


def test_device_object_link_positions(monkeypatch):
    """link_positions() against numpy at the 24 configurations, the one-step lag after a step, zeros
    in the zero mode, and get_cost in both modes for both objectives on the cached positions."""
    monkeypatch.delenv("MPPI_LINK_POSITIONS", raising=False)
    model = am.FrankaRidgebackDynamics().model
    x = am.huddled_state()
    kin = am.PinocchioDynamicsObject.create(x, link_positions=True)
    zero = am.PinocchioDynamicsObject.create(x)
    for q in configurations():
        x[:12] = q
        kin.set_state(x, 0.0)
        zero.set_state(x, 0.0)
        np.testing.assert_allclose(kin.link_positions(), LR.fk_links(model, q), rtol=0, atol=1e-12)
        assert np.all(zero.link_positions() == 0.0) and zero.link_positions().shape == (13, 3)
    u = np.array([0.2, -0.1, 0.3, 5.0, -4.0, 3.0, -2.0, 1.0, 2.0, -3.0, 0.0, 0.0])
    x = am.huddled_state()
    kin.set_state(x, 0.0)
    zero.set_state(x, 0.0)
    xn = kin.step(u, 0.01)
    zero.step(u, 0.01)
    assert np.abs(xn[:12] - x[:12]).max() > 1e-4   # the state moved; the cached positions did not
    np.testing.assert_allclose(kin.link_positions(), LR.fk_links(model, x[:12]), rtol=0, atol=1e-12)
    links = kin.link_positions()
    for objective in ("am", "track_point"):
        for arm_radius in (None, 0.04):
            cost = _cost(objective, arm_radius)
            c = cost.configuration
            tp = objective == "track_point"
            radii = [float(r) for r in c.self_collision_radii]
            live = LR.self_collision(c.self_collision_limit, radii, links, tp)[0]
            stub = LR.stub_constant(c.self_collision_limit, radii, tp)
            bare = LR.Composition(am.frankaridgeback_configuration(), model, cost, "off").bare
            base = am.evaluate_cost(bare, zero, xn)[0]
            for obj, term in ((kin, live), (zero, stub)):
                total, terms = am.evaluate_cost(cost, obj, xn)
                assert abs(total - (base + term)) <= COST_RTOL * max(abs(base + term), 1.0), (objective, arm_radius, total, base, term)
                if not tp:   # the barrier quotient's ~1e-15 (fr_cost_terms.hpp fquot) over the 20 pairs
                    assert abs(terms[1] - term) <= 64e-15 * max(abs(term), 1.0), (objective, arm_radius, terms[1], term)
    kin.set_link_positions(abi.MPPI_LINK_POSITIONS_ZERO)
    assert np.all(kin.link_positions() == 0.0)
    with pytest.raises(EngineError):
        kin.set_link_positions(2)


def _philox(conf, link_positions, graph=0):
    t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=link_positions), am.AssistedManipulation())
    assert t is not None
    t.set_graph(graph)
    t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
    t.set_forecast(am.constant_forecast(t.H))
    return t


def _record(t):
    return (t.noise().copy(), t.costs().copy(), t.get_optimal_rollout().copy(), t.get_weights().copy())


def test_graph_path_kinematic(monkeypatch):
    """1000 x 64 in the kinematic mode: the hipGraph path recognises the link-position rollout
    kernels and gives the eager launches' bits.  The first update of a handle is never a graph
    update (nothing is drawn ahead and no filter() is pending yet), so it runs first; the three
    updates after it must all be counted by graph_updates."""
    _set_env(monkeypatch, 0, "")
    conf = am.frankaridgeback_configuration(rollouts=1000, horison=0.64, keep_best_rollouts=20, threads=8)
    out = {}
    for graph in (0, 1):
        t = _philox(conf, True, graph)
        x = am.huddled_state()
        rec = []
        for j, tm in enumerate([0.0, 0.05, 0.07, 0.12]):
            if j == 2:
                x = x.copy()
                x[12 + 4] = 0.3
            t.update(x, tm)
            assert t.update_info()["wait_timeouts"] == 0
            rec.append(_record(t))
        out[graph] = (rec, t.graph_updates(), t.get_optimal_total_cost())
    assert out[0][1] == 0 and out[1][1] == 3, (out[0][1], out[1][1])
    assert out[0][2] == out[1][2]
    for j, (a, b) in enumerate(zip(out[0][0], out[1][0])):
        for what, u, v in zip(("noise", "costs", "optimal", "weights"), a, b):
            np.testing.assert_array_equal(u, v, err_msg="update %d %s" % (j, what))
    zero = _philox(conf, False)   # and the term is live: the costs are not the zero mode's
    zero.update(am.huddled_state(), 0.0)
    assert not np.array_equal(zero.costs(), out[0][0][0][1])


def _hip():
    L = C.CDLL("libamdhip64.so.7")
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipDeviceSynchronize.argtypes = []
    return L


def test_two_shards_kinematic_equal_one_handle(monkeypatch):
    """Two phase-split shards in the kinematic mode (every rank sets the mode) against one handle, at
    r147_h20: test_gpu_scale.py's pattern and bars."""
    _, S, H, keep, req, sw, _, _ = by_name("r147_h20")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    world = 2
    single, shards = _philox(conf, True), [_philox(conf, True) for _ in range(world)]
    for r, sh in enumerate(shards):
        sh.set_shard(world, r)
        assert sh.link_positions
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
        for sh in shards:
            cs = sh.costs()
            if j == 0:
                np.testing.assert_array_equal(cs, cu)
            assert np.all(np.abs(cs - cu) <= 1e-11 * (delta + np.abs(cu)))
            assert np.max(np.abs(sh.get_optimal_rollout() - single.get_optimal_rollout())) <= 1e-12
            assert np.max(np.abs(sh.get_weights() - single.get_weights())) <= 3e-15
            assert sh.argmin() == single.argmin()


def test_zero_mode_untouched(monkeypatch):
    """set_link_positions(0) against a handle that never called it: costs, weights and U* bit for bit
    over three updates at r147_h20; the mode is fixed once an update has run; a point mass has none."""
    _, S, H, keep, req, sw, _, _ = by_name("r147_h20")
    _set_env(monkeypatch, req, sw)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    plain, zero = _philox(conf, None), _philox(conf, False)
    assert not plain.link_positions and not zero.link_positions
    x = am.huddled_state()
    for j in range(3):
        for t in (plain, zero):
            t.update(x, 0.05 * j)
        for what, u, v in zip(("noise", "costs", "optimal", "weights"), _record(plain), _record(zero)):
            np.testing.assert_array_equal(u, v, err_msg="update %d %s" % (j, what))
    assert plain.get_optimal_total_cost() == zero.get_optimal_total_cost()
    for t in (plain, zero):
        with pytest.raises(EngineError) as e:
            t.set_link_positions(abi.MPPI_LINK_POSITIONS_KINEMATIC)
        assert e.value.status == abi.MPPI_ERR_INVALID
    fresh = _philox(conf, None)
    with pytest.raises(EngineError) as e:
        fresh.set_link_positions(2)
    assert e.value.status == abi.MPPI_ERR_INVALID
    pm = am.Trajectory.create(am.point_mass_configuration(rollouts=64), am.PointMassDynamics(), am.QuadraticCost())
    with pytest.raises(EngineError) as e:
        pm.set_link_positions(abi.MPPI_LINK_POSITIONS_KINEMATIC)
    assert e.value.status == abi.MPPI_ERR_UNSUPPORTED and not pm.link_positions


def test_environment_switch(monkeypatch):
    """MPPI_LINK_POSITIONS=1: new handles and dynamics objects start in the kinematic mode; anything
    but 0 or 1 is refused with a message."""
    conf = am.frankaridgeback_configuration(rollouts=17, horison=0.05, keep_best_rollouts=5)
    mk = lambda: am.Trajectory.create(conf, am.FrankaRidgebackDynamics(), am.AssistedManipulation())
    monkeypatch.setenv("MPPI_LINK_POSITIONS", "1")
    assert mk().link_positions
    obj = am.PinocchioDynamicsObject.create(am.huddled_state())
    assert np.abs(obj.link_positions()).max() > 0.1
    monkeypatch.setenv("MPPI_LINK_POSITIONS", "0")
    assert not mk().link_positions
    for bad in ("", "2", "10", "1 ", "yes"):
        monkeypatch.setenv("MPPI_LINK_POSITIONS", bad)
        assert mk() is None
        assert "MPPI_LINK_POSITIONS" in am._lib.load().mppi_last_error(None).decode()
        with pytest.raises(EngineError):
            am.PinocchioDynamicsObject.create(am.huddled_state())


def test_cpp_link_surface_on_the_device(monkeypatch):
    """get_link_position equals the C-ABI's rows in both models, and Configuration::link_positions
    reaches the handle."""
    monkeypatch.delenv("MPPI_LINK_POSITIONS", raising=False)
    cpp = os.path.join(REPO, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "link_positions.mk"])
    out = subprocess.check_output([os.path.join(cpp, "build", "link_positions"), "gpu"], timeout=300).decode()
    lines = [json.loads(l) for l in out.strip().split("\n")]
    assert lines[0] == {"cpu": "ok"}
    assert lines[1]["mode"] == 0 and lines[1]["same"] and lines[1]["zero"]
    assert lines[2]["mode"] == 1 and lines[2]["same"] and not lines[2]["zero"]
    d = am.PinocchioDynamicsObject.create(am.huddled_state(), link_positions=True)
    d.set_state(am.huddled_state(), 0.0)
    d.step(np.array([(5.0 - i) if 3 <= i < 10 else 0.1 for i in range(12)]), 0.01)
    assert lines[2]["panda_link7"] == list(d.link_positions()[abi.MPPI_LINK_PANDA_LINK7])
    assert lines[3] == {"configured": 0, "handle": 0} and lines[4] == {"configured": 1, "handle": 1}
