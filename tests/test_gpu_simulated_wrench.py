"""The simulated end-effector wrench on the device (mppi_set_simulated_wrench, mppi_dynamics_add_
end_effector_simulated_wrench) against the CPU composition of wrench_reference.py, which
test_simulated_wrench_cpu.py pins to the oracle: the device object, the rollouts' states in every
launch plan (read through the predicted trajectories, which read the launches' step records), the
update (costs, argmin, weights, gradient, U*), the tank, TrackPoint, the link-position objective
beside it, shards, the graph path, the errors - and the mode off left bit for bit as it was.

The fixture wrench is W0 = (2, -1, 0.5, 0.1, -0.2, 0.05): STATE mode reads it from x[24:30] of the
update's state (scaled by 1 + j / 4 in update j, so that the folded filter() row of update j - 1 is
seen to take its own update's rows), FORECAST mode reads row k = W0 (1 + k / H) of the table.
Three updates with injected noise at times 0, 2 dt, 2.5 dt: shifts of 0, 2 and 0 steps.

Bars of the states: ten times the worst error measured for the case on an MI355X, relative to
max(1, |x|), never above test_gpu_predicted.py's caps 1e-8 (q) / 1e-7 (qd) - three orders above the
2e-12 / 1.3e-11 by which the oracle's own two operation orders differ under W0 over 32 steps.
MEASURED holds the figures.  The update is held to helpers.py's bars.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi
from oracle import oracle as O

import link_reference as LR
import wrench_reference as WR
from helpers import CONTROL_ATOL, COST_RTOL, WEIGHT_ATOL, cost_errors
from launch_shapes import TIME_STEP, by_name, horizon

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMES = [0.0, 2 * TIME_STEP, 2.5 * TIME_STEP]
EPS = np.finfo(np.float64).eps
CAPS = (1e-8, 1e-7)   # q, qd
MODES = {"state": abi.MPPI_SIMULATED_WRENCH_STATE, "forecast": abi.MPPI_SIMULATED_WRENCH_FORECAST}
SHAPES = ["r20_h33", "r48_h33", "r10_h33", "r147_h64", "r19_h2", "r3_h33"]
# the object's bars: test_gpu_dynamics.py's
STATE_RTOL, VEL_RTOL, ACC_RTOL = 1e-10, 1e-9, 1e-8

# case -> worst (q, qd) error against the composed reference, relative to max(1, |x|), as measured on
# an MI355X (the tank: (q, qd, E)); the bars are ten times these
MEASURED = {
    "r20_h33": (2.787e-12, 2.342e-11),
    "r48_h33": (5.249e-12, 2.627e-11),
    "r10_h33": (1.072e-12, 4.805e-12),
    "r147_h64": (1.362e-11, 9.972e-11),
    "r19_h2": (5.699e-15, 1.801e-13),
    "r3_h33": (1.783e-13, 9.425e-13),
    "tank": (4.009e-12, 1.651e-11, 5.953e-13),
    "track_point": (1.585e-12, 8.687e-12),
    "links": (3.893e-12, 2.767e-11),
    "shards": (3.423e-12, 1.364e-11),
}
STATS = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for case, v in sorted(STATS.items()):
        print("\nsimulated wrench %-14s worst: %s" % (case, ", ".join("%s %.3e" % kv for kv in sorted(v.items()))))


def _note(case, **figures):
    s = STATS.setdefault(case, {})
    for k, v in figures.items():
        s[k] = max(s.get(k, 0.0), float(v))


def _bars(case):
    return tuple(min(c, max(10 * v, 10 * EPS)) for v, c in zip(MEASURED[case][:2], CAPS))


def _set_env(monkeypatch, req=0):
    for v in ("MPPI_RELAY_K", "MPPI_TAIL_DRAWS", "MPPI_DRAW_AHEAD", "MPPI_LINK_POSITIONS", "MPPI_GRAPH", "MPPI_SIMULATED_WRENCH",
              "MPPI_COSTS_IN_LAUNCH", "MPPI_HANDOVER", "MPPI_SPLIT"):
        monkeypatch.delenv(v, raising=False)
    if req:
        monkeypatch.setenv("MPPI_RELAY_K", str(req))


def _state(j=0):
    """The update's state: huddled, the arm moving, W0 (1 + j / 4) in the wrench slots."""
    x = am.huddled_state()
    x[12 + 3:12 + 10] = np.linspace(-0.2, 0.2, 7)
    x[24:30] = WR.W0 * (1.0 + j / 4.0)
    return x


def _handle(conf, mode, cost, table, links=None):
    dyn = am.FrankaRidgebackDynamics(simulated_wrench=mode, link_positions=links)
    dev = am.Trajectory.create(conf, dyn, cost)
    assert dev is not None
    dev.set_noise_source(abi.MPPI_NOISE_HOST_INJECTED)
    dev.set_forecast(table)
    return dyn, dev


def _errors(dev_rows, ref_states):
    eq = np.abs(dev_rows[..., :12] - ref_states[..., :12]) / np.maximum(1.0, np.abs(ref_states[..., :12]))
    ev = np.abs(dev_rows[..., 12:24] - ref_states[..., 12:24]) / np.maximum(1.0, np.abs(ref_states[..., 12:24]))
    return float(eq.max()), float(ev.max())


def _check_own(raw, x0, dt, tag):
    """Row 0 is x0 bit for bit, and the Euler identity of DESIGN section 2 on every row."""
    raw = raw.reshape((-1,) + raw.shape[-2:])
    q, qd = raw[..., :12], raw[..., 12:24]
    assert np.isfinite(raw[..., :24]).all(), tag
    N = raw.shape[0]
    assert np.array_equal(q[:, 0], np.broadcast_to(x0[:12], (N, 12))) and np.array_equal(qd[:, 0], np.broadcast_to(x0[12:24], (N, 12))), \
        tag + " row 0 is x0"
    if raw.shape[1] > 1:
        lhs = np.abs(q[:, 1:] - (q[:, :-1] + qd[:, 1:] * dt))
        rhs = 4 * EPS * np.maximum(1.0, np.maximum(np.abs(q[:, 1:]), np.abs(q[:, :-1])))
        assert not (lhs > rhs).any(), "%s Euler identity fails at %s" % (tag, np.argwhere(lhs > rhs)[:4].tolist())


def _check_states(raw, ref, x0, dt, case, tag):
    _check_own(raw, x0, dt, tag)
    eq, ev = _errors(raw, ref)
    _note(case, q=eq, qd=ev)
    bq, bv = _bars(case)
    print("%s: q err %.3e, qd err %.3e" % (tag, eq, ev))
    assert eq <= bq and ev <= bv, "%s: q err %.3e (bar %.1e), qd err %.3e (bar %.1e)" % (tag, eq, bq, ev, bv)


def _rollout_states(ref, x0, U_shift, noise, rows):
    H = U_shift.shape[0]
    w = ref.wrench_rows(x0, H)
    return WR.states_stack(ref.model, x0, U_shift[None] + noise[rows], ref.dt, w)


def _assert_update(tag, dev, J, w, g, Un, H):
    Jd = dev.costs()
    assert np.array_equal(np.isnan(Jd), np.isnan(J)), tag + " NaN pattern"
    rel, dfrac, sfrac, worst = cost_errors(Jd, J, H)
    print("%s: cost rel err %.3e, err / Delta %.3e, (J - Jmin) err / Delta %.3e, %.3f of the allowance" % (tag, rel, dfrac, sfrac, worst))
    _note("update", cost_rel=rel, allowance=worst)
    assert rel <= COST_RTOL, "%s cost rel err %.3e" % (tag, rel)
    ok = ~np.isnan(J)
    if ok.sum() > 1 and J[ok].max() - J[ok].min() >= 1e-6:
        assert worst <= 1.0, "%s cost err / Delta %.3e, (J - Jmin) err / Delta %.3e: %.2f x the allowance" % (tag, dfrac, sfrac, worst)
    assert int(np.nanargmin(Jd)) == int(np.nanargmin(J)) == dev.argmin(), tag + " argmin"
    if w is not None:
        np.testing.assert_allclose(dev.get_weights(), w, rtol=0, atol=WEIGHT_ATOL, err_msg=tag + " weights")
        np.testing.assert_allclose(dev.get_gradient(), g, rtol=0, atol=CONTROL_ATOL, err_msg=tag + " gradient")
        _note("update", U=np.abs(dev.get_optimal_rollout() - Un).max())
    np.testing.assert_allclose(dev.get_optimal_rollout(), Un, rtol=0, atol=CONTROL_ATOL, err_msg=tag + " U*")


# ---- the device object --------------------------------------------------------------------------

def _rel(a, b):
    return float((np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(b))).max())


def test_object_steps_under_a_wrench(monkeypatch):
    _set_env(monkeypatch)
    model = am.FrankaRidgebackDynamics().model
    x0 = _state()
    x0[30] = 15.0
    dev = am.PinocchioDynamicsObject.create(x0)
    plain = am.PinocchioDynamicsObject.create(x0)   # never sees a new call
    assert not dev.simulated_wrench and not dev.get_end_effector_simulated_wrench().any()
    rng = np.random.default_rng(3)
    u = np.zeros((10, 12))
    u[:, :3], u[:, 3:10] = rng.normal(0, 0.3, (10, 3)), rng.normal(0, 20.0, (10, 7))
    x = x0
    for k in range(8):
        dev.add_end_effector_simulated_wrench(WR.W0)
        xd = dev.step(u[k], 0.01)
        x, v, a = WR.step(model, x, u[k], WR.W0, 0.01)
        es, ev, ea = _rel(xd[:12], x[:12]), _rel(xd[12:24], x[12:24]), _rel(dev.query()["joint_acceleration"], a)
        ee = _rel(xd[30], x[30])
        _note("object", q=es, qd=ev, qdd=ea, E=ee)
        assert es <= STATE_RTOL and ev <= VEL_RTOL and ea <= ACC_RTOL and ee <= STATE_RTOL, (k, es, ev, ea, ee)
        np.testing.assert_array_equal(dev.get_end_effector_simulated_wrench(), WR.W0)
        assert np.array_equal(xd[24:30], x0[24:30])
    free = WR.states(model, x0, u[:9], 0.01, None)[0][8]
    assert np.abs(x[3:10] - free[3:10]).max() > 1e-4   # the wrench moved the arm
    # two adds sum; the sum is zeroed by the step that applies it
    a, b = WR.W0 * 0.25, WR.W0 * np.array([0.5, -1.0, 2.0, 0.0, 1.0, 3.0])
    twin = am.PinocchioDynamicsObject.create(x0)
    for o in (dev, twin):
        o.set_state(xd, 0.08)
    dev.add_end_effector_simulated_wrench(a)
    dev.add_end_effector_simulated_wrench(b)
    twin.add_end_effector_simulated_wrench(a + b)
    x1, x2 = dev.step(u[8], 0.01), twin.step(u[8], 0.01)
    np.testing.assert_array_equal(x1, x2)
    np.testing.assert_array_equal(dev.get_end_effector_simulated_wrench(), a + b)
    # a step with nothing added is today's step, bit for bit, and applies a zero wrench
    for o in (dev, plain):
        o.set_state(x1, 0.09)
    x1, x2 = dev.step(u[9], 0.01), plain.step(u[9], 0.01)
    np.testing.assert_array_equal(x1, x2)
    np.testing.assert_array_equal(dev.query_row()[:36], plain.query_row()[:36])
    assert not dev.get_end_effector_simulated_wrench().any()


def test_object_forecast_modes(monkeypatch):
    _set_env(monkeypatch)
    model = am.FrankaRidgebackDynamics().model
    x0 = _state()
    x0[30] = 15.0
    steps = 16
    rows = WR.forecast_table(steps)
    dev = am.PinocchioDynamicsObject.create(x0)
    plain = am.PinocchioDynamicsObject.create(x0)
    off = dev.forecast_rows(x0, 0.0, 0.01, steps, rows)
    np.testing.assert_array_equal(off, plain.forecast_rows(x0, 0.0, 0.01, steps, rows))   # OFF: the rows are only copied
    np.testing.assert_array_equal(off[:, abi.MPPI_DF_WRENCH:abi.MPPI_DF_WRENCH + 6], rows)
    dev.set_simulated_wrench(abi.MPPI_SIMULATED_WRENCH_ON)
    assert dev.simulated_wrench and dev.copy().simulated_wrench and not plain.copy().simulated_wrench
    on = dev.forecast_rows(x0, 0.0, 0.01, steps, rows)
    ref, _ = WR.states(model, x0, np.zeros((steps, 12)), 0.01, rows)
    q = on[:, abi.MPPI_DF_JOINT_POSITION:abi.MPPI_DF_JOINT_POSITION + 12]
    eq, ee = _rel(q, ref[:, :12]), _rel(on[:, abi.MPPI_DF_ENERGY], ref[:, 30])
    _note("object forecast", q=eq, E=ee)
    assert eq <= STATE_RTOL and ee <= STATE_RTOL, (eq, ee)
    np.testing.assert_array_equal(on[:, abi.MPPI_DF_WRENCH:abi.MPPI_DF_WRENCH + 6], rows)
    assert np.abs(q[-1] - off[-1, :12]).max() > 1e-4
    np.testing.assert_array_equal(dev.get_end_effector_simulated_wrench(), rows[-1])
    with pytest.raises(am.EngineError) as ei:
        dev.set_simulated_wrench(2)
    assert ei.value.status == abi.MPPI_ERR_INVALID


# ---- the rollouts' states -----------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", SHAPES)
def test_rollout_states(name, mode, monkeypatch):
    """Every rollout after each of three updates and the optimal row after the last (read alone: the
    standalone filter()); where the launch folds the previous filter() row (r147_h64), that row as the
    launch of the third update wrote it, read after its phase 1."""
    _, S, H, keep, req, sw, first, pend = by_name(name)
    _set_env(monkeypatch, req)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    cost, table = am.AssistedManipulation(), WR.forecast_table(H)
    dyn, dev = _handle(conf, mode, cost, table)
    assert dev.H == H and dev.R == S + 2 and dev.simulated_wrench == MODES[mode]
    ref = WR.Reference(conf, dyn.model, cost, mode, table)
    sd = np.sqrt(np.diag(conf.covariance))
    rng, shift, dt = np.random.default_rng(3), WR.Shift(), dev.get_time_step()
    rows = np.arange(dev.R)
    U_opt = None
    for j, t in enumerate(TIMES):
        tag = "%s %s upd %d" % (name, mode, j)
        x0 = _state(j)
        U_prev = dev.get_optimal_rollout()
        U_shift = WR.shifted(U_prev, shift(t, dt))
        dev.inject_noise(rng.standard_normal((dev.noise_draws(t), 12)) * sd)
        folds = j == 2 and pend[5] == 1
        if folds:   # the previous update's filter() row rides in this launch: read it before phase 3
            dev.update_phase1(x0, t)
            assert dev.update_info()["folded_filter"] == 1
            xp = _state(j - 1)
            fr = WR.states(dyn.model, xp, U_prev, dt, ref.wrench_rows(xp, H))[0]
            _check_states(dev.predicted_optimal().raw, fr, xp, dt, name, tag + " folded filter() row")
            dev.update_phase2()
            dev.update_phase3(t)
        else:
            dev.update(x0, t)
        info = dev.update_info()
        want = first if j == 0 else pend
        assert info["wait_timeouts"] == 0 and (info["folded_filter"], info["objective_in_launch"]) == (want[5], want[6]), (tag, info)
        pred = dev.predicted_rollouts(rows)
        _check_states(pred.raw, _rollout_states(ref, x0, U_shift, dev.noise(), rows), x0, dt, name, tag)
    U_opt = dev.get_optimal_rollout()
    _check_states(dev.predicted_optimal().raw, WR.states(dyn.model, x0, U_opt, dt, ref.wrench_rows(x0, H))[0], x0, dt, name,
                  "%s %s optimal" % (name, mode))
    free = WR.states(dyn.model, x0, U_opt, dt, None)[0]
    if H > 2:
        assert np.abs(dev.predicted_optimal().raw[-1, 3:10] - free[-1, 3:10]).max() > 1e-3   # the pushed robot, not the free one


# ---- the update ---------------------------------------------------------------------------------

def _update_run(name, mode, cost, case, monkeypatch, links=None, x_energy=None, S=None, H=None, keep=None):
    if name is not None:
        _, S, H, keep, req, sw, first, pend = by_name(name)
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    table = WR.forecast_table(H)
    dyn, dev = _handle(conf, mode, cost, table, links)
    assert dev.H == H and dev.R == S + 2
    ref = WR.Reference(conf, dyn.model, cost, mode, table, links=bool(links))
    sd = np.sqrt(np.diag(conf.covariance))
    rng, shift, dt = np.random.default_rng(11), WR.Shift(), dev.get_time_step()
    rows = np.arange(dev.R)
    xs_prev = None
    for j, t in enumerate(TIMES):
        tag = "%s %s upd %d" % (case, mode, j)
        x0 = _state(j)
        if x_energy is not None:
            x0[30] = x_energy
        U_prev = dev.get_optimal_rollout()
        U_shift = WR.shifted(U_prev, shift(t, dt))
        dev.inject_noise(rng.standard_normal((dev.noise_draws(t), 12)) * sd)
        dev.update(x0, t)
        info = dev.update_info()
        assert info["wait_timeouts"] == 0, (tag, info)
        if info["folded_filter"]:   # the previous update's filter() row, before any optimal-cost read
            want = ref.rollout(xs_prev, U_prev)[0]
            got = dev.debug_folded_cost()
            assert abs(got - want) <= COST_RTOL * max(abs(want), 1.0), (tag, got, want)
        eps = dev.noise()
        J, xs = ref.costs(x0, U_shift, eps)
        w, g, Un = LR.mppi_update(conf, J, eps, U_shift)
        _assert_update(tag, dev, J, w, g, Un, H)
        pred = dev.predicted_rollouts(rows)
        _check_states(pred.raw, xs, x0, dt, case, tag)
        if x_energy is not None:
            assert np.array_equal(pred.energy[..., 0], np.broadcast_to(x0[30], pred.energy[..., 0].shape)), tag
            ee = float((np.abs(pred.energy - xs[..., 30]) / np.maximum(1.0, np.abs(xs[..., 30]))).max())
            _note(case, E=ee)
            bar = min(1e-11, max(10 * MEASURED[case][2], 10 * EPS))   # the existing tank bar
            assert ee <= bar, "%s: energy err %.3e (bar %.1e)" % (tag, ee, bar)
            assert np.abs(xs[..., 30] - x0[30]).max() > 1e-3   # the tank moves
        xs_prev = x0
    want, xo = ref.rollout(x0, dev.get_optimal_rollout())
    got = dev.get_optimal_total_cost()
    assert abs(got - want) <= COST_RTOL * max(abs(want), 1.0), (case, got, want)
    return dev


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["r20_h33", "r48_h33"])
def test_update_parity(name, mode, monkeypatch):
    _update_run(name, mode, am.AssistedManipulation(), name, monkeypatch)


def test_update_parity_without_the_constant(monkeypatch):
    """The same without the 2e11-per-step self-collision constant, whose ulp swallows the dynamics:
    here the relative cost bar sees the pushed states."""
    cost = am.AssistedManipulation()
    cost.configuration.enable_self_collision_limit = 0
    _update_run("r20_h33", "forecast", cost, "r20_h33", monkeypatch)


def test_tank(monkeypatch):
    """128 x 32 with enable_energy_limit, E0 = 15: (u + tau_w + NLE) . v_new in the tank."""
    cost = am.AssistedManipulation()
    cost.configuration.enable_energy_limit = 1
    for mode in MODES:
        _update_run(None, mode, cost, "tank", monkeypatch, x_energy=15.0, S=128, H=32, keep=20)


def test_track_point(monkeypatch):
    _update_run("r20_h33", "state", am.TrackPoint(), "track_point", monkeypatch)


def test_link_positions_and_wrench_together(monkeypatch):
    cost = am.AssistedManipulation()
    for i in range(1, 8):   # the arm's spheres clear of each other: the barrier's inverse branch
        cost.configuration.self_collision_radii[i] = 0.04
    dev = _update_run("r48_h33", "forecast", cost, "links", monkeypatch, links=True)
    assert dev.link_positions


# ---- off is off, and the modes agree ------------------------------------------------------------

SD = np.sqrt(np.diag(am.frankaridgeback_configuration(rollouts=16, horison=0.08).covariance))


def _three_updates(dev, seed=5, states=_state):
    out = []
    rng = np.random.default_rng(seed)
    for j, t in enumerate(TIMES):
        x0 = states(j)
        dev.inject_noise(rng.standard_normal((dev.noise_draws(t), 12)) * SD)
        dev.update(x0, t)
        out.append((dev.costs(), dev.get_weights(), dev.get_optimal_rollout(), dev.predicted_rollouts(np.arange(dev.R)).raw))
    out.append((dev.predicted_optimal().raw,))
    return out


def _same(a, b, tag):
    for j, (ra, rb) in enumerate(zip(a, b)):
        for i, (va, vb) in enumerate(zip(ra, rb)):
            np.testing.assert_array_equal(va, vb, err_msg="%s update %d item %d" % (tag, j, i))


def test_off_is_off(monkeypatch):
    """Mode OFF with W0 in the state and the forecast table set: bit for bit a handle that never
    called the new functions."""
    _, S, H, keep, req, sw, first, pend = by_name("r20_h33")
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    table = WR.forecast_table(H)
    _, off = _handle(conf, False, am.AssistedManipulation(), table)
    _, never = _handle(conf, None, am.AssistedManipulation(), table)
    assert off.simulated_wrench == abi.MPPI_SIMULATED_WRENCH_OFF == never.simulated_wrench
    _same(_three_updates(off), _three_updates(never), "off")
    _, on = _handle(conf, "state", am.AssistedManipulation(), table)
    assert np.abs(_three_updates(on)[0][3] - _three_updates(never)[0][3])[..., -1, 3:10].max() > 1e-3   # (and on is not off)


def test_modes_agree_on_a_constant_table(monkeypatch):
    """A constant table equal to the state's wrench: STATE and FORECAST are bit-identical."""
    _, S, H, keep, req, sw, first, pend = by_name("r48_h33")
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    table = np.tile(WR.W0, (H, 1))

    def fixed(j):
        x = _state(0)
        x[3] += 0.02 * j
        return x

    _, a = _handle(conf, "state", am.AssistedManipulation(), table)
    _, b = _handle(conf, "forecast", am.AssistedManipulation(), table)
    _same(_three_updates(a, states=fixed), _three_updates(b, states=fixed), "modes")


# ---- shards, the graph path, the errors ---------------------------------------------------------

def test_shards(monkeypatch):
    """Two phase-split shards of 128 x 32 on one device equal one handle."""
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=128, horison=0.32, keep_best_rollouts=20, threads=8)
    table = WR.forecast_table(32)
    _, single = _handle(conf, "forecast", am.AssistedManipulation(), table)
    shards = []
    for r in range(2):
        _, t = _handle(conf, "forecast", am.AssistedManipulation(), table)
        t.set_shard(2, r)
        shards.append(t)
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    R, HC = single.R, single.H * single.C

    def allreduce(ptrs, n):
        bufs = [np.zeros(n) for _ in ptrs]
        for p, b in zip(ptrs, bufs):
            assert hip.hipMemcpy(b.ctypes.data, p, n * 8, 2) == 0
        s = bufs[0] + bufs[1]
        for p in ptrs:
            assert hip.hipMemcpy(p, s.ctypes.data, n * 8, 1) == 0

    rng, shift, dt = np.random.default_rng(9), WR.Shift(), single.get_time_step()
    model = O.default_model()
    for j, t in enumerate(TIMES[:2]):
        x0 = _state(j)
        sh_n = shift(t, dt)
        U_shift = [WR.shifted(sh.get_optimal_rollout(), sh_n) for sh in shards]
        eps = rng.standard_normal((single.noise_draws(t), 12)) * SD
        single.inject_noise(eps)
        single.update(x0, t)
        for sh in shards:
            sh.inject_noise(eps)
            sh.update_phase1(x0, t)
        hip.hipDeviceSynchronize()
        allreduce([sh.device_costs_ptr() for sh in shards], R + 1)
        for sh in shards:
            sh.update_phase2()
        hip.hipDeviceSynchronize()
        allreduce([sh.device_gradient_ptr() for sh in shards], HC)
        for sh in shards:
            sh.update_phase3(t)
        whole = single.predicted_rollouts(np.arange(R)).raw
        for r, sh in enumerate(shards):   # test_gpu_parity's shard bars
            b, e = am.shard_range(R, 2, r)
            mine = sh.predicted_rollouts(np.arange(b, e)).raw[..., :24]
            if j == 0:   # identical inputs: per-rollout bit-exact
                np.testing.assert_array_equal(sh.costs(), single.costs())
                np.testing.assert_array_equal(mine, whole[b:e, :, :24])
            else:        # U* differs in the last bit (the gradient summed per shard, then across)
                np.testing.assert_allclose(sh.costs(), single.costs(), rtol=1e-13, atol=0)
            # the shard's own rows against the reference stepped through the shard's own controls
            want = WR.states_stack(model, x0, U_shift[r][None] + sh.noise()[b:e], dt, table)
            _check_states(mine, want, x0, dt, "shards", "shard %d upd %d" % (r, j))
            np.testing.assert_allclose(sh.get_optimal_rollout(), single.get_optimal_rollout(), rtol=0, atol=1e-12)
            np.testing.assert_allclose(sh.get_weights(), single.get_weights(), rtol=0, atol=1e-15)
            assert sh.argmin() == single.argmin()
        free = WR.states(model, x0, single.get_optimal_rollout(), dt, None)[0]
        assert np.abs(single.predicted_optimal().raw[-1, 3:10] - free[-1, 3:10]).max() > 1e-3   # (the pushed robot)


def test_graph_equals_eager(monkeypatch):
    """1000 x 64 with the mode on and the hipGraph path against an eager twin, device Philox, five
    updates with the state's wrench changing: bit for bit, and the graph ran."""
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=1000, horison=0.64, keep_best_rollouts=20, threads=8)
    for mode in MODES:
        out = {}
        for graph in (0, 1):
            t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(simulated_wrench=mode), am.AssistedManipulation())
            t.set_graph(graph)
            t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
            t.set_forecast(WR.forecast_table(t.H))
            rec = []
            for j, tm in enumerate((0.0, 0.05, 0.07, 0.12, 0.12)):
                t.update(_state(j), tm)
                rec.append(t.costs())
                rec.append(t.get_weights())
            rec.append(t.predicted_rollouts(np.arange(t.R)).raw)
            rec.append(t.predicted_optimal().raw)
            rec.append(t.get_optimal_rollout())
            out[graph] = (rec, t.graph_updates())
        assert out[0][1] == 0 and out[1][1] > 0, (mode, out[0][1], out[1][1])
        for j, (a, b) in enumerate(zip(out[0][0], out[1][0])):
            np.testing.assert_array_equal(a, b, err_msg="%s item %d" % (mode, j))


def test_errors(monkeypatch):
    _set_env(monkeypatch)
    conf = am.point_mass_configuration(rollouts=64, horison=0.08, keep_best_rollouts=20)
    pm = am.Trajectory.create(conf, am.PointMassDynamics(), am.QuadraticCost())
    with pytest.raises(am.EngineError) as ei:
        pm.set_simulated_wrench(abi.MPPI_SIMULATED_WRENCH_STATE)
    assert ei.value.status == abi.MPPI_ERR_UNSUPPORTED
    assert pm.simulated_wrench == abi.MPPI_SIMULATED_WRENCH_OFF
    conf = am.frankaridgeback_configuration(rollouts=15, horison=horizon(5), keep_best_rollouts=5)
    dev = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(), am.AssistedManipulation())
    for bad in (-1, 3):
        with pytest.raises(am.EngineError) as ei:
            dev.set_simulated_wrench(bad)
        assert ei.value.status == abi.MPPI_ERR_INVALID
    dev.set_simulated_wrench(abi.MPPI_SIMULATED_WRENCH_FORECAST)
    dev.set_simulated_wrench(abi.MPPI_SIMULATED_WRENCH_STATE)
    assert dev.simulated_wrench == abi.MPPI_SIMULATED_WRENCH_STATE
    dev.update(_state(), 0.0)
    with pytest.raises(am.EngineError) as ei:
        dev.set_simulated_wrench(abi.MPPI_SIMULATED_WRENCH_OFF)
    assert ei.value.status == abi.MPPI_ERR_INVALID and "first update" in str(ei.value)
    with pytest.raises(ValueError):
        am.FrankaRidgebackDynamics(simulated_wrench="on")


def test_environment_switch():
    """MPPI_SIMULATED_WRENCH sets the mode new handles and objects start in; 3 fails the create.  A
    fresh child process each: the variable is read at create."""
    prog = ("import sys, assistedmanipulation_amd as am\n"
            "conf = am.frankaridgeback_configuration(rollouts=15, horison=0.045, keep_best_rollouts=5)\n"
            "t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(), am.AssistedManipulation())\n"
            "if t is None:\n"
            "    print('create failed')\n"
            "    sys.exit(0)\n"
            "o = am.PinocchioDynamicsObject.create(am.huddled_state())\n"
            "print('mode', t.simulated_wrench, int(o.simulated_wrench))\n")
    for value, want in (("2", "mode 2 1"), ("1", "mode 1 1"), ("0", "mode 0 0"), ("3", "create failed")):
        env = dict(os.environ, MPPI_SIMULATED_WRENCH=value, PYTHONPATH=REPO)
        r = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == want, (value, r.stdout, r.stderr)
        if value == "3":
            assert "MPPI_SIMULATED_WRENCH must be 0, 1 or 2" in r.stderr
