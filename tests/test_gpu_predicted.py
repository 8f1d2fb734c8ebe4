"""Predicted trajectories (mppi_predicted_optimal / mppi_predicted_rollouts) on the device: the states
the rollout launches left in their step records, and forward kinematics at them, for every launch
plan of launch_shapes, the tank, a rollout that goes NaN, the two-launch split and one-wave rounds,
both ways the filter() row is written, shards, the graph path, the error statuses and the logger.

The reference of a rollout is an O.OracleDynamics stepped from x0 through U_shifted[k] + noise[r, k],
U_shifted[k] = U_prev[min(k + shift, H - 1)] with U_prev = get_optimal_rollout() read before the
update and shift = int((t - last shift time) / dt); the optimal row steps U* from x0.  Checks:
  (a) row 0 is x0's q and qd bit for bit;
  (b) the Euler identity |q_k - (q_{k-1} + qd_k dt)| <= 4 eps max(1, |q_k|, |q_{k-1}|) on the
      device's own rows (one or two roundings): any mis-addressed row or step breaks it;
  (c) q and qd against the oracle stepping, error relative to max(1, |x|), bars below;
  (d) the grasp-frame, arm-mount and link columns against link_reference.fk on the device's q_k,
      1e-12 m (test_gpu_link_positions.py's bar for the device's link positions);
  (e) the energy column all NaN with the tank off.

Bars of (c): the device and the oracle solve the dynamics in different operation orders and the
difference compounds over the horizon; the oracle's own two orders differ by up to 3.9e-12 (q) and
1.9e-11 (qd) over 33 steps, 1.9e-11 / 1.4e-10 over 64, 4.7e-10 / 1.9e-9 over 128 (absolute, |x| up
to 195).  Each bar is ten times the worst error measured for its case, never above the caps
1e-8 (q) / 1e-7 (qd) at H <= 65 and 1e-7 / 1e-6 at H >= 128: a wrong row or a one-step shift is an
error of 1e-2 or more.  MEASURED holds the figures the bars come from.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi
from assistedmanipulation_amd.csvlog import MPPILogger
from oracle import oracle as O

import link_reference as LR
from helpers import fr_pair, pm_pair, step_both
from launch_shapes import TIME_STEP, by_name, horizon

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH_ENV = {"c": "MPPI_COSTS_IN_LAUNCH", "h": "MPPI_HANDOVER", "s": "MPPI_SPLIT"}
SHAPES = ["r20_h33", "r48_h33", "r147_h33", "r10_h33", "r3_h33", "r19_h129", "r19_h1", "r19_h2"]
TIMES = [0.0, 2 * TIME_STEP, 2.5 * TIME_STEP]   # shifts of 0, 2 and 0 steps
EPS = np.finfo(np.float64).eps
FK_BAR = 1e-12
CAPS = {False: (1e-8, 1e-7), True: (1e-7, 1e-6)}   # H >= 128: (q, qd)

# case -> worst (q, qd) error against the oracle, relative to max(1, |x|), as measured on an MI355X
# (the energy case: (q, qd, E)); the bars are ten times these
MEASURED = {
    "r20_h33": (1.675e-12, 8.009e-12),
    "r48_h33": (2.122e-12, 1.795e-11),
    "r147_h33": (2.180e-12, 1.623e-11),
    "r10_h33": (5.165e-13, 2.289e-12),
    "r3_h33": (5.497e-15, 1.530e-13),
    "r19_h129": (3.106e-11, 1.177e-10),
    "r19_h1": (0.0, 0.0),
    "r19_h2": (5.285e-15, 1.952e-13),
    "tank": (2.416e-12, 1.586e-11, 5.587e-13),
    "nan": (2.508e-12, 1.023e-11),
    "split_8192x128": (6.599e-11, 5.845e-10),
    "rounds_8190x64": (9.987e-12, 2.853e-11),
    "optimal_formats": (4.735e-14, 5.111e-13),
    "shards": (2.890e-12, 1.037e-11),
}
STATS = {}   # case -> the worst figures of this run


def _bars(case, H):
    """Ten times the measured worst, at most the cap.  A measured zero (the one-step horizon: row 0
    alone, bit for bit) leaves 10 eps."""
    return tuple(min(c, max(10 * v, 10 * EPS)) for v, c in zip(MEASURED[case][:2], CAPS[H >= 128]))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for case, v in STATS.items():
        print("\npredicted %-16s worst vs oracle: %s" % (case, ", ".join("%s %.3e" % kv for kv in sorted(v.items()))))


def _note(case, **figures):
    s = STATS.setdefault(case, {})
    for k, v in figures.items():
        s[k] = max(s.get(k, 0.0), float(v))


def _set_env(monkeypatch, req=0, sw=""):
    for v in ("MPPI_RELAY_K", "MPPI_TAIL_DRAWS", "MPPI_DRAW_AHEAD", "MPPI_LINK_POSITIONS", "MPPI_GRAPH") + tuple(SWITCH_ENV.values()):
        monkeypatch.delenv(v, raising=False)
    if req:
        monkeypatch.setenv("MPPI_RELAY_K", str(req))
    for s in sw:
        monkeypatch.setenv(SWITCH_ENV[s], "0")


class Shift:
    """sample()'s shift count (mppi.cpp:194-201): truncation, the last shift time kept while 0."""

    def __init__(self):
        self.last = 0.0

    def __call__(self, t, dt):
        n = int((t - self.last) / dt)
        if n > 0:
            self.last = t
        return max(n, 0)


def _shifted(U_prev, shift):
    H = U_prev.shape[0]
    return U_prev[np.minimum(np.arange(H) + shift, H - 1)]


def _oracle_states(dyn, x0, t, u, dt):
    """x_0 .. x_{H-1} of the controls u (H, C) from x0: (H, 31)."""
    H = u.shape[0]
    out = np.zeros((H, abi.MPPI_FR_STATE))
    dyn.set_state(x0, t)
    out[0] = x0
    for k in range(H - 1):
        out[k + 1] = dyn.step(u[k], dt)
    return out


def _fk_stack(model, Q):
    """link_reference.fk's chain on a stack of configurations (N, 12): (links (N, 13, 3), grasp frame
    (N, 3), arm mount (N, 3)); its first and last rows are checked against link_reference.fk itself."""
    N = Q.shape[0]
    R, p = [], []
    for i in range(model.nbodies):
        b = model.bodies[i]
        Rp, pp, axis = np.array(b.rotation[:]).reshape(3, 3), np.array(b.translation[:]), np.array(b.axis[:])
        if b.type == abi.MPPI_JOINT_REVOLUTE:
            c, s = np.cos(Q[:, i]), np.sin(Q[:, i])
            Rj = np.zeros((N, 3, 3))
            Rj[:, 0, 0], Rj[:, 0, 1], Rj[:, 1, 0], Rj[:, 1, 1], Rj[:, 2, 2] = c, -s, s, c, 1.0
            Rl, pl = Rp @ Rj, np.broadcast_to(pp, (N, 3))
        else:
            Rl, pl = np.broadcast_to(Rp, (N, 3, 3)), pp + (Rp @ axis) * Q[:, i:i + 1]
        if b.parent < 0:
            R.append(Rl)
            p.append(pl)
        else:
            R.append(R[b.parent] @ Rl)
            p.append(p[b.parent] + np.einsum("nij,nj->ni", R[b.parent], pl))
    links = np.stack([np.zeros((N, 3))] + p, axis=1)

    def frame(f):
        return p[f.parent] + np.einsum("nij,j->ni", R[f.parent], np.array(f.translation[:]))

    ee, amount = frame(model.end_effector), frame(model.arm_mount)
    for n in (0, N - 1):
        l1, e1, a1 = LR.fk(model, Q[n])
        assert max(np.abs(links[n] - l1).max(), np.abs(ee[n] - e1).max(), np.abs(amount[n] - a1).max()) <= 1e-14
    return links, ee, amount


def _check_own(pred, x0, dt, tag, energy_nan=True, finite=None):
    """(a), (b), (d), (e) on the device's own rows: pred a Predicted with leading rollout axis or
    without; finite: a mask (..., H) of the rows expected finite (default: all)."""
    raw = pred.raw.reshape((-1,) + pred.raw.shape[-2:])
    N, H, _ = raw.shape
    fin = np.ones((N, H), dtype=bool) if finite is None else finite.reshape(N, H)
    q, qd = raw[..., :12], raw[..., 12:24]
    assert np.isfinite(raw[fin][:, list(range(24)) + list(range(25, 70))]).all(), tag + " finite rows"
    assert np.isnan(raw[~fin]).all(), tag + " rows behind a NaN state: every column NaN"
    assert np.array_equal(q[:, 0], np.broadcast_to(x0[:12], (N, 12))) and np.array_equal(qd[:, 0], np.broadcast_to(x0[12:24], (N, 12))), \
        tag + " row 0 is x0"
    if H > 1:
        both = fin[:, 1:] & fin[:, :-1]
        lhs = np.abs(q[:, 1:] - (q[:, :-1] + qd[:, 1:] * dt))
        rhs = 4 * EPS * np.maximum(1.0, np.maximum(np.abs(q[:, 1:]), np.abs(q[:, :-1])))
        bad = (lhs > rhs) & both[..., None]
        assert not bad.any(), "%s Euler identity fails at (rollout, step, joint) %s" % (tag, np.argwhere(bad)[:4].tolist())
    model = O.default_model()
    links, ee, amount = _fk_stack(model, q[fin])
    err = max(np.abs(pred.links.reshape(N, H, 13, 3)[fin] - links).max(), np.abs(pred.end_effector.reshape(N, H, 3)[fin] - ee).max(),
              np.abs(pred.arm_mount.reshape(N, H, 3)[fin] - amount).max())
    assert err <= FK_BAR, "%s positions differ from the numpy chain at q_k by %.3e m" % (tag, err)
    if energy_nan:
        assert np.isnan(raw[..., abi.MPPI_PRED_ENERGY]).all(), tag + " energy column with the tank off"
    return err


def _errors(dev_rows, ref_states):
    """Worst |dev - oracle| / max(1, |oracle|) over q and over qd."""
    eq = np.abs(dev_rows[..., :12] - ref_states[..., :12]) / np.maximum(1.0, np.abs(ref_states[..., :12]))
    ev = np.abs(dev_rows[..., 12:24] - ref_states[..., 12:24]) / np.maximum(1.0, np.abs(ref_states[..., 12:24]))
    return float(eq.max()), float(ev.max())


def _check_rollouts(dev, rows, x0, t, U_shift, noise, case, tag, dyn, energy=False, finite=None):
    """Checks (a)-(e) of the rollouts `rows` (global indices) of the last update; noise: dev.noise()."""
    dt = dev.get_time_step()
    pred = dev.predicted_rollouts(rows)
    assert pred.raw.shape == (len(rows), dev.H, abi.MPPI_PRED_N) and list(pred.rollouts) == list(rows)
    np.testing.assert_array_equal(pred.time, t + np.arange(dev.H) * dt)
    _check_own(pred, x0, dt, tag, energy_nan=not energy, finite=finite)
    ref = np.stack([_oracle_states(dyn, x0, t, U_shift + noise[r], dt) for r in rows])
    fin = np.ones(ref.shape[:2], dtype=bool) if finite is None else finite
    eq, ev = _errors(pred.raw[fin], ref[fin])
    _note(case, q=eq, qd=ev)
    bq, bv = _bars(case, dev.H)
    assert eq <= bq and ev <= bv, "%s: q err %.3e (bar %.1e), qd err %.3e (bar %.1e)" % (tag, eq, bq, ev, bv)
    return pred, ref


def _check_optimal(dev, x0, t, case, tag, dyn, energy=False):
    dt = dev.get_time_step()
    pred = dev.predicted_optimal()
    assert pred.raw.shape == (dev.H, abi.MPPI_PRED_N) and pred.rollouts is None
    _check_own(pred, x0, dt, tag, energy_nan=not energy)
    ref = _oracle_states(dyn, x0, t, dev.get_optimal_rollout(), dt)
    eq, ev = _errors(pred.raw, ref)
    _note(case, q=eq, qd=ev)
    bq, bv = _bars(case, dev.H)
    assert eq <= bq and ev <= bv, "%s: q err %.3e (bar %.1e), qd err %.3e (bar %.1e)" % (tag, eq, bq, ev, bv)
    return pred, ref


@pytest.mark.parametrize("name", SHAPES)
def test_launch_shapes(name, monkeypatch):
    """Every rollout and the optimal row after each of three updates.  Reading the optimal row runs a
    pending filter() by itself, so it would never fold: the first pass reads it after the last
    update only (the launches are the table's: the x kernel, then what a pending filter() makes of
    it), the second pass after every update."""
    _, S, H, keep, req, sw, first, pend = by_name(name)
    _set_env(monkeypatch, req, sw)
    x0 = am.huddled_state()
    for optimal_each in (False, True):
        conf, dev, orc, sd = fr_pair(S=S, horison=horizon(H), K=keep)
        assert dev.H == H and dev.R == S + 2
        dyn = O.OracleDynamics(x0)
        rng, shift = np.random.default_rng(3), Shift()
        for j, t in enumerate(TIMES):
            tag = "%s pass %d upd %d" % (name, optimal_each, j)
            U_shift = _shifted(dev.get_optimal_rollout(), shift(t, dev.get_time_step()))
            step_both(dev, orc, x0, t, rng, sd)
            info = dev.update_info()
            assert info["wait_timeouts"] == 0, (tag, info)
            if not optimal_each:
                want = first if j == 0 else pend
                assert (info["folded_filter"], info["objective_in_launch"]) == (want[5], want[6]), (tag, info)
                _check_rollouts(dev, np.arange(dev.R), x0, t, U_shift, dev.noise(), name, tag, dyn)
            if optimal_each or j + 1 == len(TIMES):
                _check_optimal(dev, x0, t, name, tag + " optimal", dyn)


def test_tank_on(monkeypatch):
    """enable_energy_limit on the default stack: the energy column against slot 30 of the oracle's
    stepped states, the tank inside its barriers and the arm moving."""
    _set_env(monkeypatch)
    cost = am.AssistedManipulation()
    cost.configuration.enable_energy_limit = 1
    conf, dev, orc, sd = fr_pair(S=128, horison=0.32, K=20, cost=cost)
    assert dev.H == 32
    x0 = am.huddled_state()
    x0[30] = 15.0
    x0[12 + 3:12 + 10] = np.random.default_rng(32).normal(0, 0.5, 7)
    dyn = O.OracleDynamics(x0)
    rng, shift = np.random.default_rng(5), Shift()
    for j, t in enumerate(TIMES):
        tag = "tank upd %d" % j
        U_shift = _shifted(dev.get_optimal_rollout(), shift(t, dev.get_time_step()))
        step_both(dev, orc, x0, t, rng, sd)
        for what, (pred, ref) in (("rollouts", _check_rollouts(dev, np.arange(dev.R), x0, t, U_shift, dev.noise(), "tank", tag, dyn, energy=True)),
                                  ("optimal", _check_optimal(dev, x0, t, "tank", tag + " optimal", dyn, energy=True))):
            assert np.array_equal(pred.energy[..., 0], np.broadcast_to(x0[30], pred.energy[..., 0].shape)), tag
            ee = float((np.abs(pred.energy - ref[..., 30]) / np.maximum(1.0, np.abs(ref[..., 30]))).max())
            _note("tank", E=ee)
            # ten times the measured worst: 5.6e-12, inside the project's tank bar of 1e-11
            bar = min(1e-11, 10 * MEASURED["tank"][2])
            assert ee <= bar, "%s %s: energy err %.3e (bar %.1e)" % (tag, what, ee, bar)
            assert np.abs(ref[..., 30] - x0[30]).max() > 1e-3   # the tank moves


def test_nan_rollout(monkeypatch):
    """One NaN in the noise of one rollout at step 5: its rows 0-5 meet the bars, rows >= 6 are NaN in
    all 70 columns (x_6 is the first state the NaN control reaches), every other rollout is finite."""
    _set_env(monkeypatch)
    conf, dev, orc, sd = fr_pair(S=128, horison=0.32, K=20)
    x0 = am.huddled_state()
    dyn = O.OracleDynamics(x0)
    rng = np.random.default_rng(7)
    U_shift = _shifted(dev.get_optimal_rollout(), 0)
    n = dev.noise_draws(0.0)
    eps = rng.standard_normal((n, 12)) * sd
    eps[37 * dev.H + 5, 4] = np.nan   # the 38th resampled rollout's column 5, an arm torque
    dev.inject_noise(eps)
    dev.update(x0, 0.0)
    noise = dev.noise()
    where = np.argwhere(np.isnan(noise))
    assert where.shape == (1, 3) and where[0, 1] == 5 and where[0, 2] == 4, where
    bad = int(where[0, 0])
    finite = np.ones((dev.R, dev.H), dtype=bool)
    finite[bad, 6:] = False
    clean = np.where(np.isnan(noise), 0.0, noise)   # the oracle steps rows 0-5 of the bad rollout: u_5 is never used
    pred, _ = _check_rollouts(dev, np.arange(dev.R), x0, 0.0, U_shift, clean, "nan", "nan", dyn, finite=finite)
    assert np.isnan(pred.raw[bad, 6:]).all() and np.isfinite(pred.raw[bad, :6, :24]).all()
    others = np.delete(np.arange(dev.R), bad)
    assert np.isfinite(pred.raw[others][..., list(range(24)) + list(range(25, 70))]).all()


@pytest.mark.parametrize("S,H,case", [(8192, 128, "split_8192x128"), (8190, 64, "rounds_8190x64")])
def test_large_plans(S, H, case, monkeypatch):
    """The two-launch split and one-wave workgroups over several rounds (256 CUs), the first update
    with the device's own Philox draws read back: rollouts 0, 1, the last 40 and 200 drawn."""
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=20, threads=8)
    dev = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(), am.AssistedManipulation())
    assert dev.H == H and dev.R == S + 2
    dev.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
    dev.set_forecast(am.constant_forecast(H))
    x0 = am.huddled_state()
    U_shift = _shifted(dev.get_optimal_rollout(), 0)
    assert not U_shift.any()
    dev.update(x0, 0.0)
    assert dev.update_info()["wait_timeouts"] == 0
    R = dev.R
    rows = np.concatenate([[0, 1], np.arange(R - 40, R), np.random.default_rng(2024).choice(np.arange(2, R - 40), 200, replace=False)])
    _check_rollouts(dev, rows, x0, 0.0, U_shift, dev.noise(), case, case, O.OracleDynamics(x0))


def test_optimal_row_both_ways(monkeypatch):
    """The filter() row of update n read right after it (the standalone filter()) and, on a twin,
    after update n + 1's phase 1 folded it into the rollout launch: both meet the oracle bars."""
    _, S, H, keep, req, sw, first, pend = by_name("r147_h33")
    _set_env(monkeypatch, req, sw)
    x0 = am.huddled_state()
    dyn = O.OracleDynamics(x0)
    got = {}
    for which in "AB":
        conf, dev, orc, sd = fr_pair(S=S, horison=horizon(H), K=keep)
        rng = np.random.default_rng(3)
        for t in TIMES[:2]:
            step_both(dev, orc, x0, t, rng, sd)
        U = dev.get_optimal_rollout()
        if which == "B":
            t = TIMES[2]
            eps = rng.standard_normal((dev.noise_draws(t), 12)) * sd
            dev.inject_noise(eps)
            dev.update_phase1(x0, t)
            assert dev.update_info()["folded_filter"] == 1
        pred = dev.predicted_optimal()
        _check_own(pred, x0, dev.get_time_step(), "optimal " + which)
        ref = _oracle_states(dyn, x0, TIMES[1], U, dev.get_time_step())
        eq, ev = _errors(pred.raw, ref)
        _note("optimal_formats", q=eq, qd=ev)
        bq, bv = _bars("optimal_formats", H)
        assert eq <= bq and ev <= bv, "optimal %s: q err %.3e (bar %.1e), qd err %.3e (bar %.1e)" % (which, eq, bq, ev, bv)
        if which == "B":
            dev.update_phase2()
            dev.update_phase3(t)
        got[which] = pred.raw.copy()
    # measured bit-identical on an MI355X (both rows are 768-B records: the standalone filter() keeps
    # them, fr_coop_compact), so asserted
    _note("optimal_formats", A_minus_B=np.nanmax(np.abs(got["A"] - got["B"])))
    np.testing.assert_array_equal(got["A"], got["B"])


def test_shards(monkeypatch):
    """Two phase-split shards of 128 x 32 on one device: each answers its own rows within the bars
    and refuses the other's."""
    _set_env(monkeypatch)
    conf, single, orc, sd = fr_pair(S=128, horison=0.32)
    shards = []
    for r in range(2):
        t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(), am.AssistedManipulation())
        t.set_noise_source(abi.MPPI_NOISE_HOST_INJECTED)
        t.set_forecast(am.constant_forecast(t.H))
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

    x0 = am.huddled_state()
    dyn = O.OracleDynamics(x0)
    rng, shift = np.random.default_rng(9), Shift()
    for j, t in enumerate(TIMES[:2]):
        sh_n = shift(t, single.get_time_step())
        U_shift = [_shifted(sh.get_optimal_rollout(), sh_n) for sh in shards]
        eps = rng.standard_normal((shards[0].noise_draws(t), 12)) * sd
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
        for r, sh in enumerate(shards):
            b, e = am.shard_range(R, 2, r)
            _check_rollouts(sh, np.arange(b, e), x0, t, U_shift[r], sh.noise(), "shards", "shard %d upd %d" % (r, j), dyn)
            ob, oe = am.shard_range(R, 2, 1 - r)
            for other in (ob, oe - 1):
                with pytest.raises(am.EngineError) as ei:
                    sh.predicted_rollouts([b, other])
                assert ei.value.status == abi.MPPI_ERR_INVALID and "shard" in str(ei.value)


def test_graph_equals_eager(monkeypatch):
    """1000 x 64 with the hipGraph path against an eager twin, device Philox: every rollout after each
    update and the optimal row after the last, bit for bit."""
    _set_env(monkeypatch)
    conf = am.frankaridgeback_configuration(rollouts=1000, horison=0.64, keep_best_rollouts=20, threads=8)
    out = {}
    for graph in (0, 1):
        t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(), am.AssistedManipulation())
        t.set_graph(graph)
        t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
        t.set_forecast(am.constant_forecast(t.H))
        x0 = am.huddled_state()
        rec = []
        for tm in (0.0, 0.05, 0.07, 0.12, 0.12):
            t.update(x0, tm)
            rec.append(t.predicted_rollouts(np.arange(t.R)).raw)
        rec.append(t.predicted_optimal().raw)
        out[graph] = (rec, t.graph_updates())
    assert out[0][1] == 0 and out[1][1] > 0, (out[0][1], out[1][1])
    for j, (a, b) in enumerate(zip(out[0][0], out[1][0])):
        assert np.isfinite(a[..., :24]).all()
        np.testing.assert_array_equal(a, b, err_msg="update %d" % j)


def test_error_statuses(monkeypatch):
    _set_env(monkeypatch)
    conf, pm, orc, sd = pm_pair(S=64, horison=0.08)
    for call in (pm.predicted_optimal, lambda: pm.predicted_rollouts([0])):
        with pytest.raises(am.EngineError) as ei:
            call()
        assert ei.value.status == abi.MPPI_ERR_UNSUPPORTED
    conf, dev, orc, sd = fr_pair(S=17, horison=horizon(5), K=5)
    for call in (dev.predicted_optimal, lambda: dev.predicted_rollouts([0])):
        with pytest.raises(am.EngineError) as ei:
            call()
        assert ei.value.status == abi.MPPI_ERR_INVALID and "yet" in str(ei.value)
    step_both(dev, orc, am.huddled_state(), 0.0, np.random.default_rng(1), sd)
    for bad in (-1, dev.R, 2 ** 40):
        with pytest.raises(am.EngineError) as ei:
            dev.predicted_rollouts([0, bad])
        assert ei.value.status == abi.MPPI_ERR_INVALID and "outside" in str(ei.value)
    assert dev.predicted_rollouts([]).raw.shape == (0, dev.H, abi.MPPI_PRED_N)   # n = 0: a no-op
    best = dev.predicted_best(3)
    c = dev.costs()
    assert list(best.rollouts) == list(np.argsort(np.where(np.isnan(c), np.inf, c), kind="stable")[:3])
    np.testing.assert_array_equal(best.raw, dev.predicted_rollouts(best.rollouts).raw)


def test_logger_cpp_and_python_write_the_same_predicted_csv(tmp_path):
    """log_predicted on: logger::MPPI (the C++ program) and MPPILogger write identical predicted.csv
    files for the same run (64 rollouts, 0.16 s horizon, three updates); off: no such file."""
    cpp = os.path.join(REPO, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "predicted.mk"])
    exe = os.path.join(cpp, "build", "predicted")
    for on in (1, 0):
        cdir, pdir = tmp_path / ("cpp%d" % on), tmp_path / ("py%d" % on)
        subprocess.check_output([exe, "log", str(cdir), str(on)], timeout=300)
        conf = am.frankaridgeback_configuration(rollouts=64, horison=0.16)
        t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(), am.AssistedManipulation())
        t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
        t.set_forecast(am.constant_forecast(t.H))
        log = MPPILogger(str(pdir), control_dof=t.C, rollouts=t.get_rollout_count(), log_predicted=bool(on))
        x = am.huddled_state()
        for j in range(3):
            t.update(x, 0.05 * j)
            log.log(t)
            log.log(t)
        log.close()
        if not on:
            assert not (cdir / "predicted.csv").exists() and not (pdir / "predicted.csv").exists()
            continue
        text = (cdir / "predicted.csv").read_text()
        assert text == (pdir / "predicted.csv").read_text()
        lines = text.splitlines()
        head = lines[0].split(", ")
        assert head[:3] == ["update", "time", "q0"] and head[14] == "v0" and head[26:30] == ["energy", "ee_x", "ee_y", "ee_z"]
        assert head[30] == "arm_mount_x" and head[33] == "omni_base_root_link_x" and head[-1] == "panda_rightfinger_z"
        assert len(head) == 2 + abi.MPPI_PRED_N and len(lines) == 1 + 3 * t.H
        assert (cdir / "costs.csv").read_text() == (pdir / "costs.csv").read_text()
