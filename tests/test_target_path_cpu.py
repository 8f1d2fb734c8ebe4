"""Target tracking's host-side surface and its CPU reference (no GPU): TargetPath.sample against the
reference's sampler, the quaternions' normalisation and sign fix, every refusal that needs no device,
the reference's grasp-frame rotation against the oracle object's, the composition with a constant path
against the plain TrackPoint oracle costs, the placement of the parity tests' path, and the ABI structs."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi
from oracle import oracle as O

import link_reference as LR
import state_space as SS
import target_paths as TP
import target_reference as TR
from helpers import COST_RTOL, cost_errors
from launch_shapes import TIME_STEP, by_name, horizon

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a sample is a handful of fp64 operations on values of order 1 on both sides
SAMPLE_ATOL = 1e-15


def _times_of_interest(path):
    T = path.times
    out = [T[0] - 1.0, T[0] - 1e-9, T[-1] + 1e-9, T[-1] + 5.0] + list(T)
    for a, b in zip(T[:-1], T[1:]):
        out += [a + f * (b - a) for f in (1e-9, 0.25, 0.5, 0.9, 1.0 - 1e-9)]
    return out


@pytest.mark.parametrize("make", [TP.path_a, TP.path_b, TP.path_c, TP.constant_path])
def test_sample_against_the_reference_sampler(make):
    """Before the first waypoint, on every waypoint, inside every segment, past the last."""
    path = make()
    regimes = set()
    for t in _times_of_interest(path):
        p, q = path.sample(t)
        rp, rq, regime, i = TR.sample_rule(path.times, path.positions, path.orientations, t)
        regimes.add(regime if regime != "inside" else ("inside", i))
        np.testing.assert_allclose(p, rp, rtol=0, atol=SAMPLE_ATOL)
        if path.has_orientation:
            np.testing.assert_allclose(q, rq, rtol=0, atol=SAMPLE_ATOL)
            assert abs(np.linalg.norm(q) - 1.0) <= 4e-16
        else:
            assert q is None and rq is None
    assert {"before", "after"} <= regimes
    assert {("inside", i) for i in range(len(path) - 1)} <= regimes
    for i, t in enumerate(path.times):   # on a waypoint the sample is the waypoint
        p, q = path.sample(t)
        np.testing.assert_allclose(p, path.positions[i], rtol=0, atol=SAMPLE_ATOL)
        if path.has_orientation:
            np.testing.assert_allclose(q, path.orientations[i], rtol=0, atol=SAMPLE_ATOL)


def test_the_interpolant_is_continuous_across_waypoints():
    path = TP.path_a()
    for t in path.times[1:-1]:
        lo, hi = path.sample(np.nextafter(t, -np.inf)), path.sample(np.nextafter(t, np.inf))
        np.testing.assert_allclose(lo[0], hi[0], rtol=0, atol=1e-13)
        np.testing.assert_allclose(lo[1], hi[1], rtol=0, atol=1e-13)


def test_sign_fix_and_normalisation():
    assert TP.raw_dots(TP.A_QUATERNIONS)[1] < 0.0 and TP.raw_dots(TP.C_QUATERNIONS)[2] < 0.0   # the fixtures do exercise it
    for path in (TP.path_a(), TP.path_b(), TP.path_c()):
        q = path.orientations
        np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, rtol=0, atol=4e-16)
        assert np.all(np.sum(q[1:] * q[:-1], axis=1) >= 0.0)
        raw = path.raw_orientations / np.linalg.norm(path.raw_orientations, axis=1)[:, None]
        sign = np.sum(raw * q, axis=1)
        np.testing.assert_allclose(np.abs(sign), 1.0, rtol=0, atol=1e-15)   # the same rotation, either sign
        # the interpolated quaternion's norm before the division is >= sqrt(1/2)
        for a, b in zip(q[:-1], q[1:]):
            for f in np.linspace(0.0, 1.0, 11):
                assert np.linalg.norm(a + f * (b - a)) >= np.sqrt(0.5) - 1e-15
    a = TP.path_a()
    assert np.array_equal(a.raw_orientations, np.asarray(TP.A_QUATERNIONS))
    assert np.sum(a.raw_orientations[2] * a.orientations[2]) < 0.0   # waypoint 2 was negated
    # the fix chains: each waypoint is compared with the one before it as already fixed
    chain = am.TargetPath((0.0, 1.0, 2.0), np.zeros((3, 3)), ((0, 0, 0, 1), (0, 0, 0.1, -1), (0, 0, 0.2, -1)))
    assert np.all(chain.orientations[:, 3] > 0.0)
    # to_c carries what was given; from_c takes stored values as they are
    c = a.to_c()
    assert c.count == 4 and c.has_orientation == 1 and list(c.waypoints[2].quaternion) == list(TP.A_QUATERNIONS[2])
    assert TP.path_a(False).to_c().has_orientation == 0


def test_refusals_that_need_no_device():
    ok_p = [(0.0, 0.0, 0.0)]
    with pytest.raises(ValueError):
        am.TargetPath((), np.zeros((0, 3)))
    with pytest.raises(ValueError):
        am.TargetPath(np.arange(33.0), np.zeros((33, 3)))
    assert len(am.TargetPath(np.arange(32.0), np.zeros((32, 3)))) == abi.MPPI_TARGET_WAYPOINTS_MAX == 32
    for times in ((0.0, 0.2, 0.1), (0.0, 0.1, 0.1), (0.0, np.nan, 0.2), (0.0, np.inf, 0.2)):
        with pytest.raises(ValueError):
            am.TargetPath(times, np.zeros((3, 3)))
    with pytest.raises(ValueError):
        am.TargetPath((0.0, 5e-324), np.zeros((2, 3)))   # 1 / (time difference) overflows
    with pytest.raises(ValueError):
        am.TargetPath((0.0,), [(0.0, np.nan, 0.0)])
    with pytest.raises(ValueError):
        am.TargetPath((0.0, 1.0), ok_p)   # one row per time
    for q in ((0, 0, 0, 0.49), (0, 0, 0, 2.01), (0, 0, 0, 0), (np.nan, 0, 0, 1), (np.inf, 0, 0, 1)):
        with pytest.raises(ValueError):
            am.TargetPath((0.0,), ok_p, [q])
    for q in ((0, 0, 0, 0.5), (0, 0, 0, 2.0)):
        assert am.TargetPath((0.0,), ok_p, [q]).orientations[0, 3] == 1.0
    with pytest.raises(ValueError):
        am.TargetPath((0.0,), ok_p, [(0, 0, 1)])
    t = am.TargetTracking()
    assert (t.orientation_weight, t.track_orientation) == (10.0, False) and t == am.TargetTracking.from_c(t.to_c())
    d = abi.mppi_target_tracking_config()
    am._lib.load().mppi_default_target_tracking_config(C.byref(d))
    assert (d.orientation_weight, d.track_orientation) == (10.0, 0)


def test_reference_grasp_rotation_matches_the_oracle():
    """The orientation term's precondition: the reference's Ree against the oracle object's
    end-effector rotation at state_space.py's states (the far yaws included), the tolerance
    test_link_positions_cpu.py uses for the positions."""
    model = O.default_model()
    x = am.huddled_state()
    dyn = O.OracleDynamics(x, model)
    assert len(SS.ENTRIES) > 40
    for entry in SS.ENTRIES:
        x = SS.state(entry)
        dyn.set_state(x, 0.0)
        ee = dyn.end_effector()
        pos, Ree = TR.grasp_rotation(model, x[:12])
        np.testing.assert_allclose(Ree.reshape(-1), ee[abi.MPPI_EE_ROTATION:abi.MPPI_EE_ROTATION + 9], rtol=0, atol=1e-12, err_msg=entry[0])
        np.testing.assert_allclose(pos, ee[:3], rtol=0, atol=1e-12, err_msg=entry[0])
        np.testing.assert_allclose(Ree @ Ree.T, np.eye(3), rtol=0, atol=1e-14)
        # the term is 0 at the frame's own orientation (the oracle's quaternion of the same rotation:
        # 3 - trace(Rt^T Ree) is then a sum of nine products' roundings, times the weight)
        q = ee[abi.MPPI_EE_QUATERNION:abi.MPPI_EE_QUATERNION + 4]
        assert abs(TR.orientation_term(10.0, q, Ree)) <= 1e-12, entry[0]
    Rz = am.quaternion_rotation((0.0, 0.0, np.sin(0.15), np.cos(0.15)))   # 0.3 rad about z
    assert abs(TR.orientation_term(10.0, (0, 0, 0, 1), Rz) - 40.0 * np.sin(0.15) ** 2) <= 1e-14
    np.testing.assert_allclose(Rz, LR._rz(0.3), rtol=0, atol=1e-16)


def _setup(name="r19_h33"):
    _, S, H, keep = by_name(name)[:4]
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=4)
    return conf, H, am.FrankaRidgebackDynamics(), am.TrackPoint(point=TP.POINT)


def test_constant_path_reproduces_the_plain_track_point_costs():
    """A one-waypoint path at the objective's point, and no path at all, against the plain TrackPoint
    composition (link_reference, pinned to the oracle's update by its scaffold): exactly; and against
    an OracleTrajectory's own costs at the bars."""
    conf, H, dyn, cost = _setup()
    cc, keepalive = conf.to_c()
    orc = O.OracleTrajectory(cc, dyn.descriptor(), cost.descriptor(), scalar=0, mode=0)
    rng = np.random.default_rng(5)
    orc.inject_noise(rng.standard_normal((orc.noise_draws(0.0), 12)) * np.sqrt(np.diag(conf.covariance)))
    x = am.huddled_state()
    orc.update(x, 0.0)
    eps, U = orc.noise(), np.zeros((H, 12))
    plain = LR.Composition(conf, dyn.model, cost, "zero").costs(x, U, eps)
    for tracking in (am.TargetTracking(), am.TargetTracking(5.0, True)):
        comp = TR.Composition(conf, dyn.model, cost, tracking)
        assert np.array_equal(comp.costs(x, U, eps), plain)
        assert comp.targets.books["none"] == H * len(eps)
        comp.set_path(TP.constant_path())
        assert np.array_equal(comp.costs(x, U, eps), plain)   # (positions only: no orientation term)
        assert comp.targets.books["before"] + comp.targets.books["after"] == H * len(eps) and not comp.targets.books["segments"]
    rel, _, _, worst = cost_errors(plain, orc.costs(), H)
    assert rel <= COST_RTOL and worst <= 1.0, (rel, worst)
    # a moving path and the orientation term do change the costs, and the read-out's sums are the terms'
    comp = TR.Composition(conf, dyn.model, cost, am.TargetTracking(10.0, True))
    comp.set_path(TP.path_a())
    J, pos, ori = comp.rollout(x, U + eps[3])
    assert J != plain[3] and np.all(pos >= 0.0) and np.all(ori >= 0.0) and ori.sum() > 0.0
    off = TR.Composition(conf, dyn.model, cost, am.TargetTracking(10.0, False))
    off.set_path(TP.path_a())
    J0, pos0, ori0 = off.rollout(x, U + eps[3])
    assert np.array_equal(pos0, pos) and not ori0.any() and abs((J - J0) - ori.sum()) <= 1e-12 * abs(J)


def test_path_a_covers_every_regime_in_one_horizon():
    """The parity tests' first path at t0 = 0 over 33 steps: steps before the first waypoint, steps in
    all three segments (so across both interior waypoints), steps past the last - from the reference's books."""
    targets = TR.Targets(am.TargetTracking(10.0, True), TP.POINT)
    targets.set_path(TP.path_a())
    for k in range(33):
        targets.at(0.0 + k * TIME_STEP)
    b = targets.books
    assert b["before"] == 5 and b["after"] == 7 and b["inside"] == 21 and b["segments"] == {0, 1, 2} and b["none"] == 0, b
    for t in TP.A_TIMES:   # no step of the grid falls on a waypoint, or within rounding of one
        assert abs(t / TIME_STEP - round(t / TIME_STEP)) > 0.4


def test_abi_structs(tmp_path):
    src = tmp_path / "sizes.c"
    items = [("sizeof(mppi_target_tracking_config)", C.sizeof(abi.mppi_target_tracking_config)),
             ("offsetof(mppi_target_tracking_config, track_orientation)", abi.mppi_target_tracking_config.track_orientation.offset),
             ("sizeof(mppi_target_waypoint)", C.sizeof(abi.mppi_target_waypoint)),
             ("offsetof(mppi_target_waypoint, position)", abi.mppi_target_waypoint.position.offset),
             ("offsetof(mppi_target_waypoint, quaternion)", abi.mppi_target_waypoint.quaternion.offset),
             ("sizeof(mppi_target_path)", C.sizeof(abi.mppi_target_path)),
             ("offsetof(mppi_target_path, has_orientation)", abi.mppi_target_path.has_orientation.offset),
             ("offsetof(mppi_target_path, waypoints)", abi.mppi_target_path.waypoints.offset),
             ("(size_t)MPPI_TARGET_WAYPOINTS_MAX", abi.MPPI_TARGET_WAYPOINTS_MAX)]
    body = "\n".join('printf("%%zu\\n", %s);' % expr for expr, _ in items)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mppi_amd.h"\nint main(void){%s return 0;}\n' % body)
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [v for _, v in items], list(zip(items, got))
    assert got[0] == 16 and got[2] == 64 and got[5] == 8 + 32 * 64
    L = am._lib.load()
    for name in ("mppi_set_target_tracking", "mppi_get_target_tracking", "mppi_set_target_path", "mppi_get_target_path",
                 "mppi_optimal_target_cost", "mppi_dynamics_target_cost", "mppi_default_target_tracking_config"):
        assert getattr(L, name) is not None


def test_cpp_target_surface_compiles_and_checks_the_layout():
    cpp = os.path.join(REPO, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "target_path.mk"])
    out = subprocess.run([os.path.join(cpp, "build", "target_path")], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    assert json.loads(out.stdout.decode().strip().split("\n")[0]) == {"cpu": "ok"}
