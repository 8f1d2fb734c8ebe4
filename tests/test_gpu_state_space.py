"""Device against oracle across the robot's state space (tests/state_space.py), not only at the
huddled pose: every quadrant of fsincos up to |x| just under 2^26, all four branches of the dynamics
object's rotation-to-quaternion code, the joint-limit barriers on, next to and beyond their bounds,
the saturated workspace barriers, and the stretched arm.  test_state_space_cpu.py certifies on the
CPU that the table's entries reach what they claim.

No test here has a bar of its own:
  (a) the object:         test_gpu_dynamics.py's STATE_RTOL, VEL_RTOL, ACC_RTOL, TAU_RTOL
  (b) get_cost:           1e-11 relative on the total, rtol 1e-10 / atol 1e-9 on the seven terms
                          (test_get_cost_against_object_matches_oracle's)
  (c) one-step horizon:   helpers.py's bars, FK_BAR = 1e-12 m, 1e-12 max(1, |p|) on the grasp frame
  (d) updates:            helpers.py's bars (the tank's: test_gpu_launch_shapes._bars)
  (e) predicted states:   30 times the oracle's own two-order gap measured by the test at that state,
                          never above test_gpu_predicted.py's CAPS, never below 100 eps
Each group prints its worst error over its bar at the end of the module.
"""
import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi
from oracle import oracle as O

import link_reference as LR
import state_space as SS
from helpers import COST_RTOL, assert_update_parity, cost_errors, energy_only_cost, fr_pair, step_both
from launch_shapes import by_name, horizon
from obstacle_sets import ARM_RADIUS
from test_gpu_dynamics import STATE_RTOL, _close, _controls, _tol_ee, _tol_query, _tol_state
from test_gpu_launch_shapes import _assert_launch, _bars
from test_gpu_parity import _track_point_all_terms
from test_gpu_predicted import CAPS, FK_BAR, _check_own, _errors, _oracle_states
from wrench_reference import Shift, shifted

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TIMES = [0.0, 0.05, 0.07]
WRENCH = np.array([20.0, 5.0, -3.0, 0.0, 0.0, 0.0])
ENV = ("MPPI_RELAY_K", "MPPI_TAIL_DRAWS", "MPPI_DRAW_AHEAD", "MPPI_LINK_POSITIONS", "MPPI_GRAPH", "MPPI_COSTS_IN_LAUNCH",
       "MPPI_HANDOVER", "MPPI_SPLIT", "MPPI_SIMULATED_WRENCH")
STATS = {}      # group -> (worst error over its bar, where)
BRANCHES = {}   # entry -> the quaternion branch of the device's own rotation after set_state


def _note(group, ratio, where):
    if ratio > STATS.get(group, (-1.0, ""))[0]:
        STATS[group] = (float(ratio), where)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for group in sorted(STATS):
        print("\nstate space %-22s worst error %.3e of its bar (%s)" % ((group,) + STATS[group]))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)


def _ratio(a, b, rtol):
    """test_gpu_dynamics._close's measure: the worst |a - b| / max(|b|, 1) over its tolerance."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1.0) / np.broadcast_to(rtol, b.shape)).max())


# ---- (a) the dynamics object ----------------------------------------------------------------------

def _object_compare(dev, orc, tag):
    """The end-effector row (position, quaternion with its sign, rotation, velocities, accelerations,
    Jacobian) and the query row.  The oracle's rotation must be off every tie of the quaternion's
    branches by far more than the rotations' bar, or the sign is a matter of rounding."""
    ed, eo = dev.get_end_effector_state_row(), orc.end_effector()
    Ro = eo[abi.MPPI_EE_ROTATION:abi.MPPI_EE_ROTATION + 9].reshape(3, 3)
    assert SS.quaternion_branch(Ro)[1] >= 1e3 * STATE_RTOL, tag + ": the reference sits on a quaternion branch tie"
    _note("a object EE", _ratio(ed, eo, _tol_ee()), tag)
    _close(ed, eo, _tol_ee(), tag + " EE")
    qd, qo = dev.query_row(), orc.query()
    _note("a object members", _ratio(qd, qo, _tol_query()), tag)
    _close(qd, qo, _tol_query(), tag + " members")
    return ed


@pytest.mark.parametrize("name", [e[0] for e in SS.using("a")])
def test_object_matches_oracle(name):
    """create (the constructor's set_state), set_state at another time, then five steps with
    test_gpu_dynamics._controls, at every entry of the table."""
    x0 = SS.state(SS.by_name(name), energy=15.0)
    dev = am.PinocchioDynamicsObject.create(x0)
    orc = O.OracleDynamics(x0)
    _object_compare(dev, orc, name + " create")
    dev.set_state(x0, 0.25)
    orc.set_state(x0, 0.25)
    ee = _object_compare(dev, orc, name + " set_state")
    Rd = ee[abi.MPPI_EE_ROTATION:abi.MPPI_EE_ROTATION + 9].reshape(3, 3)
    BRANCHES[name] = SS.quaternion_branch(Rd)[0]
    qv = ee[abi.MPPI_EE_QUATERNION:abi.MPPI_EE_QUATERNION + 4]
    assert abs(np.linalg.norm(qv) - 1.0) < 1e-14
    assert qv["xyzw".index(BRANCHES[name])] > 0.0   # Eigen's branch makes its own component positive
    for k, u in enumerate(_controls(np.random.default_rng(3), 5)):
        xd, xo = dev.step(u, 0.01), orc.step(u, 0.01)
        _note("a object state", _ratio(xd, xo, _tol_state()), "%s step %d" % (name, k))
        _close(xd, xo, _tol_state(), "%s state step %d" % (name, k))
        _object_compare(dev, orc, "%s step %d" % (name, k))


def test_every_quaternion_branch_entered():
    """From the device's own rotation matrices: all four branches, each at the entry named for it."""
    for e in SS.using("a"):
        if e[0] not in BRANCHES:   # (run alone: the object test fills it)
            dev = am.PinocchioDynamicsObject.create(SS.state(e))
            R = dev.get_end_effector_state_row()[abi.MPPI_EE_ROTATION:abi.MPPI_EE_ROTATION + 9].reshape(3, 3)
            BRANCHES[e[0]] = SS.quaternion_branch(R)[0]
    assert set(BRANCHES.values()) == set("wxyz"), BRANCHES
    for b in "wxyz":
        assert BRANCHES["quat_" + b] == b, BRANCHES


# ---- (b) get_cost against the object --------------------------------------------------------------

def _tank():
    cost = am.AssistedManipulation()
    cost.configuration.enable_energy_limit = 1
    return cost


OBJECTIVES = {"default": am.AssistedManipulation, "tank": _tank, "track_point": _track_point_all_terms}


def _right_barrier(b, v):
    """link_reference.left_barrier's mirror image: the reference's right barrier."""
    if v >= b.bound:
        d = v - b.bound
        return b.maximum_cost + b.scale * (d * d)
    with np.errstate(divide="ignore"):
        return min(np.float64(b.scale) / np.float64(b.bound - v), b.maximum_cost)


def _joint_limit_term(c, q):
    """AssistedManipulation's joint-limit term in numpy, each barrier on its own branch, summed as the
    device sums it: (joints 0 .. 5) + (6 .. 11)."""
    with np.errstate(divide="ignore", over="ignore"):
        t = [LR.left_barrier(c.lower_joint_limit[j], np.float64(q[j])) + _right_barrier(c.upper_joint_limit[j], q[j])
             for j in range(12)]
    return float(sum(t[:6], 0.0) + sum(t[6:], 0.0))


@pytest.mark.parametrize("objective", list(OBJECTIVES))
@pytest.mark.parametrize("name", [e[0] for e in SS.using("b")])
def test_get_cost_matches_oracle(name, objective):
    """Set the state, take one step, then evaluate: at the entry's own state (the joints exactly on
    the table's edges, against the kinematics the step cached) and at the stepped state.  On a bound
    and one ulp either side both totals are finite, and the joint term is the numpy barrier's on
    the branch the CPU test certified."""
    cost = OBJECTIVES[objective]()
    x0 = SS.state(SS.by_name(name), energy=15.0)
    dev = am.PinocchioDynamicsObject.create(x0)
    orc = O.OracleDynamics(x0)
    dev.set_state(x0, 0.0)
    orc.set_state(x0, 0.0)
    u = _controls(np.random.default_rng(4), 1)[0]
    x1 = orc.step(u, 0.01)
    dev.step(u, 0.01)
    for what, x in (("x0", x0), ("x1", x1)):
        tag = "%s %s %s" % (name, objective, what)
        cd, td = am.evaluate_cost(cost, dev, x, u, WRENCH)
        co, to = orc.evaluate_cost(cost.descriptor(), x, WRENCH)
        assert np.isfinite(co) and np.isfinite(to).all(), (tag, co, to)
        assert np.isfinite(cd) and np.isfinite(td).all(), (tag, cd, td)
        _note("b get_cost total", abs(cd - co) / (1e-11 * max(abs(co), 1.0)), tag)
        _note("b get_cost terms", float((np.abs(td - to) / (1e-9 + 1e-10 * np.abs(to))).max()), tag)
        assert abs(cd - co) <= 1e-11 * max(abs(co), 1.0), (tag, cd, co)
        np.testing.assert_allclose(td, to, rtol=1e-10, atol=1e-9, err_msg=tag + " terms")
        if objective != "track_point":
            ref = _joint_limit_term(cost.configuration, x[:12])
            np.testing.assert_allclose([to[0], td[0]], [ref, ref], rtol=1e-10, atol=1e-9, err_msg=tag + " joint term")


# ---- (c) fsincos at x0: the one-step horizon --------------------------------------------------------

def _arm004():
    cost = am.AssistedManipulation()
    for i in range(1, 8):
        cost.configuration.self_collision_radii[i] = ARM_RADIUS
    return cost


def _check_predicted_x0(dev, x0, tag, model):
    """Row 0 of the optimal and of every sampled rollout: x0 itself, and forward kinematics at it."""
    k = O.kinematics(model, x0[:12], x0[12:24], np.zeros(12), 0)
    for what, pred in (("optimal", dev.predicted_optimal()), ("rollouts", dev.predicted_rollouts(np.arange(dev.R)))):
        err = _check_own(pred, x0, dev.get_time_step(), "%s %s" % (tag, what))   # links, grasp frame, arm mount: FK_BAR
        _note("c predicted FK", err / FK_BAR, tag)
        ee = pred.end_effector.reshape(-1, 3)
        bar = 1e-12 * max(1.0, np.abs(k["ee"]).max())
        _note("c grasp frame", np.abs(ee - k["ee"]).max() / bar, tag)
        assert np.abs(ee - k["ee"]).max() <= bar, (tag, what, ee[0], k["ee"])


@pytest.mark.parametrize("name", [e[0] for e in SS.using("c")])
def test_one_step_horizon(name):
    """H = 1: record 0 is x0 itself, so the objective's and the predicted rows' fsincos take the sine
    of the same double as the oracle, the far yaws included.  r19_h1 (the x kernel) and r3_h33's
    one-wave kernel shortened to one step, host-injected noise, one update each; then r19_h1 with the
    kinematic link positions and 0.04 arm radii, whose live self-collision term (link_fk's own
    fsincos) is checked against link_reference's composition."""
    x0 = SS.state(SS.by_name(name))
    model = O.default_model()
    for S, keep in ((by_name("r19_h1")[1], by_name("r19_h1")[3]), (by_name("r3_h33")[1], by_name("r3_h33")[3])):
        tag = "%s r%d_h1" % (name, S + 2)
        conf, dev, orc, sd = fr_pair(S=S, horison=horizon(1), K=keep)
        assert dev.H == 1 and dev.R == S + 2
        step_both(dev, orc, x0, 0.0, np.random.default_rng(3), sd)
        assert dev.update_info()["wait_timeouts"] == 0
        stats = []
        # (the costs are flat: the early return, so the weights and U* compared are the untouched ones)
        assert_update_parity(dev, orc, tag, stats=stats)
        _note("c cost", stats[0][1] / COST_RTOL, tag)
        _check_predicted_x0(dev, x0, tag, model)
    S, keep = by_name("r19_h1")[1], by_name("r19_h1")[3]
    tag = name + " r19_h1 links"
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(1), keep_best_rollouts=keep, threads=8)
    dyn, cost, table = am.FrankaRidgebackDynamics(link_positions=True), _arm004(), am.constant_forecast(1)
    dev = am.Trajectory.create(conf, dyn, cost)
    assert dev is not None and dev.H == 1 and dev.link_positions
    dev.set_noise_source(abi.MPPI_NOISE_HOST_INJECTED)
    dev.set_forecast(table)
    sd = np.sqrt(np.diag(conf.covariance))
    dev.inject_noise(np.random.default_rng(11).standard_normal((dev.noise_draws(0.0), dev.C)) * sd)
    dev.update(x0, 0.0)
    comp = LR.Composition(conf, dyn.model, cost, "kinematic", table)
    J, Jd = comp.costs(x0, np.zeros((1, dev.C)), dev.noise()), dev.costs()
    assert np.isfinite(J).all() and np.isfinite(Jd).all(), tag
    rel = cost_errors(Jd, J, 1)[0]
    _note("c cost, live links", rel / COST_RTOL, tag)
    assert rel <= COST_RTOL, "%s cost rel err %.3e" % (tag, rel)
    np.testing.assert_array_equal(dev.get_optimal_rollout(), np.zeros((1, dev.C)))   # flat costs: the early return
    _check_predicted_x0(dev, x0, tag, model)


# ---- (d) updates away from the huddled pose -------------------------------------------------------

def _no_self_collision():
    cost = am.AssistedManipulation()
    cost.configuration.enable_self_collision_limit = 0
    return cost


UPDATE_COSTS = {"am": am.AssistedManipulation, "energy": energy_only_cost, "track_point": _track_point_all_terms,
                "no_self_collision": _no_self_collision}
THREE = ["quat_z", "stretched", "yaw_100"]
UPDATE_CASES = ([(e[0], "r20_h33", "am") for e in SS.using("d") if e[0] != "huddled"]
                + [(n, s, "am") for s in ("r48_h33", "r10_h33", "r147_h33") for n in THREE]
                + [(n, "r20_h33", o) for o in ("energy", "track_point", "no_self_collision") for n in THREE])


@pytest.mark.parametrize("name,shape,objective", UPDATE_CASES)
def test_updates_match_oracle(name, shape, objective):
    """Three updates at 0, 0.05 and 0.07 s (shifts of 0, 5 and 2 steps) from the entry's state with
    the moving velocity, host-injected noise: assert_update_parity at helpers.py's bars, the launch
    the table of launch_shapes.py expects, and the folded filter() row where the launch folds it."""
    _, S, H, keep, req, sw, first, pend = by_name(shape)
    entry = SS.by_name(name)
    assert entry[2], name   # the moving velocity
    x0 = SS.state(entry, energy=15.0 if objective == "energy" else 100.0)
    conf, dev, orc, sd = fr_pair(S=S, horison=horizon(H), K=keep, cost=UPDATE_COSTS[objective]())
    assert dev.H == H and dev.R == S + 2
    rng = np.random.default_rng(3)
    bars = _bars(objective, shape)
    prev_opt, stats = None, []
    for j, t in enumerate(TIMES):
        tag = "%s %s %s upd %d" % (name, shape, objective, j)
        step_both(dev, orc, x0, t, rng, sd)
        if _assert_launch(dev, S, first if j == 0 else pend, tag):
            got = dev.debug_folded_cost()
            assert abs(got - prev_opt) <= bars.get("cost_rtol", COST_RTOL) * max(1.0, abs(prev_opt)), (tag, got, prev_opt)
        assert_update_parity(dev, orc, tag, stats=stats, check_optimal=j + 1 == len(TIMES), **bars)
        prev_opt = orc.optimal_cost()
    for tag, rel, dfrac, sfrac, worst in stats:
        _note("d cost rel, " + objective, rel / bars.get("cost_rtol", COST_RTOL), tag)
        _note("d cost allowance, " + objective, worst, tag)


# ---- (e) predicted states ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", THREE)
def test_predicted_states(name):
    """test_gpu_predicted.py's checks (a), (b) and (c) at r20_h33: row 0 is x0, the Euler identity on
    the device's own rows, and q, qd against the oracle stepping.  The bar of (c) is never taken from
    the device: the test measures the oracle's own two operation orders at this state (the final q
    and qd of O.rollout in mode 0 against mode 1 over the same controls, worst over the rows), and the
    bar is 30 times that gap - the device sits at 1.4 to 2.2 times the oracle's gap in the project's
    records (test_gpu_launch_shapes.LOOSER) - at most CAPS, at least 100 eps.
    Measured on an MI355X, worst over the three updates, device q / qd against the
    oracle's own gap q / qd: quat_z 1.7e-12 / 7.7e-12 against 1.3e-12 / 7.4e-12, stretched 1.9e-12 /
    9.5e-12 against 2.9e-12 / 6.6e-12, yaw 100 9.0e-13 / 7.2e-12 against 2.2e-12 / 3.1e-12; the worst
    single update is stretched's first, qd 8.9e-12 against a gap of 1.3e-12: 0.23 of its bar."""
    _, S, H, keep, req, sw, first, pend = by_name("r20_h33")
    x0 = SS.state(SS.by_name(name))
    conf, dev, orc, sd = fr_pair(S=S, horison=horizon(H), K=keep)
    dyn, model, cconf = O.OracleDynamics(x0), O.default_model(), am.AssistedManipulation().configuration
    dt = dev.get_time_step()
    rng, shift = np.random.default_rng(3), Shift()
    worst = [0.0, 0.0, 0.0, 0.0]   # device q, qd; oracle gap q, qd
    for j, t in enumerate(TIMES):
        tag = "%s upd %d" % (name, j)
        U_shift = shifted(dev.get_optimal_rollout(), shift(t, dt))
        step_both(dev, orc, x0, t, rng, sd)
        assert dev.update_info()["wait_timeouts"] == 0
        noise = dev.noise()
        pred = dev.predicted_rollouts(np.arange(dev.R))
        _check_own(pred, x0, dt, tag)
        gq = gv = 0.0
        for r in range(dev.R):
            xa, xb = (O.rollout(model, cconf, x0, U_shift + noise[r], dt, t, mode=m)[2] for m in (0, 1))
            g = _errors(xb[None], xa[None])
            gq, gv = max(gq, g[0]), max(gv, g[1])
        ref = np.stack([_oracle_states(dyn, x0, t, U_shift + noise[r], dt) for r in range(dev.R)])
        eq, ev = _errors(pred.raw, ref)
        bq, bv = (min(cap, max(30.0 * g, 100.0 * EPS)) for g, cap in zip((gq, gv), CAPS[False]))
        print("%s: device q %.3e qd %.3e, oracle orders q %.3e qd %.3e, bars %.3e %.3e" % (tag, eq, ev, gq, gv, bq, bv))
        worst = [max(a, b) for a, b in zip(worst, (eq, ev, gq, gv))]
        _note("e predicted q", eq / bq, tag)
        _note("e predicted qd", ev / bv, tag)
        assert eq <= bq and ev <= bv, "%s: q err %.3e (bar %.1e), qd err %.3e (bar %.1e)" % (tag, eq, bq, ev, bv)
    # the optimal row after the last update (reading it runs the pending filter()), at that update's bars
    pred = dev.predicted_optimal()
    _check_own(pred, x0, dt, name + " optimal")
    eq, ev = _errors(pred.raw, _oracle_states(dyn, x0, TIMES[-1], dev.get_optimal_rollout(), dt))
    _note("e predicted q", eq / bq, name + " optimal")
    _note("e predicted qd", ev / bv, name + " optimal")
    assert eq <= bq and ev <= bv, "%s optimal: q err %.3e (bar %.1e), qd err %.3e (bar %.1e)" % (name, eq, bq, ev, bv)
    print("%s: worst device q %.3e qd %.3e; oracle orders q %.3e qd %.3e" % ((name,) + tuple(worst)))
