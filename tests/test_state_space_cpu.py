"""The oracle alone certifies tests/state_space.py, so that the GPU sweep over it
(test_gpu_state_space.py) cannot pass for the wrong reason: every entry reaches the branch it is in
the table for, with a margin the device's rounding cannot cross, and every state a horizon is
integrated from is one at which the oracle's own two operation orders agree far inside the bars."""
import numpy as np
import pytest

import assistedmanipulation_amd as am
from oracle import oracle as O

import state_space as SS
from helpers import COST_RTOL, cost_errors
from launch_shapes import horizon


@pytest.fixture(scope="module")
def model():
    return O.default_model()


def _kin(model, entry):
    x = SS.state(entry)
    return O.kinematics(model, x[:12], x[12:24], np.zeros(12), 0)


def barrier_branch(bound, scale, maximum, v, left):
    """The branch of the reference's barrier at v: "over" on or beyond the bound, else "sat" where
    scale / d reaches the maximum cost, else "free"."""
    d = (v - bound) if left else (bound - v)
    if d <= 0.0:
        return "over"
    with np.errstate(over="ignore"):
        return "sat" if np.float64(scale) / np.float64(d) >= maximum else "free"


def joint_branches(entry):
    """{"lower<j>": branch, "upper<j>": branch} of the default configuration's joint limits at q."""
    c = am.AssistedManipulation().configuration
    out = {}
    for j in range(12):
        lo, up = c.lower_joint_limit[j], c.upper_joint_limit[j]
        out["lower%d" % j] = barrier_branch(lo.bound, lo.scale, lo.maximum_cost, entry[1][j], True)
        out["upper%d" % j] = barrier_branch(up.bound, up.scale, up.maximum_cost, entry[1][j], False)
    return out


def workspace_branches(model, entry):
    """The three workspace barriers (assisted_manipulation.cpp workspace_cost) in numpy from the
    oracle's grasp-frame and arm-mount positions: the robot point is the arm mount + R_z(yaw)
    (0.1, 0, 0.15), forward = R_z(yaw) e_x."""
    c = am.AssistedManipulation().configuration
    k = _kin(model, entry)
    yaw = entry[1][2]
    fw = np.array([np.cos(yaw), np.sin(yaw), 0.0])
    t = k["ee"] - (k["arm_mount"] + np.array([0.1 * fw[0], 0.1 * fw[1], 0.15]))
    out = {}
    for name, b, v, left in (("infront", c.workspace_limit_infront, float(t @ fw), True),
                             ("reach", c.workspace_limit_reach, float(np.linalg.norm(t)), False),
                             ("above", c.workspace_limit_above, float(t[2]), True)):
        out[name] = barrier_branch(b.bound, b.scale, b.maximum_cost, v, left)
        out[name + "_distance"] = abs(v - b.bound)
    return out


def test_names_are_unique_and_uses_known():
    names = [e[0] for e in SS.ENTRIES]
    assert len(set(names)) == len(names)
    for e in SS.ENTRIES:
        assert len(e[1]) == 12 and set(e[3]) <= set("abcde") and "a" in e[3] and "b" in e[3] and "c" in e[3], e[0]
    # the far yaws and the edges are never integrated from
    for e in SS.ENTRIES:
        if e[0] in SS.FAR or e[0].startswith("j"):
            assert not set(e[3]) & set("de"), e[0]
    assert {e[0] for e in SS.using("d")} >= {"quat_w", "quat_x", "quat_y", "quat_z", "low_cost", "stretched", "ahead",
                                             "yaw_3pi4", "yaw_m6", "yaw_7", "yaw_m40", "yaw_100"}
    assert {e[0] for e in SS.using("e")} >= {"quat_z", "stretched", "yaw_100"}


def test_quaternion_branch_claims(model):
    """Each quat_* entry takes the branch its name says, by QUAT_MARGIN on the trace and on every
    diagonal comparison that decides it: the device and the oracle (rotations equal to ~1e-15) cannot
    disagree about the branch.  All four branches are claimed."""
    claimed = set()
    for e in SS.ENTRIES:
        for cl in e[4]:
            if cl.startswith("quat:"):
                branch, margin = SS.quaternion_branch(_kin(model, e)["R_ee"])
                assert branch == cl[5:], (e[0], branch, cl)
                assert margin >= SS.QUAT_MARGIN, (e[0], margin)
                claimed.add(branch)
    assert claimed == set("wxyz")
    # and no entry sits on a tie: the quaternion is compared with its sign at every entry
    for e in SS.ENTRIES:
        assert SS.quaternion_branch(_kin(model, e)["R_ee"])[1] >= 1e-3, e[0]
    for b in "wxyz":
        assert SS.quaternion_branch(_kin(model, SS.by_name("quat_" + b))["R_ee"])[0] == b


def test_quadrant_coverage():
    """rint(2 q / pi) of the revolute joints covers every n in -4 .. 4 over the table, and an even and
    an odd n of each sign among the far yaws; the tie entries sit on a tie to rounding."""
    seen = set()
    for e in SS.ENTRIES:
        seen |= set(int(n) for n in SS.quadrant(e[1]))
    assert seen >= set(range(-4, 5)), sorted(seen)
    far = [int(SS.quadrant(SS.by_name(n)[1])[0]) for n in SS.FAR]
    for sign in (1, -1):
        for parity in (0, 1):
            assert any(n * sign > 1000 and n % 2 == parity for n in far), (sign, parity, far)
    assert max(abs(SS.by_name(n)[1][2]) for n in SS.FAR) < 2.0 ** 26
    assert max(abs(SS.by_name(n)[1][2]) for n in SS.FAR) > 0.99 * 2.0 ** 26
    for name in ("yaw_3pi4", "yaw_mpi4", "yaw_5pi4"):
        y = 2.0 * SS.by_name(name)[1][2] / np.pi
        assert abs(abs(y - np.trunc(y)) - 0.5) <= 4 * np.finfo(np.float64).eps * abs(y), (name, y)


def test_barrier_branch_claims(model):
    """Every barrier branch claimed for an entry is the one the default configuration's bounds give,
    and the table covers: `over` and `under` of a lower and an upper joint limit, `under` saturated
    and unsaturated, and each workspace barrier on both sides.  The crossover entries sit within
    1e-6 relative of d = scale / max."""
    c = am.AssistedManipulation().configuration
    seen = set()
    for e in SS.ENTRIES:
        jb, wb = joint_branches(e), None
        for cl in e[4]:
            what, branch = cl.split(":")
            if what == "quat":
                continue
            if what in ("infront", "reach", "above"):
                wb = wb or workspace_branches(model, e)
                got = wb[what]
                assert wb[what + "_distance"] >= 1e-3, (e[0], cl, wb)   # the device cannot land on the other side
            else:
                got = jb[what]
            if branch == "cross":
                side, j = what[:5], int(what[5:])
                b = (c.lower_joint_limit if side == "lower" else c.upper_joint_limit)[j]
                x = b.scale / b.maximum_cost
                assert x > 0 and abs(abs(e[1][j] - b.bound) / x - 1.0) <= 1e-6, (e[0], cl)
                assert got in ("sat", "free")
            else:
                assert got == branch, (e[0], cl, got)
            seen.add((what.rstrip("0123456789"), branch))
    for side in ("lower", "upper"):
        for branch in ("over", "sat", "free", "cross"):
            assert (side, branch) in seen, (side, branch)
    # every joint-limit edge asked for is in the table: the bound, one ulp either side, beyond it
    names = {e[0] for e in SS.ENTRIES}
    for j in SS.EDGE_JOINTS:
        for side in ("lo", "up"):
            for tag in ("at", "in1", "out1", "out") + (("x", "xh", "x2") if c.lower_joint_limit[j].scale > 0 else ()):
                assert "j%d_%s_%s" % (j, side, tag) in names
    assert c.upper_joint_limit[6].bound == 0.0 and c.lower_joint_limit[10].bound == 0.0
    for what in ("infront", "reach", "above"):
        assert (what, "free") in seen, what
        assert (what, "over") in seen, what


@pytest.mark.parametrize("name", [e[0] for e in SS.ENTRIES if set(e[3]) & set("de")])
def test_oracle_orders_gap(name):
    """A condition on the inputs: at every state a horizon is integrated from, the oracle's own two
    operation orders (mode 0 against mode 1; 33 steps, 16 draws at the configured deviations, the
    objective without the three barrier families) differ by at most 0.2 COST_RTOL relative.  An
    entry that breaks this is replaced by a neighbouring pose, not given a looser bar."""
    e = SS.by_name(name)
    conf = am.frankaridgeback_configuration(rollouts=14, horison=horizon(33), keep_best_rollouts=5, threads=8)
    cc, keep = conf.to_c()
    cost = am.AssistedManipulation()
    c = cost.configuration
    c.enable_joint_limit = c.enable_self_collision_limit = c.enable_workspace_limit = 0
    d = am.FrankaRidgebackDynamics().descriptor()
    a, b = (O.OracleTrajectory(cc, d, cost.descriptor(), scalar=0, mode=m) for m in (0, 1))
    assert a.H == 33 and a.R == 16
    rng = np.random.default_rng(5)
    eps = rng.standard_normal((a.noise_draws(0.0), 12)) * np.sqrt(np.diag(conf.covariance))
    for t in (a, b):
        t.set_forecast(am.constant_forecast(t.H))
        t.inject_noise(eps)
        t.update(SS.state(e), 0.0)
    gap = cost_errors(b.costs(), a.costs(), a.H)[0]
    print("%s: oracle orders %.3e relative (%.3f COST_RTOL)" % (name, gap, gap / COST_RTOL))
    assert np.isfinite(a.costs()).all() and np.nanmax(a.costs()) < 1e9   # the barrier-free objective
    assert gap <= 0.2 * COST_RTOL, (name, gap)
