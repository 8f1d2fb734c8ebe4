"""Obstacle avoidance without a GPU: the numpy reference of obstacle_reference.py against clearances
and barrier values worked out by hand, the mask, a moving obstacle, the composition with an empty
set, the guards the GPU tests rely on (checked here on the reference alone), and the library's
host-side surface: symbols, struct layouts, defaults and the clearance helper."""
import ctypes as C
import re

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi
from assistedmanipulation_amd._lib import HEADER, load
from oracle import oracle as O

import link_reference as LR
import obstacle_reference as OR
import obstacle_sets as SETS
from launch_shapes import by_name, horizon

NEW_SYMBOLS = ["mppi_default_obstacle_config", "mppi_set_obstacle_avoidance", "mppi_get_obstacle_avoidance", "mppi_set_obstacles",
               "mppi_get_obstacles", "mppi_optimal_obstacle_cost", "mppi_dynamics_obstacle_cost"]


def _points():
    """Nine points on a line along x, one metre apart, at height 1."""
    return np.array([[float(i), 0.0, 1.0] for i in range(9)])


def test_sphere_by_hand():
    """Sphere of radius 0.25 centred on point 3, all radii 0.5: point 3 is 0.75 inside (saturated:
    1e10 + 0.75^2), points 2 and 4 clear by 0.25 (inverse: 4), 1 and 5 by 1.25 (0.8), 0 and 6 by
    2.25, 7 by 3.25, 8 by 4.25."""
    conf = am.ObstacleAvoidance(radii=(0.5,) * 9)
    ob = am.SphereObstacle((3.0, 0.0, 1.0), 0.25)
    v = OR.clearance(ob, np.asarray(conf.radii), _points(), 0.0)
    np.testing.assert_allclose(v, [2.25, 1.25, 0.25, -0.75, 0.25, 1.25, 2.25, 3.25, 4.25], rtol=0, atol=1e-15)
    t = OR.Term(conf, [ob], 0.0)
    want = (1e10 + 0.75 ** 2) + 2 * 4.0 + 2 * 0.8 + 2 / 2.25 + 1 / 3.25 + 1 / 4.25
    assert abs(t.at(_points(), 0.0) - want) <= 1e-15 * want
    assert t.branches == [{"inverse", "saturated"}] and t.least_v == -0.75 and t.least_margin == 0.25 and t.evaluated == 9


def test_half_space_by_hand():
    """The plane x = 2.5 with free space towards +x (normal (1, 0, 0)), radii 0.25: v = x - 2.5 -
    0.25; points 0..2 are inside the solid (saturated), 3.. clear by 0.25, 1.25, ...  The radius
    field is ignored, and so is the position's component along the plane."""
    conf = am.ObstacleAvoidance(limit=(0.0, 2.0, 1e6), radii=(0.25,) * 9)
    ob = am.HalfSpaceObstacle((2.5, 7.0, -3.0), (1.0, 0.0, 0.0))
    ob.radius = 123.0
    v = OR.clearance(ob, np.asarray(conf.radii), _points(), 0.0)
    np.testing.assert_allclose(v, [x - 2.75 for x in range(9)], rtol=0, atol=1e-15)
    t = OR.Term(conf, [ob], 0.0)
    want = sum(1e6 + 2.0 * (2.75 - x) ** 2 for x in range(3)) + sum(2.0 / (x - 2.75) for x in range(3, 9))
    assert abs(t.at(_points(), 0.0) - want) <= 1e-15 * want
    # a nonzero bound shifts the branch point: v <= bound is saturated
    t2 = OR.Term(am.ObstacleAvoidance(limit=(0.3, 1.0, 1e6), radii=(0.25,) * 9), [ob], 0.0)
    want2 = sum(1e6 + (0.3 - (x - 2.75)) ** 2 for x in range(4)) + sum(1.0 / (x - 2.75 - 0.3) for x in range(4, 9))
    assert abs(t2.at(_points(), 0.0) - want2) <= 1e-15 * want2


def test_mask():
    conf = am.ObstacleAvoidance(radii=(0.5,) * 9)
    full = OR.Term(conf, [am.SphereObstacle((3.0, 0.0, 1.0), 0.25)], 0.0).at(_points(), 0.0)
    # without the penetrating point the 1e10 is gone; one point alone gives its own barrier
    t = OR.Term(conf, [am.SphereObstacle((3.0, 0.0, 1.0), 0.25, mask=0x1FF & ~(1 << 3))], 0.0)
    assert abs(t.at(_points(), 0.0) - (full - (1e10 + 0.75 ** 2))) < 1e-5 and t.branches == [{"inverse"}] and t.evaluated == 8
    t = OR.Term(conf, [am.SphereObstacle((3.0, 0.0, 1.0), 0.25, mask=1 << 8)], 0.0)
    assert t.at(_points(), 0.0) == 1.0 / 4.25 and t.evaluated == 1
    t = OR.Term(conf, [am.SphereObstacle((3.0, 0.0, 1.0), 0.25, mask=0)], 0.0)
    assert t.at(_points(), 0.0) == 0.0 and t.evaluated == 0 and t.least_margin == np.inf
    # two obstacles add up, obstacle by obstacle
    two = OR.Term(conf, [am.SphereObstacle((3.0, 0.0, 1.0), 0.25, mask=1 << 8), am.HalfSpaceObstacle((-1, 0, 0), (1, 0, 0), mask=1)], 0.0)
    assert two.at(_points(), 0.0) == 1.0 / 4.25 + 1.0 / 0.5


def test_moving_obstacle_at_three_times():
    """A sphere leaving point 0 along +x at 2 m/s, seen from point 0 alone: at tau = 0.5, 1.0 and
    -0.5 its centre is at x = 1, 2 and -1; radii 0.25 + 0.25."""
    conf = am.ObstacleAvoidance(radii=(0.25,) * 9)
    ob = am.SphereObstacle((0.0, 0.0, 1.0), 0.25, velocity=(2.0, 0.0, 0.0), mask=1)
    for tau, centre_x in ((0.5, 1.0), (1.0, 2.0), (-0.5, -1.0)):
        t = OR.Term(conf, [ob], 0.0)
        assert t.at(_points(), tau) == 1.0 / (abs(centre_x) - 0.5)
    # steps(): tau_k = (t0 + k dt) - t_ref, at the lagged configuration
    model = O.default_model()
    q = am.huddled_state()[:12]
    qs = np.array([q, q + 0.01, q + 0.02])
    t = OR.Term(am.ObstacleAvoidance(), [am.SphereObstacle((3.0, 0.0, 1.0), 0.2, velocity=(-1.0, 0.0, 0.0))], 0.25)
    got = t.steps(model, qs, 1.0, 0.5)
    for k in range(3):
        again = OR.Term(am.ObstacleAvoidance(), t.obstacles, 0.25).at(OR.robot_points(model, qs[max(k - 1, 0)]), (1.0 + k * 0.5) - 0.25)
        assert got[k] == again
    assert got[0] != got[1] != got[2]


def test_robot_points_are_the_link_model():
    model = O.default_model()
    q = am.huddled_state()[:12]
    links, ee, _ = LR.fk(model, q)
    p = OR.robot_points(model, q)
    assert p.shape == (9, 3) and np.array_equal(p[:8], links[abi.MPPI_LINK_PIVOT:abi.MPPI_LINK_PANDA_LINK7 + 1]) and np.array_equal(p[8], ee)
    np.testing.assert_allclose(p[0], [0.2, 0.2, 0.0], rtol=0, atol=1e-12)   # the base sphere sits on the floor


def _updates(name, sets, objective="am", n_rollouts=None):
    """Three reference-only updates in the GPU test's pattern; yields (j, comp, J)."""
    _, S, H, keep = by_name(name)[:4]
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=4)
    model = am.FrankaRidgebackDynamics().model
    comp = OR.Composition(conf, model, SETS.objective(objective), am.constant_forecast(H))
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance))
    U = np.zeros((H, 12))
    x = am.huddled_state()
    R = n_rollouts or S + 2
    for j, (obstacles, t_ref) in enumerate(sets):
        x = x.copy()
        x[3 + j] += 0.03
        term = comp.set_obstacles(obstacles, t_ref)
        eps = rng.standard_normal((R, H, 12)) * sd
        eps[0] = 0.0
        J = comp.costs(x, U, eps)
        yield j, comp, term, J, (x, U, eps)
        _, _, U = LR.mppi_update(conf, J, eps, U)


def test_empty_set_reproduces_the_kinematic_composition_bit_for_bit():
    for j, comp, term, J, (x, U, eps) in _updates("r19_h33", [([], 0.0), ([], -0.07)], n_rollouts=6):
        base = comp.base.costs(x, U, eps)
        assert np.array_equal(J, base) and term.evaluated == 0


def test_the_sets_meet_the_guards_on_the_reference():
    """What test_gpu_obstacles.py asserts from the reference's own books, here without a device at
    r19_h33: set A stays 0.02 m clear on the inverse branch, set B takes both branches on both of
    its spheres, nothing comes within 1e-6 of the branch discontinuity, and the term moves the costs."""
    sets = [(SETS.set_a(), SETS.T_REF_A), (SETS.set_b(), 0.0), ([], 0.0)]
    for j, comp, term, J, (x, U, eps) in _updates("r19_h33", sets):
        assert not np.isnan(J).any()
        if j == 0:
            assert term.least_v >= 0.02 and all(b == {"inverse"} for b in term.branches), (term.least_v, term.branches)
        if j == 1:
            assert all(b == {"inverse", "saturated"} for b in term.branches), term.branches
        if j < 2:
            assert term.least_margin >= 1e-6, (j, term.least_margin)
            assert np.abs(J - comp.base.costs(x, U, eps)).min() > 1e-3
    full = OR.Term(am.ObstacleAvoidance(), SETS.set_16(), 0.0)
    full.at(OR.robot_points(O.default_model(), am.huddled_state()[:12]), 0.1)
    assert full.least_margin >= 1e-6 and all(full.branches)


# ---- the library, without a device --------------------------------------------------------------

def test_symbols_and_version():
    L = load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert L.mppi_abi_version() == 5
    text = open(HEADER).read()
    assert re.search(r"^#define MPPI_AMD_ABI_VERSION 5\b", text, re.M)
    for macro in ("MPPI_MAX_OBSTACLES", "MPPI_OBSTACLE_POINTS", "MPPI_OBSTACLE_SPHERE", "MPPI_OBSTACLE_HALF_SPACE"):
        m = re.search(r"^#define %s (\d+)\b" % macro, text, re.M)
        assert m and int(m.group(1)) == getattr(abi, macro), macro


def test_struct_layouts_match_the_header():
    """mppi_obstacle: int32, uint32, then 3 + 3 + 3 + 1 doubles = 88 bytes, 8-aligned; the
    configuration: a barrier (3 doubles) and 9 radii = 96 bytes."""
    assert C.sizeof(abi.mppi_obstacle) == 4 + 4 + 10 * 8 == 88 and C.alignment(abi.mppi_obstacle) == 8
    assert abi.mppi_obstacle.mask.offset == 4 and abi.mppi_obstacle.position.offset == 8
    assert abi.mppi_obstacle.velocity.offset == 32 and abi.mppi_obstacle.normal.offset == 56 and abi.mppi_obstacle.radius.offset == 80
    assert C.sizeof(abi.mppi_obstacle_config) == (3 + 9) * 8 == 96 and abi.mppi_obstacle_config.radii.offset == 24
    # the header's declarations, field for field
    text = open(HEADER).read()
    body = re.search(r"typedef struct mppi_obstacle \{(.*?)\} mppi_obstacle;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [f.strip() for f in body.split(";") if f.strip()] == ["int32_t kind", "uint32_t mask",
                                                                 "double position[3], velocity[3], normal[3], radius"]
    body = re.search(r"typedef struct mppi_obstacle_config \{(.*?)\} mppi_obstacle_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [f.strip() for f in body.split(";") if f.strip()] == ["mppi_barrier limit", "double radii[MPPI_OBSTACLE_POINTS]"]


def test_default_configuration():
    c = abi.mppi_obstacle_config()
    load().mppi_default_obstacle_config(C.byref(c))
    assert (c.limit.bound, c.limit.scale, c.limit.maximum_cost) == (0.0, 1.0, 1e10)
    assert list(c.radii) == [0.75] + [0.1] * 8
    assert am.ObstacleAvoidance.from_c(c) == am.ObstacleAvoidance()
    assert list(c.radii[:8]) == [float(r) for r in am.AssistedManipulation().configuration.self_collision_radii]
    back = am.ObstacleAvoidance(limit=(0.1, 2.0, 1e6), radii=tuple(0.01 * i for i in range(9)))
    assert am.ObstacleAvoidance.from_c(back.to_c()) == back
    with pytest.raises(ValueError):
        am.ObstacleAvoidance(radii=(0.1,) * 8)


def test_obstacle_objects_round_trip():
    s = am.SphereObstacle((1, 2, 3), 0.5, velocity=(0.1, 0.2, 0.3), mask=0x155)
    h = am.HalfSpaceObstacle((0, 0, -1), (0, 0, 1))
    assert s.kind == abi.MPPI_OBSTACLE_SPHERE and h.kind == abi.MPPI_OBSTACLE_HALF_SPACE and h.mask == 0x1FF and h.radius == 0.0
    from assistedmanipulation_amd.obstacles import obstacle_from_c, obstacles_to_c
    arr, n = obstacles_to_c([s, h])
    assert n == 2 and len(arr) == abi.MPPI_MAX_OBSTACLES
    s2, h2 = obstacle_from_c(arr[0]), obstacle_from_c(arr[1])
    assert isinstance(s2, am.SphereObstacle) and np.array_equal(s2.centre, s.centre) and s2.radius == 0.5 and s2.mask == 0x155
    assert np.array_equal(s2.velocity, s.velocity)
    assert isinstance(h2, am.HalfSpaceObstacle) and np.array_equal(h2.normal, [0, 0, 1]) and np.array_equal(h2.point, [0, 0, -1])
    np.testing.assert_allclose(s.at(2.0), [1.2, 2.4, 3.6])
    # a mask that does not fit the 32-bit field is refused here, not truncated to an accepted one
    for bad in (1 << 32, (1 << 32) | 1, -1):
        with pytest.raises(ValueError):
            obstacles_to_c([am.SphereObstacle((1, 2, 3), 0.5, mask=bad)])
    assert obstacles_to_c([am.SphereObstacle((1, 2, 3), 0.5, mask=0x200)])[0][0].mask == 0x200   # the engine's to refuse


def test_obstacle_clearance_on_a_synthetic_predicted():
    """A Predicted of two rollouts over three steps whose links and end effector are put by hand:
    every point at the origin except PANDA_LINK7 (point 7), which walks along x, and the end effector
    (point 8) 1 m above it.  Positions at q_k, not lagged: row k is compared with the obstacle at
    time[k] - t_ref."""
    H = 3
    raw = np.zeros((2, H, abi.MPPI_PRED_N))
    for r in range(2):
        for k in range(H):
            x = 1.0 + k + 10.0 * r
            raw[r, k, abi.MPPI_PRED_LINKS + 3 * abi.MPPI_LINK_PANDA_LINK7:][:3] = (x, 0.0, 0.0)
            raw[r, k, abi.MPPI_PRED_EE:abi.MPPI_PRED_EE + 3] = (x, 0.0, 1.0)
    pred = am.Predicted(raw, 0.5, 0.1, rollouts=[0, 1])
    conf = am.ObstacleAvoidance(radii=(0.1,) * 9)
    wall = am.HalfSpaceObstacle((0.5, 0, 0), (1, 0, 0), mask=(1 << 7) | (1 << 8))       # v = x - 0.5 - 0.1
    got = am.obstacle_clearance(pred, conf, [wall], 0.0)
    assert got.shape == (2, H)
    np.testing.assert_allclose(got, [[0.4, 1.4, 2.4], [10.4, 11.4, 12.4]], rtol=0, atol=1e-12)
    # a sphere that flies at PANDA_LINK7 of rollout 0 from x = 5 at 10 m/s, given at t_ref = 0.4:
    # tau = 0.1, 0.2, 0.3 -> centre x = 4, 3, 2 against the link at 1, 2, 3; the end effector is 1 m higher
    ball = am.SphereObstacle((5.0, 0, 0), 0.2, velocity=(-10.0, 0, 0), mask=(1 << 7) | (1 << 8))
    got = am.obstacle_clearance(pred, conf, [ball], 0.4)
    np.testing.assert_allclose(got[0], [3.0 - 0.3, 1.0 - 0.3, 1.0 - 0.3], rtol=0, atol=1e-12)
    # every point: the base and the other links sit at the origin, inside the wall's solid
    got = am.obstacle_clearance(pred, conf, [am.HalfSpaceObstacle((0.5, 0, 0), (1, 0, 0))], 0.0)
    np.testing.assert_allclose(got, np.full((2, H), -0.6), rtol=0, atol=1e-12)
    assert np.all(np.isinf(am.obstacle_clearance(pred, conf, [], 0.0)))
    assert "not lagged" in am.obstacle_clearance.__doc__.lower().replace("\n", " ") or "NOT lagged" in am.obstacle_clearance.__doc__
    # the optimal rollout's Predicted has no rollout axis
    assert am.obstacle_clearance(am.Predicted(raw[0], 0.5, 0.1), conf, [wall], 0.0).shape == (H,)
