"""Obstacle avoidance with capsules without a GPU: the segment-segment distance of capsule_reference.py
against answers worked out by hand, the hole the capsules close (an obstacle inside a link, between two
robot points), the half-space and zero-length cases, the reference against obstacle_reference.py where
the two must agree bit for bit, the guards the GPU tests rely on, and the library's host-side surface:
symbols, struct layout, defaults, the Python round trips and the clearance helper."""
import ctypes as C
import re

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi
from assistedmanipulation_amd._lib import HEADER, load
from oracle import oracle as O

import capsule_reference as CR
import capsule_sets as CS
import link_reference as LR
import obstacle_reference as OR
import obstacle_sets as SETS
from launch_shapes import by_name, horizon

NEW_SYMBOLS = ["mppi_default_capsule_config", "mppi_set_obstacle_capsules", "mppi_get_obstacle_capsules", "mppi_dynamics_capsule_cost"]

# the robot segment of the hand cases: (0, 0, 0) -> (4, 0, 0), A = 16; dyadic, axis-aligned, exact
A0, B0 = (0.0, 0.0, 0.0), (4.0, 0.0, 0.0)
BY_HAND = [
    # c, e, d, class
    ((-3.0, 4.0, 0.0), (-1.0, 1.0, 0.0), 5.0, "s0 t0"),    # t = -4 -> 0, s re-solved to clamp(-12/16) = 0 (s was 0.25)
    ((-3.0, -1.0, 0.0), (0.0, 2.0, 0.0), 3.0, "s0 ti"),    # s = clamp(-48/64), t = 2/4
    ((-3.0, -6.0, 0.0), (0.0, 2.0, 0.0), 5.0, "s0 t1"),    # t = 3 -> 1, to (-3, -4, 0)
    ((2.0, 1.0, 0.0), (0.0, 1.0, 0.0), 1.0, "si t0"),      # t = -1 -> 0, s = 8/16
    ((2.0, -1.0, 1.0), (0.0, 2.0, 0.0), 1.0, "si ti"),     # the common perpendicular, one above the other
    ((2.0, -3.0, 0.0), (0.0, 2.0, 0.0), 1.0, "si t1"),     # t = 1.5 -> 1
    ((7.0, 4.0, 0.0), (1.0, 1.0, 0.0), 5.0, "s1 t0"),      # s = 0.75, t = -4 -> 0, s re-solved to clamp(28/16) = 1
    ((7.0, -1.0, 0.0), (0.0, 2.0, 0.0), 3.0, "s1 ti"),     # s = clamp(112/64)
    ((7.0, -6.0, 0.0), (0.0, 2.0, 0.0), 5.0, "s1 t1"),
    ((2.0, -1.0, 0.0), (0.0, 2.0, 0.0), 0.0, "si ti"),     # crossing
    ((1.0, 2.0, 0.0), (2.0, 0.0, 0.0), 2.0, "si t0"),      # exactly parallel, overlapping: den = 0, s = 0, t = -0.5 -> 0, s = 0.25
    ((7.0, 4.0, 0.0), (2.0, 0.0, 0.0), 5.0, "s1 t0"),      # parallel, past the end: den = 0
    ((-2.0, 0.0, 0.0), (-2.0, 0.0, 0.0), 2.0, "s0 t0"),    # collinear, apart
    ((1.0, 0.0, 3.0), (0.0, 0.0, 0.0), 3.0, "E=0"),        # a point above s = 0.25
    ((9.0, 0.0, 0.0), (0.0, 0.0, 0.0), 5.0, "E=0"),        # a point past the end
]


@pytest.mark.parametrize("c,e,d,cls", BY_HAND)
def test_segment_distance_by_hand(c, e, d, cls):
    got, got_cls = CR.segment_distance(A0, B0, c, e)
    assert got == d and got_cls == cls
    assert float(am.segment_distance(A0, B0, c, e)) == d                  # the package's vectorised helper
    if cls != "E=0":   # the other way round: the classes swap, the distance stays
        back, back_cls = CR.segment_distance(c, np.add(c, e), A0, B0)
        assert back == d and back_cls == "s%s t%s" % (cls[4], cls[1])


def test_segment_distance_degenerate_by_hand():
    assert CR.segment_distance((1, 0, 0), (1, 0, 0), (0, 3, 0), (4, 0, 0)) == (3.0, "A=0")        # t = 4/16
    assert CR.segment_distance((9, 3, 0), (9, 3, 0), (0, 3, 0), (4, 0, 0)) == (5.0, "A=0")        # t = 36/16 -> 1
    assert CR.segment_distance((0, 0, 0), (0, 0, 0), (3, 4, 0), (0, 0, 0)) == (5.0, "A=0 E=0")
    assert float(am.segment_distance((1, 0, 0), (1, 0, 0), (0, 3, 0), (4, 0, 0))) == 3.0
    assert float(am.segment_distance((0, 0, 0), (0, 0, 0), (3, 4, 0), (0, 0, 0))) == 5.0
    assert set(cls for _, _, _, cls in BY_HAND) >= set(CR.PROPER) | {"E=0"}


def test_the_vectorised_helper_against_the_reference():
    rng = np.random.default_rng(5)
    a, b, c, e = (rng.integers(-4, 5, (400, 3)).astype(float) / 4.0 for _ in range(4))   # many parallel and degenerate pairs
    got = am.segment_distance(a, b, c, e)
    for i in range(len(a)):
        assert got[i] == CR.segment_distance(a[i], b[i], c[i], e[i])[0], i


def _huddled_points():
    return OR.robot_points(O.default_model(), am.huddled_state()[:12])


def test_the_hole():
    """A 0.03-m sphere on the midpoint of segment 4 (the forearm) at huddled_state(): the nine points
    clear it on the inverse branch, 0.196 - 0.1 - 0.03 m at the nearest, while it sits inside the link;
    the segment is saturated."""
    p = _huddled_points()
    mid = 0.5 * (p[4] + p[5])
    ball = am.SphereObstacle(mid, 0.03, mask=am.MASK_ALL | am.mask_segment(4))
    points_only = OR.Term(am.ObstacleAvoidance(), [am.SphereObstacle(mid, 0.03)], 0.0)
    cheap = points_only.at(p, 0.0)
    assert points_only.branches == [{"inverse"}] and 0.06 < points_only.least_v < 0.07 and cheap < 100.0
    v = CR.point_clearance(ball, np.asarray(am.ObstacleAvoidance().radii), p, 0.0)
    assert np.all(v > 0.0)
    vs, cls = CR.segment_clearance(ball, np.asarray(CS.SEGMENT_RADII), p, 0.0, 4)
    assert cls == "E=0" and abs(vs + 0.09) < 1e-12          # the axis passes through the centre: -(0.06 + 0.03)
    term = CR.Term(am.ObstacleAvoidance(), CS.capsules(), [ball], 0.0)
    total = term.at(p, 0.0)
    assert term.branches == [{"inverse", "saturated"}] and term.evaluated == 10
    assert abs(total - (cheap + (1e10 + vs * vs))) <= 1e-15 * total


def test_half_space_against_a_segment_is_the_lesser_end():
    p = _huddled_points()
    radii = np.asarray(am.ObstacleAvoidance().radii)
    wall = am.HalfSpaceObstacle((-1.0, 0.0, -0.5), (0.6, 0.0, 0.8), velocity=(0.1, 0.0, 0.0), mask=am.MASK_SEGMENTS)
    ends = OR.clearance(wall, np.zeros(9), p, 0.3)            # n . (p_i - c)
    for s in range(8):
        v, cls = CR.segment_clearance(wall, np.asarray(CS.SEGMENT_RADII), p, 0.3, s)
        assert cls is None and v == min(ends[s], ends[s + 1]) - CS.SEGMENT_RADII[s]
    assert radii.shape == (9,)


def test_zero_length_robot_segment_is_a_point():
    """Segments 1 and 5 have zero length on this robot: against a sphere they are the point formula at
    that point with the segment's radius, bit for bit."""
    p = _huddled_points()
    assert np.array_equal(p[1], p[2]) and np.array_equal(p[5], p[6])
    ball = am.SphereObstacle((0.9, 0.2, 1.3), 0.07, velocity=(0.0, 0.5, 0.0))
    for s in (1, 5):
        radii = np.zeros(9)
        radii[s] = CS.SEGMENT_RADII[s]
        v, cls = CR.segment_clearance(ball, np.asarray(CS.SEGMENT_RADII), p, 0.2, s)
        assert cls == "A=0 E=0" and v == OR.clearance(ball, radii, p, 0.2)[s]
        bar = am.CapsuleObstacle((0.9, 0.2, 1.3), (0.0, 0.4, 0.1), 0.07)
        v, cls = CR.segment_clearance(bar, np.asarray(CS.SEGMENT_RADII), p, 0.2, s)
        assert cls == "A=0" and v == CR.point_clearance(bar, radii, p, 0.2)[s]


def test_point_only_masks_reproduce_the_obstacle_reference_bit_for_bit():
    model = O.default_model()
    q = am.huddled_state()[:12]
    config = am.ObstacleAvoidance(limit=(0.01, 2.0, 1e8), radii=(0.7, 0.11, 0.12, 0.13, 0.1, 0.09, 0.08, 0.07, 0.06))
    for obstacles, conf in ((SETS.set_a(), None), (SETS.set_b(), None), (SETS.set_16(), config)):
        conf = conf or am.ObstacleAvoidance()
        old, new = OR.Term(conf, obstacles, 0.1), CR.Term(conf, CS.capsules(), obstacles, 0.1)
        qs = np.array([q + 0.02 * k for k in range(5)])
        assert np.array_equal(old.steps(model, qs, 0.3, 0.015), new.steps(model, qs, 0.3, 0.015))
        assert (old.least_margin, old.least_v, old.branches, old.evaluated) == (new.least_margin, new.least_v, new.branches, new.evaluated)
        assert new.classes == [set() for _ in obstacles]


def _updates(name, sets, n_rollouts=None):
    """test_obstacles_cpu.py::_updates with the capsule composition."""
    _, S, H, keep = by_name(name)[:4]
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=4)
    model = am.FrankaRidgebackDynamics().model
    comp = CR.Composition(conf, model, CS.objective(), am.constant_forecast(H), capsules=CS.capsules())
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
        assert np.array_equal(J, comp.base.costs(x, U, eps)) and term.evaluated == 0


def test_the_sets_meet_the_guards_on_the_reference():
    """What test_gpu_capsules.py asserts from the reference's own books, here without a device at
    r19_h33: set C stays 0.02 m clear on the inverse branch, every obstacle of set D takes both
    branches, nothing comes within 1e-6 of the branch discontinuity, no cost is NaN and the term moves
    the costs.  (This reference gives: set C's least v 0.76, set D's least |v - bound| 1.1e-5, the
    flying bar in six of the nine (s, t) classes; the test prints them.)"""
    for j, comp, term, J, (x, U, eps) in _updates("r19_h33", CS.cde()):
        assert not np.isnan(J).any()
        if j < 2:
            print("set %s: least margin %.3e, least v %.4f, classes %s" % ("CD"[j], term.least_margin, term.least_v,
                                                                           [sorted(c) for c in term.classes]))
        if j == 0:
            assert term.least_v >= 0.02 and all(b == {"inverse"} for b in term.branches), (term.least_v, term.branches)
        if j == 1:
            assert all(b == {"inverse", "saturated"} for b in term.branches), term.branches
        if j < 2:
            assert term.least_margin >= 1e-6, (j, term.least_margin)
            assert np.abs(J - comp.base.costs(x, U, eps)).min() > 1e-3


# ---- the library, without a device --------------------------------------------------------------

def test_symbols_and_constants():
    L = load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert L.mppi_abi_version() == 5
    text = open(HEADER).read()
    for macro in ("MPPI_OBSTACLE_CAPSULE", "MPPI_OBSTACLE_SEGMENTS"):
        m = re.search(r"^#define %s (\d+)\b" % macro, text, re.M)
        assert m and int(m.group(1)) == getattr(abi, macro), macro
    assert abi.MPPI_OBSTACLE_CAPSULE == 2 and abi.MPPI_OBSTACLE_SEGMENTS == 8
    assert re.search(r"^#define MPPI_OBSTACLE_MASK_SEGMENTS 0xFF0000u$", text, re.M) and abi.MPPI_OBSTACLE_MASK_SEGMENTS == 0xFF0000
    assert re.search(r"^#define MPPI_OBSTACLE_MASK_SEGMENT\(s\) \(1u << \(16 \+ \(s\)\)\)$", text, re.M)
    assert re.search(r"^#define MPPI_OBSTACLE_MASK_ALL 0x1FFu$", text, re.M) and abi.MPPI_OBSTACLE_MASK_ALL == 0x1FF
    assert [abi.MPPI_OBSTACLE_MASK_SEGMENT(s) for s in range(8)] == [1 << (16 + s) for s in range(8)]
    assert sum(am.mask_segment(s) for s in range(8)) == am.MASK_SEGMENTS and CS.ARM == 0xFE0000
    with pytest.raises(ValueError):
        am.mask_segment(8)


def test_struct_layout_matches_the_header():
    assert C.sizeof(abi.mppi_capsule_config) == 64 and abi.mppi_capsule_config.segment_radii.offset == 0
    assert C.sizeof(abi.mppi_obstacle) == 88   # unchanged: the axis is the normal field
    text = open(HEADER).read()
    body = re.search(r"typedef struct mppi_capsule_config \{(.*?)\} mppi_capsule_config;", text, re.S).group(1)
    assert [f.strip() for f in body.split(";") if f.strip()] == ["double segment_radii[MPPI_OBSTACLE_SEGMENTS]"]


def test_default_configuration():
    c = abi.mppi_capsule_config()
    load().mppi_default_capsule_config(C.byref(c))
    assert list(c.segment_radii) == [0.1] * 8
    assert am.ObstacleCapsules.from_c(c) == am.ObstacleCapsules()
    back = am.ObstacleCapsules(tuple(0.01 * (i + 1) for i in range(8)))
    assert am.ObstacleCapsules.from_c(back.to_c()) == back and back != am.ObstacleCapsules()
    with pytest.raises(ValueError):
        am.ObstacleCapsules((0.1,) * 9)


def test_capsule_objects_round_trip():
    cap = am.CapsuleObstacle((1, 2, 3), (0.5, 0.0, -2.0), 0.25, velocity=(0.1, 0.2, 0.3), mask=CS.ARM | 0x101)
    assert cap.kind == abi.MPPI_OBSTACLE_CAPSULE and np.array_equal(cap.start, [1, 2, 3]) and np.array_equal(cap.axis, [0.5, 0.0, -2.0])
    assert am.CapsuleObstacle((0, 0, 0), (0, 0, 1), 0.1).mask == am.MASK_ALL | am.MASK_SEGMENTS
    arr, n = am.obstacles_to_c([cap, am.SphereObstacle((1, 2, 3), 0.5, mask=am.mask_segment(3)), am.HalfSpaceObstacle((0, 0, -1), (0, 0, 1))])
    assert n == 3 and arr[0].kind == 2 and arr[0].mask == 0xFE0101 and list(arr[0].normal) == [0.5, 0.0, -2.0]
    back = [am.obstacle_from_c(arr[i]) for i in range(3)]
    assert isinstance(back[0], am.CapsuleObstacle) and back[0].radius == 0.25 and back[0].mask == cap.mask
    assert np.array_equal(back[0].axis, cap.axis) and np.array_equal(back[0].velocity, cap.velocity)
    assert isinstance(back[1], am.SphereObstacle) and back[1].mask == 1 << 19 and isinstance(back[2], am.HalfSpaceObstacle)
    np.testing.assert_allclose(cap.at(2.0), [1.2, 2.4, 3.6])


def test_obstacle_clearance_with_segments_on_a_synthetic_predicted():
    """test_obstacles_cpu.py's synthetic Predicted: every point at the origin except PANDA_LINK7
    (point 7), which walks along x, and the end effector (point 8) 1 m above it; so segment 6 runs from
    the origin to point 7 along x and segment 7 is vertical above point 7."""
    H = 3
    raw = np.zeros((2, H, abi.MPPI_PRED_N))
    for r in range(2):
        for k in range(H):
            x = 1.0 + k + 10.0 * r
            raw[r, k, abi.MPPI_PRED_LINKS + 3 * abi.MPPI_LINK_PANDA_LINK7:][:3] = (x, 0.0, 0.0)
            raw[r, k, abi.MPPI_PRED_EE:abi.MPPI_PRED_EE + 3] = (x, 0.0, 1.0)
    pred = am.Predicted(raw, 0.5, 0.1, rollouts=[0, 1])
    conf, caps = am.ObstacleAvoidance(radii=(0.125,) * 9), am.ObstacleCapsules((0.25,) * 8)
    # a ball 2 m beside the middle of segment 7 and level with it: its points are 0.5 m higher and lower
    ball = am.SphereObstacle((1.0, 2.0, 0.5), 0.5, mask=(1 << 7) | (1 << 8) | am.mask_segment(7))
    plain = am.obstacle_clearance(pred, conf, [ball], 0.0)
    pts, seg = am.obstacle_clearance(pred, conf, [ball], 0.0, capsules=caps)
    assert np.array_equal(pts, plain) and pts.shape == seg.shape == (2, H)
    np.testing.assert_allclose(seg[0], [2.0 - 0.75, np.sqrt(5.0) - 0.75, np.sqrt(8.0) - 0.75], rtol=0, atol=1e-12)
    np.testing.assert_allclose(pts[0, 0], np.sqrt(4.25) - 0.625, rtol=0, atol=1e-12)
    # a bar along y over the middle of segment 6 of rollout 0 at step 0, 0.75 above it, flying along x
    bar = am.CapsuleObstacle((0.5, -1.0, 0.75), (0.0, 2.0, 0.0), 0.25, velocity=(10.0, 0.0, 0.0), mask=am.mask_segment(6))
    pts, seg = am.obstacle_clearance(pred, conf, [bar], 0.5, capsules=caps)   # tau = 0, 0.1, 0.2: x = 0.5, 1.5, 2.5
    assert np.all(np.isinf(pts))
    np.testing.assert_allclose(seg[0], [0.25, 0.25, 0.25], rtol=0, atol=1e-12)
    np.testing.assert_allclose(seg[1], [0.25, 0.25, 0.25], rtol=0, atol=1e-12)
    # a wall against the segments: the lesser end
    wall = am.HalfSpaceObstacle((0.5, 0, 0), (1, 0, 0), mask=am.mask_segment(6) | am.mask_segment(7))
    pts, seg = am.obstacle_clearance(pred, conf, [wall], 0.0, capsules=caps)
    np.testing.assert_allclose(seg, np.full((2, H), -0.75), rtol=0, atol=1e-12)   # segment 6 starts at the origin
    with pytest.raises(ValueError):
        am.obstacle_clearance(pred, conf, [bar], 0.0)
    assert am.obstacle_clearance(am.Predicted(raw[0], 0.5, 0.1), conf, [ball], 0.0, capsules=caps)[1].shape == (H,)
