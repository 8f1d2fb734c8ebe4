"""Obstacle avoidance with a held object without a GPU: the reference of held_object_reference.py against
geometry worked out by hand, where it must agree with field_reference.py bit for bit, the guards the GPU
tests rely on, and the library's host-side surface: symbols, constants, struct layout, HeldObject's
validation and round trip, the mask helpers, the refusals that need no device, and the clearance helper."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi
from assistedmanipulation_amd._lib import HEADER, load

import field_reference as FR
import held_object_reference as HR
import held_object_sets as HS
import link_reference as LR
from launch_shapes import by_name, horizon
from test_gpu_link_positions import _noise_scale, _states

NEW_SYMBOLS = ["mppi_set_held_object_avoidance", "mppi_get_held_object_avoidance", "mppi_set_held_object", "mppi_get_held_object",
               "mppi_optimal_held_cost", "mppi_dynamics_held_object_cost", "mppi_predicted_held_optimal", "mppi_predicted_held_rollouts"]
MARGIN = 1e-6     # the project's: least |v - bound|, and the least distance of a sample to the grid's boundary in grid units
CLEAR_0 = 0.02    # the first update's object stays this clear


# ---- the reference's geometry, by hand -----------------------------------------------------------

def _model():
    return am.FrankaRidgebackDynamics().model


def test_offsets_along_each_grasp_axis():
    """At huddled_state(): an offset d e_a sits d along column a of Ree from the grasp position (its length d
    to a few ulp, nothing along the other two columns), the zero offset is the grasp position exactly, and a
    quarter turn of the base about z (joint 2) turns every world offset by a quarter turn: (x, y, z) -> (-y, x, z)."""
    model = _model()
    q = am.huddled_state()[:12]
    p, R = HR.grasp_pose(model, q)
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1.0) < 1e-14
    d = 0.3
    held = am.HeldObject([(d, 0, 0), (0, d, 0), (0, 0, d), (0, 0, 0)], (0.0,) * 4, (0.0,) * 3)
    h = np.array(HR.world_points(held, p, R))
    assert np.array_equal(h[3], p)                                        # p + ((R 0 + R 0) + R 0)
    for a in range(3):
        off = h[a] - p
        assert abs(np.linalg.norm(off) - d) < 1e-15
        assert np.allclose(off, d * R[:, a], rtol=0, atol=1e-16)
        for b in range(3):
            if b != a:
                assert abs(off @ R[:, b]) < 1e-16
    q2 = q.copy()
    q2[2] += math.pi / 2
    p2, R2 = HR.grasp_pose(model, q2)
    h2 = np.array(HR.world_points(held, p2, R2))
    for a in range(3):
        x, y, z = h[a] - p
        assert np.allclose(h2[a] - p2, (-y, x, z), rtol=0, atol=1e-15)
    # the package's vectorised form, bit for bit
    assert np.array_equal(held.world(p, R), h)
    assert np.array_equal(held.world(np.stack([p, p2]), np.stack([R, R2])), np.stack([h, h2]))


def test_the_term_by_hand():
    """One obstacle at a time around a known pose (the identity rotation at the origin, so the held points
    are their centres): a sphere on a point is v = -(r + r_o), a half-space takes the lower end of a
    segment, a capsule parallel to a segment is their distance, and the field's samples sit at j / (m + 1)."""
    conf = am.ObstacleAvoidance(limit=(0.0, 1.0, 1e10))
    caps = am.ObstacleCapsules()
    p, R = np.zeros(3), np.eye(3)
    held = am.HeldObject([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 0.0, 2.0)], (0.25, 0.125, 0.5), (0.0625, 0.03125))
    left = lambda v: LR.left_barrier(FR.Term(conf, caps, [], 0.0).limit, v)   # noqa: E731

    def term(obstacles, field=None, tau=0.0):
        t = HR.Term(conf, caps, obstacles, 0.0, field, held)
        return t.held_at(p, R, tau), t

    on1 = am.SphereObstacle((1.0, 0.0, 0.0), 0.5, mask=am.mask_held_point(1))
    got, t = term([on1])
    assert got == left(-(0.125 + 0.5)) == 1e10 + 0.625 ** 2 and t.hbooks.branches == {"saturated"} and t.hbooks.evaluated == 1
    moving = am.SphereObstacle((4.0, -3.0, 0.0), 0.5, velocity=(0.0, 1.5, 0.0), mask=am.mask_held_point(0))
    assert term([moving], tau=2.0)[0] == left(4.0 - 0.75) == 1.0 / 3.25     # the centre at (4, 0, 0) after 2 s
    floor = am.HalfSpaceObstacle((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), mask=am.mask_held_segment(1) | am.mask_held_point(2))
    assert term([floor])[0] == left(3.0 - 0.5) + left(1.0 - 0.03125)        # point 2 at z = 2; segment 1: its lower end at z = 0
    bar = am.CapsuleObstacle((0.0, 3.0, 0.0), (1.0, 0.0, 0.0), 0.25, mask=am.mask_held_segment(0) | am.mask_held_segment(2))
    assert term([bar])[0] == left(3.0 - (0.0625 + 0.25))                    # (bit 26 names a segment this object does not have)
    absent = am.SphereObstacle((0.0, 0.0, 0.0), 0.1, mask=am.mask_held_point(3) | am.mask_held_segment(2) | am.MASK_ALL)
    got, t = term([absent])
    assert got == 0.0 and t.hbooks.evaluated == 0
    # order: obstacle by obstacle, points before segments
    both = term([floor, bar])[0]
    assert both == (left(2.5) + left(0.96875)) + left(2.6875)
    # the field: D = z + 0.5 exactly on a dyadic grid; point 2 and segment 1's samples at z = 0.5, 1.0, 1.5
    field = am.DistanceField.from_function(lambda x, y, z: z + 0.5, (-1.0, -1.0, -1.0), 0.5, (7, 5, 9),
                                           mask=am.mask_held_point(2) | am.mask_held_segment(1) | am.mask_held_segment(2), segment_samples=3)
    got, t = term([], field)
    assert got == ((left(2.5 - 0.5) + left(1.0 - 0.03125)) + left(1.5 - 0.03125)) + left(2.0 - 0.03125)
    assert t.hbooks.inside == 4 and t.hbooks.outside == 0 and t.hbooks.edge == 2.0   # (g = (4, 2, 3..6) in a grid of 7 x 5 x 9)
    out = am.HeldObject([(9.0, 0.0, 0.0)], (0.1,))
    t = HR.Term(conf, caps, [], 0.0, am.DistanceField(field.values, field.origin, field.voxel, mask=am.MASK_HELD), out)
    assert t.held_at(p, R, 0.0) == 0.0 and t.hbooks.outside == 1
    nan = HR.Term(conf, caps, [on1], 0.0, None, held).held_at(np.array([math.nan, 0.0, 0.0]), R, 0.0)
    assert math.isnan(nan)


def _updates(name, held_on=True, n_rollouts=None):
    _, S, H, keep = by_name(name)[:4]
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=4)
    comp = HR.Composition(conf, _model(), HS.objective(), am.constant_forecast(H), capsules=HS.capsules())
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance)) * _noise_scale(H)
    U = np.zeros((H, 12))
    R = n_rollouts or S + 2
    for j, (x, held, field, (obstacles, t_ref)) in enumerate(zip(_states(), HS.objects(), HS.fields(), HS.sets())):
        comp.field, comp.held = field, held if held_on else None
        term = comp.set_obstacles(obstacles, t_ref)
        eps = rng.standard_normal((R, H, 12)) * sd
        eps[0] = 0.0
        J = comp.costs(x, U, eps)
        yield j, comp, term, J, (x, U, eps)
        _, _, U = LR.mppi_update(conf, J, eps, U)


def test_no_object_reproduces_the_field_reference_bit_for_bit():
    """With nothing held - and with held bits in every mask - the costs are field_reference's."""
    _, S, H, keep = by_name("r19_h33")[:4]
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=4)
    old = FR.Composition(conf, _model(), HS.objective(), am.constant_forecast(H), capsules=HS.capsules())
    for j, comp, term, J, (x, U, eps) in _updates("r19_h33", held_on=False, n_rollouts=4):
        old.field = HS.fields()[j]
        old.set_obstacles(*HS.sets()[j])
        assert np.array_equal(J, old.costs(x, U, eps)) and term.hbooks.evaluated == 0 and not term.held_steps.any()
        if j == 1:
            break


def check_books(term, j, tag):
    """The guards on the reference's own books for held_object_sets: what every parity run asserts, on the
    device's own noise."""
    b = term.hbooks
    assert b.evaluated > 0, (tag, j)
    assert b.least_margin >= MARGIN, (tag, j, b.least_margin)
    assert b.edge >= MARGIN, (tag, j, b.edge)
    assert term.least_margin >= MARGIN and term.fbooks.least_margin >= MARGIN and term.fbooks.edge >= MARGIN, (tag, j)
    if j == 0:
        assert b.least_v >= CLEAR_0 and b.branches == {"inverse"}, (tag, b.least_v, b.branches)
    if j == 1:
        assert b.branches == {"inverse", "saturated"}, (tag, b.branches)


def test_the_sets_meet_the_guards_on_the_reference():
    """What test_gpu_held_object.py asserts from the reference's books, here without a device at r19_h33: nothing
    within 1e-6 of the barrier's branch point or of the grid's boundary, the beam 0.02 m clear on the inverse
    branch, the tray on both branches, no NaN cost, and the held term moves every rollout's cost in the first
    two updates."""
    with_held = list(_updates("r19_h33"))
    without = list(_updates("r19_h33", held_on=False))
    for (j, comp, term, J, (x, U, eps)), (_, comp0, _, _, _) in zip(with_held, without):
        b = term.hbooks
        print("update %d: least margin %.3e, least v %.4f, %s, evaluated %d, inside %d, outside %d, edge %.3e"
              % (j, b.least_margin, b.least_v, sorted(b.branches), b.evaluated, b.inside, b.outside, b.edge))
        assert not np.isnan(J).any()
        check_books(term, j, "r19_h33")
        if j < 2:   # the same rollouts without the object (update 0: the same U; update 1: this run's U)
            comp.held = None
            comp.set_obstacles(*HS.sets()[j])
            assert np.all(J != comp.costs(x, U, eps)), j


# ---- the library, without a device ---------------------------------------------------------------

def test_symbols_and_constants():
    L = load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert L.mppi_abi_version() == 5
    text = open(HEADER).read()
    for macro in ("MPPI_HELD_POINTS", "MPPI_HELD_SEGMENTS"):
        m = re.search(r"^#define %s (\d+)\b" % macro, text, re.M)
        assert m and int(m.group(1)) == getattr(abi, macro), macro
    assert abi.MPPI_HELD_POINTS == 4 and abi.MPPI_HELD_SEGMENTS == 3
    assert re.search(r"^#define MPPI_OBSTACLE_MASK_HELD 0x07001E00u$", text, re.M)
    assert re.search(r"^#define MPPI_OBSTACLE_MASK_HELD_POINT\(i\) \(1u << \(9 \+ \(i\)\)\)$", text, re.M)
    assert re.search(r"^#define MPPI_OBSTACLE_MASK_HELD_SEGMENT\(s\) \(1u << \(24 \+ \(s\)\)\)$", text, re.M)
    assert re.search(r"^#define MPPI_OBSTACLE_MASK_ALL 0x1FFu$", text, re.M) and re.search(r"^#define MPPI_OBSTACLE_MASK_SEGMENTS 0xFF0000u$", text, re.M)


def test_mask_helpers():
    assert am.MASK_HELD == 0x07001E00 == sum(am.mask_held_point(i) for i in range(4)) + sum(am.mask_held_segment(s) for s in range(3))
    assert [am.mask_held_point(i) for i in range(4)] == [1 << 9, 1 << 10, 1 << 11, 1 << 12]
    assert [am.mask_held_segment(s) for s in range(3)] == [1 << 24, 1 << 25, 1 << 26]
    assert am.MASK_HELD & (am.MASK_ALL | am.MASK_SEGMENTS) == 0
    assert am.MASK_ALL == 0x1FF and am.MASK_SEGMENTS == 0xFF0000                      # unchanged
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            am.mask_held_point(bad)
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            am.mask_held_segment(bad)
    # Python's default masks do not change: a set written without a held object means what it meant
    assert am.SphereObstacle((0, 0, 0), 0.1).mask == am.MASK_ALL and am.CapsuleObstacle((0, 0, 0), (0, 0, 1), 0.1).mask == am.MASK_ALL | am.MASK_SEGMENTS
    assert am.DistanceField(np.zeros((2, 2, 2)), (0, 0, 0), 0.1).mask == am.MASK_ALL | am.MASK_SEGMENTS


def test_struct_layout_matches_the_header():
    o = abi.mppi_held_object
    assert C.sizeof(o) == 8 + 96 + 32 + 24
    assert (o.count.offset, o.pad.offset, o.centres.offset, o.radii.offset, o.segment_radii.offset) == (0, 4, 8, 104, 136)
    text = open(HEADER).read()
    body = re.search(r"typedef struct mppi_held_object \{(.*?)\} mppi_held_object;", text, re.S).group(1)
    assert [x.strip() for x in body.split(";") if x.strip()] == ["int32_t count", "int32_t pad", "double centres[MPPI_HELD_POINTS][3]",
                                                                "double radii[MPPI_HELD_POINTS]", "double segment_radii[MPPI_HELD_SEGMENTS]"]


def test_held_object_validation_and_round_trip():
    tray = HS.tray()
    c = tray.to_c()
    assert c.count == 4 and c.pad == 0 and [list(r) for r in c.centres] == tray.centres.tolist()
    assert list(c.radii) == list(tray.radii) and list(c.segment_radii) == list(tray.segment_radii)
    assert am.HeldObject.from_c(c) == tray and am.HeldObject.from_c(c) != HS.beam()
    beam = HS.beam().to_c()
    assert beam.count == 2 and list(beam.centres[2]) == [0.0, 0.0, 0.0] and beam.radii[3] == 0.0 and list(beam.segment_radii)[1:] == [0.0, 0.0]
    assert am.HeldObject.from_c(beam) == HS.beam()
    tip = am.HeldObject([(0.0, 0.0, 0.1)], (0.02,))
    assert tip.count == 1 and tip.segment_radii == () and am.HeldObject.from_c(tip.to_c()) == tip
    assert am.HeldObject([(0, 0, 0), (0, 0, 0)], (0.1, 0.1)).segment_radii == (0.0,)     # coincident points are legal; default segment radii
    assert am.HeldObject(np.zeros((0, 3)), ()).count == 0
    for bad in (lambda: am.HeldObject(np.zeros((5, 3)), (0.1,) * 5),                  # a count of 5
                lambda: am.HeldObject([(0, 0, 0)], (0.1, 0.2)),                       # radii that do not fit
                lambda: am.HeldObject([(0, 0, 0), (1, 0, 0)], (0.1, 0.1), (0.1, 0.1)),
                lambda: am.HeldObject([(0, 0, 0)], (-0.1,)),
                lambda: am.HeldObject([(0, 0, 0)], (math.nan,)),
                lambda: am.HeldObject([(0, 0, 0), (1, 0, 0)], (0.1, 0.1), (math.inf,)),
                lambda: am.HeldObject([(0, math.inf, 0)], (0.1,)),
                lambda: am.HeldObject([(0, 0)], (0.1,))):
        with pytest.raises(ValueError):
            bad()


def test_refusals_without_a_device():
    """NULL handles, and the dynamics object's NULL check that comes before any device call."""
    L = load()
    o = HS.beam().to_c()
    on = C.c_int(0)
    v = C.c_double(0.0)
    out = np.zeros(12)
    idx = np.zeros(1, dtype=np.int64)
    assert L.mppi_set_held_object_avoidance(None) == abi.MPPI_ERR_INVALID
    assert L.mppi_get_held_object_avoidance(None, C.byref(on)) == abi.MPPI_ERR_INVALID
    assert L.mppi_set_held_object(None, C.byref(o)) == abi.MPPI_ERR_INVALID
    assert L.mppi_get_held_object(None, C.byref(o), C.byref(on)) == abi.MPPI_ERR_INVALID
    assert L.mppi_optimal_held_cost(None, C.byref(v)) == abi.MPPI_ERR_INVALID
    assert L.mppi_predicted_held_optimal(None, out.ctypes.data_as(C.POINTER(C.c_double))) == abi.MPPI_ERR_INVALID
    assert L.mppi_predicted_held_rollouts(None, idx.ctypes.data_as(C.POINTER(C.c_int64)), 1, out.ctypes.data_as(C.POINTER(C.c_double))) == abi.MPPI_ERR_INVALID
    assert L.mppi_dynamics_held_object_cost(None, None, None, 0, 0.0, None, None, C.byref(o), C.byref(v)) == abi.MPPI_ERR_INVALID


def test_held_object_clearance_on_a_hand_made_path():
    """A beam along x walking along x, one metre a step: a sphere ahead of it, a floor under it, a capsule beside
    it, and the exact plane D = z on a dyadic grid; +inf where nothing is tested and for points the object lacks."""
    H = 3
    time = 0.5 + 0.25 * np.arange(H)
    paths = np.full((2, H, 4, 3), np.nan)
    for r in range(2):
        for k in range(H):
            x = 1.0 * k + 10.0 * r
            paths[r, k, 0] = (x, 0.0, 1.0)
            paths[r, k, 1] = (x + 2.0, 0.0, 2.0)
    beam = am.HeldObject([(0, 0, 0), (2, 0, 1)], (0.25, 0.125), (0.0625,))
    ahead = am.SphereObstacle((8.0, 0.0, 2.0), 0.5, velocity=(0.0, 0.0, 0.0), mask=am.mask_held_point(1))
    got = am.held_object_clearance(paths, time, None, [ahead], 0.5, beam)
    assert got.shape == (2, H) and np.array_equal(got[0], [6.0 - 0.625, 5.0 - 0.625, 4.0 - 0.625])
    moving = am.SphereObstacle((8.0, 0.0, 2.0), 0.5, velocity=(-4.0, 0.0, 0.0), mask=am.mask_held_point(1))
    assert np.array_equal(am.held_object_clearance(paths, time, None, [moving], 0.5, beam)[0], [6.0 - 0.625, 4.0 - 0.625, 2.0 - 0.625])
    floor = am.HalfSpaceObstacle((0.0, 0.0, 0.5), (0.0, 0.0, 1.0), mask=am.MASK_HELD)
    assert np.array_equal(am.held_object_clearance(paths, time, None, [floor], 0.0, beam), np.full((2, H), 0.5 - 0.25))   # point 0, the lower one
    seg_only = am.HalfSpaceObstacle((0.0, 0.0, 0.5), (0.0, 0.0, 1.0), mask=am.mask_held_segment(0))
    assert np.array_equal(am.held_object_clearance(paths, time, None, [seg_only], 0.0, beam), np.full((2, H), 0.5 - 0.0625))
    bar = am.CapsuleObstacle((-100.0, 3.0, 1.0), (200.0, 0.0, 0.0), 0.25, mask=am.mask_held_segment(0))
    assert np.allclose(am.held_object_clearance(paths, time, None, [bar], 0.0, beam), 3.0 - 0.3125, rtol=0, atol=1e-15)
    robot_only = am.SphereObstacle((0.0, 0.0, 1.0), 0.5)                       # MASK_ALL: no held bit
    assert np.all(np.isinf(am.held_object_clearance(paths, time, None, [robot_only], 0.0, beam)))
    absent = am.SphereObstacle((0.0, 0.0, 1.0), 0.5, mask=am.mask_held_point(2) | am.mask_held_point(3) | am.mask_held_segment(1))
    assert np.all(np.isinf(am.held_object_clearance(paths, time, None, [absent], 0.0, beam)))
    field = am.DistanceField.from_function(lambda x, y, z: z, (0.0, -1.0, 0.0), 0.5, (9, 5, 7), mask=am.MASK_HELD, segment_samples=1)
    got = am.held_object_clearance(paths, time, None, [], 0.0, beam, field)
    assert np.array_equal(got[0], [0.75, 0.75, 0.75])                          # point 0 at z = 1 less 0.25; x + 2 stays in [0, 4]
    assert np.all(np.isinf(got[1]))                                            # rollout 1 is outside the grid
    assert np.all(np.isinf(am.held_object_clearance(paths, time, None, [ahead], 0.5, None)))
    assert am.held_object_clearance(paths[0], time, None, [ahead], 0.5, beam).shape == (H,)
