"""The held object against the robot's own segments without a GPU: the reference of held_self_reference.py
against geometry worked out by hand, where it must agree with held_object_reference.py bit for bit, the
guards the GPU tests rely on, and the library's host-side surface: symbols, constants, struct layout,
HeldSelf's validation and round trip, the refusals that need no device, and the clearance helper."""
import ctypes as C
import math
import re
from types import SimpleNamespace

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi
from assistedmanipulation_amd._lib import HEADER, load

import capsule_reference as CR
import held_object_reference as HR
import held_self_reference as SR
import held_self_sets as SS
import link_reference as LR
from launch_shapes import by_name, horizon
from test_gpu_link_positions import _noise_scale, _states

NEW_SYMBOLS = ["mppi_default_held_self", "mppi_set_held_self_avoidance", "mppi_get_held_self_avoidance", "mppi_set_held_self",
               "mppi_get_held_self", "mppi_optimal_held_self_cost", "mppi_dynamics_held_self_cost"]
MARGIN = 1e-6     # test_held_object_cpu.MARGIN: least |v - bound|


def _model():
    return am.FrankaRidgebackDynamics().model


# ---- the reference's geometry, by hand -----------------------------------------------------------

def _points(**named):
    """Nine robot points far away from everything (x = 100 + i), except those given by index."""
    p = [[100.0 + i, 0.0, 0.0] for i in range(9)]
    for k, v in named.items():
        p[int(k[1:])] = list(v)
    return np.array(p, dtype=np.float64)


def test_the_term_by_hand():
    """At the identity grasp pose at the origin the held points are their centres.  Robot segment 2 runs
    from (0, 3, -1) to (0, 3, 1): a held point at the origin is 3 from its axis (s inside, "E=0"); the held
    segment from the origin to (4, 0, 0) is 3 from it too (t = 0); robot segment 1, both ends at (0, 0, 2), is a
    point, 2 from the held point ("A=0 E=0") and 2 from the held segment ("A=0")."""
    conf = am.ObstacleAvoidance(limit=(0.0, 1.0, 1e10))
    caps = am.ObstacleCapsules()
    p, R = np.zeros(3), np.eye(3)
    held = am.HeldObject([(0.0, 0.0, 0.0), (4.0, 0.0, 0.0)], (0.25, 0.125), (0.0625,))
    pts = _points(p1=(0.0, 0.0, 2.0), p2=(0.0, 0.0, 2.0), p3=(0.0, 3.0, -1.0), p4=(0.0, 3.0, 1.0))
    left = lambda v: LR.left_barrier(SimpleNamespace(bound=0.0, scale=1.0, maximum_cost=1e10), v)   # noqa: E731

    def term(units, segments, radii=(0.5,) * 8, obj=held):
        t = SR.Term(conf, caps, [], 0.0, None, obj, am.HeldSelf(units, segments, radii))
        return t.self_at(pts, p, R), t

    # robot segment 3 (points 3 and 4) against held point 0: d = 3, v = 3 - (0.5 + 0.25)
    got, t = term(am.held_self_unit_point(0), 1 << 3)
    assert got == left(3.0 - 0.75) == 1.0 / 2.25 and t.sbooks.classes == {"E=0"} and t.sbooks.evaluated == 1
    assert t.sbooks.branches == {"inverse"} and t.sbooks.least_v == 2.25
    # ... against held segment 0 with its own radius: the closest points are (0, 3, 0) and the origin
    got, t = term(am.held_self_unit_segment(0), 1 << 3)
    assert got == left(3.0 - (0.5 + 0.0625)) and t.sbooks.classes == {"si t0"}
    # the zero-length robot segment 1 against the point and against the segment
    got, t = term(am.held_self_unit_point(0), 1 << 1)
    assert got == left(2.0 - 0.75) and t.sbooks.classes == {"A=0 E=0"}
    got, t = term(am.held_self_unit_segment(0), 1 << 1)
    assert got == left(2.0 - 0.5625) and t.sbooks.classes == {"A=0"}
    # held point 1 at (4, 0, 0): 5 from (0, 3, 0); a radius of 5 saturates: v = 5 - (5 + 0.125) <= 0
    got, t = term(am.held_self_unit_point(1), 1 << 3, radii=(0.0, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0, 0.0))
    assert got == left(-0.125) == 1e10 + 0.125 ** 2 and t.sbooks.branches == {"saturated"}
    # order: units 0, 1, 4, per unit the segments 1, 3
    got, t = term(abi.MPPI_HELD_SELF_UNITS, (1 << 1) | (1 << 3))
    p1 = math.sqrt(16.0 + 4.0) - 0.625     # held point 1 to (0, 0, 2)
    want = 0.0
    for v in (2.0 - 0.75, 3.0 - 0.75, p1, 5.0 - 0.625, 2.0 - 0.5625, 3.0 - 0.5625):
        want += left(v)
    assert got == want and t.sbooks.evaluated == 6 and t.units == [0, 1, 4]
    # bits that name what the object does not have select nothing; empty masks and no object give +0.0
    tip = am.HeldObject([(0.0, 0.0, 0.0)], (0.25,))
    got, t = term(abi.MPPI_HELD_SELF_UNITS, 1 << 3, obj=tip)
    assert got == left(3.0 - 0.75) and t.units == [0]
    for units, segments, obj in ((0, 0xFF, held), (0x7F, 0, held), (0x7F, 0xFF, None), (0x7E, 0xFF, tip)):
        got, t = term(units, segments, obj=obj)
        assert got == 0.0 and math.copysign(1.0, got) == 1.0 and t.sbooks.evaluated == 0
    assert SR.Term(conf, caps, [], 0.0, None, held, None).self_at(pts, p, R) == 0.0
    # a NaN pose makes the term NaN
    got = SR.Term(conf, caps, [], 0.0, None, held, am.HeldSelf(1, 1 << 3)).self_at(pts, np.array([math.nan, 0.0, 0.0]), R)
    assert math.isnan(got)
    bad = _points(p3=(0.0, math.nan, -1.0), p4=(0.0, 3.0, 1.0))
    assert math.isnan(SR.Term(conf, caps, [], 0.0, None, held, am.HeldSelf(1, 1 << 3)).self_at(bad, p, R))


def test_robot_segment_first_held_unit_second():
    """The orientation is capsule_term's: the robot's segment is a -> b and the held unit c -> c + e, so the
    clearance is capsule_reference.segment_clearance of that segment against a capsule obstacle laid on the held
    segment, bit for bit, with the same split of the radii."""
    model = _model()
    held = SS.objects()[0]
    for x in _states()[:2]:
        q = x[:12]
        pts = SR.OR.robot_points(model, q)
        h = HR.world_points(held, *HR.grasp_pose(model, q))
        e = [h[1][k] - h[0][k] for k in range(3)]
        for s in range(8):
            ob = am.CapsuleObstacle(h[0], e, held.segment_radii[0], mask=am.mask_segment(s))
            radii = [0.03 * (i + 1) for i in range(8)]
            want, cls = CR.segment_clearance(ob, radii, pts, 0.0, s)
            got, gcls = SR.clearance(pts, s, radii[s], h[0], e, held.segment_radii[0])
            assert got == want and gcls == cls, s


def _updates(name, self_on=True, configurations=None, n_rollouts=None):
    _, S, H, keep = by_name(name)[:4]
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=4)
    comp = SR.Composition(conf, _model(), SS.objective(), am.constant_forecast(H), capsules=SS.capsules())
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance)) * _noise_scale(H)
    U = np.zeros((H, 12))
    R = n_rollouts or S + 2
    cfgs = configurations or SS.configurations()
    for j, (x, held, field, (obstacles, t_ref), cfg) in enumerate(zip(_states(), SS.objects(), SS.fields(), SS.sets(), cfgs)):
        comp.field, comp.held, comp.held_self = field, held, cfg if self_on else None
        term = comp.set_obstacles(obstacles, t_ref)
        eps = rng.standard_normal((R, H, 12)) * sd
        eps[0] = 0.0
        J = comp.costs(x, U, eps)
        yield j, comp, term, J, (x, U, eps)
        _, _, U = LR.mppi_update(conf, J, eps, U)


def test_no_configuration_reproduces_the_held_reference_bit_for_bit():
    """With no configuration, with no unit masked and with no robot segment masked the costs are
    held_object_reference's."""
    _, S, H, keep = by_name("r19_h33")[:4]
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=4)
    old = HR.Composition(conf, _model(), SS.objective(), am.constant_forecast(H), capsules=SS.capsules())
    empties = [None, am.HeldSelf(units=0), am.HeldSelf(segments=0)]
    for j, comp, term, J, (x, U, eps) in _updates("r19_h33", configurations=empties, n_rollouts=3):
        old.field, old.held = SS.fields()[j], SS.objects()[j]
        old.set_obstacles(*SS.sets()[j])
        assert np.array_equal(J, old.costs(x, U, eps)) and term.sbooks.evaluated == 0 and not term.self_steps.any()


def check_books(term, j, tag, H=33):
    """The guards on the reference's own books for held_self_sets: what every parity run asserts, on the
    device's own noise.  (With one step a horizon every rollout's only step is at x0, where the tray is clear of
    the tower by construction - a tray inside it at x0 would saturate every rollout alike - so the second
    update's saturated branch needs H > 1.)"""
    b = term.sbooks
    assert b.evaluated > 0, (tag, j)
    assert b.least_margin >= MARGIN, (tag, j, b.least_margin)
    if j == 0:
        assert b.branches == {"inverse"}, (tag, b.least_v, b.branches)
    if j == 1:
        assert b.branches == ({"inverse", "saturated"} if H > 1 else {"inverse"}), (tag, b.branches)


def test_the_sets_meet_the_guards_on_the_reference():
    """What test_gpu_held_self.py asserts from the reference's books, here without a device at r19_h33: nothing
    within 1e-6 of the barrier's branch point, no NaN cost, the self term moves every rollout's cost in the first
    two updates, update 0 on the inverse branch only, update 1 on both, and across the three updates every
    degenerate class of segment_distance and at least one general one."""
    classes = set()
    for j, comp, term, J, (x, U, eps) in _updates("r19_h33"):
        b = term.sbooks
        print("update %d: least margin %.3e, least v %.4f, %s, evaluated %d, classes %s"
              % (j, b.least_margin, b.least_v, sorted(b.branches), b.evaluated, sorted(b.classes)))
        assert not np.isnan(J).any()
        check_books(term, j, "r19_h33")
        classes |= b.classes
        if j < 2:   # the same rollouts without the configuration
            comp.held_self = None
            comp.set_obstacles(*SS.sets()[j])
            assert np.all(J != comp.costs(x, U, eps)), j
    assert set(CR.DEGENERATE) <= classes and classes & set(CR.PROPER), classes


# ---- the library, without a device ---------------------------------------------------------------

def test_symbols_and_constants():
    L = load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert L.mppi_abi_version() == 5
    text = open(HEADER).read()
    assert re.search(r"^#define MPPI_HELD_SELF_UNITS 0x7Fu$", text, re.M) and abi.MPPI_HELD_SELF_UNITS == 0x7F
    assert re.search(r"^#define MPPI_HELD_SELF_SEGMENTS 8$", text, re.M) and abi.MPPI_HELD_SELF_SEGMENTS == 8
    assert re.search(r"^#define MPPI_HELD_SELF_UNIT_POINT\(i\) \(1u << \(i\)\)$", text, re.M)
    assert re.search(r"^#define MPPI_HELD_SELF_UNIT_SEGMENT\(s\) \(1u << \(4 \+ \(s\)\)\)$", text, re.M)
    assert [am.held_self_unit_point(i) for i in range(4)] == [1, 2, 4, 8]
    assert [am.held_self_unit_segment(s) for s in range(3)] == [16, 32, 64]
    assert sum(am.held_self_unit_point(i) for i in range(4)) + sum(am.held_self_unit_segment(s) for s in range(3)) == 0x7F
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            am.held_self_unit_point(bad)
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            am.held_self_unit_segment(bad)
    d = abi.mppi_held_self()
    L.mppi_default_held_self(C.byref(d))
    assert (d.units, d.segments, list(d.radii)) == (0x7F, 0x1F, [0.1] * 8)
    assert am.HeldSelf.from_c(d) == am.HeldSelf()


def test_struct_layout_matches_the_header():
    o = abi.mppi_held_self
    assert C.sizeof(o) == 8 + 64
    assert (o.units.offset, o.segments.offset, o.radii.offset) == (0, 4, 8)
    text = open(HEADER).read()
    body = re.search(r"typedef struct mppi_held_self \{(.*?)\} mppi_held_self;", text, re.S).group(1)
    assert [x.strip() for x in body.split(";") if x.strip()] == ["uint32_t units", "uint32_t segments", "double radii[MPPI_HELD_SELF_SEGMENTS]"]


def test_held_self_validation_and_round_trip():
    cfg = SS.tower()
    c = cfg.to_c()
    assert (c.units, c.segments, list(c.radii)) == (cfg.units, cfg.segments, list(cfg.radii))
    assert am.HeldSelf.from_c(c) == cfg and am.HeldSelf.from_c(c) != am.HeldSelf()
    assert am.HeldSelf(units=0, segments=0).to_c().units == 0
    assert am.HeldSelf(radii=[0.0] * 8).radii == (0.0,) * 8
    for bad in (lambda: am.HeldSelf(units=0x80), lambda: am.HeldSelf(units=-1), lambda: am.HeldSelf(segments=0x100),
                lambda: am.HeldSelf(radii=(0.1,) * 7), lambda: am.HeldSelf(radii=(0.1,) * 7 + (-0.1,)),
                lambda: am.HeldSelf(radii=(math.nan,) + (0.1,) * 7), lambda: am.HeldSelf(radii=(0.1,) * 7 + (math.inf,))):
        with pytest.raises(ValueError):
            bad()


def test_refusals_without_a_device():
    """NULL handles, and the dynamics object's NULL check that comes before any device call."""
    L = load()
    c = am.HeldSelf().to_c()
    o = SS.objects()[0].to_c()
    on = C.c_int(0)
    v = C.c_double(0.0)
    assert L.mppi_set_held_self_avoidance(None) == abi.MPPI_ERR_INVALID
    assert L.mppi_get_held_self_avoidance(None, C.byref(on)) == abi.MPPI_ERR_INVALID
    assert L.mppi_set_held_self(None, C.byref(c)) == abi.MPPI_ERR_INVALID
    assert L.mppi_get_held_self(None, C.byref(c), C.byref(on)) == abi.MPPI_ERR_INVALID
    assert L.mppi_optimal_held_self_cost(None, C.byref(v)) == abi.MPPI_ERR_INVALID
    assert L.mppi_dynamics_held_self_cost(None, None, C.byref(o), C.byref(c), C.byref(v)) == abi.MPPI_ERR_INVALID
    L.mppi_default_held_self(None)   # (a NULL is ignored)


def test_held_self_clearance_on_a_hand_made_path():
    """A robot whose segment 3 stands at y = 3 from z = -1 to 1 and whose segment 1 is the point (0, 0, 2), and a
    beam from the origin along x that walks along y, one metre a step."""
    H = 3
    links = np.zeros((H, abi.MPPI_LINK_N, 3))
    links[:, abi.MPPI_LINK_PIVOT:abi.MPPI_LINK_PIVOT + 8] = _points(p1=(0.0, 0.0, 2.0), p2=(0.0, 0.0, 2.0), p3=(0.0, 3.0, -1.0),
                                                                      p4=(0.0, 3.0, 1.0))[:8]
    predicted = SimpleNamespace(links=links, end_effector=np.tile([108.0, 0.0, 0.0], (H, 1)))
    paths = np.full((H, 4, 3), np.nan)
    for k in range(H):
        paths[k, 0] = (0.0, 1.0 * k, 0.0)
        paths[k, 1] = (4.0, 1.0 * k, 0.0)
    beam = am.HeldObject([(0, 0, 0), (4, 0, 0)], (0.25, 0.125), (0.0625,))
    cfg = am.HeldSelf(units=0x7F, segments=(1 << 1) | (1 << 3), radii=(0.5,) * 8)
    got = am.held_self_clearance(predicted, paths, beam, cfg)
    assert got.shape == (H, 7, 8)
    assert np.array_equal(got[:, 0, 3], [3.0 - 0.75, 2.0 - 0.75, 1.0 - 0.75])             # held point 0 to segment 3
    assert np.array_equal(got[:, 4, 3], [3.0 - 0.5625, 2.0 - 0.5625, 1.0 - 0.5625])       # held segment 0 to segment 3
    assert np.array_equal(got[:, 0, 1], [2.0 - 0.75, math.sqrt(5.0) - 0.75, math.sqrt(8.0) - 0.75])
    assert np.array_equal(got[0, 1, 3], 5.0 - 0.625)
    on = np.zeros((7, 8), dtype=bool)
    on[np.ix_([0, 1, 4], [1, 3])] = True
    assert np.array_equal(np.isnan(got), np.broadcast_to(~on, got.shape))                 # off bits and absent units are NaN
    assert np.isnan(am.held_self_clearance(predicted, paths, None, cfg)).all()
    assert np.isnan(am.held_self_clearance(predicted, paths, beam, None)).all()
    two = SimpleNamespace(links=np.stack([links, links]), end_effector=np.stack([predicted.end_effector] * 2))
    assert np.array_equal(am.held_self_clearance(two, np.stack([paths, paths]), beam, cfg)[1], got, equal_nan=True)
