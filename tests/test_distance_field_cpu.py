"""Obstacle avoidance with a distance field without a GPU: the sample of field_reference.py against
answers worked out by hand on dyadic grids (where trilinear interpolation is exact), the package's
vectorised sample against it bit for bit, the reference against capsule_reference.py where the two
must agree bit for bit, the guards the GPU tests rely on, and the library's host-side surface: symbols,
struct layout, the Python round trips, the refusals that need no device, and the clearance helper."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi
from assistedmanipulation_amd._lib import HEADER, load

import capsule_reference as CR
import capsule_sets as CS
import field_reference as FR
import field_sets as FS
import link_reference as LR
from launch_shapes import by_name, horizon

NEW_SYMBOLS = ["mppi_set_distance_field_avoidance", "mppi_get_distance_field_avoidance", "mppi_set_distance_field",
               "mppi_get_distance_field", "mppi_optimal_field_cost", "mppi_dynamics_distance_field_cost"]
MARGIN = 1e-6     # the project's: least |v - bound|, and here the least distance to the grid's boundary in grid units
CLEAR_F = 0.02

# dyadic grids: origin, voxel and the values are dyadic, so every operation of the sample is exact
DIMS = (5, 4, 3)
ORIGIN, VOXEL = (-1.0, 0.5, 2.0), 0.25


def linear(x, y, z):
    return 2.0 * x - 3.0 * y + 0.5 * z + 1.0


def multilinear(x, y, z):
    return x * y * z


def _dyadic(fn, origin=ORIGIN):
    return am.DistanceField.from_function(fn, origin, VOXEL, DIMS)


def _world(g, origin=ORIGIN):
    return [origin[a] + VOXEL * g[a] for a in range(3)]


# grid coordinates of the by-hand points: interior dyadic points, nodes, every top face, the last corner
TOP = [DIMS[a] - 1 for a in range(3)]
INSIDE = [(0.0, 0.0, 0.0), (0.5, 0.25, 0.75), (1.0, 2.0, 1.0), (3.75, 2.5, 1.125), (2.0, 1.5, 0.0),
          (TOP[0], 1.5, 0.5), (1.25, TOP[1], 0.5), (1.25, 1.5, TOP[2]), (TOP[0], TOP[1], 0.25), tuple(TOP),
          (TOP[0] - 0.125, TOP[1] - 0.5, TOP[2] - 0.25)]


@pytest.mark.parametrize("fn", [linear, multilinear])
@pytest.mark.parametrize("g", INSIDE)
def test_sample_by_hand_on_a_dyadic_grid(fn, g):
    f = _dyadic(fn)
    p = _world(g)
    D, edge = FR.sample(f, p)
    assert D == fn(*p)                                   # trilinear interpolation is exact on both
    assert float(f.sample(p)) == D                       # the package's vectorised sample
    assert edge == min(min(abs(g[a]), abs(g[a] - TOP[a])) for a in range(3))


def test_outside_each_face_by_one_ulp_and_nan():
    """The grid at the origin here: p - 0 is p, and p * 4 keeps p's ulp, so that one ulp of p outside a
    face is one ulp of g outside [0, n - 1] (the definition tests g)."""
    origin = (0.0, 0.0, 0.0)
    f = _dyadic(linear, origin)
    mid = [1.5, 1.25, 0.5]
    for a in range(3):
        lo, hi = _world(mid, origin), _world(mid, origin)
        lo[a] = math.nextafter(origin[a], -math.inf)
        hi[a] = math.nextafter(origin[a] + VOXEL * TOP[a], math.inf)
        for p in (lo, hi):
            assert FR.sample(f, p)[0] is None and float(f.sample(p)) == math.inf
        on_lo, on_hi = _world(mid, origin), _world(mid, origin)
        on_lo[a], on_hi[a] = origin[a], origin[a] + VOXEL * TOP[a]
        for p in (on_lo, on_hi):                         # the faces themselves are inside
            assert FR.sample(f, p)[0] == linear(*p) and float(f.sample(p)) == linear(*p)
        bad = _world(mid, origin)
        bad[a] = math.nan
        assert math.isnan(FR.sample(f, bad)[0]) and math.isnan(float(f.sample(bad)))
    far = _world(mid, origin)
    far[0] = math.inf
    assert FR.sample(f, far)[0] is None and float(f.sample(far)) == math.inf


def test_a_transposed_index_shows():
    """x y z + 2 y on a grid whose three dimensions differ: swapping two axes gives another value."""
    f = _dyadic(lambda x, y, z: x * y * z + 2.0 * y)
    p = _world((3.5, 1.25, 0.5))
    assert FR.sample(f, p)[0] == p[0] * p[1] * p[2] + 2.0 * p[1]
    assert f.values.shape == DIMS and f.values.flags["C_CONTIGUOUS"] and f.values.dtype == np.float32
    assert f.values[3, 1, 2] == np.float32(multilinear(*_world((3, 1, 2))) + 2.0 * _world((3, 1, 2))[1])


def test_the_vectorised_sample_against_the_scalar_reference_bit_for_bit():
    rng = np.random.default_rng(3)
    for f in (FS.field_h(), FS.field_g()):
        n = np.asarray(f.dims)
        lo = f.origin - 2.0 * f.voxel
        pts = lo + rng.random((600, 3)) * ((n + 3) * f.voxel)           # inside and around the grid
        nodes = f.origin + rng.integers(0, n, (100, 3)) * f.voxel       # nodes, faces among them
        pts = np.concatenate([pts, nodes, f.origin[None, :] + (n - 1) * f.voxel * rng.integers(0, 2, (20, 3))])
        got = f.sample(pts)
        seen = set()
        for i, p in enumerate(pts):
            D, _ = FR.sample(f, p)
            seen.add(D is None)
            assert (got[i] == math.inf) if D is None else (got[i] == D), (i, p)
        assert seen == {True, False}
    assert f.sample(np.zeros((2, 5, 3))).shape == (2, 5)


def _updates(name, fields, primitives=(), n_rollouts=None, cls=FR.Composition):
    """test_capsules_cpu.py::_updates with the field composition: one field per update."""
    _, S, H, keep = by_name(name)[:4]
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=4)
    model = am.FrankaRidgebackDynamics().model
    comp = cls(conf, model, CS.objective(), am.constant_forecast(H), capsules=CS.capsules())
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance))
    U = np.zeros((H, 12))
    x = am.huddled_state()
    R = n_rollouts or S + 2
    for j, field in enumerate(fields):
        x = x.copy()
        x[3 + j] += 0.03
        if isinstance(comp, FR.Composition):
            comp.field = field
        term = comp.set_obstacles(*(primitives[j] if primitives else ([], 0.0)))
        eps = rng.standard_normal((R, H, 12)) * sd
        eps[0] = 0.0
        J = comp.costs(x, U, eps)
        yield j, comp, term, J, (x, U, eps)
        _, _, U = LR.mppi_update(conf, J, eps, U)


def test_no_field_reproduces_the_capsule_reference_bit_for_bit():
    sets = CS.cde()[:2]
    new = _updates("r19_h33", [None, None], sets, n_rollouts=5)
    old = _updates("r19_h33", [None, None], sets, n_rollouts=5, cls=CR.Composition)
    for (j, _, term, J, _), (_, _, cap, Jc, _) in zip(new, old):
        assert np.array_equal(J, Jc) and term.fbooks.inside == term.fbooks.outside == 0
        assert (term.least_margin, term.least_v, term.branches, term.evaluated) == (cap.least_margin, cap.least_v, cap.branches, cap.evaluated)


def check_books(term, j, tag):
    """The guards on the reference's own bookkeeping for the fields of field_sets.fgh(): what every
    parity run asserts, on the device's own noise."""
    b = term.fbooks
    assert b.least_margin >= MARGIN, (tag, j, b.least_margin)
    assert b.edge >= MARGIN, (tag, j, b.edge)
    if j == 0:
        assert b.least_v >= CLEAR_F and b.branches == {"inverse"}, (tag, b.least_v, b.branches)
    else:
        assert b.branches == {"inverse", "saturated"}, (tag, j, b.branches)
    if j == 2:
        assert b.inside > 0 and b.outside > 0, (tag, b.inside, b.outside)
    else:
        assert b.inside > 0 and b.outside == 0, (tag, j, b.inside, b.outside)


def test_the_fields_meet_the_guards_on_the_reference():
    """What test_gpu_distance_field.py asserts from the reference's own books, here without a device at
    r19_h33: field F stays 0.02 m clear on the inverse branch, G and H take both branches, H has inside
    and outside samples, nothing comes within 1e-6 of the barrier's branch discontinuity or, in grid
    units, of the grid's boundary, no cost is NaN and the term moves every cost."""
    for j, comp, term, J, (x, U, eps) in _updates("r19_h33", FS.fgh()):
        b = term.fbooks
        print("field %s: least margin %.3e, least v %.4f, %s, inside %d, outside %d, least distance to the grid's edge %.3e"
              % ("FGH"[j], b.least_margin, b.least_v, sorted(b.branches), b.inside, b.outside, b.edge))
        assert not np.isnan(J).any()
        check_books(term, j, "r19_h33")
        assert np.abs(J - comp.base.costs(x, U, eps)).min() > 1e3


# ---- the library, without a device --------------------------------------------------------------

def test_symbols_and_constants():
    L = load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert L.mppi_abi_version() == 5
    text = open(HEADER).read()
    for macro in ("MPPI_DISTANCE_FIELD_MIN_DIM", "MPPI_DISTANCE_FIELD_MAX_DIM", "MPPI_DISTANCE_FIELD_MAX_SAMPLES"):
        m = re.search(r"^#define %s (\d+)\b" % macro, text, re.M)
        assert m and int(m.group(1)) == getattr(abi, macro), macro
    assert re.search(r"^#define MPPI_DISTANCE_FIELD_MAX_VALUES \(1 << 24\)$", text, re.M) and abi.MPPI_DISTANCE_FIELD_MAX_VALUES == 2 ** 24


def test_struct_layout_matches_the_header():
    f = abi.mppi_distance_field
    assert C.sizeof(f) == 56
    assert (f.dims.offset, f.segment_samples.offset, f.mask.offset, f.pad.offset, f.origin.offset, f.voxel.offset) == (0, 12, 16, 20, 24, 48)
    text = open(HEADER).read()
    body = re.search(r"typedef struct mppi_distance_field \{(.*?)\} mppi_distance_field;", text, re.S).group(1)
    assert [x.strip() for x in body.split(";") if x.strip()] == ["int32_t dims[3]", "int32_t segment_samples", "uint32_t mask", "int32_t pad",
                                                                "double origin[3]", "double voxel"]


def test_defaults_and_round_trips():
    f = am.DistanceField(np.zeros((2, 3, 4)), (0, 0, 0), 0.1)
    assert f.mask == am.MASK_ALL | am.MASK_SEGMENTS == 0xFF01FF and f.segment_samples == 3 and f.dims == (2, 3, 4)
    g = FS.field_h()
    c = g.to_c()
    assert list(c.dims) == [13, 11, 9] and c.segment_samples == 3 and c.mask == FS.EVERYTHING and c.pad == 0
    assert list(c.origin) == [0.5, 0.5, 0.9] and c.voxel == 0.05 and g.inv_voxel == 1.0 / 0.05
    back = am.DistanceField(g.values, list(c.origin), c.voxel, c.mask, c.segment_samples)
    assert back == g and back != FS.field_f()
    assert g.values_ptr()[(3 * 11 + 2) * 9 + 5] == g.values[3, 2, 5]            # z fastest
    assert FS.field_f().dims == (63, 61, 47) and FS.field_f().mask == 0xFE01FE
    h = am.DistanceField.from_function(lambda x, y, z: x + 10.0 * y + 100.0 * z, (1.0, 2.0, 3.0), 0.5, (2, 3, 4), segment_samples=0)
    assert h.values[1, 2, 3] == 1.5 + 10.0 * 3.0 + 100.0 * 4.5 and h.segment_samples == 0
    for bad in (np.zeros((2, 2)), np.zeros(8)):
        with pytest.raises(ValueError):
            am.DistanceField(bad, (0, 0, 0), 0.1)
    with pytest.raises(ValueError):
        am.DistanceField(np.zeros((2, 2, 2)), (0, 0), 0.1)
    with pytest.raises(ValueError):
        am.DistanceField(np.zeros((2, 2, 2)), (0, 0, 0), 0.1, mask=-1)


def test_refusals_without_a_device():
    """NULL handles, and the dynamics object's argument checks that come before any device call."""
    L = load()
    f = FS.field_h().to_c()
    on = C.c_int(0)
    v = C.c_double(0.0)
    assert L.mppi_set_distance_field_avoidance(None) == abi.MPPI_ERR_INVALID
    assert L.mppi_get_distance_field_avoidance(None, C.byref(on)) == abi.MPPI_ERR_INVALID
    assert L.mppi_set_distance_field(None, C.byref(f), FS.field_h().values_ptr()) == abi.MPPI_ERR_INVALID
    assert L.mppi_get_distance_field(None, C.byref(f), C.byref(on)) == abi.MPPI_ERR_INVALID
    assert L.mppi_optimal_field_cost(None, C.byref(v)) == abi.MPPI_ERR_INVALID
    assert L.mppi_dynamics_distance_field_cost(None, None, None, C.byref(f), FS.field_h().values_ptr(), C.byref(v)) == abi.MPPI_ERR_INVALID


def test_field_clearance_on_a_synthetic_predicted():
    """test_capsules_cpu.py's synthetic Predicted: every point at the origin except PANDA_LINK7 (point 7),
    which walks along x, and the end effector 1 m above it; the field is the exact plane x - 0.25 on a
    dyadic grid that holds x in [0, 4] only, so rollout 1 (x >= 11) is outside."""
    H = 3
    raw = np.zeros((2, H, abi.MPPI_PRED_N))
    for r in range(2):
        for k in range(H):
            x = 1.0 + k + 10.0 * r
            raw[r, k, abi.MPPI_PRED_LINKS + 3 * abi.MPPI_LINK_PANDA_LINK7:][:3] = (x, 0.0, 0.0)
            raw[r, k, abi.MPPI_PRED_EE:abi.MPPI_PRED_EE + 3] = (x, 0.0, 1.0)
    pred = am.Predicted(raw, 0.5, 0.1, rollouts=[0, 1])
    conf, caps = am.ObstacleAvoidance(radii=(0.125,) * 9), am.ObstacleCapsules((0.25,) * 8)
    field = am.DistanceField.from_function(lambda x, y, z: x - 0.25, (0.0, -1.0, -1.0), 0.5, (9, 5, 7),
                                           mask=(1 << 7) | (1 << 8) | am.mask_segment(6) | am.mask_segment(7), segment_samples=3)
    pts, seg = am.field_clearance(pred, conf, field, caps)
    assert pts.shape == seg.shape == (2, H)
    assert np.array_equal(pts[0], [0.625, 1.625, 2.625])                     # x - 0.25 - 0.125 at points 7 and 8
    assert np.array_equal(seg[0], [0.25 - 0.25 - 0.25, 0.5 - 0.25 - 0.25, 0.75 - 0.25 - 0.25])   # segment 6 from the origin: its first sample, at x / 4
    assert np.all(np.isinf(pts[1]))                                          # rollout 1: points 7 and 8 outside
    np.testing.assert_array_equal(seg[1], [11.0 / 4 - 0.5, 12.0 / 4 - 0.5, 13.0 / 4 - 0.5])   # segment 6's samples at x / 4 are inside
    none = am.DistanceField(field.values, field.origin, field.voxel, mask=0)
    a, b = am.field_clearance(pred, conf, none, caps)
    assert np.all(np.isinf(a)) and np.all(np.isinf(b))
    assert am.field_clearance(am.Predicted(raw[0], 0.5, 0.1), None, field)[1].shape == (H,)
