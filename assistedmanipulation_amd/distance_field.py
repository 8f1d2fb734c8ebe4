"""The sensed environment as a signed-distance grid (mppi_set_distance_field_avoidance /
mppi_set_distance_field): the field, a numpy restatement of its sample and a host-side clearance
check.  The semantics are those of include/mppi_amd.h: a regular grid of fp32 distances in metres,
negative inside matter, sample (0, 0, 0) at `origin`, one edge length `voxel` on every axis; D(p) is
the trilinear interpolant of the cell that holds p (z, then y, then x), a point outside the grid
contributes nothing, and the robot is sampled at its nine points and at `segment_samples` interior
points of each of its eight segments."""
import ctypes as C

import numpy as np

from . import abi
from .obstacles import MASK_ALL, MASK_SEGMENTS, ObstacleAvoidance, ObstacleCapsules


class DistanceField:
    """mppi_distance_field and its values.  `values`: an (nx, ny, nz) array (stored as C-contiguous
    fp32), every dimension in [2, 512] and at most 2^24 values, all finite; `mask`: bits 0..8 the
    robot's points, bits 16..23 its segments; `segment_samples`: 0..8 interior points per segment."""

    def __init__(self, values, origin, voxel, mask=MASK_ALL | MASK_SEGMENTS, segment_samples=3):
        self.values = np.ascontiguousarray(values, dtype=np.float32)
        if self.values.ndim != 3:
            raise ValueError("values is an (nx, ny, nz) array")
        self.origin = np.asarray(origin, dtype=np.float64).reshape(-1)
        if self.origin.shape != (3,):
            raise ValueError("origin has three components")
        self.voxel = float(voxel)
        self.mask = int(mask)
        self.segment_samples = int(segment_samples)
        if not 0 <= self.mask <= 0xFFFFFFFF:
            raise ValueError("mask %#x does not fit the field (points: bits 0..8, segments: 16..23)" % self.mask)
        if not -2 ** 31 <= self.segment_samples < 2 ** 31:
            raise ValueError("segment_samples does not fit the field")

    @staticmethod
    def from_function(fn, origin, voxel, dims, **kw):
        """The field of fn(x, y, z) -> distance, called once with three (nx, ny, nz) arrays of the
        samples' world coordinates origin + index * voxel."""
        origin = np.asarray(origin, dtype=np.float64)
        ax = [origin[a] + np.arange(int(dims[a]), dtype=np.float64) * float(voxel) for a in range(3)]
        x, y, z = np.meshgrid(*ax, indexing="ij")
        return DistanceField(np.asarray(fn(x, y, z), dtype=np.float64), origin, voxel, **kw)

    @property
    def dims(self):
        return tuple(int(n) for n in self.values.shape)

    @property
    def inv_voxel(self):
        return 1.0 / self.voxel   # (what the engine stores: one fp64 division on the host)

    def to_c(self):
        f = abi.mppi_distance_field()
        for a in range(3):
            f.dims[a] = self.values.shape[a]
            f.origin[a] = self.origin[a]
        f.segment_samples = self.segment_samples
        f.mask = self.mask
        f.pad = 0
        f.voxel = self.voxel
        return f

    def values_ptr(self):
        return self.values.ctypes.data_as(C.POINTER(C.c_float))

    def sample(self, points):
        """D at `points` (..., 3): include/mppi_amd.h's definition operation for operation (numpy's
        fp64 elementwise operations round one by one), +inf outside the grid, NaN for a NaN coordinate."""
        p = np.asarray(points, dtype=np.float64)
        n = np.asarray(self.values.shape, dtype=np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            g = (p - self.origin) * self.inv_voxel
            nan = np.isnan(g).any(axis=-1)
            inside = ((g >= 0.0) & (g <= (n - 1).astype(np.float64))).all(axis=-1)
            gc = np.where(np.isnan(g), 0.0, np.minimum(np.maximum(g, 0.0), (n - 2).astype(np.float64)))
            i = gc.astype(np.int64)   # floor of a non-negative number, at most n - 2
            f = g - i.astype(np.float64)
            v = self.values
            c = lambda dx, dy, dz: v[i[..., 0] + dx, i[..., 1] + dy, i[..., 2] + dz].astype(np.float64)   # noqa: E731
            L = lambda a, b, t: a + t * (b - a)   # noqa: E731
            fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
            y0 = L(L(c(0, 0, 0), c(0, 0, 1), fz), L(c(0, 1, 0), c(0, 1, 1), fz), fy)
            y1 = L(L(c(1, 0, 0), c(1, 0, 1), fz), L(c(1, 1, 0), c(1, 1, 1), fz), fy)
            D = L(y0, y1, fx)
        return np.where(nan, np.nan, np.where(inside, D, np.inf))

    def __eq__(self, other):
        return (isinstance(other, DistanceField) and self.dims == other.dims and np.array_equal(self.origin, other.origin) and
                self.voxel == other.voxel and self.mask == other.mask and self.segment_samples == other.segment_samples and
                np.array_equal(self.values, other.values))

    def __repr__(self):
        return (f"DistanceField(dims={self.dims}, origin={self.origin.tolist()}, voxel={self.voxel}, mask={self.mask:#x}, "
                f"segment_samples={self.segment_samples})")


def field_descriptor_from_c(f):
    """(dims, origin, voxel, mask, segment_samples) of an abi.mppi_distance_field."""
    return tuple(f.dims), np.array(list(f.origin)), f.voxel, f.mask, f.segment_samples


def field_clearance(predicted, config, field, capsules=None):
    """The least clearance per step of a `Predicted` to `field`, beside obstacle_clearance: a pair of
    arrays of predicted.raw's leading shape (..., H), over the masked points (D(p_i) - radii[i]) and
    over the masked segments' samples (D(p) - segment_radii[s]), +inf where nothing inside the grid is
    tested.  Host only, plain numpy; the positions are the Predicted's own (not lagged), like
    obstacle_clearance's."""
    config = config or ObstacleAvoidance()
    capsules = capsules or ObstacleCapsules()
    radii, seg_radii = np.asarray(config.radii), np.asarray(capsules.segment_radii)
    pts = np.concatenate([predicted.links[..., abi.MPPI_LINK_PIVOT:abi.MPPI_LINK_PIVOT + 8, :],
                          predicted.end_effector[..., None, :]], axis=-2)   # (..., H, 9, 3)
    on = np.array([(field.mask >> i) & 1 for i in range(abi.MPPI_OBSTACLE_POINTS)], dtype=bool)
    least = np.where(on, field.sample(pts) - radii, np.inf).min(axis=-1)
    seg_least = np.full(pts.shape[:-2], np.inf)
    son = np.array([(field.mask >> (16 + s)) & 1 for s in range(abi.MPPI_OBSTACLE_SEGMENTS)], dtype=bool)
    m = field.segment_samples
    a, b = pts[..., :-1, :], pts[..., 1:, :]
    for j in range(1, m + 1):
        phi = j / (m + 1)
        v = np.where(son, field.sample(a + phi * (b - a)) - seg_radii, np.inf)
        seg_least = np.minimum(seg_least, v.min(axis=-1))
    return least, seg_least
