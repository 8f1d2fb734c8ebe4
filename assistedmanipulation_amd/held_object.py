"""A held object (mppi_set_held_object_avoidance / mppi_set_held_object): what the gripper carries,
as up to four spheres fixed in the grasp frame and the segments between consecutive ones, and a
host-side clearance check on its predicted paths.  The semantics are those of include/mppi_amd.h:
held point i sits at p_ee + Ree c_i, held segment s joins held points s and s + 1; in an obstacle's
mask and in the field's, held point i is bit 9 + i and held segment s bit 24 + s."""
import numpy as np

from . import abi
from .obstacles import ObstacleAvoidance, segment_distance

MASK_HELD = abi.MPPI_OBSTACLE_MASK_HELD


def mask_held_point(i):
    """MPPI_OBSTACLE_MASK_HELD_POINT(i): the mask bit of held point i."""
    if not 0 <= int(i) < abi.MPPI_HELD_POINTS:
        raise ValueError("held points are 0..3")
    return abi.MPPI_OBSTACLE_MASK_HELD_POINT(int(i))


def mask_held_segment(s):
    """MPPI_OBSTACLE_MASK_HELD_SEGMENT(s): the mask bit of held segment s (held points s and s + 1)."""
    if not 0 <= int(s) < abi.MPPI_HELD_SEGMENTS:
        raise ValueError("held segments are 0..2")
    return abi.MPPI_OBSTACLE_MASK_HELD_SEGMENT(int(s))


class HeldObject:
    """mppi_held_object: `centres` (count, 3) in the grasp frame, in metres, count in 0..4; `radii`
    one per point, >= 0; `segment_radii` one per segment (count - 1 of them; None: zeros), >= 0.
    A beam is two points and one segment, a tray about four points and three segments, a tool tip one
    point."""

    def __init__(self, centres, radii, segment_radii=None):
        self.centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
        self.radii = tuple(float(r) for r in np.asarray(radii, dtype=np.float64).reshape(-1))
        n = self.centres.shape[0]
        if n > abi.MPPI_HELD_POINTS:
            raise ValueError("a held object has at most four points")
        if len(self.radii) != n:
            raise ValueError("radii has one entry per held point")
        nseg = max(n - 1, 0)
        if segment_radii is None:
            segment_radii = (0.0,) * nseg
        self.segment_radii = tuple(float(r) for r in np.asarray(segment_radii, dtype=np.float64).reshape(-1))
        if len(self.segment_radii) != nseg:
            raise ValueError("segment_radii has one entry per held segment (count - 1)")
        if not np.isfinite(self.centres).all():
            raise ValueError("the centres must be finite")
        for r in self.radii + self.segment_radii:
            if not np.isfinite(r) or r < 0.0:
                raise ValueError("the radii must be finite and >= 0")

    @property
    def count(self):
        return int(self.centres.shape[0])

    def to_c(self):
        o = abi.mppi_held_object()
        o.count = self.count
        o.pad = 0
        for i in range(self.count):
            for a in range(3):
                o.centres[i][a] = self.centres[i, a]
            o.radii[i] = self.radii[i]
        for s, r in enumerate(self.segment_radii):
            o.segment_radii[s] = r
        return o

    @staticmethod
    def from_c(o):
        n = int(o.count)
        return HeldObject([[o.centres[i][a] for a in range(3)] for i in range(n)], [o.radii[i] for i in range(n)],
                          [o.segment_radii[s] for s in range(max(n - 1, 0))])

    def world(self, p_ee, Ree):
        """The held points' world positions (..., count, 3) at grasp positions p_ee (..., 3) and
        rotations Ree (..., 3, 3): include/mppi_amd.h's sum, operation for operation."""
        p_ee, Ree = np.asarray(p_ee, dtype=np.float64), np.asarray(Ree, dtype=np.float64)
        c = self.centres
        with np.errstate(invalid="ignore", over="ignore"):
            rot = (Ree[..., None, :, 0] * c[:, None, 0] + Ree[..., None, :, 1] * c[:, None, 1]) + Ree[..., None, :, 2] * c[:, None, 2]
            return p_ee[..., None, :] + rot

    def __eq__(self, other):
        return (isinstance(other, HeldObject) and np.array_equal(self.centres, other.centres) and self.radii == other.radii and
                self.segment_radii == other.segment_radii)

    def __repr__(self):
        return f"HeldObject(centres={self.centres.tolist()}, radii={self.radii}, segment_radii={self.segment_radii})"


def held_object_clearance(paths, time, config, obstacles, t_ref, held, field=None):
    """The least clearance per step of a held object's predicted paths to `obstacles` (a set given at
    reference time `t_ref`) and, with `field`, to a DistanceField: an array of paths' leading shape
    (..., H), +inf where nothing is tested.  `paths` is what Trajectory.predicted_held_optimal /
    predicted_held_rollouts return, (..., H, 4, 3) with NaN rows for the points `held` does not have;
    `time` the H step times (Predicted.time).  Only the held bits of the masks are read (bit 9 + i point
    i, bit 24 + s segment s); a bit that names what `held` does not have selects nothing.  `config`
    gives nothing but a place beside obstacle_clearance's signature: the held radii are the object's.
    Host only, plain numpy; the positions are at q_k itself, not lagged, like obstacle_clearance's."""
    config = config or ObstacleAvoidance()
    paths = np.asarray(paths, dtype=np.float64)
    n = held.count if held is not None else 0
    least = np.full(paths.shape[:-2], np.inf)
    if n == 0:
        return least
    pts = paths[..., :n, :]
    radii, seg_radii = np.asarray(held.radii), np.asarray(held.segment_radii)
    tau = np.asarray(time, dtype=np.float64) - float(t_ref)

    def pon(mask):
        return np.array([(mask >> (9 + i)) & 1 for i in range(n)], dtype=bool)

    def son(mask):
        return np.array([(mask >> (24 + s)) & 1 for s in range(n - 1)], dtype=bool)

    for o in obstacles:
        c = o.position[None, :] + tau[:, None] * o.velocity[None, :]   # (H, 3)
        d = pts - c[:, None, :]
        if o.kind == abi.MPPI_OBSTACLE_HALF_SPACE:
            h = d @ o.normal
            v = h - radii
        else:
            e = o.normal if o.kind == abi.MPPI_OBSTACLE_CAPSULE else np.zeros(3)
            v = segment_distance(pts, pts, c[:, None, :], e) - (radii + o.radius)
        on = pon(o.mask)
        if on.any():
            least = np.minimum(least, np.where(on, v, np.inf).min(axis=-1))
        on = son(o.mask)
        if on.any():
            if o.kind == abi.MPPI_OBSTACLE_HALF_SPACE:
                vs = np.minimum(h[..., :-1], h[..., 1:]) - seg_radii
            else:
                vs = segment_distance(pts[..., :-1, :], pts[..., 1:, :], c[:, None, :], e) - (seg_radii + o.radius)
            least = np.minimum(least, np.where(on, vs, np.inf).min(axis=-1))
    if field is not None:
        on = pon(field.mask)
        if on.any():
            least = np.minimum(least, np.where(on, field.sample(pts) - radii, np.inf).min(axis=-1))
        on = son(field.mask)
        m = field.segment_samples
        if on.any():
            a, b = pts[..., :-1, :], pts[..., 1:, :]
            for j in range(1, m + 1):
                phi = j / (m + 1)
                v = np.where(on, field.sample(a + phi * (b - a)) - seg_radii, np.inf)
                least = np.minimum(least, v.min(axis=-1))
    return least
