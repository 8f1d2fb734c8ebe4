"""Obstacle avoidance (mppi_set_obstacle_avoidance / mppi_set_obstacles): the configuration, the
obstacle kinds and a host-side clearance check.  The semantics are those of include/mppi_amd.h:
obstacle o sits at position + velocity * tau, tau the time elapsed since the set's reference time;
the robot is nine spheres (the links PIVOT, PANDA_LINK1..7, then the end effector) and, with capsules
(mppi_set_obstacle_capsules), the eight segments between consecutive points."""
import ctypes as C

import numpy as np

from . import abi

MASK_ALL = abi.MPPI_OBSTACLE_MASK_ALL
MASK_SEGMENTS = abi.MPPI_OBSTACLE_MASK_SEGMENTS


def mask_segment(s):
    """MPPI_OBSTACLE_MASK_SEGMENT(s): the mask bit of robot segment s (points s and s + 1)."""
    if not 0 <= int(s) < abi.MPPI_OBSTACLE_SEGMENTS:
        raise ValueError("robot segments are 0..7")
    return abi.MPPI_OBSTACLE_MASK_SEGMENT(int(s))


def _vec3(v, what):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.shape != (3,):
        raise ValueError(f"{what} must have three components")
    return a


class ObstacleAvoidance:
    """mppi_obstacle_config: the left barrier (bound, scale, maximum_cost) every clearance goes
    through and the radii of the robot's nine points.  The defaults are mppi_default_obstacle_config's:
    {0, 1, 1e10}, and 0.75, 0.1 x 7 (the objective's default self-collision radii), 0.1 for the end
    effector."""

    def __init__(self, limit=(0.0, 1.0, 1e10), radii=(0.75, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1)):
        self.limit = tuple(float(v) for v in limit)
        self.radii = tuple(float(v) for v in radii)
        if len(self.limit) != 3 or len(self.radii) != abi.MPPI_OBSTACLE_POINTS:
            raise ValueError("limit is (bound, scale, maximum_cost); radii has one entry per robot point (9)")

    def to_c(self):
        c = abi.mppi_obstacle_config()
        c.limit.bound, c.limit.scale, c.limit.maximum_cost = self.limit
        for i, r in enumerate(self.radii):
            c.radii[i] = r
        return c

    @staticmethod
    def from_c(c):
        return ObstacleAvoidance((c.limit.bound, c.limit.scale, c.limit.maximum_cost), tuple(c.radii))

    def __eq__(self, other):
        return isinstance(other, ObstacleAvoidance) and self.limit == other.limit and self.radii == other.radii

    def __repr__(self):
        return f"ObstacleAvoidance(limit={self.limit}, radii={self.radii})"


class ObstacleCapsules:
    """mppi_capsule_config: the radii of the robot's eight segments, segment s between robot points s
    and s + 1.  The default is mppi_default_capsule_config's: 0.1 for every segment."""

    def __init__(self, segment_radii=(0.1,) * 8):
        self.segment_radii = tuple(float(v) for v in segment_radii)
        if len(self.segment_radii) != abi.MPPI_OBSTACLE_SEGMENTS:
            raise ValueError("segment_radii has one entry per robot segment (8)")

    def to_c(self):
        c = abi.mppi_capsule_config()
        for i, r in enumerate(self.segment_radii):
            c.segment_radii[i] = r
        return c

    @staticmethod
    def from_c(c):
        return ObstacleCapsules(tuple(c.segment_radii))

    def __eq__(self, other):
        return isinstance(other, ObstacleCapsules) and self.segment_radii == other.segment_radii

    def __repr__(self):
        return f"ObstacleCapsules(segment_radii={self.segment_radii})"


class _Obstacle:
    kind = None

    def __init__(self, position, velocity, normal, radius, mask):
        self.position = _vec3(position, "position")
        self.velocity = _vec3(velocity, "velocity")
        self.normal = _vec3(normal, "normal")
        self.radius = float(radius)
        self.mask = int(mask)

    def to_c(self):
        o = abi.mppi_obstacle()
        o.kind = self.kind
        if not 0 <= self.mask <= 0xFFFFFFFF:   # (what fits the field reaches the engine's own check of bits 9..31)
            raise ValueError("obstacle mask %#x does not fit the field (points: bits 0..8, segments: 16..23)" % self.mask)
        o.mask = self.mask
        for i in range(3):
            o.position[i] = self.position[i]
            o.velocity[i] = self.velocity[i]
            o.normal[i] = self.normal[i]
        o.radius = self.radius
        return o

    def at(self, tau):
        """The obstacle's reference point after `tau` seconds."""
        return self.position + self.velocity * tau


class SphereObstacle(_Obstacle):
    """A sphere of `radius` >= 0 whose centre starts at `centre` and moves with `velocity`; `mask` bit
    i: robot point i is tested against it."""
    kind = abi.MPPI_OBSTACLE_SPHERE

    def __init__(self, centre, radius, velocity=(0, 0, 0), mask=MASK_ALL):
        super().__init__(centre, velocity, (0, 0, 0), radius, mask)

    @property
    def centre(self):
        return self.position

    def __repr__(self):
        return f"SphereObstacle({self.position.tolist()}, {self.radius}, velocity={self.velocity.tolist()}, mask={self.mask:#x})"


class HalfSpaceObstacle(_Obstacle):
    """The solid {x : normal . (x - point) <= 0}: `normal` is a unit vector pointing into free space,
    `point` moves with `velocity`."""
    kind = abi.MPPI_OBSTACLE_HALF_SPACE

    def __init__(self, point, normal, velocity=(0, 0, 0), mask=MASK_ALL):
        super().__init__(point, velocity, normal, 0.0, mask)

    @property
    def point(self):
        return self.position

    def __repr__(self):
        return f"HalfSpaceObstacle({self.position.tolist()}, {self.normal.tolist()}, velocity={self.velocity.tolist()}, mask={self.mask:#x})"


class CapsuleObstacle(_Obstacle):
    """The segment from `start` to `start + axis` with `radius` >= 0, moving as a whole with `velocity`
    (capsule handles: Trajectory.set_obstacle_capsules).  `axis` is any finite vector; zero gives a
    sphere.  `mask`: bits 0..8 the robot's points, bits 16..23 (mask_segment) its segments."""
    kind = abi.MPPI_OBSTACLE_CAPSULE

    def __init__(self, start, axis, radius, velocity=(0, 0, 0), mask=MASK_ALL | MASK_SEGMENTS):
        super().__init__(start, velocity, axis, radius, mask)

    @property
    def start(self):
        return self.position

    @property
    def axis(self):
        return self.normal

    def __repr__(self):
        return (f"CapsuleObstacle({self.position.tolist()}, {self.normal.tolist()}, {self.radius}, "
                f"velocity={self.velocity.tolist()}, mask={self.mask:#x})")


def obstacle_from_c(o):
    p, v, n = list(o.position), list(o.velocity), list(o.normal)
    if o.kind == abi.MPPI_OBSTACLE_CAPSULE:
        return CapsuleObstacle(p, n, o.radius, v, o.mask)
    if o.kind == abi.MPPI_OBSTACLE_HALF_SPACE:
        return HalfSpaceObstacle(p, n, v, o.mask)
    return SphereObstacle(p, o.radius, v, o.mask)


def obstacles_to_c(obstacles):
    """(array, count) for mppi_set_obstacles; the array always has room for MPPI_MAX_OBSTACLES, so a
    longer list reaches the engine's own count check."""
    obstacles = list(obstacles)
    arr = (abi.mppi_obstacle * max(len(obstacles), abi.MPPI_MAX_OBSTACLES))()
    for i, o in enumerate(obstacles):
        arr[i] = o.to_c()
    return arr, len(obstacles)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def segment_distance(a, b, c, e):
    """The distance between the segments a -> b and c -> c + e (arrays of (..., 3), broadcast against
    each other): include/mppi_amd.h's definition, Ericson's closest-point form with exact-zero guards
    only.  A zero-length segment is a point."""
    a, b, c, e = (np.asarray(v, dtype=np.float64) for v in (a, b, c, e))
    d1, r = b - a, a - c
    A, E, F = _dot(d1, d1), _dot(e, e), _dot(e, r)
    Cc, B = _dot(d1, r), _dot(d1, e)
    den = A * E - B * B
    clamp = lambda x: np.minimum(np.maximum(x, 0.0), 1.0)   # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        s0 = np.where(den > 0.0, clamp((B * F - Cc * E) / den), 0.0)
        tg = (B * s0 + F) / E
        lo = (E == 0.0) | (tg < 0.0)
        hi = ~lo & (tg > 1.0)
        sr = clamp(np.where(lo, -Cc, B - Cc) / A)
        s = np.where(A == 0.0, 0.0, np.where(lo | hi, sr, s0))
        t = np.where(lo, 0.0, np.where(hi, 1.0, tg))
    d = (a + s[..., None] * d1) - (c + t[..., None] * e)
    return np.sqrt(_dot(d, d))


def obstacle_clearance(predicted, config, obstacles, time, capsules=None):
    """The least clearance per step of a `Predicted` (Trajectory.predicted_optimal / _rollouts) to
    `obstacles`, a set given at reference time `time`: an array of predicted.raw's leading shape
    (..., H), +inf where no point is tested.  Host only, plain numpy.

    With `capsules` (an ObstacleCapsules) the result is a pair: that array over the masked points
    (a capsule obstacle by the point-to-segment distance), and the same over the masked segments,
    segment s between points s and s + 1 of the same row, with the capsules' radii.  Without it a set
    may hold spheres and half-spaces only, and segment bits are ignored.

    The positions are the Predicted's link and end-effector columns, which are forward kinematics at
    q_k itself, NOT lagged: the objective's term of step k reads the links at q_{k-1} (q_0 for k = 0),
    so row k here is what the cost of step k + 1 saw.  This is the geometric answer to "how close does
    this path come", not a re-evaluation of the cost."""
    config = config or ObstacleAvoidance()
    radii = np.asarray(config.radii)
    pts = np.concatenate([predicted.links[..., abi.MPPI_LINK_PIVOT:abi.MPPI_LINK_PIVOT + 8, :],
                          predicted.end_effector[..., None, :]], axis=-2)   # (..., H, 9, 3)
    tau = np.asarray(predicted.time) - float(time)                          # (H,)
    least = np.full(pts.shape[:-2], np.inf)
    seg_least = np.full(pts.shape[:-2], np.inf)
    seg_radii = np.asarray(capsules.segment_radii) if capsules is not None else None
    for o in obstacles:
        c = o.position[None, :] + tau[:, None] * o.velocity[None, :]        # (H, 3)
        d = pts - c[:, None, :]
        if o.kind == abi.MPPI_OBSTACLE_CAPSULE and capsules is None:
            raise ValueError("a capsule obstacle needs capsules= (an ObstacleCapsules)")
        if o.kind == abi.MPPI_OBSTACLE_HALF_SPACE:
            h = d @ o.normal
            v = h - radii
        elif o.kind == abi.MPPI_OBSTACLE_CAPSULE:
            v = segment_distance(pts, pts, c[:, None, :], o.normal) - (radii + o.radius)
        else:
            v = np.sqrt((d * d).sum(axis=-1)) - (radii + o.radius)
        on = np.array([(o.mask >> i) & 1 for i in range(abi.MPPI_OBSTACLE_POINTS)], dtype=bool)
        if on.any():
            least = np.minimum(least, np.where(on, v, np.inf).min(axis=-1))
        if capsules is None:
            continue
        if o.kind == abi.MPPI_OBSTACLE_HALF_SPACE:
            vs = np.minimum(h[..., :-1], h[..., 1:]) - seg_radii
        else:
            e = o.normal if o.kind == abi.MPPI_OBSTACLE_CAPSULE else np.zeros(3)
            vs = segment_distance(pts[..., :-1, :], pts[..., 1:, :], c[:, None, :], e) - (seg_radii + o.radius)
        on = np.array([(o.mask >> (16 + s)) & 1 for s in range(abi.MPPI_OBSTACLE_SEGMENTS)], dtype=bool)
        if on.any():
            seg_least = np.minimum(seg_least, np.where(on, vs, np.inf).min(axis=-1))
    return least if capsules is None else (least, seg_least)
