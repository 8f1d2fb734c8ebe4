"""Obstacle avoidance (mppi_set_obstacle_avoidance / mppi_set_obstacles): the configuration, the two
obstacle kinds and a host-side clearance check.  The semantics are those of include/mppi_amd.h:
obstacle o sits at position + velocity * tau, tau the time elapsed since the set's reference time;
the robot is nine spheres (the links PIVOT, PANDA_LINK1..7, then the end effector)."""
import ctypes as C

import numpy as np

from . import abi

MASK_ALL = abi.MPPI_OBSTACLE_MASK_ALL


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
            raise ValueError("obstacle mask %#x: bits above bit 8 (nine robot points)" % self.mask)
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


def obstacle_from_c(o):
    p, v, n = list(o.position), list(o.velocity), list(o.normal)
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


def obstacle_clearance(predicted, config, obstacles, time):
    """The least clearance per step of a `Predicted` (Trajectory.predicted_optimal / _rollouts) to
    `obstacles`, a set given at reference time `time`: an array of predicted.raw's leading shape
    (..., H), +inf where no point is tested.  Host only, plain numpy.

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
    for o in obstacles:
        c = o.position[None, :] + tau[:, None] * o.velocity[None, :]        # (H, 3)
        d = pts - c[:, None, :]
        if o.kind == abi.MPPI_OBSTACLE_HALF_SPACE:
            v = d @ o.normal - radii
        else:
            v = np.sqrt((d * d).sum(axis=-1)) - (radii + o.radius)
        on = np.array([(o.mask >> i) & 1 for i in range(abi.MPPI_OBSTACLE_POINTS)], dtype=bool)
        if on.any():
            least = np.minimum(least, np.where(on, v, np.inf).min(axis=-1))
    return least
