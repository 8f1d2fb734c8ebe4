"""Target tracking (mppi_set_target_tracking / mppi_set_target_path): TrackPoint follows a timed
end-effector pose path over the horizon.  The semantics are those of include/mppi_amd.h: a path is at
most 32 waypoints (time, position and optionally a quaternion x, y, z, w) with strictly increasing
times; it holds its ends, and between two waypoints position and quaternion are interpolated
linearly, the quaternion renormalised.  `TargetPath.sample` is the host's own evaluation of that rule,
operation for operation what the engine's table launch computes."""
import ctypes as C

import numpy as np

from . import abi

WAYPOINTS_MAX = abi.MPPI_TARGET_WAYPOINTS_MAX


class TargetTracking:
    """mppi_target_tracking_config: the orientation term's weight (finite, >= 0) and whether the
    orientation of a path is tracked (which needs the kinematic link-position model).  The defaults are
    mppi_default_target_tracking_config's: weight 10 (0.1 rad then costs about what 3 cm does), off."""

    def __init__(self, orientation_weight=10.0, track_orientation=False):
        self.orientation_weight = float(orientation_weight)
        self.track_orientation = bool(track_orientation)

    def to_c(self):
        c = abi.mppi_target_tracking_config()
        c.orientation_weight = self.orientation_weight
        c.track_orientation = 1 if self.track_orientation else 0
        return c

    @staticmethod
    def from_c(c):
        return TargetTracking(c.orientation_weight, bool(c.track_orientation))

    def __eq__(self, other):
        return (isinstance(other, TargetTracking) and self.orientation_weight == other.orientation_weight
                and self.track_orientation == other.track_orientation)

    def __repr__(self):
        return f"TargetTracking(orientation_weight={self.orientation_weight}, track_orientation={self.track_orientation})"


def _norm4(q):
    return np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


class TargetPath:
    """A timed pose path: `times` (N,), `positions` (N, 3) and optionally `orientations` (N, 4)
    quaternions (x, y, z, w), 1 <= N <= 32.  Refuses what the engine refuses (ValueError): times that
    are not finite and strictly increasing, positions or quaternions that are not finite, a quaternion
    norm outside [0.5, 2].  The quaternions are stored as the engine stores them: each normalised, then
    waypoint i + 1's negated whenever its dot product with waypoint i's stored one is negative
    (`raw_orientations` keeps what was given)."""

    def __init__(self, times, positions, orientations=None):
        t = np.array(times, dtype=np.float64).reshape(-1)
        n = t.shape[0]
        if not 1 <= n <= WAYPOINTS_MAX:
            raise ValueError(f"a target path has 1 to {WAYPOINTS_MAX} waypoints, not {n}")
        p = np.array(positions, dtype=np.float64)
        if p.shape != (n, 3):
            raise ValueError("positions must be (N, 3), one row per time")
        if not np.all(np.isfinite(t)):
            raise ValueError("the times must be finite")
        if not np.all(t[1:] > t[:-1]):
            raise ValueError("the times must be strictly increasing")
        if not np.all(np.isfinite(p)):
            raise ValueError("the positions must be finite")
        self.times, self.positions = t, p
        with np.errstate(over="ignore"):
            self.inv = 1.0 / (t[1:] - t[:-1])
        if not np.all(np.isfinite(self.inv)):
            raise ValueError("two times are too close together")
        self.raw_orientations = self.orientations = None
        if orientations is not None:
            q = np.array(orientations, dtype=np.float64)
            if q.shape != (n, 4):
                raise ValueError("orientations must be (N, 4) quaternions (x, y, z, w)")
            if not np.all(np.isfinite(q)):
                raise ValueError("the quaternions must be finite")
            s = np.zeros_like(q)
            for i in range(n):
                nn = _norm4(q[i])
                if not 0.5 <= nn <= 2.0:
                    raise ValueError(f"waypoint {i}: the quaternion's norm must be in [0.5, 2]")
                s[i] = q[i] / nn
                if i > 0:
                    b = s[i - 1]
                    if ((b[0] * s[i][0] + b[1] * s[i][1]) + b[2] * s[i][2]) + b[3] * s[i][3] < 0.0:
                        s[i] = -s[i]
            self.raw_orientations, self.orientations = q, s

    def __len__(self):
        return self.times.shape[0]

    @property
    def has_orientation(self):
        return self.orientations is not None

    def segment(self, t):
        """(i, f, regime) of time t: the waypoint index, the fraction to the next one, and 'before'
        (t <= time[0]), 'after' (t >= time[N - 1]) or 'inside'."""
        T, n = self.times, len(self)
        if t >= T[n - 1]:
            # (a single waypoint is both ends; it reads as 'after' unless t lies before it)
            return n - 1, 0.0, "after"
        if not t > T[0]:
            return 0, 0.0, "before"
        i = 0
        for j in range(1, n - 1):
            if T[j] <= t:
                i = j
        return i, (t - T[i]) * self.inv[i], "inside"

    def sample(self, t):
        """(position (3,), quaternion (4,) or None) of the path at time t."""
        i, f, _ = self.segment(float(t))
        i1 = min(i + 1, len(self) - 1)
        p = self.positions[i] + f * (self.positions[i1] - self.positions[i])
        if self.orientations is None:
            return p, None
        q = self.orientations[i] + f * (self.orientations[i1] - self.orientations[i])
        return p, q / _norm4(q)

    def to_c(self):
        """mppi_target_path with the orientations as they were given (the engine stores them its way)."""
        c = abi.mppi_target_path()
        c.count = len(self)
        c.has_orientation = 1 if self.raw_orientations is not None else 0
        for i in range(len(self)):
            w = c.waypoints[i]
            w.time = self.times[i]
            for k in range(3):
                w.position[k] = self.positions[i, k]
            for k in range(4):
                w.quaternion[k] = self.raw_orientations[i, k] if self.raw_orientations is not None else 0.0
        return c

    @staticmethod
    def from_c(c):
        """The path of a mppi_target_path read back from the engine (mppi_get_target_path): stored
        quaternions are taken as they are."""
        n = c.count
        t = [c.waypoints[i].time for i in range(n)]
        p = [list(c.waypoints[i].position) for i in range(n)]
        path = TargetPath(t, p)
        if c.has_orientation:
            q = np.array([list(c.waypoints[i].quaternion) for i in range(n)], dtype=np.float64)
            path.raw_orientations, path.orientations = q, q.copy()
        return path

    def __repr__(self):
        return f"TargetPath({len(self)} waypoints, t = {self.times[0]} .. {self.times[-1]}, orientations={self.has_orientation})"


def quaternion_rotation(q):
    """The rotation matrix (3, 3) of a unit quaternion (x, y, z, w)."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                     [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                     [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])
