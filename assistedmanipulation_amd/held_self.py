"""The held object against the robot's own links (mppi_set_held_self_avoidance / mppi_set_held_self):
which held units are tested against which robot segments, with radii of this term's own, and a
host-side clearance check on predicted paths.  The semantics are those of include/mppi_amd.h: held
unit u = 0..3 is held point u, unit 4 + s held segment s; robot segment s joins robot points s and
s + 1; the clearance is d(a, b; c, e) - (radii[s] + r_u) with the robot's segment first."""
import numpy as np

from . import abi
from .obstacles import segment_distance

HELD_SELF_UNITS = abi.MPPI_HELD_SELF_UNITS
DEFAULT_SEGMENTS = 0x1F


def held_self_unit_point(i):
    """MPPI_HELD_SELF_UNIT_POINT(i): the units bit of held point i."""
    if not 0 <= int(i) < abi.MPPI_HELD_POINTS:
        raise ValueError("held points are 0..3")
    return abi.MPPI_HELD_SELF_UNIT_POINT(int(i))


def held_self_unit_segment(s):
    """MPPI_HELD_SELF_UNIT_SEGMENT(s): the units bit of held segment s (held points s and s + 1)."""
    if not 0 <= int(s) < abi.MPPI_HELD_SEGMENTS:
        raise ValueError("held segments are 0..2")
    return abi.MPPI_HELD_SELF_UNIT_SEGMENT(int(s))


class HeldSelf:
    """mppi_held_self: `units` (bit i held point i, bit 4 + s held segment s), `segments` (bit s robot
    segment s) and `radii`, one per robot segment for this term only, finite and >= 0.  The defaults are
    mppi_default_held_self's: every unit, robot segments 0..4 - without the wrist and hand segments
    5..7, which anything in the gripper touches - and 0.1 m."""

    def __init__(self, units=HELD_SELF_UNITS, segments=DEFAULT_SEGMENTS, radii=(0.1,) * abi.MPPI_HELD_SELF_SEGMENTS):
        self.units, self.segments = int(units), int(segments)
        self.radii = tuple(float(r) for r in np.asarray(radii, dtype=np.float64).reshape(-1))
        if self.units < 0 or self.units & ~abi.MPPI_HELD_SELF_UNITS:
            raise ValueError("units has bits above bit 6")
        if self.segments < 0 or self.segments & ~0xFF:
            raise ValueError("segments has bits above bit 7")
        if len(self.radii) != abi.MPPI_HELD_SELF_SEGMENTS:
            raise ValueError("radii has one entry per robot segment (8)")
        for r in self.radii:
            if not np.isfinite(r) or r < 0.0:
                raise ValueError("the radii must be finite and >= 0")

    def to_c(self):
        c = abi.mppi_held_self()
        c.units, c.segments = self.units, self.segments
        for s, r in enumerate(self.radii):
            c.radii[s] = r
        return c

    @staticmethod
    def from_c(c):
        return HeldSelf(int(c.units), int(c.segments), [c.radii[s] for s in range(abi.MPPI_HELD_SELF_SEGMENTS)])

    def __eq__(self, other):
        return isinstance(other, HeldSelf) and (self.units, self.segments, self.radii) == (other.units, other.segments, other.radii)

    def __repr__(self):
        return f"HeldSelf(units={self.units:#x}, segments={self.segments:#x}, radii={self.radii})"


def held_self_clearance(predicted, paths, held, held_self):
    """The clearances of a held object's predicted paths to the robot's own segments on the same
    predicted path: (..., H, 7, 8), entry [k, u, s] held unit u against robot segment s at step k, NaN
    where `held` lacks the unit or a bit of `held_self` is off.  `predicted` is what
    Trajectory.predicted_optimal / predicted_rollouts return, `paths` what predicted_held_optimal /
    predicted_held_rollouts return for the same rollouts.  Host only, plain numpy; the positions are at
    q_k itself, not lagged, like obstacle_clearance's."""
    pts = np.concatenate([predicted.links[..., abi.MPPI_LINK_PIVOT:abi.MPPI_LINK_PIVOT + 8, :],
                          predicted.end_effector[..., None, :]], axis=-2)   # (..., H, 9, 3)
    paths = np.asarray(paths, dtype=np.float64)
    out = np.full(paths.shape[:-2] + (abi.MPPI_HELD_POINTS + abi.MPPI_HELD_SEGMENTS, abi.MPPI_HELD_SELF_SEGMENTS), np.nan)
    n = held.count if held is not None else 0
    if n == 0 or held_self is None:
        return out
    a, b = pts[..., :-1, :], pts[..., 1:, :]                                # (..., H, 8, 3)
    son = np.array([(held_self.segments >> s) & 1 for s in range(abi.MPPI_HELD_SELF_SEGMENTS)], dtype=bool)
    radii = np.asarray(held_self.radii)
    for u in range(abi.MPPI_HELD_POINTS + abi.MPPI_HELD_SEGMENTS):
        if not (held_self.units >> u) & 1:
            continue
        if u < abi.MPPI_HELD_POINTS:
            if u >= n:
                continue
            c, e, ru = paths[..., u, :], np.zeros(3), held.radii[u]
        else:
            s = u - abi.MPPI_HELD_POINTS
            if s + 1 >= n:
                continue
            c, ru = paths[..., s, :], held.segment_radii[s]
            e = paths[..., s + 1, :] - c
        e = np.broadcast_to(e, c.shape)
        v = segment_distance(a, b, c[..., None, :], e[..., None, :]) - (radii + ru)
        out[..., u, :] = np.where(son, v, np.nan)
    return out
