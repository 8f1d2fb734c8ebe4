"""The trajectory safety filter (mppi_set_safety_filter): FrankaRidgeback::TrajectorySafetyFilter's
Configuration (frankaridgeback/safety.hpp:15-40), live.  Joint position, velocity and acceleration
limits on joints 0..9 of the plan, applied on the device between optimise() and the publish; the
semantics are those of include/mppi_amd.h and DESIGN.md section 1."""
import ctypes as C

import numpy as np

from . import abi

_LIMITS = ("position_minimum", "position_maximum", "velocity_minimum", "velocity_maximum",
           "acceleration_minimum", "acceleration_maximum")
_SWITCHES = ("limit_joints", "limit_velocity", "limit_acceleration", "limit_reach")


class TrajectorySafetyFilter:
    """mppi_safety_filter_desc.  The defaults are mppi_default_safety_filter's: every switch off,
    robot.urdf's joint position and velocity limits, and no acceleration limits (+-inf: robot.urdf
    has none).  A limit may be +-inf; NaN or minimum > maximum is refused when the filter is set,
    and so is limit_reach."""

    def __init__(self, **fields):
        from ._lib import load
        c = abi.mppi_safety_filter_desc()
        load().mppi_default_safety_filter(C.byref(c))
        for name in _LIMITS:
            setattr(self, name, np.array(getattr(c, name)[:], dtype=np.float64))
        self.reach_maximum, self.reach_minimum = c.reach_maximum, c.reach_minimum
        for name in _SWITCHES:
            setattr(self, name, bool(getattr(c, name)))
        for name, value in fields.items():
            if name in _LIMITS:
                a = np.asarray(value, dtype=np.float64).reshape(-1)
                if a.shape != (abi.MPPI_FR_JOINTS,):
                    raise ValueError(f"{name} has one entry per joint (12)")
                setattr(self, name, a.copy())
            elif name in _SWITCHES:
                setattr(self, name, bool(value))
            elif name in ("reach_maximum", "reach_minimum"):
                setattr(self, name, float(value))
            else:
                raise TypeError(f"TrajectorySafetyFilter has no field {name!r}")

    def to_c(self):
        c = abi.mppi_safety_filter_desc()
        for name in _LIMITS:
            arr = getattr(c, name)
            for i, v in enumerate(getattr(self, name)):
                arr[i] = float(v)
        c.reach_maximum, c.reach_minimum = self.reach_maximum, self.reach_minimum
        for name in _SWITCHES:
            setattr(c, name, 1 if getattr(self, name) else 0)
        return c

    @staticmethod
    def from_c(c):
        f = TrajectorySafetyFilter()
        for name in _LIMITS:
            setattr(f, name, np.array(getattr(c, name)[:], dtype=np.float64))
        f.reach_maximum, f.reach_minimum = c.reach_maximum, c.reach_minimum
        for name in _SWITCHES:
            setattr(f, name, bool(getattr(c, name)))
        return f

    def __eq__(self, other):
        return (isinstance(other, TrajectorySafetyFilter)
                and all(np.array_equal(getattr(self, n), getattr(other, n)) for n in _LIMITS)
                and all(getattr(self, n) == getattr(other, n) for n in _SWITCHES + ("reach_maximum", "reach_minimum")))

    def __repr__(self):
        on = [n for n in _SWITCHES if getattr(self, n)]
        return f"TrajectorySafetyFilter({', '.join(on) or 'off'})"
