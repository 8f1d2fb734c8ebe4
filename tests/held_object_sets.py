"""The held objects of the held-object tests with the obstacle sets and fields that stand beside them, as
plain data shared by the CPU checks of the reference (test_held_object_cpu.py) and the GPU parity tests
(test_gpu_held_object.py).

The grasp frame at test_gpu_link_positions._states()[0] sits at (0.856, 0.891, 0.891) with its x axis
along (0.67, 0.71, -0.20) (forward), its y axis along (0.73, -0.69, 0) (sideways) and its z axis along
(-0.14, -0.14, -0.98) (down, away from the wrist).  Under the injected noise the end effector strays up
to 0.65 m within a horizon, so what is "clear" of an object that reaches 0.3 m from the grasp keeps about a
metre from it.

Three updates, three objects:
  0 "clear":   a beam - two points 0.6 m apart across the grasp, one segment - with capsule_sets.set_c()
               for the robot and, for the beam alone, a sphere, a floor and a drifting post; the field is a
               floor and a far wall.  Every held clearance stays 0.02 m and more on the inverse branch.
  1 "breach":  a tray - four points, three segments - with set_c() again for the robot and, for the tray, a
               sphere, a bar that flies past under it and an oblique wall, all clear; the field is field_sets'
               G (thresholded) with a ball of matter on one of the tray's corners.  Both branches, the saturated
               one through the field: a thresholded map crosses the barrier's bound within a voxel, so a sample
               within 1e-6 of it is some four hundred times less likely than with a true distance.
  2 "tip":     one point 0.15 m below the grasp, a sphere beside it, field_sets' G.  (Not H, the small grid around
               the forearm: the robot's own samples cross its boundary all the time, and at r19_h129 one of them
               came within 2e-7 of it in grid units.)
Every formula is taken: held point and held segment against sphere, half-space and capsule, and the
field's point and segment samples.
"""
import numpy as np

import assistedmanipulation_amd as am

import capsule_sets as CS
import field_sets as FS
from capsule_sets import capsules, objective   # noqa: F401  (the tests' objective and segment radii)

HELD_SEGMENTS = sum(am.mask_held_segment(s) for s in range(3))


def beam():
    return am.HeldObject([(0.0, -0.3, 0.05), (0.0, 0.3, 0.05)], (0.03, 0.035), (0.025,))


def tray():
    return am.HeldObject([(-0.15, -0.15, 0.08), (0.15, -0.15, 0.08), (0.15, 0.15, 0.08), (-0.15, 0.15, 0.08)],
                         (0.02, 0.025, 0.03, 0.035), (0.02, 0.015, 0.01))


def tip():
    return am.HeldObject([(0.02, -0.01, 0.15)], (0.02,))


def objects():
    return [beam(), tray(), tip()]


def _with_held(field, mask=am.MASK_HELD):
    return am.DistanceField(field.values, field.origin, field.voxel, mask=field.mask | mask, segment_samples=field.segment_samples)


def field_clear():
    """A floor 0.1 m under the origin and a wall at x = 2.0, over field_sets' room: true distances."""
    return am.DistanceField.from_function(lambda x, y, z: np.minimum(z + 0.1, 2.0 - x), mask=FS.ABOVE_BASE | am.MASK_HELD,
                                          segment_samples=3, **FS.ROOM)


def field_breach():
    """field_sets' G with a 0.1 m ball of matter on the tray's corner 2 at the second state, thresholded like
    G: the tray's samples cross the barrier's bound within a voxel."""
    g = lambda x, y, z: np.minimum(np.minimum(FS._ball(x, y, z, (0.7106, 0.7176, 1.1857), 0.08), 1.6 - x),   # noqa: E731
                                   FS._ball(x, y, z, (1.0494, 0.8775, 0.7591), 0.1))
    return am.DistanceField.from_function(FS._thresholded(g, 10.0), mask=FS.ABOVE_BASE | am.MASK_HELD, segment_samples=3, **FS.ROOM)


def fields():
    return [field_clear(), field_breach(), _with_held(FS.field_g())]


def set_clear():
    return CS.set_c() + [
        am.SphereObstacle((1.9, 0.9, 0.9), 0.3, mask=am.MASK_HELD),
        am.HalfSpaceObstacle((0.0, 0.0, -0.1), (0.0, 0.0, 1.0), mask=am.MASK_HELD),
        am.CapsuleObstacle((1.9, 1.9, 0.0), (0.0, 0.0, 2.0), 0.05, velocity=(0.0, -0.3, 0.0), mask=am.MASK_HELD | am.MASK_SEGMENTS),
    ]


def set_breach():
    """The robot's set stays set C; for the tray a bar that passes 0.5 m under it, a sphere and an oblique wall, all
    clear: the tray's saturated clearances come from the field alone, whose thresholded map keeps them away from
    the barrier's bound."""
    return CS.set_c() + [
        am.SphereObstacle((1.7, 0.5, 0.8), 0.2, mask=am.MASK_HELD),
        am.CapsuleObstacle((0.55, 0.5, 0.1), (0.6, 0.0, 0.0), 0.03, velocity=(0.0, 1.0, 0.0), mask=HELD_SEGMENTS | am.mask_held_point(0)),
        am.HalfSpaceObstacle((1.9, 0.0, 0.0), (-0.8, 0.0, 0.6), mask=am.MASK_HELD),
    ]


def set_tip():
    return [am.SphereObstacle((1.6, 1.5, 0.3), 0.05, mask=am.MASK_HELD | 0x100)]


def sets():
    return [(set_clear(), CS.T_REF_C), (set_breach(), CS.T_REF_D), (set_tip(), 0.0)]
