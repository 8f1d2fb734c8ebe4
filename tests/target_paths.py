"""The timed pose paths of the target-tracking tests (mppi_set_target_path), as plain data shared by
the CPU tests of the host's sampler and the GPU parity tests.

The grasp frame of the huddled state sits at (0.870, 0.877, 0.891); the paths stay within 0.25 m of it.
Times are seconds on the updates' clock; the rollouts' time step is launch_shapes.TIME_STEP = 0.01.
A quaternion is (x, y, z, w) and need not be normalised (norm in [0.5, 2]).
"""
import numpy as np

import assistedmanipulation_amd as am

POINT = (0.9, 0.8, 0.95)   # the objective's fixed point in these tests

# Path A: four waypoints inside one 33-step horizon at t0 = 0 (steps at 0, 0.01 .. 0.32): steps 0 .. 4
# lie before the first waypoint, steps cross the interior waypoints at 0.105 and 0.175 (no step falls
# on a waypoint: every time is half a step off the grid), and steps 26 .. 32 lie past the last.
# Waypoint 2's raw quaternion has a negative dot product with waypoint 1's (the sign fix), and the norms differ from 1.
A_TIMES = (0.045, 0.105, 0.175, 0.255)
A_POSITIONS = ((0.90, 0.80, 0.90), (0.80, 0.90, 1.00), (0.70, 0.95, 0.85), (0.85, 0.70, 0.80))
A_QUATERNIONS = ((0.0, 0.0, 0.0, 1.0),
                 (0.30, -0.10, 0.20, 1.10),
                 (-0.45, 0.25, -0.40, -0.60),
                 (0.10, 0.60, 0.10, 0.40))

# Path B: two waypoints around the horizon's start, one of them before time 0
B_TIMES = (-0.10, 0.20)
B_POSITIONS = ((0.95, 0.85, 0.80), (0.75, 0.75, 1.05))
B_QUATERNIONS = ((0.5, 0.5, 0.5, 0.5), (0.0, 0.9, 0.0, 0.5))

# Path C, for advancing time: five waypoints over 0 .. 0.5 s, an update at 0.2 starts inside it
C_TIMES = (0.015, 0.085, 0.215, 0.335, 0.505)
C_POSITIONS = ((0.88, 0.86, 0.90), (0.80, 0.95, 0.95), (0.75, 0.80, 1.00), (0.90, 0.72, 0.85), (0.95, 0.90, 0.80))
C_QUATERNIONS = ((0.1, 0.0, 0.0, 1.0), (0.2, 0.1, -0.1, 0.9), (0.3, 0.3, -0.2, 0.7), (-0.2, -0.5, 0.3, -0.6), (0.0, 0.7, -0.1, 0.6))


def path_a(orientations=True):
    return am.TargetPath(A_TIMES, A_POSITIONS, A_QUATERNIONS if orientations else None)


def path_b(orientations=True):
    return am.TargetPath(B_TIMES, B_POSITIONS, B_QUATERNIONS if orientations else None)


def path_c(orientations=True):
    return am.TargetPath(C_TIMES, C_POSITIONS, C_QUATERNIONS if orientations else None)


def constant_path(point=POINT):
    """One waypoint: the target holds it at every time."""
    return am.TargetPath((0.1,), (point,))


def raw_dots(quaternions):
    """The dot products of consecutive quaternions as given, each normalised."""
    q = np.asarray(quaternions, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=1)[:, None]
    return np.sum(q[1:] * q[:-1], axis=1)
