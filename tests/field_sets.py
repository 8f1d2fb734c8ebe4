"""The distance fields of the field tests, as plain data shared by the CPU checks of the reference
(test_distance_field_cpu.py) and the GPU parity tests (test_gpu_distance_field.py).

The coordinates are capsule_sets.py's (the numpy forward kinematics at huddled_state()): the forearm,
segment 4, has its midpoint at (0.7106, 0.7176, 1.1857).  The three dimensions of every grid differ, so
that a transposed index shows.

  F "clear":   a ball of 0.3 m beside the robot and a floor 0.4 m under the origin, 63 x 61 x 47 samples
               of 0.05 m around the robot; points 1..8 and segments 1..7 (everything above the base
               column), three samples a segment.  Every clearance stays on the inverse branch.
  G "breach":  the same grid and mask, a thresholded map as a mapper's occupancy grid gives it: -10 at the
               samples inside matter and +10 outside.  Matter is a 0.08 m ball on the forearm's axis
               (test_the_hole's position, inside the link between two robot points) and a wall at
               x = 1.6.  Both branches.
  H "partial": 13 x 11 x 9 samples of 0.05 m around the forearm, thresholded likewise at 100, matter a 0.1 m
               ball on the forearm's far end (points 5 and 6); every point and segment.  The base column
               and the hand lie outside this grid.  Both branches, inside and outside samples.

G and H are thresholded because of the guards: the interpolant then crosses the barrier's bound within
one voxel (a slope of 400 or 4000 per metre instead of a true distance's 1), so a sample that lands within
1e-6 of the bound is that much less likely, while a sample deep inside matter or clear of it stays so
however the arm moves.  With true distances about one run in three at the larger shapes had such a sample;
H, whose matter sits where the arm's samples cross it most often, still had one in eight at a level of 1.
"""
import numpy as np

import assistedmanipulation_amd as am

from capsule_sets import ARM, capsules, objective   # noqa: F401  (the tests' objective and segment radii)

ABOVE_BASE = 0x1FE | ARM      # points 1..8, segments 1..7
EVERYTHING = am.MASK_ALL | am.MASK_SEGMENTS
ROOM = dict(origin=(-1.0, -1.0, -0.5), voxel=0.05, dims=(63, 61, 47))


def _ball(x, y, z, c, r):
    return np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r


def field_f():
    return am.DistanceField.from_function(lambda x, y, z: np.minimum(_ball(x, y, z, (1.5, 0.9, 1.0), 0.3), z + 0.4),
                                          mask=ABOVE_BASE, segment_samples=3, **ROOM)


def field_f_wrench():
    """F for the run with the simulated wrench, whose states have the arm moving and the robot pushed: the
    ball 0.1 m smaller and the floor 0.2 m lower, so that this run too stays 0.02 m clear."""
    return am.DistanceField.from_function(lambda x, y, z: np.minimum(_ball(x, y, z, (1.5, 0.9, 1.0), 0.2), z + 0.6),
                                          mask=ABOVE_BASE, segment_samples=3, **ROOM)


def _thresholded(sdf, level):
    return lambda x, y, z: np.where(sdf(x, y, z) < 0.0, -level, level)


def field_g():
    return am.DistanceField.from_function(_thresholded(lambda x, y, z: np.minimum(_ball(x, y, z, (0.7106, 0.7176, 1.1857), 0.08), 1.6 - x), 10.0),
                                          mask=ABOVE_BASE, segment_samples=3, **ROOM)


def field_h():
    return am.DistanceField.from_function(_thresholded(lambda x, y, z: _ball(x, y, z, (0.838, 0.845, 1.106), 0.1), 100.0), origin=(0.5, 0.5, 0.9),
                                          voxel=0.05, dims=(13, 11, 9), mask=EVERYTHING, segment_samples=3)


def fgh():
    return [field_f(), field_g(), field_h()]


def fgh_wrench():
    return [field_f_wrench(), field_g(), field_h()]


def plane(dims=(255, 257, 250)):
    """One large awkward grid near the 2^24 limit, filled from the plane 0.3 x - 0.2 y + 0.1 z + 0.5 over a
    room of 0.01 m voxels around the robot: the index arithmetic far from the origin."""
    return am.DistanceField.from_function(lambda x, y, z: 0.3 * x - 0.2 * y + 0.1 * z + 0.5, origin=(-0.8, -0.9, -0.6), voxel=0.01,
                                          dims=dims, mask=EVERYTHING, segment_samples=2)
