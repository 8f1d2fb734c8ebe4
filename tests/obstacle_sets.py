"""The obstacle sets of the obstacle-avoidance tests, as plain data shared by the CPU checks of the
reference (test_obstacles_cpu.py) and the GPU parity tests (test_gpu_obstacles.py).

The coordinates come from the numpy forward kinematics at huddled_state(): the base sphere sits at
(0.2, 0.2, 0), PANDA_LINK5 / 6 at (0.838, 0.845, 1.106), PANDA_LINK7 at (0.899, 0.906, 1.089) and
the grasp frame at (0.870, 0.877, 0.891).  Under the injected noise of test_gpu_link_positions.py
the end effector strays up to 0.65 m from there within a horizon and the wrist links up to 0.46 m,
so "clear" obstacles keep more than a metre away and "breach" ones sit on the arm.
"""
import numpy as np

import assistedmanipulation_amd as am

NO_BASE = 0x1FE          # every point but the base sphere
T_REF_A = -0.07          # set A's reference time: t0 - t_ref != 0 at t0 = 0
ARM_RADIUS = 0.04        # self-collision radii of the arm links in the tests' objective: every pair
                         # clear (link_reference: 0.008 m at the least), so the rollout costs are not
                         # buried under the saturated pair's 1e10 per step and the bars see the term


def set_a():
    """"Clear": a static sphere, a sphere moving towards the arm and a wall half-space (an oblique
    one, so every component of the normal counts) whose mask leaves out the base.  Every clearance
    is on the barrier's inverse branch, 0.02 m and more from the bound."""
    return [
        am.SphereObstacle((2.2, 0.9, 1.0), 0.3),
        am.SphereObstacle((0.9, 3.5, 1.0), 0.2, velocity=(0.0, -0.8, 0.1)),
        am.HalfSpaceObstacle((-1.0, 0.0, -0.5), (0.6, 0.0, 0.8), mask=NO_BASE),
    ]


def set_b():
    """"Breach": a sphere on the huddled grasp-frame position, which the end-effector sphere
    penetrates at x0 (rollouts that move away leave it), and a sphere that starts 0.3 m beside
    PANDA_LINK5 and flies through it at 1 m/s, entering its sphere at about step 15."""
    return [
        am.SphereObstacle((0.8703, 0.8774, 0.8908), 0.05, mask=0x180),
        am.SphereObstacle((1.1376, 0.8446, 1.1062), 0.05, velocity=(-1.0, 0.0, 0.0), mask=NO_BASE),
    ]


def set_16():
    """The full table: twelve spheres on a ring of 1.6 m around the arm's column, every third one
    moving, with masks that walk over the points, and four half-spaces (floor, ceiling, two walls)."""
    out = []
    for i in range(12):
        a = 2.0 * np.pi * i / 12.0
        centre = (0.6 + 1.6 * np.cos(a), 0.6 + 1.6 * np.sin(a), 0.4 + 0.1 * i)
        velocity = (-0.2 * np.cos(a), -0.2 * np.sin(a), 0.0) if i % 3 == 0 else (0.0, 0.0, 0.0)
        mask = 0x1FF if i % 4 == 0 else (0x1FF & ~(1 << (i % 9))) & ((0x0F << (i % 5)) | 0x100)
        out.append(am.SphereObstacle(centre, 0.05 + 0.01 * i, velocity=velocity, mask=mask))
    out.append(am.HalfSpaceObstacle((0.0, 0.0, -0.3), (0.0, 0.0, 1.0), mask=NO_BASE))             # floor
    out.append(am.HalfSpaceObstacle((0.0, 0.0, 2.6), (0.0, 0.0, -1.0), velocity=(0, 0, -0.1)))     # ceiling, sinking
    out.append(am.HalfSpaceObstacle((3.0, 0.0, 0.0), (-1.0, 0.0, 0.0), mask=0x1F0))
    out.append(am.HalfSpaceObstacle((0.0, -2.0, 0.0), (0.0, 1.0, 0.0), mask=0x00F))
    assert len(out) == 16
    return out


def objective(kind="am", energy=False, tp_self=False):
    """The tests' objective: AssistedManipulation (energy: with the tank) or TrackPoint, the arm's
    self-collision radii at ARM_RADIUS.

    TrackPoint keeps its default switches unless tp_self: its self-collision term passes radii -
    distance through the left barrier (track_point.cpp:118-144), so in the kinematic model every
    *clear* pair sits on the saturated branch, 20 pairs x 1e10 a step.  At r19_h33 that is J = 6.6e12
    against a cost range of 9e7: 1e-11 of the range is one ulp of J, and two numpy summation orders
    of the same rollout costs (the term added per step, or to the rollout's sum as the composition
    does) already move the softmin weights by 2.5e-11, past WEIGHT_ATOL.  tp_self therefore lowers
    that barrier's maximum_cost to 10, which keeps the term live on the same branch and the costs
    (about 7e3) resolvable at the bars."""
    if kind == "track_point":
        cost = am.TrackPoint()
        cost.configuration.enable_self_collision_avoidance = 1 if tp_self else 0
        if tp_self:
            cost.configuration.self_collision_limit.maximum_cost = 10.0
    else:
        cost = am.AssistedManipulation()
        if energy:
            cost.configuration.enable_energy_limit = 1
    for i in range(1, 8):
        cost.configuration.self_collision_radii[i] = ARM_RADIUS
    return cost
