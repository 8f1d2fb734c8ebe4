"""CPU reference of obstacle avoidance with capsules (mppi_set_obstacle_capsules), in numpy and plain
Python floats, on top of obstacle_reference.py (whose parts the oracle already pins).

  * segment_distance: include/mppi_amd.h's d(a, b; c, e), Ericson's closest-point form with exact-zero
    guards only, every operation rounded by itself, and the (s, t) class the test ended in.
  * Term: obstacle_reference.Term with the robot's eight segments (points s and s + 1, radii of an
    ObstacleCapsules, mask bits 16..23) and the capsule kind.  Per obstacle, the masked points in index
    order, then the masked segments in index order.  A sphere's and a half-space's point clearances are
    obstacle_reference.clearance's, so a point-only mask reproduces that class bit for bit.  It keeps
    the same books (least_margin, least_v, branches, evaluated) over points and segments alike, and
    per obstacle the set of classes its segment tests ended in (`classes`).
  * Composition, WrenchComposition: obstacle_reference's, with this Term.

The classes: for a proper pair (A != 0 and E != 0) "s0 t0", "s0 ti", ... "s1 t1" (0, interior, 1 for
each parameter); the degenerate entries are "A=0" (a zero-length robot segment against a proper one),
"E=0" (a proper robot segment against a point) and "A=0 E=0".
"""
import math

import numpy as np

from assistedmanipulation_amd import abi

import link_reference as LR
import obstacle_reference as OR

POINTS = OR.POINTS
SEGMENTS = abi.MPPI_OBSTACLE_SEGMENTS
PROPER = ["s%s t%s" % (s, t) for s in "0i1" for t in "0i1"]
DEGENERATE = ["A=0", "E=0", "A=0 E=0"]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _clamp(x):
    return min(max(x, 0.0), 1.0)


def _cls(x):
    return "0" if x == 0.0 else ("1" if x == 1.0 else "i")


def segment_distance(a, b, c, e):
    """(d, class) of the segments a -> b and c -> c + e (sequences of three floats)."""
    a, b, c, e = ([float(v) for v in x] for x in (a, b, c, e))
    d1 = [b[i] - a[i] for i in range(3)]
    r = [a[i] - c[i] for i in range(3)]
    A, E, F = _dot(d1, d1), _dot(e, e), _dot(e, r)
    if A == 0.0 and E == 0.0:
        s, t, cls = 0.0, 0.0, "A=0 E=0"
    elif A == 0.0:
        s, t, cls = 0.0, _clamp(F / E), "A=0"
    else:
        C = _dot(d1, r)
        if E == 0.0:
            t, s, cls = 0.0, _clamp(-C / A), "E=0"
        else:
            B = _dot(d1, e)
            den = A * E - B * B
            s = _clamp((B * F - C * E) / den) if den > 0.0 else 0.0
            t = (B * s + F) / E
            if t < 0.0:
                t, s = 0.0, _clamp(-C / A)
            elif t > 1.0:
                t, s = 1.0, _clamp((B - C) / A)
            cls = "s%s t%s" % (_cls(s), _cls(t))
    d = [(a[i] + s * d1[i]) - (c[i] + t * e[i]) for i in range(3)]
    return math.sqrt(_dot(d, d)), cls


def point_clearance(obstacle, radii, points, tau):
    """v of each of the nine points to one obstacle (the mask not applied): obstacle_reference's for
    a sphere and a half-space; for a capsule the point is the segment (p, p)."""
    if obstacle.kind != abi.MPPI_OBSTACLE_CAPSULE:
        return OR.clearance(obstacle, radii, points, tau)
    c = obstacle.position + obstacle.velocity * tau
    e = [float(v) for v in obstacle.normal]
    E = _dot(e, e)
    out = np.zeros(POINTS)
    for i in range(POINTS):
        p = [float(v) for v in points[i]]
        F = _dot(e, [p[k] - c[k] for k in range(3)])
        t = _clamp(F / E) if E != 0.0 else 0.0
        d = [p[k] - (c[k] + t * e[k]) for k in range(3)]
        out[i] = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - (radii[i] + obstacle.radius)
    return out


def segment_clearance(obstacle, seg_radii, points, tau, s):
    """(v, class or None) of robot segment s to one obstacle."""
    c = obstacle.position + obstacle.velocity * tau
    p, q = points[s], points[s + 1]
    if obstacle.kind == abi.MPPI_OBSTACLE_HALF_SPACE:
        n = obstacle.normal
        hp = (n[0] * (p[0] - c[0]) + n[1] * (p[1] - c[1])) + n[2] * (p[2] - c[2])
        hq = (n[0] * (q[0] - c[0]) + n[1] * (q[1] - c[1])) + n[2] * (q[2] - c[2])
        return min(hp, hq) - seg_radii[s], None
    e = obstacle.normal if obstacle.kind == abi.MPPI_OBSTACLE_CAPSULE else (0.0, 0.0, 0.0)
    d, cls = segment_distance(p, q, c, e)
    return d - (seg_radii[s] + obstacle.radius), cls


class Term(OR.Term):
    """The capsule term of one set under `config` (an ObstacleAvoidance) and `capsules` (an
    ObstacleCapsules)."""

    def __init__(self, config, capsules, obstacles, t_ref):
        super().__init__(config, obstacles, t_ref)
        self.capsules = capsules
        self.seg_radii = np.asarray(capsules.segment_radii, dtype=np.float64)
        self.classes = [set() for _ in self.obstacles]

    def _book(self, o, v):
        self.least_margin = min(self.least_margin, abs(v - self.limit.bound))
        self.least_v = min(self.least_v, v)
        self.branches[o].add("saturated" if v <= self.limit.bound else "inverse")
        self.evaluated += 1

    def at(self, points, tau):
        total = 0.0
        for o, ob in enumerate(self.obstacles):
            if ob.mask & abi.MPPI_OBSTACLE_MASK_ALL:
                v = point_clearance(ob, self.radii, points, tau)
                for i in range(POINTS):
                    if (ob.mask >> i) & 1:
                        total += LR.left_barrier(self.limit, v[i])
                        self._book(o, v[i])
            for s in range(SEGMENTS):
                if (ob.mask >> (16 + s)) & 1:
                    v, cls = segment_clearance(ob, self.seg_radii, points, tau, s)
                    total += LR.left_barrier(self.limit, v)
                    self._book(o, v)
                    if cls:
                        self.classes[o].add(cls)
        return total


class Composition(OR.Composition):
    def __init__(self, conf, model, cost, forecast=None, config=None, capsules=None):
        import assistedmanipulation_amd as am
        super().__init__(conf, model, cost, forecast, config)
        self.capsules = capsules or am.ObstacleCapsules()

    def set_obstacles(self, obstacles, t_ref):
        self.term = Term(self.config, self.capsules, obstacles, t_ref)
        self.history.append(self.term)
        return self.term


class WrenchComposition(OR.WrenchComposition):
    def __init__(self, conf, model, cost, mode, forecast=None, config=None, capsules=None):
        import assistedmanipulation_amd as am
        super().__init__(conf, model, cost, mode, forecast, config)
        self.capsules = capsules or am.ObstacleCapsules()

    def set_obstacles(self, obstacles, t_ref):
        self.term = Term(self.config, self.capsules, obstacles, t_ref)
        return self.term
