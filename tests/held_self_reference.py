"""CPU reference of the held object against the robot's own segments (mppi_set_held_self_avoidance), in
plain Python floats, on top of held_object_reference.py.

  * clearance: include/mppi_amd.h's v = d(a, b; c, e) - (radii[s] + r_u) with the robot's segment first
    (a = p_s, b = p_{s+1}, obstacle_reference.robot_points) and the held unit second: a held point has
    c = h_i and e = 0, a held segment c = h_s' and e = h_{s'+1} - h_s', one float subtraction a component
    (held_object_reference.world_points); d is capsule_reference.segment_distance(a, b, c, e).
  * Term: held_object_reference.Term with a configuration (a HeldSelf or None) behind it.  The step's self
    term runs over the masked held units that the object has in order u = 0..6, per unit over the masked
    robot segments in order s = 0..7; the step's term is ((capsule + field) + held) + self.  The self term
    has books of its own (`sbooks`): least |v - bound|, least v, the barrier branches taken, the
    segment_distance classes seen and the number evaluated.
  * Composition, WrenchComposition: held_object_reference's with this Term and a current configuration.
"""
import math
from types import SimpleNamespace

import numpy as np

import capsule_reference as CR
import held_object_reference as HR
import link_reference as LR
import obstacle_reference as OR
from oracle import oracle as O

HELD_POINTS, HELD_SEGMENTS, ROBOT_SEGMENTS = 4, 3, 8


def _books():
    return SimpleNamespace(least_margin=math.inf, least_v=math.inf, branches=set(), classes=set(), evaluated=0)


def units_of(held, held_self):
    """The tested units in order: those of `held_self.units` that `held` has."""
    if held is None or held_self is None:
        return []
    n = held.count
    out = [i for i in range(min(n, HELD_POINTS)) if (held_self.units >> i) & 1]
    return out + [HELD_POINTS + s for s in range(max(n - 1, 0)) if (held_self.units >> (HELD_POINTS + s)) & 1]


def segments_of(held_self):
    return [s for s in range(ROBOT_SEGMENTS) if held_self is not None and (held_self.segments >> s) & 1]


def unit(held, h, u):
    """(c, e, r_u) of held unit u at the world points h."""
    if u < HELD_POINTS:
        return h[u], [0.0, 0.0, 0.0], held.radii[u]
    s = u - HELD_POINTS
    return h[s], [h[s + 1][k] - h[s][k] for k in range(3)], held.segment_radii[s]


def clearance(points, s, radius, c, e, ru):
    """(v, class) of robot segment s (points: the nine robot points) with `radius` against the unit (c, e, ru)."""
    d, cls = CR.segment_distance(points[s], points[s + 1], c, e)
    return d - (radius + ru), cls


class Term(HR.Term):
    """held_object_reference.Term and the self term of `held_self` (a HeldSelf or None)."""

    def __init__(self, config, capsules, obstacles, t_ref, field=None, held=None, held_self=None):
        super().__init__(config, capsules, obstacles, t_ref, field, held)
        self.held_self = held_self
        self.sbooks = _books()
        self.units = units_of(self.held, held_self)
        self.segments = segments_of(held_self) if self.units else []

    def self_active(self):
        return bool(self.units and self.segments)

    def self_at(self, points, p_ee, Ree):
        """The self term at the nine robot points and the grasp pose of the same configuration."""
        if not self.self_active():
            return 0.0
        b = self.sbooks
        h = HR.world_points(self.held, p_ee, Ree)
        total = 0.0
        for u in self.units:
            c, e, ru = unit(self.held, h, u)
            for s in self.segments:
                v, cls = clearance(points, s, self.held_self.radii[s], c, e, ru)
                total += LR.left_barrier(self.limit, v)
                if math.isnan(v):
                    continue
                b.least_margin = min(b.least_margin, abs(v - self.limit.bound))
                b.least_v = min(b.least_v, v)
                b.branches.add("saturated" if v <= self.limit.bound else "inverse")
                b.classes.add(cls)
                b.evaluated += 1
        return total

    def steps(self, model, qs, t0, dt):
        """((capsule + field) + held) + self per step; the self parts in `self_steps`."""
        out = HR.Term.steps(self, model, qs, t0, dt)
        H = len(qs)
        self.self_steps = np.zeros(H)
        if not self.self_active():
            return out
        for k in range(H):
            q = qs[max(k - 1, 0)]
            p_ee, Ree = HR.grasp_pose(model, q)
            self.self_steps[k] = self.self_at(OR.robot_points(model, q), p_ee, Ree)
            out[k] = out[k] + self.self_steps[k]
        return out


class Composition(HR.Composition):
    def __init__(self, conf, model, cost, forecast=None, config=None, capsules=None):
        super().__init__(conf, model, cost, forecast, config, capsules)
        self.held_self = None
        self.term = Term(self.config, self.capsules, [], 0.0, None, None, None)

    def set_obstacles(self, obstacles, t_ref):
        self._set = (list(obstacles), t_ref)
        self.term = Term(self.config, self.capsules, obstacles, t_ref, self.field, self.held, self.held_self)
        self.history.append(self.term)
        return self.term

    def set_held_self(self, held_self):
        self.held_self = held_self
        return self.set_obstacles(*self._set)

    def positions(self, x0, u, t0=0.0):
        H = u.shape[0]
        if not (H > 1 and self.term.self_active()) or self.term.obstacles or self.term.field is not None:
            return super().positions(x0, u, t0)
        qs = np.zeros((H, 12))   # (the self term alone also needs the rollout's positions)
        qs[0] = x0[:12]
        dyn = O.OracleDynamics(x0, self.model)
        dyn.set_state(x0, t0)
        for k in range(H - 1):
            qs[k + 1] = dyn.step(u[k], self.dt)[:12]
        return qs


class WrenchComposition(HR.WrenchComposition):
    def __init__(self, conf, model, cost, mode, forecast=None, config=None, capsules=None):
        super().__init__(conf, model, cost, mode, forecast, config, capsules)
        self.held_self = None
        self.term = Term(self.config, self.capsules, [], 0.0, None, None, None)

    def set_obstacles(self, obstacles, t_ref):
        self._set = (list(obstacles), t_ref)
        self.term = Term(self.config, self.capsules, obstacles, t_ref, self.field, self.held, self.held_self)
        return self.term

    def set_held_self(self, held_self):
        self.held_self = held_self
        return self.set_obstacles(*self._set)
