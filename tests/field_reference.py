"""CPU reference of obstacle avoidance with a distance field (mppi_set_distance_field_avoidance), in
plain Python floats, on top of capsule_reference.py.

  * sample: include/mppi_amd.h's D(p), scalar by scalar - g_a = (p_a - origin_a) * inv_voxel, the
    inside test, i_a = min(floor(g_a), n_a - 2), f_a = g_a - i_a, the eight corners as doubles, and
    L(a, b, f) = a + f * (b - a) along z, then y, then x.  Every operation is one Python float
    operation, so it is rounded by itself.  Outside the grid: None; a NaN coordinate: NaN.
  * Term: capsule_reference.Term with a field behind it.  The step's term is the capsule term of the
    primitives plus the field's sum - over the masked points in index order, then the masked segments
    in index order, each at its samples j = 1..m, p = a + phi_j * (b - a) - through Left(limit).  The
    primitives keep their books; the field has its own (`fbooks`): least |v - bound|, least v, the
    branches taken, the numbers of inside and outside samples, and the least distance of any g_a to 0
    or n_a - 1 in grid units (over every sample, inside or not).
  * Composition, WrenchComposition: capsule_reference's with this Term and a current field.
"""
import math
from types import SimpleNamespace

import numpy as np

from assistedmanipulation_amd import abi

import capsule_reference as CR
import link_reference as LR
import obstacle_reference as OR
from oracle import oracle as O

POINTS, SEGMENTS = CR.POINTS, CR.SEGMENTS


def _lerp(a, b, f):
    return a + f * (b - a)


def sample(field, p):
    """(D, edge): D(p) of `field` (a DistanceField) at the point p (three floats) - None outside the
    grid, NaN for a NaN coordinate - and the least distance of a g_a to 0 or n_a - 1, in grid units."""
    n = field.dims
    inv = field.inv_voxel
    g = [(float(p[a]) - float(field.origin[a])) * inv for a in range(3)]
    if any(math.isnan(v) for v in g):
        return math.nan, math.nan
    edge = min(min(abs(g[a]), abs(g[a] - (n[a] - 1))) for a in range(3))
    if not all(0.0 <= g[a] <= n[a] - 1 for a in range(3)):
        return None, edge
    i = [min(int(math.floor(g[a])), n[a] - 2) for a in range(3)]
    f = [g[a] - i[a] for a in range(3)]
    v = field.values
    c = lambda dx, dy, dz: float(v[i[0] + dx, i[1] + dy, i[2] + dz])   # noqa: E731
    cz = [[_lerp(c(dx, dy, 0), c(dx, dy, 1), f[2]) for dy in range(2)] for dx in range(2)]
    cy = [_lerp(cz[dx][0], cz[dx][1], f[1]) for dx in range(2)]
    return _lerp(cy[0], cy[1], f[0]), edge


def _books():
    return SimpleNamespace(least_margin=math.inf, least_v=math.inf, branches=set(), inside=0, outside=0, edge=math.inf)


class Term(CR.Term):
    """The capsule term of one set plus the term of `field` (a DistanceField or None)."""

    def __init__(self, config, capsules, obstacles, t_ref, field=None):
        super().__init__(config, capsules, obstacles, t_ref)
        self.field = field
        self.fbooks = _books()

    def _field_v(self, p, radius):
        """Left(limit)(D(p) - radius), booked; 0 outside the grid."""
        b = self.fbooks
        D, edge = sample(self.field, p)
        if D is not None and math.isnan(D):
            return math.nan
        b.edge = min(b.edge, edge)
        if D is None:
            b.outside += 1
            return 0.0
        b.inside += 1
        v = D - radius
        b.least_margin = min(b.least_margin, abs(v - self.limit.bound))
        b.least_v = min(b.least_v, v)
        b.branches.add("saturated" if v <= self.limit.bound else "inverse")
        return LR.left_barrier(self.limit, v)

    def field_at(self, points):
        """The field's part at the nine points (9, 3)."""
        fd = self.field
        if fd is None:
            return 0.0
        total = 0.0
        for i in range(POINTS):
            if (fd.mask >> i) & 1:
                total += self._field_v([float(x) for x in points[i]], self.radii[i])
        m = fd.segment_samples
        for s in range(SEGMENTS):
            if not (fd.mask >> (16 + s)) & 1:
                continue
            a, b = [float(x) for x in points[s]], [float(x) for x in points[s + 1]]
            for j in range(1, m + 1):
                phi = j / (m + 1)
                total += self._field_v([a[k] + phi * (b[k] - a[k]) for k in range(3)], self.seg_radii[s])
        return total

    def at(self, points, tau):
        total = super().at(points, tau)
        if self.field is None:
            return total
        return total + self.field_at(points)

    def steps(self, model, qs, t0, dt):
        """(the step's terms, the field's parts of them): OR.Term.steps, also with an empty set."""
        H = len(qs)
        out = np.zeros(H)
        self.field_steps = np.zeros(H)
        if not self.obstacles and self.field is None:
            return out
        for k in range(H):
            tau = (t0 + k * dt) - self.t_ref
            p = OR.robot_points(model, qs[max(k - 1, 0)])
            cap = CR.Term.at(self, p, tau)
            if self.field is None:
                out[k] = cap
            else:
                self.field_steps[k] = self.field_at(p)
                out[k] = cap + self.field_steps[k]
        return out


class Composition(CR.Composition):
    def __init__(self, conf, model, cost, forecast=None, config=None, capsules=None):
        super().__init__(conf, model, cost, forecast, config, capsules)
        self.field = None
        self.term = Term(self.config, self.capsules, [], 0.0, None)
        self._set = ([], 0.0)

    def set_obstacles(self, obstacles, t_ref):
        self._set = (list(obstacles), t_ref)
        self.term = Term(self.config, self.capsules, obstacles, t_ref, self.field)
        self.history.append(self.term)
        return self.term

    def set_field(self, field):
        self.field = field
        return self.set_obstacles(*self._set)

    def positions(self, x0, u, t0=0.0):
        H = u.shape[0]
        qs = np.zeros((H, 12))
        qs[0] = x0[:12]
        if H > 1 and (self.term.obstacles or self.term.field is not None):
            dyn = O.OracleDynamics(x0, self.model)
            dyn.set_state(x0, t0)
            for k in range(H - 1):
                qs[k + 1] = dyn.step(u[k], self.dt)[:12]
        return qs


class WrenchComposition(CR.WrenchComposition):
    def __init__(self, conf, model, cost, mode, forecast=None, config=None, capsules=None):
        super().__init__(conf, model, cost, mode, forecast, config, capsules)
        self.field = None
        self.term = Term(self.config, self.capsules, [], 0.0, None)
        self._set = ([], 0.0)

    def set_obstacles(self, obstacles, t_ref):
        self._set = (list(obstacles), t_ref)
        self.term = Term(self.config, self.capsules, obstacles, t_ref, self.field)
        return self.term

    def set_field(self, field):
        self.field = field
        return self.set_obstacles(*self._set)
