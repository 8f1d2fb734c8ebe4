"""CPU reference of obstacle avoidance (mppi_set_obstacle_avoidance / mppi_set_obstacles), in numpy.

Nothing in the reference or the oracle computes an obstacle term, so it is composed here on top of
the compositions the oracle already pins:

  * Term: the step's term of include/mppi_amd.h on link positions from link_reference.fk_links and
    the grasp-frame position from link_reference.fk: obstacle o at position + velocity tau, the
    nine robot points (links PIVOT .. PANDA_LINK7, then the end effector) with the configuration's
    radii, the mask, the clearance of a sphere |p - c| - (r_i + r_o) or of a half-space
    n . (p - c) - r_i, and the reference's left barrier; obstacles in index order, points in index
    order.  It keeps books on everything it evaluates: the least |v - bound| (how far any point came
    to the barrier's branch discontinuity), the least v, and which branch each obstacle took.
  * Composition: link_reference.Composition(..., "kinematic")'s rollout cost plus gamma^k term_k at
    the lagged configurations (q_0 for k = 0, q_{k-1} after), tau_k = (t0 + k dt) - t_ref.
  * WrenchComposition: the same on wrench_reference.Reference(..., links=True), from the states
    that class returns.
"""
from types import SimpleNamespace

import numpy as np

from assistedmanipulation_amd import abi
from oracle import oracle as O

import link_reference as LR
import wrench_reference as WR

POINTS = abi.MPPI_OBSTACLE_POINTS
LINK0 = abi.MPPI_LINK_PIVOT


def robot_points(model, q):
    """The nine points at joint positions q (12): (9, 3)."""
    links, ee, _ = LR.fk(model, q)
    return np.vstack([links[LINK0:LINK0 + 8], ee])


def clearance(obstacle, radii, points, tau):
    """v of each of the nine points to one obstacle after tau seconds (the mask not applied): (9,)."""
    c = obstacle.position + obstacle.velocity * tau
    out = np.zeros(POINTS)
    for i in range(POINTS):
        d = points[i] - c
        if obstacle.kind == abi.MPPI_OBSTACLE_HALF_SPACE:
            n = obstacle.normal
            out[i] = ((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]) - radii[i]
        else:
            out[i] = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - (radii[i] + obstacle.radius)
    return out


class Term:
    """The obstacle term of one set (`obstacles`, reference time `t_ref`) under `config`
    (an ObstacleAvoidance), with the bookkeeping of everything evaluated so far."""

    def __init__(self, config, obstacles, t_ref):
        self.config, self.obstacles, self.t_ref = config, list(obstacles), float(t_ref)
        self.limit = SimpleNamespace(bound=config.limit[0], scale=config.limit[1], maximum_cost=config.limit[2])
        self.radii = np.asarray(config.radii, dtype=np.float64)
        self.least_margin = np.inf    # min |v - bound|
        self.least_v = np.inf         # min v
        self.branches = [set() for _ in self.obstacles]   # per obstacle: "inverse", "saturated"
        self.evaluated = 0

    def at(self, points, tau):
        """The term at the nine points (9, 3), tau seconds after t_ref."""
        total = 0.0
        for o, ob in enumerate(self.obstacles):
            v = clearance(ob, self.radii, points, tau)
            for i in range(POINTS):
                if not (ob.mask >> i) & 1:
                    continue
                total += LR.left_barrier(self.limit, v[i])
                self.least_margin = min(self.least_margin, abs(v[i] - self.limit.bound))
                self.least_v = min(self.least_v, v[i])
                self.branches[o].add("saturated" if v[i] <= self.limit.bound else "inverse")
                self.evaluated += 1
        return total

    def steps(self, model, qs, t0, dt):
        """The term of steps 0 .. H-1 of an update at t0 from the rollout's positions qs (H, 12): step k
        at the lagged configuration and tau_k = (t0 + k dt) - t_ref."""
        H = len(qs)
        out = np.zeros(H)
        if not self.obstacles:
            return out
        for k in range(H):
            tau = (t0 + k * dt) - self.t_ref
            out[k] = self.at(robot_points(model, qs[max(k - 1, 0)]), tau)
        return out


def _add_discounted(J, gamma, terms):
    for k, t in enumerate(terms):   # a NaN term makes the rollout NaN like any step cost
        J += gamma ** k * t
    return J


class Composition:
    """Rollout costs with the obstacle term on top of link_reference.Composition in kinematic mode."""

    def __init__(self, conf, model, cost, forecast=None, config=None):
        import assistedmanipulation_amd as am
        self.base = LR.Composition(conf, model, cost, "kinematic", forecast)
        self.conf, self.model = conf, model
        self.dt, self.gamma = self.base.dt, self.base.gamma
        self.config = config or am.ObstacleAvoidance()
        self.term = Term(self.config, [], 0.0)
        self.history = []   # every Term used, in order

    def set_obstacles(self, obstacles, t_ref):
        self.term = Term(self.config, obstacles, t_ref)
        self.history.append(self.term)
        return self.term

    def positions(self, x0, u, t0=0.0):
        """q_0 .. q_{H-1} of the controls u (H, C) from x0: an OracleDynamics stepped through them."""
        H = u.shape[0]
        qs = np.zeros((H, 12))
        qs[0] = x0[:12]
        if H > 1 and self.term.obstacles:
            dyn = O.OracleDynamics(x0, self.model)
            dyn.set_state(x0, t0)
            for k in range(H - 1):
                qs[k + 1] = dyn.step(u[k], self.dt)[:12]
        return qs

    def rollout(self, x0, u, t0=0.0):
        """(J, the self-collision terms, the obstacle terms) of the controls u (H, C) from x0."""
        J, sc = self.base.rollout(x0, u, t0)
        ob = self.term.steps(self.model, self.positions(x0, u, t0), t0, self.dt)
        return _add_discounted(J, self.gamma, ob), sc, ob

    def costs(self, x0, U, eps, t0=0.0):
        return np.array([self.rollout(x0, U + eps[r], t0)[0] for r in range(eps.shape[0])])


class WrenchComposition:
    """The same on wrench_reference.Reference(..., links=True): the pushed robot's states."""

    def __init__(self, conf, model, cost, mode, forecast=None, config=None):
        import assistedmanipulation_amd as am
        self.base = WR.Reference(conf, model, cost, mode, forecast, links=True)
        self.model, self.dt, self.gamma = model, self.base.dt, self.base.gamma
        self.config = config or am.ObstacleAvoidance()
        self.term = Term(self.config, [], 0.0)

    def set_obstacles(self, obstacles, t_ref):
        self.term = Term(self.config, obstacles, t_ref)
        return self.term

    def rollout(self, x0, u, t0=0.0):
        """(J, states (H, 31), the obstacle terms)."""
        J, xs = self.base.rollout(x0, u, t0)
        ob = self.term.steps(self.model, xs[:, :12], t0, self.dt)
        return _add_discounted(J, self.gamma, ob), xs, ob

    def costs(self, x0, U, eps, t0=0.0):
        return np.array([self.rollout(x0, U + eps[r], t0)[0] for r in range(eps.shape[0])])
