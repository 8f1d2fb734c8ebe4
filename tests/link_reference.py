"""CPU reference of the kinematic link-position model (mppi_set_link_positions), as a composition:
the oracle knows only the reference's stub (get_link_position = 0), so the live self-collision term
is composed here from three parts the oracle pins.

  * fk_links: forward kinematics in numpy from the mppi_frankaridgeback_desc body table alone (pose =
    parent o placement o joint, the joint R_z(q) or a slide along its axis).  Pinned by the oracle's
    grasp-frame and arm-mount positions (test_link_positions_cpu.py, 1e-12 m).
  * rollout_costs: per rollout, the oracle's per-step costs with the self-collision term switched
    off (O.rollout, or OracleDynamics.evaluate_cost step by step for TrackPoint), the joint positions
    q_k of an OracleDynamics stepped through the same controls, and the term added per step at
    q_{max(k-1, 0)} - the calculate() the step's end-effector position comes from - then discounted
    and summed in step order.  With term = the stub's constant it must reproduce an OracleTrajectory
    that has the constant switched on (the scaffold check) before it is used for the kinematic mode.
  * mppi_update: the softmin weights, gradient and clamped U* of mppi.cpp:344-448 (no smoothing).
"""
import copy

import numpy as np

from assistedmanipulation_amd import abi
from oracle import oracle as O

# self_collision_cost's pairs (assisted_manipulation.cpp:92-125, track_point.cpp:83-116), by Link
PAIRS = [(3, 6), (3, 7), (3, 8), (3, 9), (3, 10), (4, 6), (4, 7), (4, 8), (4, 9), (4, 10),
         (5, 7), (5, 8), (5, 9), (5, 10), (6, 8), (6, 9), (6, 10), (7, 9), (7, 10), (8, 10)]


def _rz(q):
    c, s = np.cos(q), np.sin(q)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def fk(model, q):
    """(link positions (13, 3), grasp-frame position, arm-mount position) at joint positions q (12):
    row 0 the universe, row 1 + i body i's frame origin in the world."""
    q = np.asarray(q, dtype=np.float64)
    R, p = [], []
    for i in range(model.nbodies):
        b = model.bodies[i]
        Rp = np.array(b.rotation[:]).reshape(3, 3)
        pp = np.array(b.translation[:])
        axis = np.array(b.axis[:])
        if b.type == abi.MPPI_JOINT_REVOLUTE:
            assert tuple(axis) == (0.0, 0.0, 1.0)
            Rj, pj = _rz(q[i]), np.zeros(3)
        else:
            Rj, pj = np.eye(3), axis * q[i]
        Rl, pl = Rp @ Rj, pp + Rp @ pj
        if b.parent < 0:
            R.append(Rl)
            p.append(pl)
        else:
            R.append(R[b.parent] @ Rl)
            p.append(p[b.parent] + R[b.parent] @ pl)
    links = np.vstack([np.zeros(3)] + p)

    def frame(f):
        return p[f.parent] + R[f.parent] @ np.array(f.translation[:])

    return links, frame(model.end_effector), frame(model.arm_mount)


def fk_links(model, q):
    """Link positions at q (12): (13, 3); or at a stack of configurations (N, 12): (N, 13, 3), the
    same chain on stacked matrices."""
    q = np.asarray(q, dtype=np.float64)
    if q.ndim == 1:
        return fk(model, q)[0]
    N = q.shape[0]
    R, p = [], []
    for i in range(model.nbodies):
        b = model.bodies[i]
        Rp = np.array(b.rotation[:]).reshape(3, 3)
        pp = np.array(b.translation[:])
        axis = np.array(b.axis[:])
        if b.type == abi.MPPI_JOINT_REVOLUTE:
            c, s = np.cos(q[:, i]), np.sin(q[:, i])
            Rj = np.zeros((N, 3, 3))
            Rj[:, 0, 0], Rj[:, 0, 1], Rj[:, 1, 0], Rj[:, 1, 1], Rj[:, 2, 2] = c, -s, s, c, 1.0
            Rl, pl = Rp @ Rj, np.broadcast_to(pp, (N, 3))
        else:
            Rl, pl = np.broadcast_to(Rp, (N, 3, 3)), pp + (Rp @ axis) * q[:, i:i + 1]
        if b.parent < 0:
            R.append(Rl)
            p.append(pl)
        else:
            R.append(R[b.parent] @ Rl)
            p.append(p[b.parent] + np.einsum("nij,nj->ni", R[b.parent], pl))
    return np.stack([np.zeros((N, 3))] + p, axis=1)


def left_barrier(b, v):
    """The reference's left barrier: over the bound the saturated branch, else min(scale / d, max)."""
    if v <= b.bound:
        d = b.bound - v
        return b.maximum_cost + b.scale * (d * d)
    return min(b.scale / (v - b.bound), b.maximum_cost)


def self_collision(limit, radii, links, track_point=False):
    """self_collision_cost on link positions (13, 3), pair order; (cost, least clearance): the
    clearance is the barrier argument's distance from its bound on the open side (AssistedManipulation:
    distance - radii - bound), negative once a pair is on the saturated branch."""
    cost, clear = 0.0, np.inf
    for a, b in PAIRS:
        d = links[a] - links[b]
        distance = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        rr = radii[a - 3] + radii[b - 3]
        v = rr - distance if track_point else distance - rr
        cost += left_barrier(limit, v)
        clear = min(clear, v - limit.bound)
    return cost, clear


def stub_constant(limit, radii, track_point=False):
    """The term with every link at the origin: the reference's PinocchioDynamics stub."""
    return self_collision(limit, radii, np.zeros((13, 3)), track_point)[0]


class Composition:
    """Rollout costs of one objective with the self-collision term composed per step.
    mode: "kinematic" (the term on fk_links at the lagged configuration), "zero" (the stub's
    constant) or "off"."""

    def __init__(self, conf, model, cost, mode, forecast=None):
        self.conf, self.model, self.mode, self.forecast = conf, model, mode, forecast
        self.dt, self.gamma = float(conf.time_step), float(conf.cost_discount_factor)
        self.track_point = cost.descriptor().kind == abi.MPPI_COST_TRACK_POINT
        c = cost.configuration
        self.enabled = bool(c.enable_self_collision_avoidance if self.track_point else c.enable_self_collision_limit)
        self.limit, self.radii = c.self_collision_limit, [float(r) for r in c.self_collision_radii]
        self.bare = copy.deepcopy(cost)   # the same objective without the term: the oracle's part
        if self.track_point:
            self.bare.configuration.enable_self_collision_avoidance = 0
        else:
            self.bare.configuration.enable_self_collision_limit = 0
        self.least_clearance = np.inf

    def _terms(self, qs):
        """The term at each configuration of qs (H, 12)."""
        H = len(qs)
        if not self.enabled or self.mode == "off":
            return np.zeros(H)
        if self.mode == "zero":
            return np.full(H, stub_constant(self.limit, self.radii, self.track_point))
        out = np.zeros(H)
        for k, links in enumerate(fk_links(self.model, np.asarray(qs))):
            out[k], clear = self_collision(self.limit, self.radii, links, self.track_point)
            self.least_clearance = min(self.least_clearance, clear)
        return out

    def rollout(self, x0, u, t0=0.0):
        """(J, per-step terms) of the controls u (H, C) from x0."""
        H = u.shape[0]
        qs, steps = [np.array(x0[:12])], np.zeros(H)
        x = np.array(x0, dtype=np.float64)
        bare_desc = self.bare.descriptor()
        if self.track_point or (self.mode == "kinematic" and self.enabled):   # the states x_k
            dyn = O.OracleDynamics(x0, self.model)
            dyn.set_state(x0, t0)
            for k in range(H):
                if self.track_point:   # get_cost against the object's cached kinematics, then the step
                    steps[k] = dyn.evaluate_cost(bare_desc, x)[0]
                if k + 1 < H:
                    x = dyn.step(u[k], self.dt)
                    qs.append(x[:12].copy())
        else:
            qs = qs * H
        if not self.track_point:
            _, steps, _ = O.rollout(self.model, self.bare.configuration, x0, u, self.dt, t0, self.forecast)
        terms = self._terms([qs[max(k - 1, 0)] for k in range(H)])
        J = 0.0
        for k in range(H):   # J += gamma^k c_k in step order (mppi.cpp:322-337); NaN stops the rollout
            sc = self.gamma ** k * (steps[k] + terms[k])
            if np.isnan(sc):
                return np.nan, terms
            J += sc
        return J, terms

    def costs(self, x0, U, eps, t0=0.0):
        """J of every rollout r with controls U + eps[r] (eps: (R, H, C))."""
        return np.array([self.rollout(x0, U + eps[r], t0)[0] for r in range(eps.shape[0])])


def mppi_update(conf, J, eps, U):
    """optimise() (mppi.cpp:344-448, no smoothing): (weights, gradient, U*) from the costs J (R), the
    noise eps (R, H, C) and U*_shifted U (H, C); None for the weights and gradient on the early return."""
    ok = ~np.isnan(J)
    assert ok.sum() > 1
    lo, hi = J[ok].min(), J[ok].max()
    if hi - lo < 1e-6:
        return None, None, U.copy()
    w = np.where(ok, np.exp(-conf.cost_scale * (np.where(ok, J, lo) - lo) / (hi - lo)), 0.0)
    w = w / w.sum()
    grad = np.tensordot(w, eps, axes=(0, 0))
    Un = U + grad * conf.gradient_step
    if conf.control_bound:
        Un = np.maximum(np.minimum(Un, conf.control_max), conf.control_min)
    return w, grad, Un
