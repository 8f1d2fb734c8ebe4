"""CPU reference of the simulated end-effector wrench (mppi_set_simulated_wrench,
mppi_dynamics_add_end_effector_simulated_wrench), as a composition: the oracle knows only the
reference's stub (the wrench never reaches the dynamics), so the pushed robot is composed here from
parts the oracle pins, as link_reference.py does for the links.

  * grasp_jacobian: the geometric Jacobian J_G(q) of the grasp frame at its own origin in world
    axes (Pinocchio's LOCAL_WORLD_ALIGNED) in numpy from the body table alone - the chain of
    link_reference.fk; column j is (a_j x (p_ee - p_j); a_j) for a revolute joint under the frame,
    (a_j; 0) for a prismatic one, zero for the fingers.  Pinned by the oracle's WORLD Jacobian and
    by central differences of the grasp position (test_simulated_wrench_cpu.py).
  * step: PinocchioDynamics::step with tau = (0, 0, 0, u_arm, 0, 0) + J_G(q)^T w: the base velocity
    overwrite, O.kinematics(model, q, v, tau)["a"] - calculate() with an arbitrary 12-vector torque -
    and the Euler integration; the tank E += (tau + nle) . v_new dt, clamped at 0.  With w = None it
    must equal OracleDynamics.step bit for bit (the scaffold) before it is used with a wrench.
  * Reference.rollout: the states of one rollout and its cost - per step OracleDynamics.evaluate_cost
    at x_k against the one-step-lagged kinematics cache: the oracle object is set to (q_{k-1}, the v
    that calculate() used, E_k), k = 0: x_0 itself.  One term cannot come from that object: the
    workspace (TrackPoint: reach) term reads the yaw of the dynamics' own state, which is x_k's while
    the cache is q_{k-1}'s, so it is restated here in numpy on the object's cached grasp-frame and
    arm-mount positions (workspace_term, reach_term); with w = 0 the whole must reproduce an
    OracleTrajectory update (the scaffold) before it is the reference of a wrench mode.
  * the update: link_reference.mppi_update.
"""
import copy
import math

import numpy as np

from assistedmanipulation_amd import abi
from oracle import oracle as O

import link_reference as LR

W0 = np.array([2.0, -1.0, 0.5, 0.1, -0.2, 0.05])   # the fixture wrench: force (N), moment (N m)


class Shift:
    """sample()'s shift count (mppi.cpp:194-201): truncation, the last shift time kept while 0."""

    def __init__(self):
        self.last = 0.0

    def __call__(self, t, dt):
        n = int((t - self.last) / dt)
        if n > 0:
            self.last = t
        return max(n, 0)


def shifted(U_prev, shift):
    H = U_prev.shape[0]
    return U_prev[np.minimum(np.arange(H) + shift, H - 1)]


def forecast_table(H, w=W0):
    """The FORECAST fixture: row k = w (1 + k / H)."""
    return np.array([w * (1.0 + k / H) for k in range(H)])


_TABLES = {}


def _table(model):
    """The body table as numpy constants (read through ctypes once per model)."""
    key = id(model)
    if key not in _TABLES:
        bodies = []
        for i in range(model.nbodies):
            b = model.bodies[i]
            axis = np.array(b.axis[:])
            revolute = b.type == abi.MPPI_JOINT_REVOLUTE
            if revolute:
                assert tuple(axis) == (0.0, 0.0, 1.0)
            bodies.append((np.array(b.rotation[:]).reshape(3, 3), np.array(b.translation[:]), axis, revolute, int(b.parent)))
        f = model.end_effector
        _TABLES[key] = (model, bodies, int(f.parent), np.array(f.translation[:]))   # (the model kept alive: its id stays its own)
    return _TABLES[key][1:]


def chain(model, q):
    """Body frames at q (12): rotations, origins, world joint axes, and the grasp-frame position."""
    bodies, ee_parent, ee_t = _table(model)
    R, p, a = [], [], []
    for i, (Rp, pp, axis, revolute, parent) in enumerate(bodies):
        if revolute:
            Rl, pl = Rp @ LR._rz(q[i]), pp
        else:
            Rl, pl = Rp, pp + Rp @ (axis * q[i])
        if parent < 0:
            R.append(Rl)
            p.append(pl)
        else:
            R.append(R[parent] @ Rl)
            p.append(p[parent] + R[parent] @ pl)
        a.append(R[i] @ axis)
    return R, p, a, p[ee_parent] + R[ee_parent] @ ee_t


def grasp_jacobian(model, q):
    """J_G(q), (6, 12): rows 0..2 the grasp origin's velocity, rows 3..5 the angular velocity."""
    R, p, a, pee = chain(model, q)
    bodies, j, _ = _table(model)
    J = np.zeros((6, len(bodies)))
    while j >= 0:   # the joints under the grasp frame
        if bodies[j][3]:
            d = pee - p[j]
            J[:3, j] = (a[j][1] * d[2] - a[j][2] * d[1], a[j][2] * d[0] - a[j][0] * d[2], a[j][0] * d[1] - a[j][1] * d[0])
            J[3:, j] = a[j]
        else:
            J[:3, j] = a[j]
        j = bodies[j][4]
    return J, pee


def wrench_torque(model, q, w):
    """tau_w = J_G(q)^T w (12)."""
    return grasp_jacobian(model, q)[0].T @ np.asarray(w, dtype=np.float64)


def step(model, x, u, w, dt):
    """One PinocchioDynamics::step from state x (31) under control u (12) and wrench w (6, or None: the
    reference's stub).  Returns (x_next, v_calc, a): the velocity calculate() ran at and its qdd."""
    x = np.asarray(x, dtype=np.float64)
    q, v = x[:12].copy(), x[12:24].copy()
    c, s = math.cos(q[2]), math.sin(q[2])
    v[0] = c * u[0] + (-s) * u[1]
    v[1] = s * u[0] + c * u[1]
    v[2] = u[2]
    tau = np.zeros(12)
    tau[3:10] = u[3:10]
    if w is not None:
        tau = tau + wrench_torque(model, q, w)
    k = O.kinematics(model, q, v, tau)
    a = k["a"].copy()
    vn = v + a * dt
    qn = q + vn * dt
    torque = tau + k["nle"]   # m_joint_torque after calculate()
    power = torque[0] * vn[0]
    for i in range(1, 12):
        power += torque[i] * vn[i]
    xn = x.copy()
    xn[:12], xn[12:24] = qn, vn
    xn[30] = max(0.0, x[30] + power * dt)   # EnergyTank::step
    return xn, v, a


def states(model, x0, u, dt, wrench=None):
    """x_0 .. x_{H-1} of the controls u (H, C) from x0 under the wrench rows (H, 6) (None: none), and the
    velocities calculate() ran at in steps 0 .. H-2: ((H, 31), (H - 1, 12))."""
    H = u.shape[0]
    out, vc = np.zeros((H, abi.MPPI_FR_STATE)), np.zeros((max(H - 1, 0), 12))
    out[0] = x0
    for k in range(H - 1):
        out[k + 1], vc[k], _ = step(model, out[k], u[k], None if wrench is None else wrench[k], dt)
    return out, vc


def wrench_torque_stack(model, Q, w):
    """tau_w at a stack of configurations Q (N, 12) under one wrench w (6): (N, 12).  The same chain
    and the same column formula on stacked matrices (checked against wrench_torque in
    test_simulated_wrench_cpu.py): what makes the reference of a whole launch affordable."""
    bodies, ee_parent, ee_t = _table(model)
    N = Q.shape[0]
    R, p, a = [], [], []
    for i, (Rp, pp, axis, revolute, parent) in enumerate(bodies):
        if revolute:
            c, s = np.cos(Q[:, i]), np.sin(Q[:, i])
            Rj = np.zeros((N, 3, 3))
            Rj[:, 0, 0], Rj[:, 0, 1], Rj[:, 1, 0], Rj[:, 1, 1], Rj[:, 2, 2] = c, -s, s, c, 1.0
            Rl, pl = Rp @ Rj, np.broadcast_to(pp, (N, 3))
        else:
            Rl, pl = np.broadcast_to(Rp, (N, 3, 3)), pp + (Rp @ axis) * Q[:, i:i + 1]
        if parent < 0:
            R.append(Rl)
            p.append(pl)
        else:
            R.append(R[parent] @ Rl)
            p.append(p[parent] + np.einsum("nij,nj->ni", R[parent], pl))
        a.append(R[i] @ axis)
    pee = p[ee_parent] + R[ee_parent] @ ee_t
    f, m = np.asarray(w[:3], dtype=np.float64), np.asarray(w[3:], dtype=np.float64)
    tau = np.zeros((N, len(bodies)))
    j = ee_parent
    while j >= 0:
        if bodies[j][3]:
            tau[:, j] = np.cross(a[j], pee - p[j]) @ f + a[j] @ m
        else:
            tau[:, j] = a[j] @ f
        j = bodies[j][4]
    return tau


def states_stack(model, x0, U, dt, wrench=None):
    """states() for a stack of control sequences U (N, H, C) from one x0: (N, H, 31).  The wrench's
    torque is formed for all N at once (wrench_torque_stack), calculate() per rollout."""
    N, H = U.shape[:2]
    out = np.zeros((N, H, abi.MPPI_FR_STATE))
    out[:, 0] = x0
    for k in range(H - 1):
        x = out[:, k]
        q, v = x[:, :12], x[:, 12:24].copy()
        c, s = np.cos(q[:, 2]), np.sin(q[:, 2])
        u = U[:, k]
        v[:, 0] = c * u[:, 0] + (-s) * u[:, 1]
        v[:, 1] = s * u[:, 0] + c * u[:, 1]
        v[:, 2] = u[:, 2]
        tau = np.zeros((N, 12))
        tau[:, 3:10] = u[:, 3:10]
        if wrench is not None:
            tau = tau + wrench_torque_stack(model, q, wrench[k])
        for n in range(N):
            kin = O.kinematics(model, q[n], v[n], tau[n])
            vn = v[n] + kin["a"] * dt
            torque = tau[n] + kin["nle"]
            power = torque[0] * vn[0]
            for i in range(1, 12):
                power += torque[i] * vn[i]
            out[n, k + 1] = x[n]
            out[n, k + 1, :12] = q[n] + vn * dt
            out[n, k + 1, 12:24] = vn
            out[n, k + 1, 30] = max(0.0, x[n, 30] + power * dt)
    return out


def _left(b, v):
    return LR.left_barrier(b, v)


def _right(b, v):
    if v >= b.bound:
        d = v - b.bound
        return b.maximum_cost + b.scale * (d * d)
    return min(b.scale / (b.bound - v), b.maximum_cost)


def _quad(qc, v):
    return (qc.constant_cost + qc.linear_cost * abs(v)) + qc.quadratic_cost * v * v


def workspace_term(cfg, ee, am_pos, ang):
    """AssistedManipulation::workspace_cost (assisted_manipulation.cpp:160-209) on the cached grasp-frame
    and arm-mount positions and the yaw `ang` of the dynamics' own state."""
    s, c = math.sin(ang), math.cos(ang)
    r22 = (1.0 - c) + c
    forward = np.array([c, s, 0.0])
    off = np.array([0.1 * c + (-s) * 0.0 + 0.0 * 0.15, 0.1 * s + c * 0.0 + 0.0 * 0.15, 0.0 * 0.1 + 0.0 * 0.0 + r22 * 0.15])
    robot = am_pos + off
    to_ee = ee - robot
    cost = 0.0
    projection = ((to_ee[0] * forward[0] + to_ee[1] * forward[1]) + to_ee[2] * forward[2]) / \
                 ((forward[0] * forward[0] + forward[1] * forward[1]) + forward[2] * forward[2])
    cost += _left(cfg.workspace_limit_infront, projection)
    reach = math.sqrt((to_ee[0] * to_ee[0] + to_ee[1] * to_ee[1]) + to_ee[2] * to_ee[2])
    cost += _right(cfg.workspace_limit_reach, reach)
    n1 = math.sqrt(to_ee[0] * to_ee[0] + to_ee[1] * to_ee[1])
    n2 = math.sqrt(forward[0] * forward[0] + forward[1] * forward[1])
    arg = (to_ee[0] * forward[0] + to_ee[1] * forward[1]) / n1 / n2
    yaw = math.acos(arg) if -1.0 <= arg <= 1.0 else math.nan
    if not math.isnan(yaw):
        cost += _quad(cfg.workspace_cost_yaw, abs(yaw))
    cost += _left(cfg.workspace_limit_above, ee[2] - robot[2])
    return cost


def reach_term(cfg, ee, am_pos, ang):
    """TrackPoint::reach_cost (track_point.cpp:162-186), likewise."""
    s, c = math.sin(ang), math.cos(ang)
    r22 = (1.0 - c) + c
    off = np.array([0.3 * c + (-s) * 0.0 + 0.0 * 0.15, 0.3 * s + c * 0.0 + 0.0 * 0.15, 0.0 * 0.3 + 0.0 * 0.0 + r22 * 0.15])
    d = ee - (am_pos + off)
    return _right(cfg.maximum_reach_limit, math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


class Reference:
    """Rollout states and costs of one objective with the wrench in the dynamics.
    mode: "off" (no wrench), "state" (x0[24:30] at every step) or "forecast" (row k of the table at
    step k; zeros without one).  links: also the kinematic link-position model's self-collision term
    (link_reference) at the lagged configuration."""

    def __init__(self, conf, model, cost, mode, forecast=None, links=False):
        self.conf, self.model, self.mode, self.forecast, self.links = conf, model, mode, forecast, links
        self.dt, self.gamma = float(conf.time_step), float(conf.cost_discount_factor)
        self.track_point = cost.descriptor().kind == abi.MPPI_COST_TRACK_POINT
        self.cfg = cost.configuration
        self.bare = copy.deepcopy(cost)   # the objective without the terms composed here
        b = self.bare.configuration
        if self.track_point:
            self.ws_on = bool(b.enable_reach_limits)
            b.enable_reach_limits = 0
            self.sc_on = bool(b.enable_self_collision_avoidance)
            if links:
                b.enable_self_collision_avoidance = 0
        else:
            self.ws_on = bool(b.enable_workspace_limit)
            b.enable_workspace_limit = 0
            self.sc_on = bool(b.enable_self_collision_limit)
            if links:
                b.enable_self_collision_limit = 0
        self.desc = self.bare.descriptor()
        self.limit, self.radii = self.cfg.self_collision_limit, [float(r) for r in self.cfg.self_collision_radii]
        self.dyn = None

    def wrench_rows(self, x0, H):
        if self.mode == "off":
            return None
        if self.mode == "state":
            return np.tile(np.asarray(x0[24:30], dtype=np.float64), (H, 1))
        return np.zeros((H, 6)) if self.forecast is None else np.asarray(self.forecast, dtype=np.float64)

    def step_cost(self, k, xs, vc):
        """get_cost at x_k against the calculate() of step k - 1 (k = 0: set_state's)."""
        lag = xs[max(k - 1, 0)].copy()
        if k > 0:
            lag[12:24] = vc[k - 1]
        lag[30] = xs[k][30]   # the tank's level is the state's
        self.dyn.set_state(lag, 0.0)
        wrench = None if self.forecast is None else self.forecast[k]
        total, t = self.dyn.evaluate_cost(self.desc, xs[k], wrench)
        if not (self.ws_on or (self.links and self.sc_on)):
            return total
        ee = self.dyn.end_effector()[abi.MPPI_EE_POSITION:abi.MPPI_EE_POSITION + 3]
        am_pos = self.dyn.query()[51:54]
        if self.track_point:   # point, joint limits, self-collision, reach (track_point.cpp:10-34)
            if self.links and self.sc_on:
                total += LR.self_collision(self.limit, self.radii, LR.fk_links(self.model, lag[:12]), True)[0]
            if self.ws_on:
                total += reach_term(self.cfg, ee, am_pos, xs[k][2])
            return total
        t = list(t)   # joint, self-collision, workspace, energy, velocity, trajectory, manipulability
        if self.links and self.sc_on:
            t[1] = LR.self_collision(self.limit, self.radii, LR.fk_links(self.model, lag[:12]), False)[0]
        if self.ws_on:
            t[2] = workspace_term(self.cfg, ee, am_pos, xs[k][2])
        total = 0.0
        for v in t:   # get_cost's running sum in term order; a disabled term is 0
            total += v
        return total

    def rollout(self, x0, u, t0=0.0):
        """(J, states (H, 31)) of the controls u (H, C) from x0."""
        H = u.shape[0]
        xs, vc = states(self.model, x0, u, self.dt, self.wrench_rows(x0, H))
        if self.dyn is None:
            self.dyn = O.OracleDynamics(x0, self.model)
        J = 0.0
        for k in range(H):   # J += gamma^k c_k in step order (mppi.cpp:322-337); NaN stops the rollout
            sc = self.gamma ** k * self.step_cost(k, xs, vc)
            if np.isnan(sc):
                return np.nan, xs
            J += sc
        return J, xs

    def costs(self, x0, U, eps, t0=0.0):
        """(J (R), states (R, H, 31)) of every rollout r with controls U + eps[r] (eps: (R, H, C))."""
        out = [self.rollout(x0, U + eps[r], t0) for r in range(eps.shape[0])]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out])
