"""CPU reference of the trajectory safety filter (mppi_set_safety_filter, DESIGN section 1 "Safety
filter"), a numpy restatement on parts the oracle pins: M(q)^-1 column i is
O.kinematics(model, q, v, e_i)["a"] (calculate() with a unit torque; its NLE cancels), M is its
inverse, the wrench's joint torque is wrench_reference.wrench_torque and the step is
wrench_reference.step.

For step k of the plan, from x_k = (q, v, ...), u = U*[k] and dt:
  1. w = R_z(q[2]) u[0:3]: the base command in world axes;
  2. tau = (0, 0, 0, u[3:10], 0, 0) (+ J_G^T w_k in a simulated-wrench mode);
  3. a = M^-1 tau, v_c = (w, v[3:12]), v+ = v_c + a dt;
  4. clampseq(x; j): position, velocity, acceleration clamps in that order, a later one wins;
  5. arm: da_j = (clampseq(v+_j) - v+_j) / dt; if any, M_BB da_B = -M_BA da_A over B = {0, 1, 2, 10, 11},
     du_A = M_AA da_A + M_AB da_B, a' = a + da;
  6. base: v+'_j = w_j + a'_j dt, dw_j = clampseq(v+'_j) - v+'_j, u'[0:3] = u[0:3] + R_z(q[2])^T dw;
  7. x_{k+1} = step(x_k, u').
"""
import math

import numpy as np

from oracle import oracle as O

import wrench_reference as WR

ARM = np.arange(3, 10)
REST = np.array([0, 1, 2, 10, 11])
KINDS = ("joints", "velocity", "acceleration")


def mass_inverse(model, q, v=None):
    v = np.zeros(12) if v is None else v
    return np.stack([O.kinematics(model, q, v, np.eye(12)[i])["a"] for i in range(12)], axis=1)


def mass_matrix(model, q):
    M = np.linalg.inv(mass_inverse(model, q))
    return 0.5 * (M + M.T)


def clampseq(f, x, j, q, v, dt):
    """(the clamped value, which of the three clamps moved it)."""
    moved = [False, False, False]
    if f.limit_joints:
        y = min(max(x, (f.position_minimum[j] - q[j]) / dt), (f.position_maximum[j] - q[j]) / dt)
        moved[0], x = y != x, y
    if f.limit_velocity:
        y = min(max(x, f.velocity_minimum[j]), f.velocity_maximum[j])
        moved[1], x = y != x, y
    if f.limit_acceleration:
        y = min(max(x, v[j] + f.acceleration_minimum[j] * dt), v[j] + f.acceleration_maximum[j] * dt)
        moved[2], x = y != x, y
    return x, moved


def schur_correction(M, da_arm):
    """(du_A, da_B): the arm torque change that changes the arm accelerations by da_A with the other
    joints' torque untouched, and the other joints' change of acceleration."""
    da_rest = np.linalg.solve(M[np.ix_(REST, REST)], -M[np.ix_(REST, ARM)] @ da_arm)
    return M[np.ix_(ARM, ARM)] @ da_arm + M[np.ix_(ARM, REST)] @ da_rest, da_rest


def filter_column(model, f, x, u, w, dt):
    """The filtered control of one column at state x (31) and what bound: (u', bound) with bound[kind]
    = (an arm joint's clamp of that kind moved the value, a base joint's did)."""
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    q, v = x[:12], x[12:24]
    c, s = math.cos(q[2]), math.sin(q[2])
    wv = np.array([c * u[0] + (-s) * u[1], s * u[0] + c * u[1], u[2]])
    tau = np.zeros(12)
    tau[3:10] = u[3:10]
    if w is not None:
        tau = tau + WR.wrench_torque(model, q, w)
    Minv = mass_inverse(model, q)
    a = Minv @ tau
    vc = v.copy()
    vc[:3] = wv
    vplus = vc + a * dt
    bound = {k: [False, False] for k in KINDS}
    out = u.copy()
    da = np.zeros(7)
    for n, j in enumerate(ARM):
        t, moved = clampseq(f, vplus[j], j, q, v, dt)
        if t != vplus[j]:
            da[n] = (t - vplus[j]) / dt
        for kind, m in zip(KINDS, moved):
            bound[kind][0] |= m
    if da.any():
        M = np.linalg.inv(Minv)
        M = 0.5 * (M + M.T)
        du, db = schur_correction(M, da)
        out[3:10] = u[3:10] + du
        a = a.copy()
        a[ARM] += da
        a[REST] += db
    dw = np.zeros(3)
    for j in range(3):
        vp = wv[j] + a[j] * dt
        t, moved = clampseq(f, vp, j, q, v, dt)
        dw[j] = t - vp
        for kind, m in zip(KINDS, moved):
            bound[kind][1] |= m
    if dw.any():
        out[0] = u[0] + (c * dw[0] + s * dw[1])
        out[1] = u[1] + ((-s) * dw[0] + c * dw[1])
        out[2] = u[2] + dw[2]
    return out, bound


def filter_plan(model, f, x0, U, dt, wrench=None):
    """The filtered plan of U (H, C) from x0 under the wrench rows (H, 6) or None: (U', the states
    x_0 .. x_H (H + 1, 31), counts) with counts[kind] = [steps an arm joint bound, steps a base joint did]."""
    H = U.shape[0]
    out, xs = np.array(U, dtype=np.float64), np.zeros((H + 1, 31))
    xs[0] = x0
    counts = {k: [0, 0] for k in KINDS}
    for k in range(H):
        wk = None if wrench is None else wrench[k]
        out[k], bound = filter_column(model, f, xs[k], U[k], wk, dt)
        for kind in KINDS:
            counts[kind][0] += bound[kind][0]
            counts[kind][1] += bound[kind][1]
        xs[k + 1] = WR.step(model, xs[k], out[k], wk, dt)[0]
    return out, xs, counts


def last_limits(f, j, q, v, dt):
    """The interval the last-applied enabled limit leaves joint j's next velocity, or None."""
    if f.limit_acceleration:
        return v[j] + f.acceleration_minimum[j] * dt, v[j] + f.acceleration_maximum[j] * dt
    if f.limit_velocity:
        return f.velocity_minimum[j], f.velocity_maximum[j]
    if f.limit_joints:
        return (f.position_minimum[j] - q[j]) / dt, (f.position_maximum[j] - q[j]) / dt
    return None


def limit_excess(f, x, xn, dt):
    """How far the step x -> xn leaves the last-applied enabled limit at joints 0..9, relative to
    max(1, |bound|): 0 when every joint is inside."""
    worst = 0.0
    for j in range(10):
        iv = last_limits(f, j, x[:12], x[12:24], dt)
        if iv is None:
            continue
        vn = xn[12 + j]
        for b, over in ((iv[0], iv[0] - vn), (iv[1], vn - iv[1])):
            if np.isfinite(b):
                worst = max(worst, over / max(1.0, abs(b)))
    return worst
