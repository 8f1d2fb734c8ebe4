"""The device noise stream against an independent restatement (philox_reference.py: Philox4x32-10
from the published algorithm, pinned by the Random123 known-answer vectors in
test_philox_reference_cpu.py, and Box-Muller in fp64), element by element.

Every element of every update's noise() is compared with expected_noise(): rollout 0, rollout 1
(minus the device's own published U*), the kept rollouts' shifted columns and the components
without variance bit for bit; the fresh draws as eps / T_cc against the reference's z within Z_TOL;
all finite.  Each generating path runs at the smallest shape that selects it, and update_info()
must say that it ran:

  sample_kernel<12, diag>          MPPI_DRAW_AHEAD=0, and every one-wave shape (r10_h33)
  draw_ahead_block                 MPPI_TAIL_DRAWS=0; four-wave launches (r48_h33: no rows left over)
  the rollout launch's tail draws  r17_h33, r19_h33 (rows left over: the tail draws the main waves'
                                   rows, draw_ahead_block the rest)
  sample_kernel<12, full>          a non-diagonal covariance
  sample_kernel<3, diag>           the point mass with MPPI_PM_FUSED=0
  pm_fused.hip                     the point mass: this update's draws (sampling 1, the first update)
                                   and the next one's (sampling 2, consumed under update_count + 1)
  a shard                          the second of two handles draws with g = begin + lr

(The rollout launch has no sampling prologue any more: sampling == 1 is the fused point mass
alone, and draws made ahead go through eps_finish in draw_ahead_block.)  Each case runs with the
seed 0x5EED and with one whose high word is non-zero and whose halves differ; four more seeds put
a Box-Muller edge input into the first update (philox_reference.EDGE_SEEDS).

Not covered: counter word 1, the high half of draw = g H + k, which needs g H >= 2^32; no handle of
test size reaches it, and nothing here fakes it.

The tolerance.  The device's z differs from the reference's only by the rounding of four hardware
fp32 operations (log2, sqrt, sin / cos of revolutions, and the products).  Measured on an MI355X
over all the draws of the cases below (5.3e5 of them): max |eps / T_cc - z_ref| = 4.87e-7,
and 2.58e-7 relative to max(1, |z_ref|).  Z_TOL is eight times the first, an absolute
bound on z (near u1 -> 1 the radius is small and its relative error large), and must stay under
2^-16; a structural error (a wrong word, block, key half, update index, shift, sine for cosine)
moves nearly every draw by O(0.1 .. 1).
"""
import ctypes as C

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi

import philox_reference as P
from launch_shapes import TIME_STEP, by_name, horizon

pytestmark = pytest.mark.gpu

Z_MEASURED = 4.8661e-07   # max |eps / T_cc - z_ref| measured on the MI355X (the docstring)
Z_TOL = 8.0 * Z_MEASURED
assert Z_TOL <= 2.0 ** -16   # the cap

SEEDS = [0x5EED, 0x9E3779B97F4A7C15]
TIMES = [0.0, 0.05, 0.07, 0.07, 0.12]   # shifts of 0 (nothing to shift yet), 5, 2, 0 and 5 steps
ENV = ("MPPI_DRAW_AHEAD", "MPPI_TAIL_DRAWS", "MPPI_PM_FUSED", "MPPI_RELAY_K", "MPPI_HANDOVER", "MPPI_COSTS_IN_LAUNCH",
       "MPPI_SPLIT")
WORST = dict(abs=0.0, rel=0.0, draws=0, where="")


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nphilox stream: %d draws compared, max |eps / T_cc - z_ref| %.4e (%s), %.4e relative to max(1, |z_ref|); "
          "Z_TOL %.4e" % (WORST["draws"], WORST["abs"], WORST["where"], WORST["rel"], Z_TOL))


def _env(monkeypatch, **kw):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


class Shifts:
    """sample()'s shift count (mppi.cpp:194-201): by truncation, from the last time a shift happened."""

    def __init__(self, dt):
        self.dt, self.last = dt, 0.0

    def __call__(self, t):
        s = int((t - self.last) / self.dt)
        if s > 0:
            self.last = t
        return s


def _note(z_dev, z_ref, tag):
    """Record and assert the fresh draws' error, element by element."""
    d = np.abs(z_dev - z_ref)
    if d.size == 0:
        return
    i = int(np.argmax(d))
    rel = float(np.max(d / np.maximum(1.0, np.abs(z_ref))))
    print("%s: %d draws, max |z - z_ref| %.4e at z_ref %+.6f, relative %.4e" % (tag, d.size, d.flat[i], z_ref.flat[i], rel))
    WORST["draws"] += d.size
    WORST["rel"] = max(WORST["rel"], rel)
    if d.flat[i] > WORST["abs"]:
        WORST["abs"], WORST["where"] = float(d.flat[i]), "%s, z_ref %+.6f" % (tag, z_ref.flat[i])
    assert d.flat[i] <= Z_TOL, "%s: z differs from the reference by %.3e (bar %.3e) at z_ref %r, device %r" % (
        tag, d.flat[i], Z_TOL, z_ref.flat[i], z_dev.flat[i])


def _compare(noise, exp, z, fresh, td, tag, rows=None):
    """Every element of an update's noise [R, H, C] against the reference: diagonal transform td.
    rows: the (begin, end) of a shard, whose noise() is zero outside its own rollouts."""
    assert noise.shape == exp.shape
    assert np.all(np.isfinite(noise)), "%s: %d non-finite draws" % (tag, int((~np.isfinite(noise)).sum()))
    if rows is not None:
        b, e = rows
        assert np.all(noise[:b] == 0.0) and np.all(noise[e:] == 0.0), tag + ": rows of another shard"
        noise, exp, z, fresh = noise[b:e], exp[b:e], z[b:e], fresh[b:e]
    np.testing.assert_array_equal(noise[~fresh], exp[~fresh], err_msg=tag + ": rollouts 0, 1 and the kept columns")
    var = td > 0.0
    np.testing.assert_array_equal(noise[fresh][:, ~var], exp[fresh][:, ~var], err_msg=tag + ": components without variance")
    _note(noise[fresh][:, var] / td[var], z[fresh][:, var], tag)


def _run_updates(dev, x, seed, K, td, tag, check_info, times=TIMES, dx=0.0):
    """Updates of one handle, each compared in full; check_info(j, info) asserts the path."""
    shifts = Shifts(TIME_STEP)
    prev_costs, prev_noise = np.zeros(dev.R), np.zeros((dev.R, dev.H, dev.C))
    for j, t in enumerate(times):
        u_prev = dev.get_optimal_rollout().copy()
        index = dev.update_info()["update_count"]   # as it stands when the draws are consumed
        assert index == j
        dev.update(x, t)
        info = dev.update_info()
        assert info["wait_timeouts"] == 0, (tag, info)
        check_info(j, info)
        noise = dev.noise()
        exp, z, fresh = P.expected_noise(prev_costs, prev_noise, u_prev, K, shifts(t), seed, index, td)
        _compare(noise, exp, z, fresh, td, "%s seed %#x upd %d" % (tag, seed, j))
        prev_costs, prev_noise = dev.costs(), noise
        x = x + dx


def _fr_handle(S, H, K, seed, covariance=None):
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=K, threads=8)
    if covariance is not None:
        conf.covariance = covariance
    dev = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(), am.AssistedManipulation())
    assert dev is not None and dev.H == H and dev.R == S + 2 and dev.C == 12
    dev.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=seed)
    dev.set_forecast(am.constant_forecast(dev.H))
    return conf, dev


FR_TD = np.sqrt(am.config.FR_VARIANCE)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name,mode", [("r19_h33", "update"), ("r19_h33", "behind"), ("r48_h33", "behind"),
                                        ("r19_h33", "default"), ("r17_h33", "default"), ("r48_h33", "default"),
                                        ("r10_h33", "default")])
def test_frankaridgeback_diagonal(name, mode, seed, monkeypatch):
    """update: the sampling launch at update time (MPPI_DRAW_AHEAD=0).  behind: every row drawn
    behind the previous publish by draw_ahead_block (MPPI_TAIL_DRAWS=0).  default: r17 and r19 draw
    their main waves' rows in the rollout launch's tail (one and three rows left over, which
    draw_ahead_block draws with rollouts 0 and 1; the tail's draws are consumed from the third update
    on), r48 has no rows left over and runs the four-wave kernel, which draws nothing in its tail,
    and r10's one-wave workgroups sample at update time."""
    _, S, H, K, req, sw, first, pend = by_name(name)
    assert not req and not sw
    _env(monkeypatch, **{"update": dict(MPPI_DRAW_AHEAD="0"), "behind": dict(MPPI_DRAW_AHEAD="1", MPPI_TAIL_DRAWS="0"),
                         "default": {}}[mode])
    conf, dev = _fr_handle(S, H, K, seed)
    tails = mode == "default" and name in ("r17_h33", "r19_h33")
    ahead = mode != "update" and name != "r10_h33"

    def check(j, info):
        assert info["cooperative"] == 1 and info["fused_update"] == 0, info
        assert info["sampling"] == (2 if ahead and j > 0 else 0), (j, info)
        assert info["tail_draws"] == (1 if tails and j > 0 else 0), (j, info)

    _run_updates(dev, am.huddled_state(), seed, K, FR_TD, "%s %s" % (name, mode), check)


def _full_covariance():
    sd = np.sqrt(am.config.FR_VARIANCE)
    corr = np.eye(12)
    for a, b, r in ((0, 1, 0.5), (3, 4, -0.4), (5, 7, 0.3), (2, 9, 0.2)):   # test_non_diagonal_covariance_philox's
        corr[a, b] = corr[b, a] = r
    return corr * np.outer(sd, sd)


def recover_transform(E, Z):
    """T (n x n) and the device's own normals from fresh eps rows E = z_dev T^T (N x n) and the
    reference's normals Z (N x n), n the components with variance.

    A least-squares fit of E on Z gives T to about the device's z error over sqrt(N) (1e-9): good
    for the residual, too coarse to check T T^T to 1e-12.  But z_dev are fp32 values and E is their
    fp64 image under T, so T^-1 E lands within ~1e-8 relative of them, far inside half an fp32 ulp
    (6e-8 relative) for all but a few per cent of the elements; rounding to fp32 recovers those
    exactly, a refit on the rounded values is that much more accurate, and the iteration ends when
    nothing changes: T then fits E to fp64 rounding.  Returns (T of the plain fit, T refined,
    z_dev, worst refit residual)."""
    T0 = np.linalg.lstsq(Z, E, rcond=None)[0].T
    T, zs = T0, None
    for _ in range(12):
        zn = np.linalg.solve(T, E.T).T.astype(np.float32).astype(np.float64)
        if zs is not None and np.array_equal(zn, zs):
            break
        zs = zn
        T = np.linalg.lstsq(zs, E, rcond=None)[0].T
    return T0, T, zs, float(np.max(np.abs(E - zs @ T.T)))


@pytest.mark.parametrize("seed", SEEDS)
def test_frankaridgeback_full_transform(seed, monkeypatch):
    """eps = T z with the engine's T (Jacobi eigen-transform of a non-diagonal Sigma; not exposed):
    sample_kernel<12, full>, 62 x 8.  T is solved from the fresh rows' eps and the reference's z by
    least squares; the residual must meet Z_TOL (through sum_j |T_ij|, the most a z error of Z_TOL in
    every component can move eps_i), the device's own z recovered through T (recover_transform)
    must meet it element by element, and T T^T must be Sigma to 1e-12."""
    _env(monkeypatch)
    S, H, K = 62, 8, 20
    cov = _full_covariance()
    conf, dev = _fr_handle(S, H, K, seed, covariance=cov)
    x = am.huddled_state()
    shifts = Shifts(TIME_STEP)
    prev_costs, prev_noise = np.zeros(dev.R), np.zeros((dev.R, H, 12))
    zero_td = np.zeros(12)
    n = 10   # components with variance; the last two have none, and T is block diagonal with them
    for j, t in enumerate(TIMES):
        tag = "full transform seed %#x upd %d" % (seed, j)
        u_prev = dev.get_optimal_rollout().copy()
        index = dev.update_info()["update_count"]
        dev.update(x, t)
        info = dev.update_info()
        assert info["sampling"] == 0 and info["tail_draws"] == 0 and info["wait_timeouts"] == 0, info
        noise = dev.noise()
        assert np.all(np.isfinite(noise)), tag
        exp, z, fresh = P.expected_noise(prev_costs, prev_noise, u_prev, K, shifts(t), seed, index, zero_td)
        np.testing.assert_array_equal(noise[~fresh], exp[~fresh], err_msg=tag + ": rollouts 0, 1 and the kept columns")
        E, Z = noise[fresh], z[fresh]
        assert E.shape[0] >= (S - K) * H
        assert np.all(E[:, n:] == 0.0), tag + ": components without variance"
        T0, T, z_dev, refit = recover_transform(E[:, :n], Z[:, :n])
        resid = np.abs(E[:, :n] - Z[:, :n] @ T0.T) / np.sum(np.abs(T0), axis=1)
        print("%s: least-squares residual / sum_j |T_ij| %.4e; refit on the recovered fp32 z: %.3e" % (tag, resid.max(), refit))
        assert resid.max() <= Z_TOL, (tag, resid.max())
        assert refit <= 1e-13 * np.max(np.abs(E)), (tag, refit)
        _note(z_dev, Z[:, :n], tag)
        scale = np.sqrt(np.outer(np.diag(cov)[:n], np.diag(cov)[:n]))
        err = np.abs(T @ T.T - cov[:n, :n]) / scale
        print("%s: T T^T against Sigma %.3e (the plain fit: %.3e)" % (tag, err.max(), (np.abs(T0 @ T0.T - cov[:n, :n]) / scale).max()))
        assert err.max() <= 1e-12, (tag, err.max())
        prev_costs, prev_noise = dev.costs(), noise


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("fused", ["1", "0"])
def test_point_mass(fused, seed, monkeypatch):
    """C = 3: block 0 alone, three components of it.  Fused (pm_fused.hip): the first update draws
    for itself, every later one consumes what the launch before it drew under update_count + 1.
    MPPI_PM_FUSED=0: sample_kernel<3, diag> at update time."""
    _env(monkeypatch, MPPI_PM_FUSED=fused)
    S, K = 62, 20
    conf = am.point_mass_configuration(rollouts=S, horison=0.16, keep_best_rollouts=K)
    dev = am.Trajectory.create(conf, am.PointMassDynamics(), am.QuadraticCost())
    assert dev is not None and dev.H == 16 and dev.C == 3 and dev.R == S + 2
    dev.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=seed)

    def check(j, info):
        assert info["fused_update"] == int(fused), info
        if fused == "1":
            assert info["sampling"] == (1 if j == 0 else 2), (j, info)

    _run_updates(dev, np.zeros(6), seed, K, np.sqrt(np.diag(conf.covariance)), "point mass fused=%s" % fused, check, dx=0.01)


@pytest.mark.parametrize("seed", SEEDS)
def test_two_shards(seed, monkeypatch):
    """Two phase-split handles on one device, the all-reduces done on the host (as
    test_two_philox_shards_draw_ahead_equal_unsharded): 19 rows each (r19_h33's launch: one four-wave
    group and three rows left over), so the second shard's rollouts are g = 19 + lr, and both draw
    ahead, their main waves' rows in the launch's tail."""
    _env(monkeypatch)
    S, H, K = 36, 8, 5
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=K, threads=8)
    shards = [am.Trajectory.create(conf, am.FrankaRidgebackDynamics(), am.AssistedManipulation()) for _ in range(2)]
    for r, sh in enumerate(shards):
        sh.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=seed)
        sh.set_forecast(am.constant_forecast(sh.H))
        sh.set_shard(2, r)
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []
    R, HC = shards[0].R, H * 12
    assert [am.shard_range(R, 2, r) for r in range(2)] == [(0, 19), (19, 38)]

    def allreduce(ptrs, n):
        bufs = [np.zeros(n) for _ in ptrs]
        for p, b in zip(ptrs, bufs):
            assert hip.hipMemcpy(b.ctypes.data, p, n * 8, 2) == 0   # D2H
        s = bufs[0] + bufs[1]
        for p in ptrs:
            assert hip.hipMemcpy(p, s.ctypes.data, n * 8, 1) == 0   # H2D

    x = am.huddled_state()
    shifts = Shifts(TIME_STEP)
    prev_costs, prev_noise = np.zeros(R), [np.zeros((R, H, 12)) for _ in shards]
    for j, t in enumerate(TIMES):
        u_prev = [sh.get_optimal_rollout().copy() for sh in shards]
        index = [sh.update_info()["update_count"] for sh in shards]
        assert index == [j, j]
        for sh in shards:
            sh.update_phase1(x, t)
        hip.hipDeviceSynchronize()
        allreduce([sh.device_costs_ptr() for sh in shards], R + 1)   # + slot R: wait timeouts
        for sh in shards:
            sh.update_phase2()
        hip.hipDeviceSynchronize()
        allreduce([sh.device_gradient_ptr() for sh in shards], HC)
        for sh in shards:
            sh.update_phase3(t)
        shift = shifts(t)
        for r, sh in enumerate(shards):
            info = sh.update_info()
            assert info["wait_timeouts"] == 0 and info["sampling"] == (2 if j > 0 else 0), (j, r, info)
            assert info["tail_draws"] == (1 if j > 0 else 0), (j, r, info)
            noise = sh.noise()
            exp, z, fresh = P.expected_noise(prev_costs, prev_noise[r], u_prev[r], K, shift, seed, j, FR_TD)
            _compare(noise, exp, z, fresh, FR_TD, "shard %d seed %#x upd %d" % (r, seed, j), rows=am.shard_range(R, 2, r))
            prev_noise[r] = noise
        prev_costs = shards[0].costs()
        np.testing.assert_array_equal(prev_costs, shards[1].costs())


@pytest.mark.parametrize("kind", sorted(P.EDGE_SEEDS))
def test_box_muller_edges(kind, monkeypatch):
    """The first update under a seed that puts an edge input into a fresh draw (where, and that it
    is there: test_philox_reference_cpu.py): the whole tensor as everywhere else, and at the edge
    itself |z| = sqrt(48 ln 2) = 5.768 at u1 = 2^-24; z = +-0, not NaN, at u1 = 1 (log2 gives 0 and
    the radius is sqrt(-0)); the axes at u2 = 0 and u2 = 1/4."""
    _env(monkeypatch)
    S, H, K = P.EDGE_SHAPE
    seed, g, k, c = P.EDGE_SEEDS[kind]
    conf, dev = _fr_handle(S, H, K, seed)
    dev.update(am.huddled_state(), 0.0)
    assert dev.update_info()["sampling"] == 0
    noise = dev.noise()
    exp, z, fresh = P.expected_noise(np.zeros(dev.R), np.zeros((dev.R, H, 12)), np.zeros((H, 12)), K, 0, seed, 0, FR_TD)
    _compare(noise, exp, z, fresh, FR_TD, "edge " + kind)
    assert fresh[g, k] and FR_TD[c] > 0 and FR_TD[c + 1] > 0
    z0, z1 = noise[g, k, c] / FR_TD[c], noise[g, k, c + 1] / FR_TD[c + 1]
    w = P.words(seed, 0, g, k, H, 3)[c // 4]
    u1, u2 = P.uniforms(w[c % 4], w[c % 4 + 1])
    r = float(np.sqrt(-2.0 * np.log(u1) + 0.0))
    print("edge %s: u1 %r u2 %r: device z (%r, %r), reference (%r, %r)" % (kind, float(u1), float(u2), z0, z1, z[g, k, c], z[g, k, c + 1]))
    if kind == "a_min":
        assert abs(r - P.R_MAX) < 1e-14 and abs(np.hypot(z0, z1) - P.R_MAX) <= Z_TOL
    elif kind == "a_max":
        assert u1 == 1.0 and z0 == 0.0 and z1 == 0.0   # (+0 or -0; NaN compares unequal)
    elif kind == "b_zero":
        assert u2 == 0.0 and abs(z0 - r) <= Z_TOL and abs(z1) <= Z_TOL
    else:
        assert u2 == 0.25 and abs(z0) <= Z_TOL and abs(z1 - r) <= Z_TOL
