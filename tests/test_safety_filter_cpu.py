"""The trajectory safety filter without a GPU: the numpy reference (safety_reference.py) against its
own definition over the robot's state space, the descriptor's layout and defaults, and the C++
filter class.

The limit bar: after filter and step, the next velocity of every joint 0..9 is inside the interval
of the last-applied enabled limit to 1e-12, relative to max(1, |bound|) (safety_reference.limit_excess).
"""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import _lib, abi

import safety_reference as SR
import state_space as SS
import wrench_reference as WR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
DT = 0.01
LIMIT_RTOL = 1e-12
CONTROLS = [np.array([0.5 * a, 0.5 * b, 1.0 * c] + [80.0 * d] * 7 + [0.0, 0.0]) for a, b, c, d in
            itertools.product((1.0, -1.0), repeat=4)]
SWITCHES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1)]


@pytest.fixture(scope="module")
def model():
    return am.FrankaRidgebackDynamics().model


def tight(x, joints, velocity, acceleration):
    """Limits that bind under CONTROLS at state x: 1 mm / 1 mrad of position either side of q, 0.05 of
    velocity, 0.5 of acceleration (0.005 per step)."""
    q = np.asarray(x[:12])
    return am.TrajectorySafetyFilter(position_minimum=q - 1e-3, position_maximum=q + 1e-3, velocity_minimum=np.full(12, -0.05),
                                     velocity_maximum=np.full(12, 0.05), acceleration_minimum=np.full(12, -0.5),
                                     acceleration_maximum=np.full(12, 0.5), limit_joints=joints, limit_velocity=velocity,
                                     limit_acceleration=acceleration)


def wide(**switches):
    return am.TrajectorySafetyFilter(position_minimum=np.full(12, -1e30), position_maximum=np.full(12, 1e30),
                                     velocity_minimum=np.full(12, -1e30), velocity_maximum=np.full(12, 1e30),
                                     acceleration_minimum=np.full(12, -1e30), acceleration_maximum=np.full(12, 1e30), **switches)


def test_unbound_column_is_returned_bit_for_bit(model):
    f = wide(limit_joints=True, limit_velocity=True, limit_acceleration=True)
    for entry in SS.using("d"):
        x = SS.state(entry)
        for u in CONTROLS[::5]:
            for w in (None, WR.W0):
                out, bound = SR.filter_column(model, f, x, u, w, DT)
                assert np.array_equal(out, u), entry[0]
                assert not any(any(b) for b in bound.values())
    # the defaults' velocity limits do not bind a resting robot under a small control
    g = am.TrajectorySafetyFilter(limit_joints=True, limit_velocity=True)
    x = am.huddled_state()
    u = np.array([0.1, -0.1, 0.2, 1.0, -2.0, 0.5, 1.0, 0.1, -0.1, 0.05, 0.0, 0.0])
    assert np.array_equal(SR.filter_column(model, g, x, u, None, DT)[0], u)


def _worst_excess(model, f, x, u, w):
    out, _ = SR.filter_column(model, f, x, u, w, DT)
    xn = WR.step(model, x, out, w, DT)[0]
    assert np.array_equal(out[10:], u[10:])   # the fingers pass through
    return SR.limit_excess(f, x, xn, DT), not np.array_equal(out, u)


@pytest.mark.parametrize("switches", SWITCHES, ids=lambda s: "jva_%d%d%d" % s)
def test_limits_hold_after_filter_and_step(model, switches):
    worst, changed, n = 0.0, 0, 0
    for i, entry in enumerate(SS.ENTRIES):
        x = SS.state(entry)
        f = tight(x, *switches)
        for u in CONTROLS[i % 4::4]:   # four of the sixteen sign patterns per entry, all sixteen over four entries
            e, ch = _worst_excess(model, f, x, u, WR.W0 if i % 3 == 0 else None)
            worst, changed, n = max(worst, e), changed + ch, n + 1
            assert e <= LIMIT_RTOL, (entry[0], u[:4].tolist(), e)
    print("switches %s: worst excess %.3e over %d columns, %d changed" % (switches, worst, n, changed))
    assert changed == n   # tight: every column is corrected


def test_schur_correction_is_the_brute_force_solve(model):
    rng = np.random.default_rng(11)
    for entry in SS.using("d"):
        q = np.asarray(SS.state(entry)[:12])
        Minv = SR.mass_inverse(model, q)
        M = SR.mass_matrix(model, q)
        np.testing.assert_allclose(M @ Minv, np.eye(12), atol=1e-9)
        da = rng.normal(0.0, 50.0, 7)
        du, db = SR.schur_correction(M, da)
        # brute force: the arm torque change whose accelerations' arm part is da, nothing else touched
        brute = np.linalg.solve(Minv[np.ix_(SR.ARM, SR.ARM)], da)
        np.testing.assert_allclose(du, brute, rtol=1e-8, atol=1e-9 * np.abs(brute).max())
        dtau = np.zeros(12)
        dtau[SR.ARM] = du
        acc = Minv @ dtau
        np.testing.assert_allclose(acc[SR.ARM], da, rtol=1e-8, atol=1e-9 * np.abs(da).max())
        np.testing.assert_allclose(acc[SR.REST], db, rtol=1e-8, atol=1e-9 * np.abs(da).max())


def test_filter_plan_chains_columns_and_counts(model):
    rng = np.random.default_rng(5)
    x0 = SS.state(SS.by_name("quat_w"))
    U = np.zeros((6, 12))
    U[:, :3], U[:, 3:10] = rng.normal(0, 0.4, (6, 3)), rng.normal(0, 30.0, (6, 7))
    f = tight(x0, 0, 1, 1)
    out, xs, counts = SR.filter_plan(model, f, x0, U, DT)
    x = x0
    for k in range(6):
        np.testing.assert_array_equal(out[k], SR.filter_column(model, f, x, U[k], None, DT)[0])
        assert SR.limit_excess(f, xs[k], xs[k + 1], DT) <= 1e-9
        x = WR.step(model, x, out[k], None, DT)[0]
        np.testing.assert_array_equal(x, xs[k + 1])
    assert counts["joints"] == [0, 0] and counts["acceleration"][0] > 0 and counts["acceleration"][1] > 0


def test_struct_layout_and_defaults_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    fields = [n for n, _ in abi.mppi_safety_filter_desc._fields_]
    body = 'printf("size %zu\\n", sizeof(mppi_safety_filter_desc));'
    body += "".join('printf("%s %%zu\\n", offsetof(mppi_safety_filter_desc, %s));' % (n, n) for n in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mppi_amd.h"\nint main(void){%s return 0;}\n' % body)
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().split("\n") if line)
    assert int(got["size"]) == C.sizeof(abi.mppi_safety_filter_desc) == 608
    for n in fields:
        assert int(got[n]) == getattr(abi.mppi_safety_filter_desc, n).offset, n
    d = abi.mppi_safety_filter_desc()
    _lib.load().mppi_default_safety_filter(C.byref(d))
    # robot.urdf's <limit lower upper velocity>: x, y, pivot, panda_joint1..7, the fingers
    assert list(d.position_minimum) == [-10, -10, -10, -2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973, -0.001, -0.001]
    assert list(d.position_maximum) == [10, 10, 10, 2.8973, 1.7628, 2.8973, 0.0698, 2.8973, 3.7525, 2.8973, 0.04, 0.04]
    assert list(d.velocity_maximum) == [1, 1, 1, 2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61, 0.3, 0.3]
    assert list(d.velocity_minimum) == [-v for v in d.velocity_maximum]
    assert all(v == -np.inf for v in d.acceleration_minimum) and all(v == np.inf for v in d.acceleration_maximum)
    assert (d.reach_maximum, d.reach_minimum) == (0.8, 0.15)
    assert (d.limit_joints, d.limit_velocity, d.limit_acceleration, d.limit_reach) == (0, 0, 0, 0)
    f = am.TrajectorySafetyFilter()
    assert f == am.TrajectorySafetyFilter.from_c(d) and f == am.TrajectorySafetyFilter.from_c(f.to_c())
    g = am.TrajectorySafetyFilter(limit_velocity=True, velocity_maximum=np.full(12, 0.5))
    assert g != f and g.to_c().limit_velocity == 1 and g.to_c().velocity_maximum[7] == 0.5
    with pytest.raises(TypeError):
        am.TrajectorySafetyFilter(limit_speed=True)
    with pytest.raises(ValueError):
        am.TrajectorySafetyFilter(velocity_maximum=[1.0, 2.0])


def test_cpp_filter_class_compiles_against_the_header():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "safety_filter.mk"])
    out = subprocess.run([os.path.join(CPP, "build", "safety_filter")], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    assert json.loads(out.stdout.decode().strip().split("\n")[-1]) == {"cpu": "ok"}
    # a filter without a descriptor is refused with the message the engine has always printed
    assert "mppi_amd: trajectory filters are not supported on the device" in out.stderr.decode()
