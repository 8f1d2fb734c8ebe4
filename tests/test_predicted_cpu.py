"""CPU checks of the predicted trajectories (mppi_predicted_optimal / mppi_predicted_rollouts): the
symbols and their argument checks, the row layout's constants against the header, the C++ shim's
methods, and predict_plan.hpp under g++ - where each row's step records start in the record buffer -
against the address rule of DESIGN section 3 restated here."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np

from assistedmanipulation_amd import _lib, abi

import launch_shapes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "assistedmanipulation_amd", "csrc")
HEADER = os.path.join(REPO, "include", "mppi_amd.h")
FR_REC, FR_REC_C = 96, 48   # doubles per 768-B and per compact step record (kernels.hpp)
ONE, FOUR, X = launch_shapes.ONE, launch_shapes.FOUR, launch_shapes.X


def test_symbols_exported_and_null_arguments_refused():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mppi_\w+)", out))
    assert {"mppi_predicted_optimal", "mppi_predicted_rollouts"} <= exported
    L = _lib.load()
    row = np.zeros(abi.MPPI_PRED_N)
    idx = np.zeros(1, dtype=np.int64)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.mppi_predicted_optimal(None, abi.dptr(row)) == abi.MPPI_ERR_INVALID
    assert L.mppi_predicted_rollouts(None, ip, 1, abi.dptr(row)) == abi.MPPI_ERR_INVALID
    assert L.mppi_predicted_rollouts(None, ip, 0, abi.dptr(row)) == abi.MPPI_ERR_INVALID
    assert L.mppi_abi_version() == 5   # no struct changed: the calls are detected by symbol


def test_row_layout_constants_match_the_header():
    text = open(HEADER).read()
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (MPPI_PRED_\w+) (\d+)\b", text, re.M)}
    assert sorted(macros) == ["MPPI_PRED_ARM_MOUNT", "MPPI_PRED_EE", "MPPI_PRED_ENERGY", "MPPI_PRED_LINKS", "MPPI_PRED_N",
                              "MPPI_PRED_Q", "MPPI_PRED_QD"]
    for name, value in macros.items():
        assert getattr(abi, name) == value, name
    assert abi.MPPI_PRED_N == abi.MPPI_PRED_LINKS + 3 * abi.MPPI_LINK_N == 70
    for name in ("mppi_predicted_optimal", "mppi_predicted_rollouts"):
        assert _lib.PROTOTYPES[name] is abi.PREDICTED_PROTOTYPES[name]


def _rule(launches, H, lr):
    """DESIGN section 3's address rule: (offset in doubles, compact) of shard row lr.  launches:
    [(kind, row0, rows)] of the plan."""
    for kind, row0, rows in launches:
        if row0 <= lr < row0 + rows:
            rs = FR_REC if kind == X else FR_REC_C
            base = row0 * H * FR_REC if len(launches) > 1 else 0
            return base + (lr - row0) * H * rs, int(kind != X)
    raise AssertionError("row %d in no launch" % lr)


def test_record_addresses_follow_the_launch_plan(tmp_path):
    cases = []   # (count, H, relay request, c, h, s, cus, pending)
    for name, S, H, keep, req, sw, first, pend in launch_shapes.SHAPES:
        for pending in (0, 1):
            cases.append((S + 2, H, req, int("c" in sw), int("h" in sw), int("s" in sw), 256, pending))
    for count in (8193, 8194):   # the split: two launches
        for pending in (0, 1):
            cases.append((count, 128, 0, 0, 0, 0, 256, pending))
    src = tmp_path / "predict.cpp"
    src.write_text(r'''
#include <cstdio>
#include "predict_plan.hpp"
using namespace mppi_eng;
static void show(long count, int H, int req, int c, int h, int s, unsigned cus, int pending)
{
    EnvSwitches env{};
    env.costs_in_launch_off = c;
    env.handover_off = h;
    env.split_off = s;
    env.relay_k = req;
    env.cus = cus;
    const CoopPlan p = coop_plan(count, H, pending, false, true, true, env);
    std::printf("plan %d %d", p.nlaunch, (int)p.folded);
    for (int i = 0; i < p.nlaunch; i++) std::printf(" %d %ld %ld %ld", p.l[i].kind, (long)p.l[i].row0, (long)p.l[i].rows, (long)p.l[i].xrows);
    std::printf("\n");
    for (long lr = 0; lr < count; lr++) {
        int64_t off = -1;
        int compact = -1;
        const bool ok = predict_row(p, H, lr, &off, &compact);
        std::printf("%d %ld %d\n", (int)ok, (long)off, compact);
    }
    int64_t off = -1;
    int compact = -1;
    std::printf("%d %d\n", (int)predict_row(p, H, -1, &off, &compact), (int)predict_row(p, H, count, &off, &compact));
}
int main()
{
    @CALLS@
    return 0;
}
'''.replace("@CALLS@", "\n    ".join("show(%d, %d, %d, %d, %d, %d, %d, %d);" % c for c in cases)))
    exe = tmp_path / "predict"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    lines = iter(subprocess.check_output([str(exe)]).decode().strip().split("\n"))
    kinds = set()
    for count, H, req, c, h, s, cus, pending in cases:
        tag = "count %d H %d pending %d" % (count, H, pending)
        head = next(lines).split()
        assert head[0] == "plan", tag
        nlaunch, folded = int(head[1]), int(head[2])
        launches = [tuple(int(v) for v in head[3 + 4 * i:6 + 4 * i]) for i in range(nlaunch)]
        xrows = [int(head[6 + 4 * i]) for i in range(nlaunch)]
        assert sum(rows for _, _, rows in launches) == count, tag
        kinds |= {(nlaunch, kind) for kind, _, _ in launches}
        if folded:   # the folded filter() row is counted in xrows but is no row of the record buffer
            kind, row0, rows = launches[-1]
            assert kind == X and xrows[-1] == rows % 16 + 1, tag
        spans = []
        for lr in range(count):
            ok, off, compact = (int(v) for v in next(lines).split())
            assert ok == 1 and (off, compact) == _rule(launches, H, lr), "%s row %d" % (tag, lr)
            assert off % 2 == 0, tag   # 16-byte loads
            spans.append((off, off + H * (FR_REC_C if compact else FR_REC)))
        spans.sort()
        assert spans[0][0] >= 0 and spans[-1][1] <= count * H * FR_REC, tag
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), tag + ": rows overlap"
        assert next(lines) == "0 0", tag   # rows outside the shard
    assert kinds >= {(1, ONE), (1, FOUR), (1, X), (2, X)}, kinds


def test_cpp_shim_compiles_and_refuses_null_arguments():
    cpp = os.path.join(REPO, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "predicted.mk"])
    out = subprocess.run([os.path.join(cpp, "build", "predicted")], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    assert json.loads(out.stdout.decode().strip().split("\n")[0]) == {"cpu": "ok"}
