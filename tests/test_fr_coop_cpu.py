"""CPU checks of the rollout kernel's sources: the generated solve block is what its generator
writes, and the A/B switches that were decided are gone."""
import os
import shutil
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "assistedmanipulation_amd", "csrc")
GEN_GJ = os.path.join(REPO, "tools", "gen_gj.py")


def test_generated_solve_block_is_current(tmp_path):
    src = os.path.join(CSRC, "fr_coop.hip")
    copy = tmp_path / "fr_coop.hip"
    shutil.copyfile(src, copy)
    subprocess.check_call([sys.executable, GEN_GJ, str(copy)])
    assert copy.read_bytes() == open(src, "rb").read(), "fr_coop.hip's generated block differs from tools/gen_gj.py's output"


def test_decided_switches_are_gone():
    gone = ["gj_solve", "GJ_COLS", "REGTAB_MASK", "NO_REGTAB", "COST_JG", "GJ_EXEC", "COLUMN_DOTS_PAD"]
    files = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))] + [GEN_GJ]
    files = [f for f in files if os.path.isfile(f)]
    assert len(files) > 10
    for f in files:
        text = open(f, errors="replace").read()
        for s in gone:
            assert s not in text, "%s still names %s" % (os.path.relpath(f, REPO), s)


# (count, H, switches, drawn ahead) -> kind, then "grid xbase xrows relay_k" per launch, then folded,
# objective in launch, tail draws, x kernel, coop_fusable, coop_folds.  256 CUs, both buffers present,
# filter() pending.  The values are those of the five functions the plan replaced (launch_fr_coop_update
# and its predicates), taken from a sweep of both over every count up to 70000.
ONE, FOUR, X = 0, 1, 2
PLAN_TABLE = [
    ((10, 64, "", 0), [(ONE, 3, 0, 0, 1)], dict(folded=0, costs=0, tail=0, xk=0, fusable=0, folds=0)),
    ((18, 64, "", 0), [(X, 1, 16, 3, 1)], dict(folded=1, costs=1, tail=0, xk=1, fusable=1, folds=1)),
    ((21, 64, "", 0), [(ONE, 6, 0, 0, 1)], dict(folded=0, costs=1, tail=0, xk=0, fusable=0, folds=0)),
    ((130, 32, "", 0), [(X, 8, 128, 3, 1)], dict(folded=1, costs=1, tail=0, xk=1, fusable=1, folds=1)),
    ((1002, 64, "", 0), [(X, 62, 992, 11, 2)], dict(folded=1, costs=1, tail=0, xk=1, fusable=1, folds=1)),
    ((4096, 64, "", 0), [(FOUR, 256, 4096, 0, 1)], dict(folded=0, costs=1, tail=0, xk=0, fusable=1, folds=0)),
    ((4098, 64, "", 0), [(X, 256, 4096, 3, 2)], dict(folded=1, costs=1, tail=0, xk=1, fusable=1, folds=1)),
    ((4098, 64, "", 1), [(X, 256, 4096, 3, 2)], dict(folded=1, costs=1, tail=1, xk=1, fusable=1, folds=1)),
    ((102, 136, "", 1), [(X, 6, 96, 7, 1)], dict(folded=1, costs=0, tail=0, xk=1, fusable=1, folds=0)),
    ((8192, 64, "", 0), [(ONE, 2048, 0, 0, 1)], dict(folded=0, costs=1, tail=0, xk=0, fusable=0, folds=0)),
    ((8193, 128, "", 1), [(X, 256, 4096, 0, 1), (X, 256, 4096, 2, 2)], dict(folded=1, costs=1, tail=1, xk=1, fusable=1, folds=1)),
    ((8194, 128, "", 0), [(X, 256, 4096, 0, 1), (X, 256, 4096, 3, 2)], dict(folded=1, costs=1, tail=0, xk=1, fusable=1, folds=1)),
    ((8194, 128, "s", 0), [(ONE, 2049, 0, 0, 1)], dict(folded=0, costs=1, tail=0, xk=0, fusable=0, folds=0)),
    ((20002, 64, "", 0), [(ONE, 5001, 0, 0, 1)], dict(folded=0, costs=1, tail=0, xk=0, fusable=0, folds=0)),
    ((4098, 64, "h", 0), [(X, 256, 4096, 3, 1)], dict(folded=1, costs=1, tail=0, xk=1, fusable=1, folds=1)),
    ((4098, 64, "c", 1), [(X, 256, 4096, 3, 2)], dict(folded=1, costs=0, tail=0, xk=1, fusable=1, folds=0)),
]


def test_launch_plan_table(tmp_path):
    """coop_plan.hpp alone under g++ (no HIP): the launch shapes of a short table of row counts."""
    calls = []
    for (count, H, sw, drawn), _, _ in PLAN_TABLE:
        calls.append("show(%d, %d, %d, %d, %d, %d);" % (count, H, "c" in sw, "h" in sw, "s" in sw, drawn))
    src = tmp_path / "plan.cpp"
    src.write_text(r'''
#include <cstdio>
#include "coop_plan.hpp"
using namespace mppi_eng;
static void show(long count, int H, int c, int h, int s, int drawn)
{
    EnvSwitches env{};
    env.costs_in_launch_off = c;
    env.handover_off = h;
    env.split_off = s;
    env.cus = 256;
    const CoopPlan p = coop_plan(count, H, true, drawn, true, true, env);
    std::printf("%d %d", (int)p.error, p.nlaunch);
    for (int i = 0; i < p.nlaunch; i++)
        std::printf(" %d %u %ld %ld %d %ld %ld", p.l[i].kind, p.l[i].grid, (long)p.l[i].xbase, (long)p.l[i].xrows, p.l[i].relay_k,
                    (long)p.l[i].row0, (long)p.l[i].rows);
    std::printf(" | %d %d %d %d %d %d\n", (int)p.folded, (int)p.costs_in_launch, (int)p.tail_draws, (int)p.x_kernel,
                (int)coop_fusable(count, env), (int)coop_folds(count, H, env));
}
int main()
{
    @CALLS@
    EnvSwitches env{};
    env.cus = 256;
    // draws made ahead on a shape that takes one-wave workgroups stay an error
    std::printf("%d %d\n", (int)coop_plan(20002, 64, true, true, true, true, env).error,
                (int)coop_plan(4098, 64, true, true, true, true, env).error);
    return 0;
}
'''.replace("@CALLS@", "\n    ".join(calls)))
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().strip().split("\n")
    assert len(lines) == len(PLAN_TABLE) + 1
    for line, ((count, H, sw, drawn), launches, flags) in zip(lines, PLAN_TABLE):
        head, tail = line.split(" | ")
        got = [int(v) for v in head.split()]
        tag = "count %d H %d switches '%s' drawn %d: %s" % (count, H, sw, drawn, line)
        assert got[0] == 0 and got[1] == len(launches), tag
        row0 = 0
        for i, (kind, grid, xbase, xrows, relay_k) in enumerate(launches):
            rows = 4096 if i + 1 < len(launches) else count - row0
            assert got[2 + 7 * i:9 + 7 * i] == [kind, grid, xbase, xrows, relay_k, row0, rows], tag
            row0 += rows
        want = [flags[k] for k in ("folded", "costs", "tail", "xk", "fusable", "folds")]
        assert [int(v) for v in tail.split()] == want, tag
    assert lines[-1] == "1 0"
