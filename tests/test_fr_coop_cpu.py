"""CPU checks of the rollout kernel's sources: the generated solve block is what its generator
writes, the A/B switches that were decided are gone, and the launch plan (coop_plan.hpp under g++):
a short table, the shared table of small shapes, and a sweep of its invariants."""
import os
import shutil
import subprocess
import sys

import launch_shapes

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


def _compile(tmp_path, name, text, opt="-O0"):
    src = tmp_path / (name + ".cpp")
    src.write_text(text)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", opt, "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def test_launch_shapes_table(tmp_path):
    """Every entry of launch_shapes.SHAPES is coop_plan's answer, with and without a pending filter(),
    on 256 and on 64 CUs (one round either way), and its hand-over step follows from the plan."""
    calls = []
    for name, S, H, keep, req, sw, first, pend in launch_shapes.SHAPES:
        assert keep <= S and S + 2 <= 530 and max(first[1], pend[1]) <= launch_shapes.MIN_CUS, name
        for cus in (256, 64):
            for pending in (0, 1):
                calls.append("show(%d, %d, %d, %d, %d, %d, %d, %d);" % (S + 2, H, req, "c" in sw, "h" in sw, "s" in sw, cus, pending))
    exe = _compile(tmp_path, "shapes", r"""
#include <cstdio>
#include "coop_plan.hpp"
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
    const CoopLaunch &l = p.l[0];
    std::printf("%d %d %d %u %ld %ld %d %d %d %d %d\n", (int)p.error, p.nlaunch, l.kind, l.grid, (long)l.xbase, (long)l.xrows,
                l.relay_k, (int)p.folded, (int)p.costs_in_launch, (int)p.handover, (int)coop_fusable(count, env));
}
int main()
{
    @CALLS@
    return 0;
}
""".replace("@CALLS@", "\n    ".join(calls)))
    lines = subprocess.check_output([exe]).decode().strip().split("\n")
    assert len(lines) == 4 * len(launch_shapes.SHAPES)
    i = 0
    for name, S, H, keep, req, sw, first, pend in launch_shapes.SHAPES:
        for cus in (256, 64):
            for want in (first, pend):
                got = [int(v) for v in lines[i].split()]
                i += 1
                tag = "%s on %d CUs: %s" % (name, cus, lines[i - 1])
                assert got[:2] == [0, 1], tag
                assert tuple(got[2:9]) == want[:7], tag
                K, handover = got[6], got[9]
                if got[2] != launch_shapes.X:
                    step = -1
                    assert K == 1, tag
                elif not handover:
                    step = -1
                else:   # member 0 runs loop steps [0, k1), its second stage from k1 // 4
                    step = (H - 1 if K == 1 else ((H + 15) // 16 // K) * 16 - 1) // 4
                assert step == want[7], tag
                # the engine draws ahead exactly where coop_fusable holds: the kind with a filter() pending
                assert got[10] == int(pend[0] != launch_shapes.ONE), tag


def test_launch_plan_invariants(tmp_path):
    """A sweep of coop_plan over row counts up to three rounds and past (every count on few CUs,
    around the round boundaries and thinned between them on 64 and 256), the horizons of
    launch_shapes, every MPPI_RELAY_K, the three switches and the four booleans: what the kernels
    and the engine rely on without checking it themselves."""
    exe = _compile(tmp_path, "sweep", r"""
#include <algorithm>
#include <cstdio>
#include "coop_plan.hpp"
using namespace mppi_eng;

static long plans = 0;
#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            std::printf("%s fails: count %ld H %d cus %u relay_k %d off c%d h%d s%d pending %d drawn %d tail %d relay %d\n", #c, \
                        (long)count, H, env.cus, env.relay_k, (int)env.costs_in_launch_off, (int)env.handover_off,    \
                        (int)env.split_off, (int)pending, (int)drawn, (int)tailb, (int)relayb);                       \
            return false;                                                                                              \
        }                                                                                                              \
    } while (0)

static bool check(int64_t count, int H, bool pending, bool drawn, bool tailb, bool relayb, const EnvSwitches &env, bool fusable)
{
    const CoopPlan p = coop_plan(count, H, pending, drawn, tailb, relayb, env);
    plans++;
    const int64_t cus = env.cus;
    const int nch = (H + CH - 1) / CH;
    CHECK(p.nlaunch == 1 || p.nlaunch == 2);
    int64_t row = 0;
    for (int i = 0; i < p.nlaunch; i++) {   // the launches tile [0, count)
        CHECK(p.l[i].row0 == row && p.l[i].rows > 0);
        row += p.l[i].rows;
    }
    CHECK(row == count);
    const CoopLaunch &last = p.l[p.nlaunch - 1];
    const bool coop = p.l[0].kind != COOP_ONE_WAVE;
    CHECK(p.error == (!coop && drawn));
    CHECK(!fusable || coop);   // draws made ahead never meet p.error
    CHECK(!pending || fusable == coop);
    CHECK(!p.folded || (pending && p.x_kernel));
    CHECK(!pending || coop_folds(count, H, env) == (p.folded && p.costs_in_launch));
    CHECK(p.tail_draws == (p.x_kernel && p.costs_in_launch && drawn && tailb));
    if (!coop) {
        CHECK(p.nlaunch == 1 && !p.x_kernel && !p.folded && !p.handover && p.l[0].relay_k == 1);
        CHECK(p.l[0].grid == (unsigned)((count + ROWS_PER_WAVE - 1) / ROWS_PER_WAVE));
        return true;
    }
    CHECK(p.costs_in_launch == (!env.costs_in_launch_off && H <= HC_MAX));
    CHECK(p.handover == (!env.handover_off && H - 1 >= 4));   // a loop step per stage
    CHECK(p.nlaunch == 2 || (last.kind == COOP_X) == (last.xrows > 0));
    for (int i = 0; i < p.nlaunch; i++) {
        const CoopLaunch &l = p.l[i];
        const int64_t folded = (i + 1 == p.nlaunch && p.folded) ? 1 : 0;
        CHECK(l.kind == COOP_X || l.kind == COOP_FOUR_WAVE);
        CHECK(l.grid >= 1 && (int64_t)l.grid <= cus);
        CHECK(l.xbase == (int64_t)WG_ROWS * l.grid);
        CHECK(l.xrows == l.rows - l.xbase + folded);
        CHECK(l.xrows >= 0 && l.xrows <= std::min<int64_t>(16, (int64_t)ROWS_PER_WAVE * l.grid));
        CHECK(l.kind != COOP_FOUR_WAVE || (l.xrows == 0 && !p.x_kernel && p.nlaunch == 1));
        CHECK((l.kind == COOP_X) == p.x_kernel);
        const int K = l.relay_k;
        CHECK(K >= 1 && K <= RELAY_K_MAX);
        if (K > 1) {
            const int64_t nxb = (l.xrows + ROWS_PER_WAVE - 1) / ROWS_PER_WAVE;
            CHECK(p.handover && relayb && K <= nch && l.xrows > 0);
            CHECK(nxb <= RELAY_GROUPS_MAX && nxb + (int64_t)RELAY_STRIDE * (K - 1) <= (int64_t)l.grid);
            CHECK(K <= (env.relay_k ? std::min(env.relay_k, RELAY_K_MAX) : RELAY_K_DEFAULT));
            for (int m = 0; m < K; m++) {   // relay_member_step and group_chunks (fr_coop.hip)
                const int c0 = m * nch / K, c1 = (m + 1) * nch / K;
                const int k0 = m == 0 ? 0 : c0 * CH - 1, k1 = m + 1 == K ? H - 1 : c1 * CH - 1;
                CHECK(c1 > c0 && k1 - k0 >= 4);
            }
        }
    }
    CHECK(p.tail.launches == p.nlaunch && p.tail.row0 == last.row0 && p.tail.xbase == last.row0 + last.xbase);
    CHECK(p.tail.nxb == (int)((last.xrows + ROWS_PER_WAVE - 1) / ROWS_PER_WAVE));
    return true;
}

int main()
{
    const unsigned cuss[] = {1, 2, 8, 9, 12, 64, 256};
    const int Hs[] = {1, 2, 3, 4, 5, 15, 16, 17, 19, 20, 33, 36, 52, 63, 64, 65, 100, 127, 128, 129};
    for (unsigned cus : cuss) {
        const int64_t round = (int64_t)WG_ROWS * cus, top = 3 * round + 40;
        for (int64_t count = 1; count <= top; count++) {
            // 64 and 256 CUs: every count within 40 of a round boundary, every 37th between
            const int64_t off = count % round;
            if (cus >= 64 && off > 40 && off < round - 40 && count % 37 != 0) continue;
            for (int sw = 0; sw < 8; sw++)
                for (int rk = 0; rk <= 5; rk++) {
                    EnvSwitches env{};
                    env.costs_in_launch_off = sw & 1;
                    env.handover_off = (sw >> 1) & 1;
                    env.split_off = (sw >> 2) & 1;
                    env.relay_k = rk;
                    env.cus = cus;
                    const bool fusable = coop_fusable(count, env);
                    for (int H : Hs)
                        for (int b = 0; b < 16; b++)
                            if (!check(count, H, b & 1, (b >> 1) & 1, (b >> 2) & 1, (b >> 3) & 1, env, fusable)) return 1;
                }
        }
    }
    std::printf("%ld plans\n", plans);
    return 0;
}
""", opt="-O2")
    out = subprocess.run([exe], stdout=subprocess.PIPE).stdout.decode().strip().split("\n")
    assert out[-1].endswith(" plans") and int(out[-1].split()[0]) > 10_000_000, out[-1]
