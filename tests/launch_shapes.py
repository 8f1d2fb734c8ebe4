"""The rollout launch's small and awkward shapes, as plain data shared by the host-only plan check
(test_fr_coop_cpu.py) and the GPU oracle sweep (test_gpu_launch_shapes.py).

Every shape has at most 33 workgroups and at most 530 rows, so on any device with at least MIN_CUS
compute units it fits one round and its plan does not depend on the CU count.  R = S + 2 rows
(rollout 0 carries no noise, rollout 1 carries -U*), g = R // 16 workgroups, e = R % 16 rows left over.

An entry is (name, rollouts S, steps H, keep-best, MPPI_RELAY_K request (0: unset), switches, plan
of the first update, plan of an update with a filter() pending).  A plan is (kind, grid, xbase,
xrows, relay members K, folded, objective in the launch, hand-over step): coop_plan.hpp's launch
and the step update_info()["handover"] reports, -1 without the relay.  With the relay the step is
k1 // 4, where member 0 runs loop steps [0, k1): k1 = H - 1 for one member, else
(ceil(H / 16) // K) * 16 - 1 (relay_step and relay_member_step in fr_coop.hip).  The hand-over needs
a step per stage, H - 1 >= 4; below that the rows left over stay on one wave.
Switches: "c" MPPI_COSTS_IN_LAUNCH=0, "h" MPPI_HANDOVER=0, "s" MPPI_SPLIT=0.
"""
ONE, FOUR, X = 0, 1, 2   # coop_plan.hpp's CoopKind
MIN_CUS = 33
TIME_STEP = 0.01


def horizon(H):
    """A horizon of H steps: H = ceil(horison / time_step), and H * 0.01 / 0.01 rounds up for some H
    (0.33 / 0.01 gives 34), so half a step short of H."""
    return (H - 0.5) * TIME_STEP


def by_name(name):
    return next(e for e in SHAPES if e[0] == name)


SHAPES = [
    ("r17_h33",        15,  33, 5, 0, '', (2, 1, 16, 1, 1, 0, 1, 8),
     (2, 1, 16, 2, 1, 1, 1, 8)),   # 1 row left over, 2 folded
    ("r19_h33",        17,  33, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 8),
     (2, 1, 16, 4, 1, 1, 1, 8)),   # 3 rows, 4 folded: the folded row fills the wave
    ("r20_h33",        18,  33, 5, 0, '', (2, 1, 16, 4, 1, 0, 1, 8),
     (0, 5, 0, 0, 1, 0, 1, -1)),   # 4 rows: the x kernel first, one-wave workgroups once a filter() is pending
    ("r39_h33",        37,  33, 5, 0, '', (2, 2, 32, 7, 1, 0, 1, 8),
     (2, 2, 32, 8, 1, 1, 1, 8)),   # 8 rows folded, two relay groups
    ("r79_h33",        77,  33, 5, 0, '', (2, 4, 64, 15, 1, 0, 1, 8),
     (2, 4, 64, 16, 1, 1, 1, 8)),   # 16 rows folded, four full groups
    ("r48_h33",        46,  33, 5, 0, '', (1, 3, 48, 0, 1, 0, 1, -1),
     (1, 3, 48, 0, 1, 0, 1, -1)),   # nothing left over: the four-wave kernel on 3 workgroups
    ("r10_h33",         8,  33, 5, 0, '', (0, 3, 0, 0, 1, 0, 0, -1),
     (0, 3, 0, 0, 1, 0, 0, -1)),   # one-wave workgroups, the objective outside the launch
    ("r3_h33",          1,  33, 1, 0, '', (0, 1, 0, 0, 1, 0, 0, -1),
     (0, 1, 0, 0, 1, 0, 0, -1)),   # one rollout
    ("r131_h64",      129,  64, 5, 0, '', (2, 8, 128, 3, 1, 0, 1, 15),
     (2, 8, 128, 4, 1, 1, 1, 15)),   # 8 workgroups: two members do not fit
    ("r147_h64",      145,  64, 5, 0, '', (2, 9, 144, 3, 2, 0, 1, 7),
     (2, 9, 144, 4, 2, 1, 1, 7)),   # 9: two members fit exactly
    ("r191_h64",      189,  64, 5, 0, '', (2, 11, 176, 15, 1, 0, 1, 15),
     (2, 11, 176, 16, 1, 1, 1, 15)),   # 11 with four groups: one member
    ("r207_h64",      205,  64, 5, 0, '', (2, 12, 192, 15, 2, 0, 1, 7),
     (2, 12, 192, 16, 2, 1, 1, 7)),   # 12 with four groups: two fit exactly
    ("r274_h64_k3",   272,  64, 5, 3, '', (2, 17, 272, 2, 3, 0, 1, 3),
     (2, 17, 272, 3, 3, 1, 1, 3)),   # 17: three fit exactly
    ("r402_h64_k4",   400,  64, 5, 4, '', (2, 25, 400, 2, 4, 0, 1, 3),
     (2, 25, 400, 3, 4, 1, 1, 3)),   # 25: four fit exactly
    ("r463_h64_k4",   461,  64, 5, 4, '', (2, 28, 448, 15, 4, 0, 1, 3),
     (2, 28, 448, 16, 4, 1, 1, 3)),   # 28 with four groups: four fit exactly
    ("r147_h1",       145,   1, 5, 0, '', (2, 9, 144, 3, 1, 0, 1, -1),
     (2, 9, 144, 4, 1, 1, 1, -1)),   # no loop step
    ("r19_h1",         17,   1, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, -1),
     (2, 1, 16, 4, 1, 1, 1, -1)),   # no loop step
    ("r147_h2",       145,   2, 5, 0, '', (2, 9, 144, 3, 1, 0, 1, -1),
     (2, 9, 144, 4, 1, 1, 1, -1)),   # one loop step
    ("r19_h2",         17,   2, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, -1),
     (2, 1, 16, 4, 1, 1, 1, -1)),   # one loop step
    ("r147_h3",       145,   3, 5, 0, '', (2, 9, 144, 3, 1, 0, 1, -1),
     (2, 9, 144, 4, 1, 1, 1, -1)),   # hand-over off: H - 1 < 4
    ("r19_h3",         17,   3, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, -1),
     (2, 1, 16, 4, 1, 1, 1, -1)),   # hand-over off: H - 1 < 4
    ("r147_h4",       145,   4, 5, 0, '', (2, 9, 144, 3, 1, 0, 1, -1),
     (2, 9, 144, 4, 1, 1, 1, -1)),   # hand-over off: H - 1 < 4
    ("r19_h4",         17,   4, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, -1),
     (2, 1, 16, 4, 1, 1, 1, -1)),   # hand-over off: H - 1 < 4
    ("r147_h5",       145,   5, 5, 0, '', (2, 9, 144, 3, 1, 0, 1, 1),
     (2, 9, 144, 4, 1, 1, 1, 1)),   # one step per stage
    ("r19_h5",         17,   5, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 1),
     (2, 1, 16, 4, 1, 1, 1, 1)),   # one step per stage
    ("r147_h15",      145,  15, 5, 0, '', (2, 9, 144, 3, 1, 0, 1, 3),
     (2, 9, 144, 4, 1, 1, 1, 3)),   # one partial chunk
    ("r19_h15",        17,  15, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 3),
     (2, 1, 16, 4, 1, 1, 1, 3)),   # one partial chunk
    ("r147_h16",      145,  16, 5, 0, '', (2, 9, 144, 3, 1, 0, 1, 3),
     (2, 9, 144, 4, 1, 1, 1, 3)),   # one full chunk
    ("r19_h16",        17,  16, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 3),
     (2, 1, 16, 4, 1, 1, 1, 3)),   # one full chunk
    ("r147_h17",      145,  17, 5, 0, '', (2, 9, 144, 3, 1, 0, 1, 4),
     (2, 9, 144, 4, 1, 1, 1, 4)),   # a second member would have one step
    ("r19_h17",        17,  17, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 4),
     (2, 1, 16, 4, 1, 1, 1, 4)),   # a second member would have one step
    ("r147_h19",      145,  19, 5, 0, '', (2, 9, 144, 3, 1, 0, 1, 4),
     (2, 9, 144, 4, 1, 1, 1, 4)),   # a second member would have three steps
    ("r19_h19",        17,  19, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 4),
     (2, 1, 16, 4, 1, 1, 1, 4)),   # a second member would have three steps
    ("r147_h20",      145,  20, 5, 0, '', (2, 9, 144, 3, 2, 0, 1, 3),
     (2, 9, 144, 4, 2, 1, 1, 3)),   # a four-step second member
    ("r19_h20",        17,  20, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 4),
     (2, 1, 16, 4, 1, 1, 1, 4)),   # a four-step second member
    ("r147_h63",      145,  63, 5, 0, '', (2, 9, 144, 3, 2, 0, 1, 7),
     (2, 9, 144, 4, 2, 1, 1, 7)),   # partial last chunk
    ("r19_h63",        17,  63, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 15),
     (2, 1, 16, 4, 1, 1, 1, 15)),   # partial last chunk
    ("r147_h65",      145,  65, 5, 0, '', (2, 9, 144, 3, 2, 0, 1, 7),
     (2, 9, 144, 4, 2, 1, 1, 7)),   # five chunks, a one-step last chunk
    ("r19_h65",        17,  65, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 16),
     (2, 1, 16, 4, 1, 1, 1, 16)),   # five chunks, a one-step last chunk
    ("r147_h100",     145, 100, 5, 0, '', (2, 9, 144, 3, 2, 0, 1, 11),
     (2, 9, 144, 4, 2, 1, 1, 11)),   # seven chunks
    ("r19_h100",       17, 100, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 24),
     (2, 1, 16, 4, 1, 1, 1, 24)),   # seven chunks
    ("r147_h127",     145, 127, 5, 0, '', (2, 9, 144, 3, 2, 0, 1, 15),
     (2, 9, 144, 4, 2, 1, 1, 15)),   # partial last chunk
    ("r19_h127",       17, 127, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 31),
     (2, 1, 16, 4, 1, 1, 1, 31)),   # partial last chunk
    ("r147_h128",     145, 128, 5, 0, '', (2, 9, 144, 3, 2, 0, 1, 15),
     (2, 9, 144, 4, 2, 1, 1, 15)),   # HC_MAX
    ("r19_h128",       17, 128, 5, 0, '', (2, 1, 16, 3, 1, 0, 1, 31),
     (2, 1, 16, 4, 1, 1, 1, 31)),   # HC_MAX
    ("r147_h129",     145, 129, 5, 0, '', (2, 9, 144, 3, 2, 0, 0, 15),
     (2, 9, 144, 4, 2, 1, 0, 15)),   # the objective outside the launch
    ("r19_h129",       17, 129, 5, 0, '', (2, 1, 16, 3, 1, 0, 0, 32),
     (2, 1, 16, 4, 1, 1, 0, 32)),   # the objective outside the launch
    ("r147_h33",      145,  33, 5, 0, '', (2, 9, 144, 3, 2, 0, 1, 3),
     (2, 9, 144, 4, 2, 1, 1, 3)),   # three chunks: members of one and two
    ("r79_h20",        77,  20, 5, 0, '', (2, 4, 64, 15, 1, 0, 1, 4),
     (2, 4, 64, 16, 1, 1, 1, 4)),   # four groups at a short horizon
    ("r274_h33_k3",   272,  33, 5, 3, '', (2, 17, 272, 2, 2, 0, 1, 3),
     (2, 17, 272, 3, 2, 1, 1, 3)),   # three members refused: the last would have one step
    ("r274_h36_k3",   272,  36, 5, 3, '', (2, 17, 272, 2, 3, 0, 1, 3),
     (2, 17, 272, 3, 3, 1, 1, 3)),   # three members, a four-step last one
    ("r402_h52_k4",   400,  52, 5, 4, '', (2, 25, 400, 2, 4, 0, 1, 3),
     (2, 25, 400, 3, 4, 1, 1, 3)),   # four members, a four-step last one
    ("r274_h100_k3",  272, 100, 5, 3, '', (2, 17, 272, 2, 3, 0, 1, 7),
     (2, 17, 272, 3, 3, 1, 1, 7)),   # seven chunks over three members: 2, 2, 3
    ("r402_h100_k4",  400, 100, 5, 4, '', (2, 25, 400, 2, 4, 0, 1, 3),
     (2, 25, 400, 3, 4, 1, 1, 3)),   # seven chunks over four members: 1, 2, 2, 2
    ("r147_h64_h",    145,  64, 5, 0, 'h', (2, 9, 144, 3, 1, 0, 1, -1),
     (2, 9, 144, 4, 1, 1, 1, -1)),   # MPPI_HANDOVER=0: the rows left over on one wave
    ("r147_h64_c",    145,  64, 5, 0, 'c', (2, 9, 144, 3, 2, 0, 0, 7),
     (2, 9, 144, 4, 2, 1, 0, 7)),   # MPPI_COSTS_IN_LAUNCH=0: fr_step_cost_kernel after the relay
    ("r20_h33_c",      18,  33, 5, 0, 'c', (2, 1, 16, 4, 1, 0, 0, 8),
     (0, 5, 0, 0, 1, 0, 0, -1)),   # MPPI_COSTS_IN_LAUNCH=0 on both kernel kinds
]
