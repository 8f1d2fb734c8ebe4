"""Every rollout unit is selected, and by the right cell: the 5 x 2 grid of fr_coop.hip's translation
units (link mode FR_LINKS_ZERO .. FR_LINKS_FIELD x the simulated wrench off / on) at one
shape per launch kind - r19_h33 the x kernel with rows left over, r48_h33 the four-wave kernel, r10_h33
one-wave workgroups.

A cell's handle is set up as the _philox helpers of the mode's own tests: device Philox noise, a fixed
seed, a constant forecast; the objective is those tests' (obstacle_sets.objective: no saturated pair
buries the terms).  Every term the cell has is live, on the sets those tests show to be live: the wrench
W0 of test_gpu_simulated_wrench.py in the state's wrench slots, set A's spheres and wall on a point handle
(a point handle refuses segment masks), set C's capsules, sphere and wall on a capsule handle, and field F
behind set C on a field handle.

Three updates, at times 0, 0.05 and 0.07, the arm's velocity changed before the third.  The first update
of a handle is never a graph update (nothing is drawn ahead, no filter() is pending), and later ones are
only where the pending-filter plan is the x kernel with the filter() row folded in (engine.cpp
graph_eligible): two of three at r19_h33, none at the other two shapes.  A unit whose x kernels the
engine does not recognise among the captured nodes fails the capture and counts no graph update.
"""
import itertools

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi

import capsule_sets as CS
import field_sets as FS
import obstacle_sets as OS
import wrench_reference as WR
from launch_shapes import X, by_name, horizon

pytestmark = pytest.mark.gpu

SHAPES = ["r19_h33", "r48_h33", "r10_h33"]
CELLS = list(itertools.product(range(5), (0, 1)))   # (FrRolloutArgs::link_positions, simulated_wrench != 0)
TIMES = [0.0, 0.05, 0.07]
ENV = ("MPPI_RELAY_K", "MPPI_TAIL_DRAWS", "MPPI_DRAW_AHEAD", "MPPI_LINK_POSITIONS", "MPPI_GRAPH", "MPPI_SIMULATED_WRENCH",
       "MPPI_COSTS_IN_LAUNCH", "MPPI_HANDOVER", "MPPI_SPLIT")
EAGER = {}   # (shape, links, wrench) -> run(..., graph=0), computed once


def handle(name, links, wrench, graph):
    _, S, H, keep, _, _, _, _ = by_name(name)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    dyn = am.FrankaRidgebackDynamics(link_positions=links >= 1, simulated_wrench="state" if wrench else False)
    t = am.Trajectory.create(conf, dyn, OS.objective())
    assert t is not None and t.H == H and t.R == S + 2
    if links >= 2:
        t.set_obstacle_avoidance()
    if links >= 3:
        t.set_obstacle_capsules(CS.capsules())
    if links >= 4:
        t.set_distance_field_avoidance()
        t.set_distance_field(FS.field_f())
    if links == 2:
        t.set_obstacles(OS.set_a(), OS.T_REF_A)
    elif links >= 3:
        t.set_obstacles(CS.set_c(), CS.T_REF_C)
    t.set_graph(graph)
    t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
    t.set_forecast(am.constant_forecast(t.H))
    return t


def run(name, links, wrench, graph):
    """([(costs, weights, optimal rollout) of each update], graph_updates())"""
    t = handle(name, links, wrench, graph)
    x = am.huddled_state()
    x[24:30] = WR.W0
    rec = []
    for j, tm in enumerate(TIMES):
        if j == 2:
            x = x.copy()
            x[12 + 4] = 0.3
        t.update(x, tm)
        assert t.update_info()["wait_timeouts"] == 0
        rec.append((t.costs().copy(), t.get_weights().copy(), t.get_optimal_rollout().copy()))
    return rec, t.graph_updates()


def _eager(name, links, wrench, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    key = (name, links, wrench)
    if key not in EAGER:
        EAGER[key] = run(name, links, wrench, 0)
    return EAGER[key]


@pytest.mark.parametrize("links,wrench", CELLS)
@pytest.mark.parametrize("name", SHAPES)
def test_graph_equals_eager(name, links, wrench, monkeypatch):
    eager, eager_graphs = _eager(name, links, wrench, monkeypatch)
    graph, graphs = run(name, links, wrench, 1)
    pend = by_name(name)[7]
    want = len(TIMES) - 1 if pend[0] == X and pend[5] else 0
    assert eager_graphs == 0 and graphs == want, (eager_graphs, graphs, want)
    for j, (a, b) in enumerate(zip(eager, graph)):
        for what, u, v in zip(("costs", "weights", "optimal"), a, b):
            np.testing.assert_array_equal(u, v, err_msg="update %d %s" % (j, what))


@pytest.mark.parametrize("name", SHAPES)
def test_cells_differ(name, monkeypatch):
    """Two cells with the same first-update costs ran the same unit."""
    costs = {c: _eager(name, c[0], c[1], monkeypatch)[0][0][0] for c in CELLS}
    for c, J in costs.items():
        assert np.all(np.isfinite(J)), (name, c)
    for a, b in itertools.combinations(CELLS, 2):
        assert not np.array_equal(costs[a], costs[b]), (name, a, b)
