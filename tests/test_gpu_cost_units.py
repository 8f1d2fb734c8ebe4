"""Every step-cost kernel is selected, and by the right cell: the 7 x 3 x 2 table of fr_cost.hip's
launch_fr_step_cost (link mode FR_LINKS_ZERO .. FR_LINKS_HELD_SELF x the objective - AssistedManipulation,
AssistedManipulation with the energy tank, TrackPoint - x the record layout).  The tests of
the modes themselves reach the cost kernels (MPPI_COSTS_IN_LAUNCH=0) in the (AssistedManipulation, no tank)
column at one shape only, so a cell swapped elsewhere would pass them.

Which update reads which layout (the rollouts' records are the compact FR_REC_C ones unless the x kernel wrote
them, and the filter() row's are always the 768-B FR_REC ones: fr_coop.hip fr_coop_compact, engine.cpp
cost_args):
  * r20_h33_c, first update: the x kernel, FR_REC.  Second update, a filter() pending: one-wave workgroups,
    the rollouts' costs from FR_REC_C; the filter() row by itself, FR_REC.
  * r147_h64_c, both updates: the x kernel over two relay members, FR_REC; in the second the filter() row is
    folded into the launch and its cost comes from the same kernel's extra row.

A cell's handle is set up as the mode's own tests set theirs up, every term the cell has live on the sets those
tests show to be live: test_gpu_rollout_units.handle's for modes 0..4 (set A on a point handle, set C and the
capsules on a capsule handle, field F behind them), test_gpu_held_object._unit_run's for mode 5 (the held bits in
one obstacle's mask and in the field's; the beam, then the tray) and test_gpu_held_self._unit_run's for mode 6
(the default configuration, then the wrist's).  The objectives are obstacle_sets.objective's; TrackPoint with
tp_self, so that its self-collision term is live and modes 0 and 1 differ.  Two updates from that module's state
at its first two times, host-injected noise, the same for both handles of a cell.

Each cell runs twice, the objective inside the rollout launch and through the cost kernel, and the two must
agree within helpers.py's bars.  Within one objective no two link modes may give the same first-update costs,
and the tank's costs must differ from the plain objective's: two cells with the same costs could be swapped
unseen.
"""
import itertools

import numpy as np
import pytest

import assistedmanipulation_amd as am
from assistedmanipulation_amd import abi

import capsule_sets as CS
import field_sets as FS
import held_self_sets as SS
import obstacle_sets as OS
import test_gpu_held_object as HELD
import test_gpu_rollout_units as UNITS
import wrench_reference as WR
from launch_shapes import by_name, horizon
from test_gpu_link_positions import _assert_bars, _noise_scale
from test_gpu_obstacles import _set_env

pytestmark = pytest.mark.gpu

SHAPES = ["r20_h33", "r147_h64"]   # run as they are and as their _c twins
MODES = list(range(7))             # FrCostArgs::link_positions
OBJECTIVES = {"am": lambda: OS.objective(), "tank": lambda: OS.objective(energy=True),
              "track_point": lambda: OS.objective("track_point", tp_self=True)}
RUNS = {}   # (shape, objective, mode) -> (in-launch records, cost-kernel records), computed once


def handle(conf, objective, links):
    dyn = am.FrankaRidgebackDynamics(link_positions=links >= 1)
    t = am.Trajectory.create(conf, dyn, OBJECTIVES[objective]())
    assert t is not None
    if links >= 2:
        t.set_obstacle_avoidance()
    if links >= 3:
        t.set_obstacle_capsules(CS.capsules())
    if links >= 4:
        t.set_distance_field_avoidance()
    if links >= 5:
        t.set_held_object_avoidance()
    if links >= 6:
        t.set_held_self_avoidance()
    f = FS.field_f()
    if links >= 5:
        f = am.DistanceField(f.values, f.origin, f.voxel, mask=f.mask | am.MASK_HELD, segment_samples=f.segment_samples)
    if links >= 4:
        t.set_distance_field(f)
    if links == 2:
        t.set_obstacles(OS.set_a(), OS.T_REF_A)
    elif links >= 3:
        t.set_obstacles(HELD._held_bits(CS.set_c()) if links >= 5 else CS.set_c(), CS.T_REF_C)
    t.set_noise_source(abi.MPPI_NOISE_HOST_INJECTED)
    return t


def _runs(name, objective, links, monkeypatch):
    key = (name, objective, links)
    if key in RUNS:
        return RUNS[key]
    _, S, H, keep, req = by_name(name)[:5]
    assert by_name(name + "_c")[1:5] == (S, H, keep, req)
    conf = am.frankaridgeback_configuration(rollouts=S, horison=horizon(H), keep_best_rollouts=keep, threads=8)
    _set_env(monkeypatch, req, "")
    a = handle(conf, objective, links)
    _set_env(monkeypatch, req, "c")
    b = handle(conf, objective, links)
    assert a.H == b.H == H and a.R == b.R == S + 2
    rng = np.random.default_rng(11)
    sd = np.sqrt(np.diag(conf.covariance)) * _noise_scale(H)
    x = am.huddled_state()
    x[24:30] = WR.W0
    held, configurations = SS.objects()[:2], [am.HeldSelf(), SS.wrist()]
    rec = ([], [])
    for j, tm in enumerate(UNITS.TIMES[:2]):
        eps = rng.standard_normal((a.noise_draws(tm), a.C)) * sd
        for t, out, in_launch in ((a, rec[0], 1), (b, rec[1], 0)):
            t.set_forecast(am.constant_forecast(H))
            if links >= 5:
                t.set_held_object(held[j])
            if links >= 6:
                t.set_held_self(configurations[j])
            assert t.noise_draws(tm) == eps.shape[0]
            t.inject_noise(eps)
            t.update(x, tm)
            info = t.update_info()
            assert info["wait_timeouts"] == 0 and info["objective_in_launch"] == in_launch, (key, j, info)
            out.append((t.costs().copy(), t.get_weights().copy(), t.get_optimal_rollout().copy()))
    RUNS[key] = rec
    return rec


@pytest.mark.parametrize("links", MODES)
@pytest.mark.parametrize("objective", list(OBJECTIVES))
@pytest.mark.parametrize("name", SHAPES)
def test_cost_kernel_against_the_launch(name, objective, links, monkeypatch):
    launch, kernel = _runs(name, objective, links, monkeypatch)
    H = by_name(name)[2]
    for j, ((Jr, wr, Ur), (Jd, wd, Ud)) in enumerate(zip(launch, kernel)):
        assert np.all(np.isfinite(Jr)), (name, objective, links, j)
        _assert_bars("%s %s links %d update %d" % (name, objective, links, j), Jd, Jr, wd, wr, Ud, Ur, H)


@pytest.mark.parametrize("name", SHAPES)
def test_cells_differ(name, monkeypatch):
    """Two cells with the same first-update costs could be one kernel: in the launch (what the cost kernel is held
    to) and from the cost kernel itself."""
    for side in (0, 1):
        J = {(o, m): _runs(name, o, m, monkeypatch)[side][0][0] for o in OBJECTIVES for m in MODES}
        for o in OBJECTIVES:
            for m, n in itertools.combinations(MODES, 2):
                assert not np.array_equal(J[o, m], J[o, n]), (name, side, o, m, n)
        for m in MODES:
            assert not np.array_equal(J["tank", m], J["am", m]), (name, side, m)
