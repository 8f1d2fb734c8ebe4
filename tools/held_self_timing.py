#!/usr/bin/env python3
"""What the held object against the robot's own segments costs at 4096 x 64 (device noise, warmed), by
tools/held_object_timing.py's method and on its scene: the engine's own HIP-event timing (set_timing(2) /
kernel_times) of the rollout launch with its objective and of the whole update; every configuration in a
fresh process, `--rounds` times, interleaved, the order reversed in every other round; per-round medians,
their median and spread (max - min over the rounds) to --out as JSON.

  held          a held handle: sixteen obstacles and a 64^3 field, the held bits in every mask, and a beam
                (two points, one segment)
  held_parent   the same through another build of the engine library (--parent-lib, the parent commit's): is
                the older mode inside that build's run-to-run spread?  Left out without --parent-lib.
  self_none     a held-self handle with the same scene and beam and no configuration
  self_default  the same with mppi_default_held_self: 3 units x 5 segments, fifteen clearances a step

    python tools/held_self_timing.py --out profiles/held_self/timing.json [--parent-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CASES = ["held", "held_parent", "self_none", "self_default"]


def worker(case, rollouts, steps, warmup, updates):
    sys.path.insert(0, REPO)
    import numpy as np
    import assistedmanipulation_amd as am
    from assistedmanipulation_amd import abi
    from held_object_timing import ROOM, _set
    conf = am.frankaridgeback_configuration(rollouts=rollouts, horison=(steps - 0.5) * 0.01, keep_best_rollouts=20)
    t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=True), am.AssistedManipulation())
    assert t is not None and t.H == steps
    t.set_obstacle_avoidance()
    t.set_obstacle_capsules(am.ObstacleCapsules((0.1,) + (0.06,) * 7))
    t.set_distance_field_avoidance()
    t.set_held_object_avoidance()
    if case.startswith("self_"):
        t.set_held_self_avoidance()
    fn = lambda x, y, z: np.minimum(np.sqrt((x - 1.5) ** 2 + (y - 0.9) ** 2 + (z - 1.0) ** 2) - 0.3, z + 0.4)   # noqa: E731
    t.set_distance_field(am.DistanceField.from_function(fn, ROOM, 0.05, (64, 64, 64), segment_samples=3,
                                                        mask=am.MASK_ALL | am.MASK_SEGMENTS | am.MASK_HELD))
    t.set_obstacles(_set(am, np, True), 0.0)
    t.set_held_object(am.HeldObject([(0.0, -0.3, 0.05), (0.0, 0.3, 0.05)], (0.03, 0.035), (0.025,)))
    if case == "self_default":
        t.set_held_self(am.HeldSelf())
    t.set_noise_source(abi.MPPI_NOISE_DEVICE_PHILOX, seed=0x5EED)
    t.set_forecast(am.constant_forecast(steps))
    t.set_timing(2)
    x = am.huddled_state()
    rollout, whole = [], []
    for j in range(warmup + updates):
        t.update(x, 0.01 * j)
        if j >= warmup:
            k = t.kernel_times(wait=False)
            rollout.append(k[1])
            whole.append(k[4])
    assert t.update_info()["wait_timeouts"] == 0
    print(json.dumps({"case": case, "rollout_ms": float(np.median(rollout)), "update_ms": float(np.median(whole)),
                      "objective_in_launch": int(t.update_info()["objective_in_launch"]), "updates": updates,
                      "cost0": float(t.costs()[0])}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "held_self", "timing.json"))
    ap.add_argument("--parent-lib", default=None, help="another build of libmppi_amd.so for the held_parent case")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--worker", choices=CASES)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.rollouts, a.steps, a.warmup, a.updates)
    cases = [c for c in CASES if c != "held_parent" or a.parent_lib]
    rounds = {c: [] for c in cases}
    for r in range(a.rounds):
        for c in (cases if r % 2 == 0 else cases[::-1]):
            env = dict(os.environ)
            for v in ("MPPI_AMD_LIB", "MPPI_LINK_POSITIONS", "MPPI_SIMULATED_WRENCH", "MPPI_GRAPH"):
                env.pop(v, None)
            if c == "held_parent":
                env["MPPI_AMD_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", c, "--rollouts", str(a.rollouts), "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--updates", str(a.updates)]
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:   # a failed case ends the run: nothing more is started on the device
                sys.stderr.write(out.stdout + out.stderr)
                return 1
            rec = json.loads(out.stdout.strip().split("\n")[-1])
            rounds[c].append(rec)
            print("round %d %-12s rollout %.4f ms  update %.4f ms" % (r, c, rec["rollout_ms"], rec["update_ms"]), flush=True)
    result = {"shape": "%dx%d" % (a.rollouts, a.steps), "rounds": a.rounds, "updates_per_round": a.updates, "cases": {}}
    for c in cases:
        entry = {"objective_in_launch": rounds[c][0]["objective_in_launch"], "cost0": rounds[c][0]["cost0"]}
        for key in ("rollout_ms", "update_ms"):
            v = sorted(rec[key] for rec in rounds[c])
            entry[key] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "rounds": [rec[key] for rec in rounds[c]]}
        result["cases"][c] = entry
    h, s = result["cases"]["held"]["rollout_ms"]["median"], result["cases"]["self_default"]["rollout_ms"]["median"]
    result["self_default_over_held_rollout"] = s / h
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(result, fo, indent=1)
        fo.write("\n")
    print(json.dumps(result["cases"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
