#!/usr/bin/env python3
"""What obstacle avoidance with capsules costs at 4096 x 64 (device noise, warmed), by
tools/obstacle_timing.py's method: the engine's own HIP-event timing (set_timing(2) / kernel_times) of
the rollout launch with its objective and of the whole update; every configuration in a fresh process,
`--rounds` times, the order reversed in every other round; per-round medians, their median and spread
(max - min over the rounds) to --out as JSON.

  parent      an earlier build's library (--parent-lib), obstacle mode without capsules: the obstacles of
              the tests' set C as spheres (a capsule: a sphere at its start) against the nine points
  points      this tree, the same mode and set - the same code object as `parent`
  cap_seg     capsule mode, set C with segment masks on all four obstacles (the sphere and the wall too)
  cap_pts     capsule mode, the same four obstacles (capsules as capsules) with point masks only
  cap_empty   capsule mode, an empty set

    python tools/capsule_timing.py --parent-lib /path/to/parent/libmppi_amd.so --out profiles/capsules/timing.json
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["parent", "points", "cap_seg", "cap_pts", "cap_empty"]
NO_BASE = 0x1FE
# set C (tests/capsule_sets.py): start, axis, radius, velocity; then its sphere and its wall
BARS = [((2.0, 2.0, 0.0), (0.0, 0.0, 2.0), 0.05, (0.0, 0.0, 0.0)), ((0.9, 3.0, 1.2), (0.5, 0.1, -0.3), 0.06, (0.0, -0.8, 0.1))]
BALL = ((2.2, 0.9, 1.0), 0.3)
WALL = ((-1.0, 0.0, -0.5), (0.6, 0.0, 0.8))


def _obstacles(am, case):
    if case == "cap_empty":
        return []
    if case in ("parent", "points"):
        return ([am.SphereObstacle(c, r, velocity=v) for c, e, r, v in BARS] + [am.SphereObstacle(*BALL)] +
                [am.HalfSpaceObstacle(*WALL, mask=NO_BASE)])
    if case == "cap_pts":
        return ([am.CapsuleObstacle(c, e, r, velocity=v, mask=am.MASK_ALL) for c, e, r, v in BARS] + [am.SphereObstacle(*BALL)] +
                [am.HalfSpaceObstacle(*WALL, mask=NO_BASE)])
    arm = am.MASK_SEGMENTS & ~am.mask_segment(0)
    return [am.CapsuleObstacle(*BARS[0][:3], velocity=BARS[0][3], mask=am.MASK_SEGMENTS | 1),
            am.CapsuleObstacle(*BARS[1][:3], velocity=BARS[1][3], mask=arm), am.SphereObstacle(*BALL, mask=am.MASK_SEGMENTS),
            am.HalfSpaceObstacle(*WALL, mask=arm)]


def worker(case, rollouts, steps, warmup, updates):
    sys.path.insert(0, REPO)
    import numpy as np
    import assistedmanipulation_amd as am
    from assistedmanipulation_amd import abi
    conf = am.frankaridgeback_configuration(rollouts=rollouts, horison=(steps - 0.5) * 0.01, keep_best_rollouts=20)
    t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=True), am.AssistedManipulation())
    assert t is not None and t.H == steps
    t.set_obstacle_avoidance()
    if case.startswith("cap_"):
        t.set_obstacle_capsules(am.ObstacleCapsules((0.1,) + (0.06,) * 7))
    t.set_obstacles(_obstacles(am, case), -0.07)
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
                      "updates": updates}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libmppi_amd.so of the build to compare with (omit: no `parent` case)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "capsules", "timing.json"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--worker", choices=CASES)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.rollouts, a.steps, a.warmup, a.updates)
    cases = [c for c in CASES if c != "parent" or a.parent_lib]
    rounds = {c: [] for c in cases}
    for r in range(a.rounds):
        for c in (cases if r % 2 == 0 else cases[::-1]):
            env = dict(os.environ)
            env.pop("MPPI_AMD_LIB", None)
            for v in ("MPPI_LINK_POSITIONS", "MPPI_SIMULATED_WRENCH", "MPPI_GRAPH"):
                env.pop(v, None)
            if c == "parent":
                env["MPPI_AMD_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", c, "--rollouts", str(a.rollouts), "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--updates", str(a.updates)]
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:   # a failed case ends the run: nothing more is started on the device
                sys.stderr.write(out.stdout + out.stderr)
                return 1
            rec = json.loads(out.stdout.strip().split("\n")[-1])
            rounds[c].append(rec)
            print("round %d %-9s rollout %.4f ms  update %.4f ms" % (r, c, rec["rollout_ms"], rec["update_ms"]), flush=True)
    result = {"shape": "%dx%d" % (a.rollouts, a.steps), "rounds": a.rounds, "updates_per_round": a.updates, "cases": {}}
    for c in cases:
        entry = {}
        for key in ("rollout_ms", "update_ms"):
            v = sorted(rec[key] for rec in rounds[c])
            entry[key] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "rounds": [rec[key] for rec in rounds[c]]}
        result["cases"][c] = entry
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["cases"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
