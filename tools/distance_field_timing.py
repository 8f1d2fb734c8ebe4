#!/usr/bin/env python3
"""What obstacle avoidance with a distance field costs at 4096 x 64 (device noise, warmed), by
tools/capsule_timing.py's method: the engine's own HIP-event timing (set_timing(2) / kernel_times) of
the rollout launch with its objective and of the whole update; every configuration in a fresh process,
`--rounds` times, the order reversed in every other round; per-round medians, their median and spread
(max - min over the rounds) to --out as JSON.

  cap_empty   a capsule handle with an empty set: the baseline
  df_none     a field handle with no field (the term is one uniform branch)
  df_64_m0    a 64^3 grid of 0.05 m, the nine points only (no segment samples)
  df_64_m3    the same grid, three samples a segment (33 samples a step)
  df_128_m3   a 128^3 grid of 0.025 m over the same room (8 MiB: twice an XCD's L2)
  df_256_m3   a 256^3 grid of 0.0125 m (64 MiB: past all the L2s together)

The field is a ball beside the robot and a floor, true distances, every point and segment masked in.

    python tools/distance_field_timing.py --out profiles/distance_field/timing.json
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["cap_empty", "df_none", "df_64_m0", "df_64_m3", "df_128_m3", "df_256_m3"]
ROOM = (-1.2, -1.2, -0.6)     # 3.2 m a side


def _field(am, np, case):
    n = int(case.split("_")[1])
    m = int(case.split("_")[2][1:])
    fn = lambda x, y, z: np.minimum(np.sqrt((x - 1.5) ** 2 + (y - 0.9) ** 2 + (z - 1.0) ** 2) - 0.3, z + 0.4)   # noqa: E731
    return am.DistanceField.from_function(fn, ROOM, 3.2 / n, (n, n, n), segment_samples=m)


def worker(case, rollouts, steps, warmup, updates):
    sys.path.insert(0, REPO)
    import numpy as np
    import assistedmanipulation_amd as am
    from assistedmanipulation_amd import abi
    conf = am.frankaridgeback_configuration(rollouts=rollouts, horison=(steps - 0.5) * 0.01, keep_best_rollouts=20)
    t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=True), am.AssistedManipulation())
    assert t is not None and t.H == steps
    t.set_obstacle_avoidance()
    t.set_obstacle_capsules(am.ObstacleCapsules((0.1,) + (0.06,) * 7))
    if case.startswith("df_"):
        t.set_distance_field_avoidance()
        if case != "df_none":
            t.set_distance_field(_field(am, np, case))
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
                      "objective_in_launch": int(t.update_info()["objective_in_launch"]), "updates": updates}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "distance_field", "timing.json"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--worker", choices=CASES)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.rollouts, a.steps, a.warmup, a.updates)
    rounds = {c: [] for c in CASES}
    for r in range(a.rounds):
        for c in (CASES if r % 2 == 0 else CASES[::-1]):
            env = dict(os.environ)
            for v in ("MPPI_AMD_LIB", "MPPI_LINK_POSITIONS", "MPPI_SIMULATED_WRENCH", "MPPI_GRAPH"):
                env.pop(v, None)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", c, "--rollouts", str(a.rollouts), "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--updates", str(a.updates)]
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:   # a failed case ends the run: nothing more is started on the device
                sys.stderr.write(out.stdout + out.stderr)
                return 1
            rec = json.loads(out.stdout.strip().split("\n")[-1])
            rounds[c].append(rec)
            print("round %d %-10s rollout %.4f ms  update %.4f ms" % (r, c, rec["rollout_ms"], rec["update_ms"]), flush=True)
    result = {"shape": "%dx%d" % (a.rollouts, a.steps), "rounds": a.rounds, "updates_per_round": a.updates, "cases": {}}
    for c in CASES:
        entry = {"objective_in_launch": rounds[c][0]["objective_in_launch"]}
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
