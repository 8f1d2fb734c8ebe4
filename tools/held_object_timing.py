#!/usr/bin/env python3
"""What obstacle avoidance with a held object costs at 4096 x 64 (device noise, warmed), by
tools/distance_field_timing.py's method: the engine's own HIP-event timing (set_timing(2) / kernel_times)
of the rollout launch with its objective and of the whole update; every configuration in a fresh process,
`--rounds` times, the order reversed in every other round; per-round medians, their median and spread
(max - min over the rounds) to --out as JSON.

  field       a field handle: sixteen obstacles, every one masked MASK_ALL | MASK_SEGMENTS | MASK_HELD less the
              held bits (a field handle refuses them), and a 64^3 field of 0.05 m, three samples a segment
  held_none   a held handle with the same set and field, the held bits in every mask, and nothing held
  held_4      the same with a four-point object (three segments): 16 x 7 held clearances and 13 held samples
              a step on top of the field handle's

    python tools/held_object_timing.py --out profiles/held_object/timing.json
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["field", "held_none", "held_4"]
ROOM = (-1.2, -1.2, -0.6)     # 3.2 m a side


def _set(am, np, held):
    """Sixteen obstacles on a ring of 1.6 m around the arm's column: spheres, capsules and four half-spaces."""
    mask = am.MASK_ALL | am.MASK_SEGMENTS | (am.MASK_HELD if held else 0)
    out = []
    for i in range(12):
        a = 2.0 * np.pi * i / 12.0
        c = (0.6 + 1.6 * np.cos(a), 0.6 + 1.6 * np.sin(a), 0.4 + 0.1 * i)
        if i % 2:
            out.append(am.CapsuleObstacle(c, (0.0, 0.0, 0.5), 0.05, mask=mask))
        else:
            out.append(am.SphereObstacle(c, 0.05 + 0.01 * i, mask=mask))
    out.append(am.HalfSpaceObstacle((0.0, 0.0, -0.3), (0.0, 0.0, 1.0), mask=mask & ~1))
    out.append(am.HalfSpaceObstacle((0.0, 0.0, 2.6), (0.0, 0.0, -1.0), mask=mask))
    out.append(am.HalfSpaceObstacle((3.0, 0.0, 0.0), (-1.0, 0.0, 0.0), mask=mask))
    out.append(am.HalfSpaceObstacle((0.0, -2.0, 0.0), (0.0, 1.0, 0.0), mask=mask))
    return out


def worker(case, rollouts, steps, warmup, updates):
    sys.path.insert(0, REPO)
    import numpy as np
    import assistedmanipulation_amd as am
    from assistedmanipulation_amd import abi
    held = case.startswith("held_")
    conf = am.frankaridgeback_configuration(rollouts=rollouts, horison=(steps - 0.5) * 0.01, keep_best_rollouts=20)
    t = am.Trajectory.create(conf, am.FrankaRidgebackDynamics(link_positions=True), am.AssistedManipulation())
    assert t is not None and t.H == steps
    t.set_obstacle_avoidance()
    t.set_obstacle_capsules(am.ObstacleCapsules((0.1,) + (0.06,) * 7))
    t.set_distance_field_avoidance()
    if held:
        t.set_held_object_avoidance()
    fn = lambda x, y, z: np.minimum(np.sqrt((x - 1.5) ** 2 + (y - 0.9) ** 2 + (z - 1.0) ** 2) - 0.3, z + 0.4)   # noqa: E731
    t.set_distance_field(am.DistanceField.from_function(fn, ROOM, 0.05, (64, 64, 64), segment_samples=3,
                                                        mask=am.MASK_ALL | am.MASK_SEGMENTS | (am.MASK_HELD if held else 0)))
    t.set_obstacles(_set(am, np, held), 0.0)
    if case == "held_4":
        t.set_held_object(am.HeldObject([(-0.15, -0.15, 0.08), (0.15, -0.15, 0.08), (0.15, 0.15, 0.08), (-0.15, 0.15, 0.08)],
                                        (0.02, 0.025, 0.03, 0.035), (0.02, 0.015, 0.01)))
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "held_object", "timing.json"))
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
    f, h = result["cases"]["field"]["rollout_ms"]["median"], result["cases"]["held_4"]["rollout_ms"]["median"]
    result["held_4_over_field_rollout"] = h / f
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(result, fo, indent=1)
        fo.write("\n")
    print(json.dumps(result["cases"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
