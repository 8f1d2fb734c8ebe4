"""The held-self configurations of the held-self tests, beside the objects, sets and fields of
held_object_sets.py: plain data shared by the CPU checks of the reference (test_held_self_cpu.py) and the
GPU parity tests (test_gpu_held_self.py).

Distances between the held units' surfaces and the robot's segment axes (d - r_u), measured on the CPU
reference over three updates at the tests' shapes with the tests' noise scaling:
  * the wrist and hand segments 5..7 move little or not at all against the grasp (segment 7 is rigid with
    it, segments 5 and 6 turn about joint 7 only): the beam keeps 0.227 m and more from segments 5 and 6 and
    0.025 m from segment 7; the tray 0.2687 m and 0.15 m; the tip 0.338 m, 0.332 m and 0.1317 m.
  * everything below the wrist can be reached: the beam comes down to 0.07 m from the tower's axis (segments
    0 and 1; 0.66 m at rest) and through the forearm's (segment 4: -0.02 m; 0.24 m at rest); the tray to
    0.06 m and -0.01 m (0.45 m and 0.27 m at rest); the tip to 0.12 m and -0.02 m (0.69 m and 0.34 m).

Three updates, three configurations, one per object of held_object_sets.objects():
  0 "wrist":  the beam against segments 5, 6 and 7 alone with radii inside the distances above: every
              clearance stays on the inverse branch whatever the noise does.  Segment 5 has no length, so the
              beam's points give "A=0 E=0" and its segment "A=0"; its points on segments 6 and 7 give "E=0".
  1 "tower":  the tray with the tower (segment 0) as fat as the chassis, 0.4 m: clear by 0.05 m at rest, and
              about every second rollout folds the tray into it; the forearm, wrist and hand thin enough to
              stay clear of at rest.  Both branches; the rollouts differ in whether they saturate at all.
  2 "tip":    the one point against segments 0, 4, 5 and 7 with radii of their own; the units' bits name
              held segments the tip does not have, which select nothing.
mppi_default_held_self (every unit, segments 0..4, 0.1 m) is not among them: under the tests' noise the beam
passes through the forearm, so no update with it stays on one branch.
"""
import assistedmanipulation_amd as am

from held_object_sets import objects, fields, sets, capsules, objective   # noqa: F401  (what stands beside them)


def wrist():
    return am.HeldSelf(units=0x7F, segments=0xE0, radii=(0.0, 0.0, 0.0, 0.0, 0.0, 0.1, 0.12, 0.01))


def tower():
    return am.HeldSelf(units=0x7F, segments=0xD1, radii=(0.4, 0.1, 0.1, 0.1, 0.05, 0.1, 0.1, 0.05))


def tip():
    return am.HeldSelf(units=am.held_self_unit_point(0) | am.held_self_unit_segment(0) | am.held_self_unit_segment(2), segments=0xB1,
                       radii=(0.3, 0.0, 0.0, 0.0, 0.06, 0.02, 0.0, 0.03))


def configurations():
    return [wrist(), tower(), tip()]
