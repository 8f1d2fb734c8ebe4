"""COOP_TRACE + COST_TRACE wave trace of the 4096 x 64 update launch (MPPI_WAVE_TRACE): the end of the
launch.  Slots of four words; per main wave (slot 4 b + w): loop start, loop end, HW_ID, the wave's
end after its objective work.  Past the main waves (fr_coop.hip TR_*): 0 the relay rows' start / end,
1 + m member m's stages' ends, then per traced relay host - relay group 0's first member (workgroup
0) and its last (workgroup 8 (K - 1)) - 44 slots at 40 + 44 h: chunk c of group g at 8 g + c (start,
end, wave, chunk << 8 | 1 if the wave took it ahead of its relay stage), 40 the relay group's closing (entry, the
previous member's sums arrived, rows summed, costs stored), 41 the ends of waves 4 .. 7.
Prints, for the middle and the last update and as medians over the second half of the updates: the
hosts' chunk tables, and the launch's end and each relay host's end minus the latest end among the
workgroups that host no relay member.
usage: wave_trace_tail.py file [relay members K = 2] [relay groups = 1] [extra slots = 128]"""
import sys

import numpy as np

path = sys.argv[1]
K = int(sys.argv[2]) if len(sys.argv) > 2 else 2
nxb = int(sys.argv[3]) if len(sys.argv) > 3 else 1
extra = int(sys.argv[4]) if len(sys.argv) > 4 else 128
nmain = 1024
raw = np.fromfile(path, dtype=np.uint32)
recs = raw.reshape(-1, nmain + extra, 4).astype(np.int64)
nblk = nmain // 4
hosts = sorted(q + 8 * m for q in range(nxb) for m in range(K))
traced = [0] if K == 1 else [0, 8 * (K - 1)]


def analyse(rec, verbose):
    st, le, we = rec[:nmain, 0], rec[:nmain, 1], rec[:nmain, 3]
    t0 = st[st > 0].min()
    us = lambda x: (x - t0) / 100.0
    blk = np.arange(nmain) // 4
    bend = np.array([us(we[blk == b]).max() for b in range(nblk)])
    bloop = np.array([us(le[blk == b]).max() for b in range(nblk)])
    tables = {}
    for h, b in enumerate(traced):
        base = nmain + 40 + 44 * h
        tasks = [(g, t, rec[base + 8 * g + t]) for g in range(5) for t in range(8) if rec[base + 8 * g + t][0]]
        closing, w47 = rec[base + 40], rec[base + 41]
        ends = [us(x[1]) for _, _, x in tasks] + [us(x) for x in w47 if x] + ([us(closing[3])] if closing[3] else [])
        bend[b] = max([bend[b]] + ends)   # waves 4 .. 7 may end the workgroup
        tables[b] = (tasks, closing, w47)
    other = np.array([b not in hosts for b in range(nblk)])
    last_other = bend[other].max()
    out = {"loops_p50": float(np.median(us(le))), "wg_end_p50": float(np.median(bend)), "last_other": float(last_other),
           "launch_end": float(bend.max()), "tail": float(bend.max() - last_other)}
    for b in hosts:
        out["host%d" % b] = float(bend[b] - last_other)
        out["host%d_end" % b] = float(bend[b])
        out["host%d_loops" % b] = float(bloop[b])
    if verbose:
        print("  main loop end p50 %.1f, workgroup end p50 %.1f, latest workgroup without a relay member %.1f" %
              (out["loops_p50"], out["wg_end_p50"], last_other))
        print("  launch end %.1f: %.1f after the latest workgroup without a relay member" % (out["launch_end"], out["tail"]))
        for b in hosts:
            print("  relay host %d: loops end %.1f, ends %.1f (%+.1f)" % (b, bloop[b], bend[b], bend[b] - last_other))
        fx = rec[nmain]
        print("  relay rows: start %.1f end %.1f" % (us(fx[0]), us(fx[1])))
        for m in range(K):
            print("  relay member %d stages end" % m, ["%.1f" % us(x) if x else "-" for x in rec[nmain + 1 + m]])
        for b in traced:
            tasks, closing, w47 = tables[b]
            print("  workgroup %d chunks (group 4: the relay rows; *: taken ahead of the wave's relay stage):" % b)
            for g in range(5):
                row = ["c%d %.1f-%.1f w%d%s" % (x[3] >> 8, us(x[0]), us(x[1]), x[2], "*" if x[3] & 255 else "") for gg, t, x in tasks if gg == g]
                print("    group %d: %s" % (g, "   ".join(row) if row else "-"))
            if closing[0]:
                print("    relay closing: entry %.1f, sums arrived %.1f, rows summed %.1f, costs stored %.1f" %
                      tuple(us(x) for x in closing))
            print("    waves 4..7 end:", " ".join("%.1f" % us(x) if x else "-" for x in w47))
    return out


for u in (len(recs) // 2, len(recs) - 1):
    print("update %d of %d" % (u, len(recs)))
    analyse(recs[u], True)
half = [analyse(r, False) for r in recs[len(recs) // 2:]]
print("medians over updates %d..%d:" % (len(recs) // 2, len(recs) - 1))
for k in half[0]:
    print("  %-14s %7.1f" % (k, np.median([h[k] for h in half])))
