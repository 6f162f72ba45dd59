#!/usr/bin/env python3
"""Print per-phase times of the persistent step kernel (100 MHz clock).

The kernel stamps step 1 of a multi-step launch: the first step that runs
the steady-state schedule (the tail crew's precompute under the previous
policy block, the merged forward phase).  Step 0 of a launch runs the
un-pipelined PH0-PH4 schedule instead; `--first` stamps that one through
one-step launches.  `--clip C` builds the engine with max_grad_norm=C (the
clip-on kernel; 1e30 keeps the work and never binds): its two extra phases,
the chunked |g|^2 plus the grid barrier that publishes it, are stamped in
slots 56 / 57 and sit inside the "c.adam" and "a.adam" rows.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.gpu_microbench import make_engine  # noqa: E402

# stamp map: fused regions stamp all their legacy indices back-to-back, so
# collapsed rows read ~0 us and the preceding row carries the whole block.
# On a steady-state step PH0-PH4 are collapsed too: the critic forward ran
# under the previous policy block, and the "fwd" row is the merged phase
# (quads: actor_t chain -> critic_target chain -> projection + CE; crew:
# actor forward).
PHASES = [
    "PH0 sample", "PH1 L1x4", "PH2 L2x3", "PH3 L3x3", "PH4 headsx3",
    "fwd quads+crew", "(fused)", "(fused)", "(fused)",
    "quadB c.dX", "(fused)", "(fused)", "c.dW", "c.adam",
    "quadC policy+tail", "(fused)", "(fused)", "(fused)", "(fused)",
    "(fused)", "(fused)", "(fused)", "(fused)", "(fused)",
    "(fused)", "a.dW", "a.adam", "(fused)",
]
# stamps inside a phase, us after the stamp that opens it:
# (label, slot, opening slot)
INNER = [
    ("fwd: quad 0 a2 ready", 54, 5),
    ("fwd: quad 0 end", 55, 5),
    ("fwd: actor crew end", 53, 5),
    ("policy: quad 0 end", 51, 14),
    ("policy: tail crew end", 52, 14),
    ("clip: critic |g|^2 + barrier", 56, 13),
    ("clip: actor |g|^2 + barrier", 57, 26),
]

# quad 0's walk through the policy megachain: each slot is one layer tile
# plus the quad barrier that hands its output on (the last has none)
POLICY_SLOTS = [
    ("pc.L1", 40, 41), ("pc.L2", 41, 42), ("pc.L3", 42, 43),
    ("pc.L4 + pgrad", 43, 44), ("dX c.w4", 44, 45), ("dX c.w3", 45, 46),
    ("dX narrow (a)", 46, 47), ("dX a.w4", 47, 48), ("dX a.w3", 48, 49),
    ("dX a.w2, no barrier", 49, 51),
]

first = "--first" in sys.argv[1:]
clip = 0.0
if "--clip" in sys.argv[1:]:
    clip = float(sys.argv[sys.argv.index("--clip") + 1])
eng = make_engine(max_grad_norm=clip)
eng.step(50)          # warm; stamps overwritten each launch
if first:
    eng.step(1)
ts = eng.read("tstamp").numpy()
total = 0.0
for i, name in enumerate(PHASES):
    dt_us = (ts[i + 1] - ts[i]) / 100.0   # 100 MHz -> us
    total += dt_us
    print(f"{name:18s} {dt_us:8.2f} us")
print(f"{'TOTAL':18s} {total:8.2f} us (stamped step "
      f"{'0 of a one-step launch' if first else '1 of 50'}, incl. barriers)")
for name, slot, base in INNER:
    if ts[slot] > ts[base]:               # not stamped on this schedule
        print(f"{name:24s} +{(ts[slot] - ts[base]) / 100.0:7.2f} us")
for name, lo, hi in POLICY_SLOTS:
    print(f"policy slot {name:20s} {(ts[hi] - ts[lo]) / 100.0:7.2f} us")
