#!/usr/bin/env python3
"""rocprofv3 driver: N steps of the wide-batch config (B=4096, H=1024).

Usage: gpu_profile_wide.py [steps] [fp32|bf16]"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.gpu_microbench import make_engine  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
prec = sys.argv[2] if len(sys.argv) > 2 else "fp32"      # fp32 | bf16
eng = make_engine(batch=4096, hidden=1024, obs=17, act=6, cap=1000000,
                  gemm_precision=prec)
eng.step(3)
eng.step(n)
print("done", eng.counters()["adam_t_actor"], "steps")
