#!/usr/bin/env python3
"""Wide-config A/B: uncaptured step() loop vs hipGraph-replayed steps.

--gemm_precision {fp32,bf16} picks the MFMA operand type; --runs N repeats
the graph-replay measurement on the same engine and prints the median and the
min-max range (the figures README's wide table quotes)."""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.gpu_microbench import make_engine  # noqa: E402


def rate(fn, n):
    t0 = time.perf_counter()
    fn(n)
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gemm_precision", default="fp32",
                    choices=["fp32", "bf16"])
    ap.add_argument("--runs", type=int, default=1)
    opts = ap.parse_args()
    eng = make_engine(batch=4096, hidden=1024, obs=17, act=6, cap=1000000,
                      gemm_precision=opts.gemm_precision)
    tag = "wide %s" % opts.gemm_precision
    eng.step(5)
    r_eager = rate(lambda n: eng.step(n), 100)
    print(f"{tag} step() uncaptured : {r_eager:7.1f} steps/s")
    eng.train_steps(8, steps_per_graph=8)      # capture
    rs = []
    for i in range(opts.runs):
        rs.append(rate(lambda n: eng.train_steps(n, steps_per_graph=8), 104))
        print(f"{tag} hipGraph replayed : {rs[-1]:7.1f} steps/s", flush=True)
    if opts.runs > 1:
        print(f"{tag} hipGraph replayed : median {statistics.median(rs):.1f} "
              f"min {min(rs):.1f} max {max(rs):.1f} steps/s "
              f"({opts.runs} runs)")


if __name__ == "__main__":
    main()
