#!/usr/bin/env python3
"""rp_emm_matches (the EMM readout, csrc_readout/emm_readout.hip) next to rp_emm_stats without s_out on the same q | k | v at 128 images:
both execute the same q k^T MFMAs.  Meant to run under `rocprofv3 --kernel-trace --stats -- python tools/readout_time.py`, whose kernel
statistics are the measurement (profiles/readout_kernel_stats.txt); the event timings printed here include the launch path."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rel_pose_amd import ops, readout, _lib
_lib.load()
_lib.load_readout()
Z = 128
torch.manual_seed(0)
qkv = torch.randn(Z * 576, 576, device="cuda")


def timeit(fn, n=20, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3

rlse, clse = ops.emm_stats(qkv, Z)
for rnd in range(2):      # alternating, so that both see the same machine
    print("emm_stats (no s_out)     %8.1f us" % timeit(lambda: ops.emm_stats(qkv, Z)))
    print("emm_matches rows         %8.1f us" % timeit(lambda: readout.emm_matches(qkv, rlse, clse, Z)))
    print("emm_matches columns      %8.1f us" % timeit(lambda: readout.emm_matches(qkv, rlse, clse, Z, swap=True)))
Zd = 16
print("emm_matches rows + dense A at %d images %8.1f us" % (Zd, timeit(lambda: readout.emm_matches(qkv[:Zd * 576], rlse[:Zd], clse[:Zd], Zd, dense=True), n=10)))
