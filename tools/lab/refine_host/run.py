#!/usr/bin/env python3
"""Run csrc_refine/refine_pose.hip on the host (tools/lab/eightpoint_host/shim.h: 256 fibres per workgroup, barriers and wave shuffles
emulated) under AddressSanitizer and UBSan and compare it with tests/_refine_ref.py.  No GPU is needed or used; shim.h says what this can
and cannot show.

    python tools/lab/refine_host/run.py

The program is built with g++ in a temporary directory; nothing is written into the tree."""
import os
import subprocess
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
warnings.simplefilter("ignore")
import host_emu                               # noqa: E402
from tests import _refine_ref as F              # noqa: E402

TMP = tempfile.mkdtemp(prefix="refine_host_")


exe = host_emu.build("csrc_refine/refine_pose.hip", HERE, TMP)
IN, OUT = os.path.join(TMP, "in.bin"), os.path.join(TMP, "out.bin")


def run(p0, x1, x2, w, tau, iters):
    n, P = x1.shape[:2]
    with open(IN, "wb") as f:
        np.array([n, P, iters, int(w is not None)], np.int32).tofile(f)
        p0.astype(np.float32).tofile(f); x1.astype(np.float32).tofile(f); x2.astype(np.float32).tofile(f)
        (w if w is not None else np.zeros((n, P))).astype(np.float32).tofile(f); np.broadcast_to(np.asarray(tau, np.float32), (n,)).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0")
    r = subprocess.run([exe, IN, OUT], capture_output=True, text=True, env=env)
    if r.returncode: print(r.stdout[-2000:], r.stderr[-3000:]); raise SystemExit(1)
    o = np.fromfile(OUT, np.float32)
    return o[:n * 7].reshape(n, 7), o[n * 7:n * 16].reshape(n, 3, 3), o[n * 16:n * 20].reshape(n, 4), o[n * 20:].reshape(n, P)


for P, n in [(5, 6), (8, 6), (9, 3), (255, 1), (256, 2), (257, 1), (513, 2), (1728, 1)]:
    x1, x2, _, truth = F.scenes_with_pose(n, P, seed=11)
    rng = np.random.default_rng(P)
    x1 = (x1 + 1e-3 * rng.standard_normal(x1.shape)).astype(np.float32)
    x2 = (x2 + 1e-3 * rng.standard_normal(x2.shape)).astype(np.float32)
    start = F.perturbed(truth, rng).astype(np.float32)
    for wt in (False, True):
        w = rng.uniform(0.05, 1.0, (n, P)).astype(np.float32) if wt else None
        for iters in (0, 1, 12):
            ref = F.refine_ref(start, x1, x2, w, 0.01, iters)
            f32 = F.refine_f32(start, x1, x2, w, 0.01, iters)
            pose, E, st, wo = run(start, x1, x2, w, 0.01, iters)
            print(P, n, wt, iters, "pose vs ref %.2e (f32 restatement %.2e)  E %.2e  cost rel %.1e  w_out %.1e  accepted %s / %s  kappa %.0f" % (
                np.abs(pose - ref.pose).max(), np.abs(f32.pose - ref.pose).max(), np.abs(E - ref.E).max(),
                (np.abs(st[:, :2] - ref.stat[:, :2]) / ref.stat[:, :2]).max(), np.abs(wo - ref.weights).max(), st[:, 2], ref.stat[:, 2],
                ref.kappa0.max()))
# degenerate problems and their neighbours
x1, x2, _, truth = F.scenes_with_pose(6, 300, seed=12)
w = np.random.default_rng(1).uniform(0.05, 1, (6, 300)).astype(np.float32)
w[1] = 0; w[1, [3, 50, 256, 299]] = 0.5; w[1, 7] = -1; w[3] = 0
start = F.perturbed(truth, np.random.default_rng(2)).astype(np.float32)
start[5, :3] = 0
pose, E, st, wo = run(start, x1, x2, w, 0.02, 3)
print("degenerate: pose kept", [np.array_equal(pose[b], start[b]) for b in (1, 3, 5)], "E zero", [not E[b].any() for b in (1, 3, 5)],
      "stat zero", [not st[b].any() for b in (1, 3, 5)], "w_out", [np.array_equal(wo[b], np.maximum(w[b], 0)) for b in (1, 3, 5)])
keep = [0, 2, 4]
ph, Eh, sh, wh = run(start[keep], x1[keep], x2[keep], w[keep], 0.02, 3)
print("healthy identical:", np.array_equal(ph, pose[keep]), np.array_equal(Eh, E[keep]), np.array_equal(sh, st[keep]), np.array_equal(wh, wo[keep]))
