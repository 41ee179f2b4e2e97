#!/usr/bin/env python3
"""Run csrc_eightpoint/eight_point.hip on the host (shim.h) under AddressSanitizer and UBSan and compare it with the fp64 reference of
tests/_eightpoint_ref.py on the inputs of tests/test_gpu_eightpoint.py.  No GPU is needed or used; see shim.h for what this can and
cannot show.

    python tools/lab/eightpoint_host/run.py

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
from tests import _eightpoint_ref as R          # noqa: E402
from tests import test_gpu_eightpoint as T      # noqa: E402

TMP = tempfile.mkdtemp(prefix="eightpoint_host_")


exe = host_emu.build("csrc_eightpoint/eight_point.hip", HERE, TMP)
IN, OUT = os.path.join(TMP, "in.bin"), os.path.join(TMP, "out.bin")


def run(x1, x2, w, tau, iters):
    n, P = x1.shape[:2]
    with open(IN, "wb") as f:
        np.array([n, P, iters, int(w is not None)], np.int32).tofile(f)
        x1.astype(np.float32).tofile(f); x2.astype(np.float32).tofile(f)
        (w if w is not None else np.zeros((n, P))).astype(np.float32).tofile(f); np.asarray(tau, np.float32).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0")
    r = subprocess.run([exe, IN, OUT], capture_output=True, text=True, env=env)
    if r.returncode: print(r.stdout[-2000:], r.stderr[-3000:]); raise SystemExit(1)
    o = np.fromfile(OUT, np.float32)
    return o[:n * 9].reshape(n, 3, 3), o[n * 9:n * 13].reshape(n, 4), o[n * 13:].reshape(n, P)
for P, n in [(8, 12), (9, 3), (255, 1), (256, 2), (257, 1), (513, 2), (1728, 1)]:
    for wt in (False, True):
        x1, x2, w = T.parity_inputs(P, n, wt) if (P, n) in T.PARITY_CASES else T.parity_inputs.__wrapped__(P, n, wt)
        Er, sr, _ = R.eight_point_ref(x1, x2, w)
        E, st, wo = run(x1, x2, w, np.ones(n), 0)
        sc = R.EPS32 / sr[:, 1]
        print(P, n, wt, "E ratio %.3g  strict-sign ratio %.3g  stat ratio %.3g  wsum rel %.1e  wout ok %s" % ((R.up_to_sign(E, Er) / sc).max(),
              (np.linalg.norm((E - Er).reshape(n, 9), axis=-1) / sc).max(), (np.abs(st[:, :3] - sr[:, :3]).max(-1) / sc).max(), (np.abs(st[:, 3] - sr[:, 3]) / sr[:, 3]).max(),
              np.array_equal(wo, w if w is not None else np.ones((n, P), np.float32))))
# IRLS
x1, x2, w0, tau = T.reweight_inputs()
E0, _, _ = run(x1, x2, w0, tau, 0)
E1, s1, w1 = run(x1, x2, w0, tau, 1)
want = w0.astype(np.float64) / (1 + R.sampson64(E0, x1, x2) / tau[:, None].astype(np.float64) ** 2)
print("one step w ratio", (np.abs(w1 - want) / w0 / (R.EPS32 / tau[:, None])).max())
E2, s2, _ = run(x1, x2, w1, tau, 0)
print("bit identical:", np.array_equal(E2, E1), np.array_equal(s2, s1))
a, b, Et, _ = R.noisy_scene(0)
Er, sr, wr = R.eight_point_ref(a, b, None, np.array([0.01]), 8)
E, st, wo = run(a, b, None, np.array([0.01]), 8)
print("irls8 E ratio", R.up_to_sign(E, Er)[0] / (R.EPS32 / sr[0, 1]), "dw", np.abs(wo - wr).max(), "stat", st, sr)
# degenerate
x1d, x2d, wd = np.repeat(x1, 2, 0).copy(), np.repeat(x2, 2, 0).copy(), np.repeat(w0, 2, 0).copy()
wd[1] = 0; wd[1, [3, 50, 100, 255, 256, 257, 299]] = 0.5; wd[1, 7] = -1; wd[3] = 0; x1d[5] = x1d[5, 17]
E, st, wo = run(x1d, x2d, wd, np.full(6, 0.02), 2)
print("degenerate E zero:", [not E[b].any() for b in (1, 3, 5)], "stat", st[[1, 3, 5]], "wout", [np.array_equal(wo[b], np.maximum(wd[b], 0)) for b in (1, 3, 5)])
Eh, sh, wh = run(x1d[[0, 2, 4]], x2d[[0, 2, 4]], wd[[0, 2, 4]], np.full(3, 0.02), 2)
print("healthy identical:", np.array_equal(Eh, E[[0, 2, 4]]), np.array_equal(sh, st[[0, 2, 4]]), np.array_equal(wh, wo[[0, 2, 4]]))
