#!/usr/bin/env python3
"""Run csrc_fivepoint/five_point.hip on the host (tools/lab/eightpoint_host/shim.h: 256 fibres per workgroup, barriers and wave shuffles
emulated) under AddressSanitizer and UBSan, as a stand-alone program, and assert of it what tests/test_gpu_fivepoint.py asserts of
the GPU (the checks live in tests/_fivepoint_ref.py).  No GPU is needed or used; shim.h says what this can and cannot show.  The
kernel shuffles no fp64 value, so the shim needs no extension.

    python tools/lab/fivepoint_host/run.py

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
from tests import _consensus_ref as C           # noqa: E402
from tests import _eightpoint_ref as R          # noqa: E402
from tests import _fivepoint_ref as F           # noqa: E402

TMP = tempfile.mkdtemp(prefix="fivepoint_host_")


exe = host_emu.build("csrc_fivepoint/five_point.hip", HERE, TMP)
IN, OUT = os.path.join(TMP, "in.bin"), os.path.join(TMP, "out.bin")


def run(x1, x2, w, tau, seed, M):
    n, P = x1.shape[:2]
    with open(IN, "wb") as f:
        np.array([n, P, M, seed, int(w is not None)], np.int32).tofile(f)
        x1.astype(np.float32).tofile(f); x2.astype(np.float32).tofile(f)
        (w if w is not None else np.zeros((n, P))).astype(np.float32).tofile(f); np.broadcast_to(np.asarray(tau, np.float32), (n,)).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0")
    r = subprocess.run([exe, IN, OUT], capture_output=True, text=True, env=env)
    if r.returncode: print(r.stdout[-2000:], r.stderr[-3000:]); raise SystemExit(1)
    raw = np.fromfile(OUT, np.uint8)
    sizes = [n * 9, n * 4, n * P, n * M * 90, n * M * 10]
    nf = sum(sizes)
    o, i = raw[:4 * nf].view(np.float32), raw[4 * nf:].view(np.int32)
    E, st, wo, hE, hc = np.split(o, np.cumsum(sizes)[:-1])
    return F.Consensus5(E.reshape(n, 3, 3), i[:2 * n].reshape(n, 2), st.reshape(n, 4), wo.reshape(n, P), hE.reshape(n, M, 10, 3, 3),
                        hc.reshape(n, M, 10), i[2 * n:].reshape(n, M, 5))


n, P, M = F.ROOT_SHAPE
for kind in F.ROOT_CASES:
    x1, x2 = F.root_inputs(kind)
    got = run(x1, x2, None, F.TAU, F.SEED, M)
    assert all(np.isfinite(a).all() for a in got[:6]), kind
    F.check_roots(kind, got, "host ")
    print(kind, F.check_consensus(got, x1, x2, None, F.TAU))
    F.check_winner(kind, got)
# weights, sizes off the tile, more than one chunk
for n_, P_, M_ in [(1, 5, 1), (2, 9, 257), (1, 300, 40)]:
    x1, x2, _ = R.scenes(n_, P_, seed=11)
    x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
    w = np.random.default_rng(P_).uniform(0.05, 1.0, (n_, P_)).astype(np.float32)
    if P_ > 16:
        w[:, ::3] = 0
    got = run(x1, x2, w, 0.01, 1, M_)
    assert np.array_equal(got.samples, F.sample_rows5(w, n_, P_, 1, M_)[1])
    print((n_, P_, M_), F.check_consensus(got, x1, x2, w, 0.01))
# degenerate problems and their neighbours
x1, x2, _ = R.scenes(6, 40, seed=12)
x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
w = np.random.default_rng(1).uniform(0.05, 1, (6, 40)).astype(np.float32)
w[1] = 0; w[1, [3, 5, 9, 20]] = 0.5; w[1, 7] = -1; w[1, 8] = np.nan
w[3, ::2] = np.nan; w[3, 1::4] = -1
tau = np.full(6, 0.02, np.float32); tau[5] = 0
got = run(x1, x2, w, tau, 3, 70)
wc = C.clamp(w, 6, 40, np.float32)
for b, K in ((1, 4), (5, 40)):
    assert not got.E[b].any() and np.array_equal(got.best[b], [-1, -1]) and np.array_equal(got.stat[b], [0, 0, 0, K]), (b, got.best[b], got.stat[b])
    assert np.array_equal(got.weights[b], wc[b]) and not got.hyp_E[b].any() and bool((got.hyp_cost[b] == np.float32(C.FLT_MAX)).all()), b
assert not got.samples[1].any() and np.array_equal(got.samples, F.sample_rows5(w, 6, 40, 3, 70)[1])
assert all(np.isfinite(a).all() for a in got[:6]) and bool((got.best[[0, 2, 3, 4]] >= 0).all()) and got.stat[3, 3] == 10
print("degenerate slots: the documented outputs")
print("all checks passed, no sanitizer report")
