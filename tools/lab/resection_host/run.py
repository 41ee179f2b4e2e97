#!/usr/bin/env python3
"""Run csrc_resection/resection.hip on the host (tools/lab/eightpoint_host/shim.h: 256 fibres per workgroup, barriers and wave shuffles
emulated) under AddressSanitizer and UBSan, as a stand-alone program with buffers of exact size, and assert of it what
tests/test_gpu_resection.py asserts of the GPU, at the same bounds (the checks live in tests/_resection_ref.py).  No GPU is needed or
used; shim.h says what this can and cannot show.

    python tools/lab/resection_host/run.py

One program call runs the chain consensus -> refine (from the consensus winner) -> the same refinement in place.  The program is built
with g++ in a temporary directory; nothing is written into the tree."""
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
from tests import _resection_ref as T           # noqa: E402

TMP = tempfile.mkdtemp(prefix="resection_host_")


exe = host_emu.build("csrc_resection/resection.hip", HERE, TMP)
IN, OUT = os.path.join(TMP, "in.bin"), os.path.join(TMP, "out.bin")


def run(X, x, w, tau, seed, M, iters):
    n, P = x.shape[:2]
    with open(IN, "wb") as f:
        np.array([n, P, M, seed, int(w is not None), iters], np.int32).tofile(f)
        X.astype(np.float32).tofile(f); x.astype(np.float32).tofile(f)
        (w if w is not None else np.zeros((n, P))).astype(np.float32).tofile(f); np.broadcast_to(np.asarray(tau, np.float32), (n,)).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0")
    r = subprocess.run([exe, IN, OUT], capture_output=True, text=True, env=env)
    if r.returncode: print(r.stdout[-2000:], r.stderr[-3000:]); raise SystemExit(1)
    raw = np.fromfile(OUT, np.uint8)
    sizes = [n * 7, n * 4, n * P, n * M * 7, n * M, n * 7, n * 4, n * P, n * 7]
    nf = sum(sizes)
    o, i = raw[:4 * nf].view(np.float32), raw[4 * nf:].view(np.int32)
    pose, st, wo, hp, hc, rpose, rst, rw, apose = np.split(o, np.cumsum(sizes)[:-1])
    cons = T.Consensus(pose.reshape(n, 7), i[:n], st.reshape(n, 4), wo.reshape(n, P), hp.reshape(n, M, 7), hc.reshape(n, M),
                       i[n:n + n * M].reshape(n, M), i[n + n * M:].reshape(n, M, 3), None)
    return cons, (rpose.reshape(n, 7), rst.reshape(n, 4), rw.reshape(n, P), apose.reshape(n, 7))


# the consensus at the GPU test's cases (the large ones left to the GPU: the emulation runs one fibre at a time), then the refinement
# behind it against the reference run on the program's OWN intermediate result
for case in [c for c in T.CASES if c[1] * c[2] * c[3] <= 40000]:
    kind, n, P, M, wt = case
    X, x, w = T.inputs(*case)
    ref = T.reference(*case)
    cons, (rpose, rst, rw, apose) = run(X, x, w, T.TAU, T.SEED, M, 10)
    assert all(np.isfinite(a).all() for a in cons[:8]) and np.array_equal(cons.samples, ref.samples), case
    print(case, T.check_consensus(cons, ref, X, x, w))
    rr = T.refine(X, x, w, T.TAU, cons.pose, 10)
    r = T.refine_ratios(rpose, rst, rw, rr, X, x, w)
    assert r["pose"] <= T.C_REFINE[10] and r["unit"] <= T.C_UNIT and r["cost"] <= T.C_COST and r["w"] <= T.C_W, (case, r)
    assert np.array_equal(apose, rpose), case                      # the aliased call
    print("   refine", r)
# degenerate problems and their neighbours
X, x, _ = T.exact_rows(6, 40, 12)
w = np.random.default_rng(1).uniform(0.05, 1, (6, 40)).astype(np.float32)
w[1] = 0; w[1, [9, 11]] = 0.5; w[1, 7] = -1; w[1, 8] = np.nan
tau = np.full(6, T.TAU, np.float32); tau[5] = 0
cons, (rpose, rst, rw, apose) = run(X, x, w, tau, 3, 70, 3)
wc = C.clamp(w, 6, 40, np.float32)
for b, K in ((1, 2), (5, 40)):
    assert not cons.pose[b].any() and cons.best[b] == -1 and np.array_equal(cons.stat[b], [0, 0, 0, K]), (b, cons.best[b], cons.stat[b])
    assert np.array_equal(cons.weights[b], wc[b]) and not cons.hyp_pose[b].any() and bool((cons.hyp_cost[b] == np.float32(C.FLT_MAX)).all()), b
    assert not cons.hyp_count[b].any()
    assert not rpose[b].any() and np.array_equal(rst[b], [0, 0, 0, K]) and np.array_equal(rw[b], wc[b])
assert not cons.samples[1].any() and np.array_equal(cons.samples, T.sample_rows3(w, 6, 40, 3, 70)[1])
assert all(np.isfinite(a).all() for a in (cons.pose, cons.stat, cons.weights, cons.hyp_pose, cons.hyp_cost, rpose, rst, rw))
print("degenerate slots: the documented outputs")
print("all checks passed, no sanitizer report")
