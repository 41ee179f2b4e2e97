#!/usr/bin/env python3
"""Run csrc_homography/homography.hip on the host (tools/lab/eightpoint_host/shim.h: 256 fibres per workgroup, barriers and wave shuffles
emulated) under AddressSanitizer and UBSan, as a stand-alone program with buffers of exact size, and assert of it what
tests/test_gpu_homography.py asserts of the GPU, at the same bounds (the checks live in tests/_homography_ref.py).  No GPU is needed or
used; shim.h says what this can and cannot show.

    python tools/lab/homography_host/run.py

One program call runs the chain consensus -> refine (from the consensus winner) -> decomposition (of the refined H).  The program is
built with g++ in a temporary directory; nothing is written into the tree."""
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
from tests import _homography_ref as H          # noqa: E402

TMP = tempfile.mkdtemp(prefix="homography_host_")


exe = host_emu.build("csrc_homography/homography.hip", HERE, TMP)
IN, OUT = os.path.join(TMP, "in.bin"), os.path.join(TMP, "out.bin")


def run(x1, x2, w, tau, seed, M, iters):
    n, P = x1.shape[:2]
    with open(IN, "wb") as f:
        np.array([n, P, M, seed, int(w is not None), iters], np.int32).tofile(f)
        x1.astype(np.float32).tofile(f); x2.astype(np.float32).tofile(f)
        (w if w is not None else np.zeros((n, P))).astype(np.float32).tofile(f); np.broadcast_to(np.asarray(tau, np.float32), (n,)).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0")
    r = subprocess.run([exe, IN, OUT], capture_output=True, text=True, env=env)
    if r.returncode: print(r.stdout[-2000:], r.stderr[-3000:]); raise SystemExit(1)
    raw = np.fromfile(OUT, np.uint8)
    sizes = [n * 9, n * 4, n * P, n * M * 9, n * M, n * 9, n * 4, n * P, n * 28, n * 12, n * 16]
    nf = sum(sizes)
    o, i = raw[:4 * nf].view(np.float32), raw[4 * nf:].view(np.int32)
    Hm, st, wo, hH, hc, rH, rst, rw, pose, nrm, cs = np.split(o, np.cumsum(sizes)[:-1])
    cons = H.Consensus(Hm.reshape(n, 3, 3), i[:n], st.reshape(n, 4), wo.reshape(n, P), hH.reshape(n, M, 3, 3), hc.reshape(n, M),
                       i[n:n + n * M * 4].reshape(n, M, 4), None)
    return cons, (rH.reshape(n, 3, 3), rst.reshape(n, 4), rw.reshape(n, P)), (pose.reshape(n, 4, 7), nrm.reshape(n, 4, 3), cs.reshape(n, 4, 4),
                                                                               i[n + n * M * 4:].reshape(n, 2))


# the consensus at the GPU test's cases (the large ones left to the GPU: the emulation runs one fibre at a time), then the refinement and the
# decomposition behind it against the reference run on the program's OWN intermediate results
for case in [c for c in H.CASES if c[1] * c[3] <= 1024 or c[0] == "noisy"][:9] + [("noisy", 2, 576, 256, False)]:
    kind, n, P, M, wt = case
    x1, x2, w = H.inputs(*case)
    ref = H.reference(*case) if case in H.CASES else H.consensus(x1, x2, w, H.TAU, H.SEED, M)
    cons, (rH, rst, rw), (pose, nrm, cs, pick) = run(x1, x2, w, H.TAU, H.SEED, M, 10)
    assert all(np.isfinite(a).all() for a in cons[:7]) and np.array_equal(cons.samples, ref.samples), case
    print(case, H.check_consensus(cons, ref, x1, x2, w))
    rr = H.refine(x1, x2, w, H.TAU, cons.H, 10)
    r = H.refine_ratios(rH, rst, rw, rr, x1, x2, w)
    assert r["H"] <= H.C_REFINE_H[10] and r["cost"] <= H.C_COST and r["w"] <= H.C_W, (case, r)
    inp = (rH, x1, x2, w)
    d = H.decompose_ratios(H.Poses(pose, nrm, cs, pick, None), H.decompose(rH, x1, x2, w, H.TAU), inp)
    assert d["pose"].max() <= H.C_DECOMPOSE and d["cost"].max() <= H.C_DECOMPOSE_COST and d["vis"].max() <= H.C_VIS, (case, d)
    print("   refine", r, "decompose pose %.3g cost %.3g vis %.3g" % (d["pose"].max(), d["cost"].max(), d["vis"].max()))
# degenerate problems and their neighbours
x1, x2 = H.exact_scenes(6, 40, 12)[:2]
w = np.random.default_rng(1).uniform(0.05, 1, (6, 40)).astype(np.float32)
w[1] = 0; w[1, [3, 5, 9]] = 0.5; w[1, 7] = -1; w[1, 8] = np.nan
tau = np.full(6, 0.02, np.float32); tau[5] = 0
cons, (rH, rst, rw), (pose, nrm, cs, pick) = run(x1, x2, w, tau, 3, 70, 3)
wc = C.clamp(w, 6, 40, np.float32)
for b, K in ((1, 3), (5, 40)):
    assert not cons.H[b].any() and cons.best[b] == -1 and np.array_equal(cons.stat[b], [0, 0, 0, K]), (b, cons.best[b], cons.stat[b])
    assert np.array_equal(cons.weights[b], wc[b]) and not cons.hyp_H[b].any() and bool((cons.hyp_cost[b] == np.float32(C.FLT_MAX)).all()), b
    assert not rH[b].any() and np.array_equal(rst[b], [0, 0, 0, K]) and np.array_equal(rw[b], wc[b])
    assert not pose[b].any() and not cs[b].any() and pick[b].tolist() == [-1, -1]
assert not cons.samples[1].any() and np.array_equal(cons.samples, H.sample_rows4(w, 6, 40, 3, 70)[1])
assert all(np.isfinite(a).all() for a in (cons.H, cons.stat, cons.weights, cons.hyp_H, cons.hyp_cost, rH, rst, rw, pose, nrm, cs))
print("degenerate slots: the documented outputs")
print("all checks passed, no sanitizer report")
