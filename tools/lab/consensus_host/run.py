#!/usr/bin/env python3
"""Run csrc_consensus/consensus.hip on the host (tools/lab/eightpoint_host/shim.h: 256 fibres per workgroup, barriers and wave shuffles
emulated) under AddressSanitizer and UBSan and assert of it what tests/test_gpu_consensus.py asserts of the GPU (tests/_consensus_ref.py).  No GPU is needed or used; shim.h says what this
can and cannot show.

    python tools/lab/consensus_host/run.py

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

TMP = tempfile.mkdtemp(prefix="consensus_host_")


exe = host_emu.build("csrc_consensus/consensus.hip", HERE, TMP)
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
    nf = n * 9 + n * 4 + n * P + n * M * 9 + n * M
    o, i = raw[:4 * nf].view(np.float32), raw[4 * nf:].view(np.int32)
    return C.Consensus(o[:n * 9].reshape(n, 3, 3), i[:n], o[n * 9:n * 13].reshape(n, 4), o[n * 13:n * 13 + n * P].reshape(n, P),
                       o[n * 13 + n * P:n * 13 + n * P + n * M * 9].reshape(n, M, 3, 3), o[nf - n * M:].reshape(n, M), i[n:].reshape(n, M, 8), None)


def compare(tag, kind, x1, x2, w, tau, seed, M):
    """the emulated kernel against the fp64 reference: what tests/test_gpu_consensus.py asserts of the GPU, at the same constants"""
    n, P = x1.shape[:2]
    ref, f32 = C.consensus_ref(x1, x2, w, tau, seed, M), C.consensus_f32(x1, x2, w, tau, seed, M)
    got = run(x1, x2, w, tau, seed, M)
    r, rf = C.ratios(got, ref, x1, x2, w, tau), C.ratios(f32, ref, x1, x2, w, tau)
    print(tag, "compared %.3f" % r["compared"], " ".join(" %s ratio %.3g (restatement %.3g)" % (k, r[k], rf[k]) for k in ("E", "E_gain", "cost", "w", "shift")),
          " best", got.best[:4], ref.best[:4])
    assert np.array_equal(got.samples, ref.samples), tag
    assert all(np.isfinite(a).all() for a in got[:6]), tag
    assert r["compared"] >= 0.95 and r["compared_gain"] >= 0.95, tag
    assert r["E_gain"] <= C.C_E_GAIN and r["E"] <= C.C_E[kind] and r["cost"] <= C.C_COST and r["w"] <= C.C_W and r["shift"] <= C.C_SHIFT, (tag, r)
    pick = np.arange(n)
    assert np.array_equal(got.best, got.hyp_cost.argmin(-1)), tag
    assert np.array_equal(got.E.view(np.int32), got.hyp_E[pick, got.best].view(np.int32)), tag
    assert np.array_equal(got.stat[:, 0].view(np.int32), got.hyp_cost[pick, got.best].view(np.int32)), tag
    assert np.array_equal(got.stat[:, 2:], ref.stat[:, 2:]), tag
    share, edge = C.share64(got.E, x1, x2, C.clamp(w, n, P), np.full(n, tau))
    assert bool((np.abs(got.stat[:, 1] - share) <= edge + 4e-6).all()), tag


for n, P, M in [(1, 8, 1), (3, 9, 257), (2, 257, 256), (5, 64, 64), (1, 1728, 30)]:
    x1, x2, _ = R.scenes(n, P, seed=11)
    x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
    for wt in (False, True):
        w = np.random.default_rng(P).uniform(0.05, 1.0, (n, P)).astype(np.float32) if wt else None
        if wt and P > 16:
            w[:, ::3] = 0
        compare("%d %d %d %s" % (n, P, M, wt), "exact", x1, x2, w, 0.01, 1, M)
# two of the noisy scenes with half of the matches wrong (the fibres make a whole batch of 1024 hypotheses slow: 64 here)
x1, x2, _, w = C.noisy_batch(0.5, True, seeds=(0, 1))
compare("noisy 2 576 64 weighted", "noisy", x1, x2, w, 0.01, 1, 64)
# degenerate problems and their neighbours
x1, x2, _ = R.scenes(6, 40, seed=12)
x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
w = np.random.default_rng(1).uniform(0.05, 1, (6, 40)).astype(np.float32)
w[1] = 0; w[1, [3, 5, 9, 20, 30, 38, 39]] = 0.5; w[1, 7] = -1; w[1, 8] = np.nan
x1[3] = x1[3, 17]
tau = np.full(6, 0.02, np.float32); tau[5] = 0
got = run(x1, x2, w, tau, 3, 70)
wc = C.clamp(w, 6, 40, np.float32)
for b, K in ((1, 7), (3, 40), (5, 40)):
    assert not got.E[b].any() and got.best[b] == -1 and np.array_equal(got.stat[b], [0, 0, 0, K]), (b, got.best[b], got.stat[b])
    assert np.array_equal(got.weights[b], wc[b]) and not got.hyp_E[b].any() and bool((got.hyp_cost[b] == np.float32(C.FLT_MAX)).all()), b
assert not got.samples[1].any() and np.array_equal(got.samples, C.sample_rows(w, 6, 40, 3, 70)[1])
assert all(np.isfinite(a).all() for a in got[:6]) and bool((got.best[[0, 2, 4]] >= 0).all())
print("degenerate slots: the documented outputs")
print("all checks passed, no sanitizer report")
