#!/usr/bin/env python3
"""Run csrc_triangulate/triangulate.hip on the host (tools/lab/eightpoint_host/shim.h: 256 fibres per workgroup, barriers and wave shuffles
emulated) under AddressSanitizer and UBSan, as a stand-alone program with buffers of exact size, and assert of it what
tests/test_gpu_triangulate.py asserts of the GPU, at the same bounds (the checks live in tests/_triangulate_ref.py).  No GPU is needed or
used; shim.h says what this can and cannot show.

    python tools/lab/triangulate_host/run.py

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
from tests import _triangulate_ref as T         # noqa: E402

TMP = tempfile.mkdtemp(prefix="triangulate_host_")


exe = host_emu.build("csrc_triangulate/triangulate.hip", HERE, TMP, flags=("-fno-sanitize-recover=undefined",))
IN, OUT = os.path.join(TMP, "in.bin"), os.path.join(TMP, "out.bin")


def run(pose, x1, x2, w, tau, with_xc=True):
    n, P = x1.shape[:2]
    with open(IN, "wb") as f:
        np.array([n, P, int(w is not None), int(with_xc)], np.int32).tofile(f)
        np.asarray(pose, np.float32).tofile(f); x1.astype(np.float32).tofile(f); x2.astype(np.float32).tofile(f)
        (w if w is not None else np.zeros((n, P))).astype(np.float32).tofile(f); np.broadcast_to(np.asarray(tau, np.float32), (n,)).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0")
    r = subprocess.run([exe, IN, OUT], capture_output=True, text=True, env=env)
    if r.returncode or "ERROR" in r.stderr or "runtime error" in r.stderr: print(r.stdout[-2000:], r.stderr[-3000:]); raise SystemExit(1)
    o = np.fromfile(OUT, np.float32)
    sizes = [n * P * 3, n * P * 4, n * 4] + ([n * P * 4] if with_xc else [])
    assert o.size == sum(sizes)
    parts = np.split(o, np.cumsum(sizes)[:-1])
    return T.Structure(parts[0].reshape(n, P, 3), parts[1].reshape(n, P, 4), parts[3].reshape(n, P, 4) if with_xc else None, parts[2].reshape(n, 4))


# every case of the GPU test (the emulation runs one fibre at a time: the 130-problem batch takes the longest), with and without xc
worst = {}
for case in T.CASES:
    pose, x1, x2, w, tau = T.inputs(*case)
    ref = T.reference(*case)
    out = run(pose, x1, x2, w, tau)
    assert all(np.isfinite(a).all() for a in out), case
    r = T.ratios(out, ref, w, tau)
    share = T.share_ratio(out, ref, w, tau)
    assert T.within(r, share), (case, r, share)
    bare = run(pose, x1, x2, w, tau, with_xc=False)
    assert bare.xc is None and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip((out.X, out.aux, out.stat), (bare.X, bare.aux, bare.stat)))
    r["share"] = share
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)
    print(case, {k: float("%.3g" % v) for k, v in r.items()})
print("worst ratios of the host run:", {k: float("%.3g" % v) for k, v in worst.items()})
# degenerate problems and their neighbours: the clauses of the header
x1, x2, pose, _, _ = T.scenes(8, 40, 4, 3.0, 1e-3)
w = T.weights(8, 40, 1)
K = (T.clamp(w, 8, 40) > 0).sum(-1)
tau = np.full(8, T.TAU, np.float32)
pose[1, :3] = 0; pose[2, 3:] = 0; pose[3, 5] = np.nan; pose[4, 0] = np.inf; tau[5], tau[6] = 0, np.nan
w[7] = 0; w[7, 2], w[7, 5] = -3, np.nan
o = run(pose, x1, x2, w, tau)
assert all(np.isfinite(a).all() for a in o)
for b in range(1, 7):
    assert not o.X[b].any() and not o.aux[b].any() and not o.xc[b].any() and np.array_equal(o.stat[b], [0, 0, 0, K[b]]), b
assert o.X[0].any() and o.stat[0, 0] > 0 and o.X[7].any() and not o.stat[7].any()
print("degenerate slots: the documented outputs")
print("all checks passed, no sanitizer report")
