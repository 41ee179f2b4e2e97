#!/usr/bin/env python3
"""Run csrc/svd3x3.h, csrc/geom.hip and csrc/se3loss.hip on the host (shim.h) under AddressSanitizer and UBSan, on the inputs and against
the bounds of tests/test_gpu_geometry_edges.py (tests/_geometry_edges.py).  No GPU is needed or used; shim.h says what this can and cannot
show.

    python tools/lab/geom_host/run.py              the sources of the working tree
    python tools/lab/geom_host/run.py --rev HEAD~1 the sources of that commit (git show), against the same bounds

Every check prints its worst figure and ok / FAIL; the exit status is the number of failed checks.
The program is built with g++ in a temporary directory; nothing is written into the tree."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")
from oracle import svd3x3_oracle as SO          # noqa: E402
from tests import _eightpoint_ref as R          # noqa: E402
from tests import _geometry_edges as G          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rev", default=None, help="take the three kernel sources from this commit instead of the working tree")
args = ap.parse_args()
TMP = tempfile.mkdtemp(prefix="geom_host_")


def source(rel):
    if args.rev:
        return subprocess.check_output(["git", "-C", ROOT, "show", "%s:%s" % (args.rev, rel)], text=True)
    return open(os.path.join(ROOT, rel)).read()


def build():
    svd = source("rel_pose_amd/csrc/svd3x3.h").replace('#include "common.h"', '#include "shim.h"')
    k = source("rel_pose_amd/csrc/geom.hip") + "\n" + source("rel_pose_amd/csrc/se3loss.hip")
    k = k.replace('#include "common.h"', '#include "shim.h"')
    k = re.sub(r'#include "../../include/(\w+\.h)"', r'#include "\1"', k)
    open(os.path.join(TMP, "svd3x3.h"), "w").write(svd)
    open(os.path.join(TMP, "kernel.cpp"), "w").write(k)
    exe = os.path.join(TMP, "emu")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", TMP,
                           "-I", HERE, "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "main.cpp"), "-o", exe])
    return exe


exe = build()
IN, OUT = os.path.join(TMP, "in.bin"), os.path.join(TMP, "out.bin")
failed = 0


def call(op, n, P, *arrays):
    with open(IN, "wb") as f:
        np.array([op, n, P], np.int32).tofile(f)
        for a in arrays:
            np.ascontiguousarray(a, np.float32).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0")
    r = subprocess.run([exe, IN, OUT], capture_output=True, text=True, env=env)
    if r.returncode:
        print(r.stdout[-2000:], r.stderr[-3000:])
        raise SystemExit(100)
    return np.fromfile(OUT, np.float32)


def check(name, ok, text):
    global failed
    failed += not ok
    print("%-44s %s  %s" % (name, "ok  " if ok else "FAIL", text))


def svd(A):
    n = len(A)
    o = call(0, n, 0, A)
    return o[:9 * n].reshape(n, 3, 3), o[9 * n:12 * n].reshape(n, 3), o[12 * n:].reshape(n, 3, 3)


# ------------------------------------------------------------------------------------------------ svd
print("sources:", args.rev or "working tree")
with np.errstate(all="ignore"):
    for tag, A in list(G.svd_special().items()) + [("zero", np.zeros((4, 3, 3), np.float32))] + [("generic x %g" % s, G.svd_generic() * np.float32(s)) for s in (1, 1e15, 1e-15, 1e30, 1e-30)]:
        e_s, e_rec, e_orth, ordered = G.svd_errors(A, *svd(A))
        worst = np.nan_to_num(max(e_s, e_rec, e_orth), nan=np.inf)
        check("svd " + tag, worst < 3e-6 and ordered, "values %.2e  reconstruction %.2e  orthogonality %.2e" % (e_s, e_rec, e_orth))
    A0 = G.svd_generic()
    U0, S0, V0 = svd(A0)
    for lo, hi in ((-20, 20), (-100, 100)):
        bad = []
        for k in range(lo, hi + 1):
            U, S, V = svd(np.ldexp(A0, k))
            if not (np.array_equal(U, U0) and np.array_equal(V, V0) and np.array_equal(S, np.ldexp(S0, k))):
                bad.append(k)
        check("svd scale equivariance, k = %d .. %d" % (lo, hi), not bad, "bit-identical at every k" if not bad else "differs at k = %s" % bad)

# ------------------------------------------------------------------------------------------------ decode
branches = np.zeros(4, int)
for kind in R.WIDE_KINDS:
    E, x1, x2, pose = G.decode_inputs(kind)
    n, P = x1.shape[:2]
    o = call(1, n, P, E, x1, x2)
    out, count = o[:7 * n].reshape(n, 7), o[7 * n:]
    ang, cos_t = G.decode_errors(out, pose)
    Ro, to, co = SO.decode_essential(E[:40], x1[:40], x2[:40])
    dR = np.abs(SO.rotation_from_quat(out[:40, 3:]) - Ro).max()
    dt = np.abs(out[:40, :3] - to).max()
    ok = ang.max() < 2e-3 and cos_t.min() > 1 - 1e-6 and (count == P).all() and dR < 5e-4 and dt < 5e-4 and (co == P).all() and (out[:, 6] >= 0).all()
    check("decode " + kind, ok, "angle %.2e  1 - cos_t %.1e  count %d..%d  oracle R %.1e t %.1e" % (ang.max(), 1 - cos_t.min(), count.min(), count.max(), dR, dt))
    branches += np.bincount([R.shepperd_branch(r) for r in SO.rotation_from_quat(pose[:, 3:])], minlength=4)
check("decode: every quaternion branch taken", branches.min() >= 20, "trace / R00 / R11 / R22: %s" % branches)

# ------------------------------------------------------------------------------------------------ loss
Ps, Gs, grid = G.loss_sweep()
ref = G.loss_reference()
B = len(grid)
o = call(2, B, 0, Ps.numpy(), Gs.numpy())
dmean = o[2:].reshape(2, B, 14).astype(np.float64) * 2 * B
vals = np.array([call(2, 1, 0, Ps[b].numpy(), Gs[b].numpy())[:2] for b in range(B)], np.float64)
finite = bool(np.isfinite(o).all() and np.isfinite(vals).all())
r_rot, r_tr, r_vtr, r_vrot, kink = G.loss_ratios(dmean[0], dmean[1], vals[:, 0], vals[:, 1], ref)
check("loss: finite", finite, "%d pairs, the half-turn rows included" % B)
for name, r, C in (("rotation gradient", r_rot, G.C_ROT), ("translation gradient", r_tr, G.C_TR), ("|tau| values", r_vtr, G.C_VAL_TR),
                   ("|phi| values", r_vrot, G.C_VAL_ROT)):
    k = int(np.nanargmax(r))
    check("loss " + name, bool(np.nanmax(r) <= C), "ratio %.3g (C %.3g) at theta %.3g |tau| %.3g" % (np.nanmax(r), C, grid[k, 0], grid[k, 1]))
check("loss kink and cut rows", kink <= 1 + 1e-5, "largest gradient entry over its bound %.3g" % kink)
print("%d checks failed" % failed)
sys.exit(failed)
