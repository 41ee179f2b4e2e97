#!/usr/bin/env python3
"""Run csrc_submatch/submatch.hip on the host (tools/lab/eightpoint_host/shim.h plus shim_extra.h here: 256 fibres per workgroup, the
barrier and every wave shuffle emulated) as a stand-alone program under AddressSanitizer and UBSan, and assert of it what
tests/test_gpu_submatch.py asserts of the GPU (tests/_submatch_ref.py): the invalid-idx, border and corner table, the argmax centres,
packed and padded rows.  Every buffer has its exact size, so a read through an invalid idx or past a border is a sanitizer report.
No GPU is needed or used; shim.h says what this can and cannot show.

    python tools/lab/submatch_host/run.py

The program is built with g++ in a temporary directory; nothing is written into the tree."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(os.path.dirname(HERE), "eightpoint_host")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from tests import _submatch_ref as S           # noqa: E402

TMP = tempfile.mkdtemp(prefix="submatch_host_")


def build():
    k = open(os.path.join(ROOT, "rel_pose_amd", "csrc_submatch", "submatch.hip")).read()
    k = k.replace('#include "../csrc/common.h"', '#include "shim_extra.h"')
    k = re.sub(r'#include "../../include/(\w+\.h)"', r'#include "\1"', k)
    open(os.path.join(TMP, "kernel.cpp"), "w").write(k)
    exe = os.path.join(TMP, "emu")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", TMP, "-I", HERE, "-I", SHIM, "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "main.cpp"), "-o", exe])
    return exe


exe = build()
IN, OUT = os.path.join(TMP, "in.bin"), os.path.join(TMP, "out.bin")


def run(q, k, rlse, clse, idx, swap, single, radius, pad=0):
    Z, _, H, _ = q.shape
    ld = H * S.HD + pad
    with open(IN, "wb") as f:
        np.array([Z, H, ld, swap, single, radius, int(clse is not None)], np.int32).tofile(f)
        np.array([S.SCALE], np.float32).tofile(f)
        for t in (q, k):
            rows = np.full((Z * S.TOK, ld), np.nan, np.float32)          # the gap columns hold NaN: a kernel must not use them
            rows[:, :H * S.HD] = t.reshape(Z * S.TOK, H * S.HD)
            rows.tofile(f)
        rlse.astype(np.float32).tofile(f)
        (clse if clse is not None else np.zeros_like(rlse)).astype(np.float32).tofile(f)
        idx.astype(np.int32).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0")
    r = subprocess.run([exe, IN, OUT], capture_output=True, text=True, env=env)
    if r.returncode:
        print(r.stdout[-2000:], r.stderr[-3000:])
        raise SystemExit(1)
    o = np.fromfile(OUT, np.float32).reshape(2, Z, H, S.TOK, 4)
    return o[0], o[1]


worst = {}
for case in [c for c in S.CASES if c[1] == 1 or c[4] == 2]:
    kind, H, swap, single, radius, src = case
    q, k, rlse, clse = S.case_inputs(kind, H)
    idx = S.case_idx(case, q, k, rlse, clse)
    ref = S.submatch_ref(q, k, rlse, clse, idx, S.SCALE, swap, single, radius)
    f32 = S.submatch_f32(q, k, rlse, clse, idx, S.SCALE, swap, single, radius)
    win, quad = run(q, k, rlse, None if single else clse, idx, swap, single, radius, pad=0 if H == 3 else 12)
    assert np.isfinite(win).all() and np.isfinite(quad).all(), case
    r = S.bound_ratios((win, quad), ref, radius, built=kind == "built" and not swap)
    same = np.array_equal(win.view(np.int32), f32.win.view(np.int32)) and np.array_equal(quad.view(np.int32), f32.quad.view(np.int32))
    print(case, {n: round(v, 3) for n, v in r.items()}, "bit-identical to the restatement" if same else "")
    assert r["wxy"] <= S.C_WXY and r["wmass"] <= S.C_WMASS and r["wvar"] <= S.C_WVAR and r["curv"] <= S.C_CURV and r["pxy"] <= S.C_PXY, (case, r)
    if src == "table":          # the valid neighbours of the invalid entries: the same bits as in a run without them
        clean = S.table_idx(2, H, invalid=False)
        w2, q2 = run(q, k, rlse, None if single else clse, clean, swap, single, radius, pad=0 if H == 3 else 12)
        keep = ref.valid
        assert np.array_equal(win[keep].view(np.int32), w2[keep].view(np.int32)) and np.array_equal(quad[keep].view(np.int32), q2[keep].view(np.int32))
        assert int((~keep).sum()) == 5
    for n, v in r.items():
        worst[n] = max(worst.get(n, 0), v) if n != "compared" else min(worst.get(n, 1), v)
print("largest ratios:", worst)
print("all checks passed, no sanitizer report")
