#!/usr/bin/env python3
"""Time rp_pose_covariance (include/relpose_covariance.h) next to the refinement it follows, in the same run.

    python tools/covariance_time.py [--reps 30] [--warmup 5] [--out profiles/covariance_time.txt]

At (n, P) = (10, 576) and (128, 1728), the calibration scenes of tests/_covariance_ref.py (sigma = 1e-3, 30 % wrong matches, tau = 10
sigma, the true poses): rp_pose_covariance with and without `normal`; alongside, on the same rows, rp_refine_pose with iters = 0 (the
scorer: one pass with a three-value reduction) and iters = 1 (one Levenberg-Marquardt iteration more: two passes, a 20-value reduction,
a 5 x 5 solve) -- the expectation to check is "about one refinement iteration", i.e. refine(1) - refine(0).  After `warmup` calls of the
same shape every one of `reps` calls is timed by a pair of device events of its own; the median is what is quoted, the minimum and the
maximum show the spread.  No ratio is promised: what comes out is recorded.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(10, 576), (128, 1728)]
SIGMA, TAU, WRONG = 1e-3, 1e-2, 0.3


def scenes(n, P):
    import numpy as np
    import torch
    from tests import _covariance_ref as C
    rng = np.random.default_rng([11, n, P])
    geoms = [C.mc_geometry(100 + b, P) for b in range(n)]
    draws = [C.mc_draw(g, rng, SIGMA, WRONG) for g in geoms]
    f = lambda a: torch.from_numpy(np.stack(a).astype(np.float32)).cuda()      # noqa: E731
    return f([g.pose for g in geoms]), f([d[0] for d in draws]), f([d[1] for d in draws])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("covariance_time needs a GPU")
    from rel_pose_amd import covariance, refine
    from tools.fivepoint_time import timed
    result = {"reps": args.reps, "warmup": args.warmup, "sigma": SIGMA, "tau": TAU, "wrong": WRONG, "device": torch.cuda.get_device_name(0), "rows": []}
    for n, P in SHAPES:
        pose0, x1, x2 = scenes(n, P)
        tau = torch.full((n,), TAU, device="cuda")
        pose = refine.refine_pose(pose0, x1, x2, None, tau=tau, iters=10).pose
        pc = covariance.pose_covariance(pose, x1, x2, None, tau=tau)
        row = {"n": n, "P": P, "status_ok": int((pc.stat[:, 0] == 1).sum()), "sd_rot_deg_mean": float(covariance.rotation_sd_deg(pc).mean()),
               "sd_dir_deg_mean": float(covariance.direction_sd_deg(pc).mean())}
        for name, fn in (("rp_pose_covariance", lambda: covariance.pose_covariance(pose, x1, x2, None, tau=tau)),
                         ("rp_pose_covariance_normal", lambda: covariance.pose_covariance(pose, x1, x2, None, tau=tau, return_normal=True)),
                         ("rp_refine_pose_0", lambda: refine.refine_pose(pose, x1, x2, None, tau=tau, iters=0)),
                         ("rp_refine_pose_1", lambda: refine.refine_pose(pose, x1, x2, None, tau=tau, iters=1))):
            med, lo, hi = timed(fn, args.warmup, args.reps)
            row[name + "_ms"] = {"median": med, "min": lo, "max": hi}
        row["one_refine_iteration_ms"] = row["rp_refine_pose_1_ms"]["median"] - row["rp_refine_pose_0_ms"]["median"]
        row["covariance_over_refine_1"] = row["rp_pose_covariance_ms"]["median"] / row["rp_refine_pose_1_ms"]["median"]
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        if args.out:                                                   # (after every shape: what is measured is kept)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
