#!/usr/bin/env python3
"""Time the two entry points of include/relpose_rotation.h next to the homography library's, in the same run.

    python tools/rotation_time.py [--reps 30] [--warmup 5] [--out profiles/rotation_time.txt]

At (n, P, M) = (1, 576, 256), (10, 576, 256) and (128, 1728, 256), pure-rotation scenes with a third of the matches replaced by noise:
rp_rotation_consensus and rp_rotation_refine (10 iterations, from the consensus winner); alongside, on the same inputs,
rp_homography_consensus and rp_homography_refine (10 iterations, from ITS winner).  Then, on one pair of images through a randomly
initialised model, ViTEss.rotation_from_matches against ViTEss.planar_pose_from_matches and the readout they share.  After `warmup`
calls of the same shape every one of `reps` calls is timed by a pair of device events of its own; the median is what is quoted, the
minimum and the maximum show the spread.  No ratio is promised: what comes out is recorded.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1, 576, 256), (10, 576, 256), (128, 1728, 256)]
TAU, SEED = 0.01, 1


def scenes(n, P, seed=0):
    """pure rotations of up to 0.5 rad, float32 on the CPU: x1 uniform in |xy| <= 0.55, x2 its image plus Gaussian noise 1e-3"""
    import torch
    g = torch.Generator().manual_seed(seed)
    axis = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    ang = torch.rand(n, generator=g, dtype=torch.float64) * 0.4 + 0.1
    k = torch.zeros(n, 3, 3, dtype=torch.float64)
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0], k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = torch.eye(3, dtype=torch.float64) + torch.sin(ang)[:, None, None] * k + (1 - torch.cos(ang))[:, None, None] * (k @ k)
    xy = torch.rand(n, P, 2, generator=g, dtype=torch.float64) * 1.1 - 0.55
    m = torch.cat([xy, torch.ones(n, P, 1, dtype=torch.float64)], -1) @ R.transpose(1, 2)
    x2 = m[..., :2] / m[..., 2:] + 1e-3 * torch.randn(n, P, 2, generator=g, dtype=torch.float64)
    return xy.float(), x2.float(), torch.rand(n, P, generator=g) * 0.95 + 0.05


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rotation_time needs a GPU")
    from oracle import relpose_oracle as O
    from rel_pose_amd import homography, rotation
    from tests.test_gpu_memory_contract import _model
    from tools.fivepoint_time import timed
    result = {"reps": args.reps, "warmup": args.warmup, "tau": TAU, "seed": SEED, "device": torch.cuda.get_device_name(0), "rows": [], "chains": {}}

    def save():
        if args.out:                                                   # (after every shape: what is measured is kept)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
    for n, P, M in SHAPES:
        x1, x2, w = (t.cuda() for t in scenes(n, P))
        x2[:, ::3] = torch.rand_like(x2[:, ::3]) * 1.2 - 0.6                         # a third of the matches wrong
        tau = torch.full((n,), TAU, device="cuda")
        c = rotation.rotation_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED)
        r = rotation.rotation_refine(x1, x2, w, c.R, tau=tau, iters=10)
        hc = homography.homography_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED)
        hr = homography.homography_refine(x1, x2, w, hc.H, tau=tau, iters=10)
        row = {"n": n, "P": P, "M": M}
        for name, fn in (("rp_rotation_consensus", lambda: rotation.rotation_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED, return_weights=True)),
                         ("rp_rotation_refine_10", lambda: rotation.rotation_refine(x1, x2, w, c.R, tau=tau, iters=10, return_weights=True)),
                         ("rp_homography_consensus", lambda: homography.homography_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED, return_weights=True)),
                         ("rp_homography_refine_10", lambda: homography.homography_refine(x1, x2, w, hc.H, tau=tau, iters=10, return_weights=True))):
            med, lo, hi = timed(fn, args.warmup, args.reps)
            row[name + "_ms"] = {"median": med, "min": lo, "max": hi}
        row["rotation_over_homography_consensus"] = row["rp_rotation_consensus_ms"]["median"] / row["rp_homography_consensus_ms"]["median"]
        row["rotation_over_homography_refine_10"] = row["rp_rotation_refine_10_ms"]["median"] / row["rp_homography_refine_10_ms"]["median"]
        row["rotation_inlier_share"], row["homography_inlier_share"] = float(r.stat[:, 1].mean()), float(hr.stat[:, 1].mean())
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        save()
    # the chains, one pair of 384 x 384 images through a randomly initialised model
    m = _model().eval()
    images = O.synthetic_images(1, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(1, 2, 1).contiguous().cuda()
    for name, fn in (("rotation_from_matches", lambda: m.rotation_from_matches(images, intr)),
                     ("planar_pose_from_matches", lambda: m.planar_pose_from_matches(images, intr)),
                     ("correspondences", lambda: m.correspondences(images))):
        med, lo, hi = timed(fn, args.warmup, args.reps)
        result["chains"][name + "_ms"] = {"median": med, "min": lo, "max": hi}
        print(json.dumps({name + "_ms": result["chains"][name + "_ms"]}), flush=True)
        save()
    return result


if __name__ == "__main__":
    main()
