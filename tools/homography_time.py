#!/usr/bin/env python3
"""Time the three entry points of include/relpose_homography.h next to what they stand beside.

    python tools/homography_time.py [--reps 30] [--warmup 5] [--out profiles/homography_time.txt]

At (n, P, M) = (64, 576, 1024), (64, 1728, 1024) and (6, 576, 1024), a third of the matches replaced by noise (the scenes of
tools/consensus_time.py): rp_homography_consensus, rp_homography_refine (10 iterations, from the consensus winner) and
rp_pose_from_homography; alongside, on the same inputs, rp_eight_point_consensus at the same M, one rp_eight_point solve (iters = 0), and
a torch composition of the consensus' work (batched SVD null vectors of the M 8 x 9 matrices, the [n, M, P] score, argmin).  After
`warmup` calls of the same shape every one of `reps` calls is timed by a pair of device events of its own; the median is what is
quoted, the minimum and the maximum show the spread.  No target is fixed in advance.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(64, 576, 1024), (64, 1728, 1024), (6, 576, 1024)]
TAU, SEED = 0.01, 1


def torch_consensus(x1, x2, w, tau, samples):
    """the same work in torch: the DLT matrices of the given samples [n,M,4], their null vectors by batched SVD, the robust transfer cost
    of every hypothesis on all rows, the argmin (no Hartley normalisation: calibrated coordinates are of order 1)"""
    import torch
    n, M = samples.shape[:2]
    idx = samples.long().reshape(n, M * 4, 1).expand(-1, -1, 2)
    a, b = torch.gather(x1, 1, idx).reshape(n, M, 4, 2), torch.gather(x2, 1, idx).reshape(n, M, 4, 2)
    one, zero = torch.ones_like(a[..., 0]), torch.zeros_like(a[..., 0])
    r0 = torch.stack([a[..., 0], a[..., 1], one, zero, zero, zero, -b[..., 0] * a[..., 0], -b[..., 0] * a[..., 1], -b[..., 0]], -1)
    r1 = torch.stack([zero, zero, zero, a[..., 0], a[..., 1], one, -b[..., 1] * a[..., 0], -b[..., 1] * a[..., 1], -b[..., 1]], -1)
    A = torch.cat([r0, r1], 2)                                                  # [n,M,8,9]
    Hm = torch.linalg.svd(A, full_matrices=True)[2][..., 8, :].reshape(n, M, 3, 3)
    xh = torch.cat([x1, torch.ones_like(x1[..., :1])], -1)                      # [n,P,3]
    m = torch.einsum("nmij,npj->nmpi", Hm, xh)
    e = m[..., :2] - x2[:, None] * m[..., 2:]
    d = (e.square().sum(-1) / m[..., 2].square().clamp(min=1e-30)).clamp(max=1e30)
    t2 = (tau * tau)[:, None, None]
    cost = (w[:, None] * t2 * torch.log1p(d / t2)).sum(-1) / w.sum(-1, keepdim=True)
    best = cost.argmin(-1)
    return Hm[torch.arange(n, device=x1.device), best], cost


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("homography_time needs a GPU")
    from rel_pose_amd import consensus, eightpoint, homography
    from tools.eightpoint_time import scenes
    from tools.fivepoint_time import timed
    result = {"reps": args.reps, "warmup": args.warmup, "tau": TAU, "seed": SEED, "device": torch.cuda.get_device_name(0), "rows": []}
    for n, P, M in SHAPES:
        x1, x2, w = (t.cuda() for t in scenes(n, P))
        x2[:, ::3] = torch.rand_like(x2[:, ::3]) * 1.2 - 0.6                         # a third of the matches wrong
        tau = torch.full((n,), TAU, device="cuda")
        c = homography.homography_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED, return_samples=True)
        r = homography.homography_refine(x1, x2, w, c.H, tau=tau, iters=10)
        row = {"n": n, "P": P, "M": M}
        for name, fn in (("rp_homography_consensus", lambda: homography.homography_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED, return_weights=True)),
                         ("rp_homography_refine_10", lambda: homography.homography_refine(x1, x2, w, c.H, tau=tau, iters=10, return_weights=True)),
                         ("rp_pose_from_homography", lambda: homography.pose_from_homography(r.H, x1, x2, w, tau=tau)),
                         ("rp_eight_point_consensus", lambda: consensus.eight_point_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED, return_weights=True)),
                         ("rp_eight_point_iters0", lambda: eightpoint.eight_point(x1, x2, w, tau=tau, iters=0)),
                         ("torch_consensus", lambda: torch_consensus(x1, x2, w, tau, c.samples))):
            med, lo, hi = timed(fn, args.warmup, args.reps)
            row[name + "_ms"] = {"median": med, "min": lo, "max": hi}
        row["homography_over_eight_point_consensus"] = row["rp_homography_consensus_ms"]["median"] / row["rp_eight_point_consensus_ms"]["median"]
        row["refine_10_over_eight_point_solve"] = row["rp_homography_refine_10_ms"]["median"] / row["rp_eight_point_iters0_ms"]["median"]
        row["torch_over_homography_consensus"] = row["torch_consensus_ms"]["median"] / row["rp_homography_consensus_ms"]["median"]
        row["homography_inlier_share"] = float(r.stat[:, 1].mean())
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        if args.out:                                               # (after every shape: what is measured is kept)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
