#!/usr/bin/env python3
"""Time rp_triangulate (include/relpose_triangulate.h) next to what it stands beside.

    python tools/triangulate_time.py [--reps 30] [--warmup 5] [--out profiles/triangulate_time.txt]

At (n, P) = (64, 576), (64, 1728) and (6, 576), on the scenes of tests/_triangulate_ref.py (depth 3, noise 1e-3, 30 % of x2 replaced by
noise): rp_triangulate with and without the corrected points; alongside, on the same inputs, rp_refine_pose with iters = 0 from the
unchanged refinement library -- the scorer: one pass over the rows and one reduction, too -- and a torch composition of the same
arithmetic.  After `warmup` calls of the same shape every one of `reps` calls is timed by a pair of device events of its own; the median
is what is quoted, the minimum and the maximum show the spread.  No target is fixed in advance.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(64, 576), (64, 1728), (6, 576)]
TAU = 0.01


def torch_triangulate(pose, x1, x2, w, tau):
    """the same arithmetic in torch, batched over [n,P]: Lindstrom's two steps, the ray intersection, the parallax and the four sums"""
    import torch
    t = pose[:, :3] / pose[:, :3].norm(dim=-1, keepdim=True)
    q = pose[:, 3:] / pose[:, 3:].norm(dim=-1, keepdim=True)
    x, y, z, s = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s), 2 * (x * y + z * s), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * s), 2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    E = torch.linalg.cross(t[:, :, None].expand(-1, -1, 3), R, dim=1)
    h1 = torch.cat([x1, torch.ones_like(x1[..., :1])], -1)
    h2 = torch.cat([x2, torch.ones_like(x2[..., :1])], -1)
    Et = E[:, :2, :2]
    m, mp = (h1 @ E.transpose(1, 2))[..., :2], (h2 @ E)[..., :2]
    c = (h2 * (h1 @ E.transpose(1, 2))).sum(-1)
    a = (m * (mp @ Et.transpose(1, 2))).sum(-1)
    b = 0.5 * (m.square().sum(-1) + mp.square().sum(-1))
    d = (b * b - a * c).clamp(min=0).sqrt()
    lam = c / (b + d)
    m2, mp2 = m - (lam[..., None] * mp) @ Et.transpose(1, 2), mp - (lam[..., None] * m) @ Et
    lam = lam * 2 * d / (m2.square().sum(-1) + mp2.square().sum(-1))
    d2v, d1v = lam[..., None] * m2, lam[..., None] * mp2
    xa = torch.cat([x1 - d1v, torch.ones_like(x1[..., :1])], -1)
    xb = torch.cat([x2 - d2v, torch.ones_like(x1[..., :1])], -1)
    dd = d1v.square().sum(-1) + d2v.square().sum(-1)
    r = xa @ R.transpose(1, 2)
    g = torch.linalg.cross(xb, r, dim=-1)
    gg = g.square().sum(-1)
    tt = t[:, None].expand_as(xb)
    z1 = (torch.linalg.cross(tt, xb, dim=-1) * g).sum(-1) / gg
    z2 = (torch.linalg.cross(tt, r, dim=-1) * g).sum(-1) / gg
    phi = torch.atan2(gg.sqrt(), (xb * r).sum(-1))
    t2 = (tau * tau)[:, None]
    om = w / (1 + dd / t2)
    stat = torch.stack([(w * t2 * torch.log1p(dd / t2)).sum(-1) / w.sum(-1), (om * ((z1 > 0) & (z2 > 0))).sum(-1) / om.sum(-1),
                        (om * phi).sum(-1) / om.sum(-1), (w > 0).sum(-1).float()], -1)
    return z1[..., None] * xa, torch.stack([z1, z2, dd, phi], -1), torch.cat([xa[..., :2], xb[..., :2]], -1), stat


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("triangulate_time needs a GPU")
    from rel_pose_amd import refine, triangulate
    from tests import _triangulate_ref as T
    from tools.fivepoint_time import timed
    result = {"reps": args.reps, "warmup": args.warmup, "tau": TAU, "device": torch.cuda.get_device_name(0), "rows": []}
    for n, P in SHAPES:
        a, b, pose = T.scenes(n, P, 1, 3.0, 1e-3, 0.3)[:3]
        x1, x2, pose = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(pose).float().cuda()
        w = (torch.rand(n, P, generator=torch.Generator().manual_seed(P)) * 0.95 + 0.05).cuda()
        tau = torch.full((n,), TAU, device="cuda")
        row = {"n": n, "P": P}
        for name, fn in (("rp_triangulate", lambda: triangulate.triangulate(pose, x1, x2, w, tau=tau, return_corrected=True)),
                         ("rp_triangulate_no_xc", lambda: triangulate.triangulate(pose, x1, x2, w, tau=tau)),
                         ("rp_refine_pose_iters0", lambda: refine.refine_pose(pose, x1, x2, w, tau=tau, iters=0, return_weights=True)),
                         ("torch_triangulate", lambda: torch_triangulate(pose, x1, x2, w, tau))):
            med, lo, hi = timed(fn, args.warmup, args.reps)
            row[name + "_ms"] = {"median": med, "min": lo, "max": hi}
        row["triangulate_over_scorer"] = row["rp_triangulate_ms"]["median"] / row["rp_refine_pose_iters0_ms"]["median"]
        row["torch_over_triangulate"] = row["torch_triangulate_ms"]["median"] / row["rp_triangulate_ms"]["median"]
        s = triangulate.triangulate(pose, x1, x2, w, tau=tau, return_corrected=True)
        ref = torch_triangulate(pose, x1, x2, w, tau)
        row["agreement_with_torch"] = {"stat": float((s.stat - ref[3]).abs().max()), "corrected": float((s.corrected - ref[2]).abs().max())}
        row["front_share"], row["mean_parallax_deg"] = float(s.stat[:, 1].mean()), float(torch.rad2deg(s.stat[:, 2]).mean())
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        if args.out:                                               # (after every shape: what is measured is kept)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
