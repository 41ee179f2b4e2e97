#!/usr/bin/env python3
"""demo.py -- predict the relative pose of one image pair (counterpart of reference demo.py:24-101, same flags).

    python demo.py --img1 a.png --img2 b.png --ckpt pretrained_models/matterport.pth

Checkpoints are the reference's own files ({'model': state_dict} with an optional 'module.' prefix); the pretrained
ones are not obtainable offline, so without --ckpt the model keeps its random initialisation (plumbing check only).
cv2 is absent in this image: PNGs are read with a tiny stdlib reader (8-bit RGB/RGBA, non-interlaced), channels
reordered to BGR like cv2.imread, alpha dropped.
"""
import argparse
import struct
import zlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from rel_pose_amd.model import ViTEss
from rel_pose_amd.se3 import SE3


def read_png_bgr(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype, _, _, interlace = hdr
    assert depth == 8 and ctype in (2, 6) and interlace == 0, "only 8-bit RGB/RGBA non-interlaced PNGs"
    ch = 3 if ctype == 2 else 4
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + w * ch)
    out = np.zeros((h, w * ch), dtype=np.uint8)
    prev = np.zeros(w * ch, dtype=np.int32)
    for y in range(h):
        ft, line = raw[y, 0], raw[y, 1:].astype(np.int32)
        cur = np.zeros(w * ch, dtype=np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        else:                                   # Sub / Average / Paeth need the running left neighbour
            for i in range(w * ch):
                a = cur[i - ch] if i >= ch else 0
                b = prev[i]
                c = prev[i - ch] if i >= ch else 0
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (line[i] + p) & 255
        out[y] = cur
        prev = cur
    img = out.reshape(h, w, ch)[:, :, :3]
    return img[:, :, ::-1].copy()               # RGB -> BGR (cv2 order)


def load_pair(img1, img2, matterport):
    """[1,2,3,H,W] float32 BGR 0..255 on the CPU: reference demo.py:65-76 (cv2.imread order, nearest resize to 384x512 for the
    Matterport checkpoints, whose training data was resized that way)."""
    images = np.stack([read_png_bgr(img1), read_png_bgr(img2)]).astype(np.float32)
    images = torch.from_numpy(images).permute(0, 3, 1, 2)
    if matterport:
        images = F.interpolate(images, size=[384, 512])                                         # demo.py:72-73
    return images.unsqueeze(0)


def postprocess(raw7, matterport):
    """reference demo.py:86-92: undo the training-time depth scale and reorder the quaternion (yzxw -> xyzw) on Matterport."""
    preds = np.array(raw7, dtype=np.float32, copy=True)
    if matterport:
        preds[:3] = preds[:3] * 5                                                               # DEPTH_SCALE
        preds[3:] = np.array([raw7[4], raw7[5], raw7[3], raw7[6]])
    return preds


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--datapath"); ap.add_argument("--weights")
    ap.add_argument("--image_size", default=[384, 512])
    ap.add_argument("--img1"); ap.add_argument("--img2"); ap.add_argument("--ckpt", default="")
    for flag in ("no_pos_encoding", "noess", "cross_features", "use_single_softmax", "l1_pos_encoding"):
        ap.add_argument("--" + flag, action="store_true")
    ap.add_argument("--fc_hidden_size", type=int, default=512)
    ap.add_argument("--pool_size", type=int, default=60)
    ap.add_argument("--transformer_depth", type=int, default=6)
    ap.add_argument("--matches", metavar="OUT.npz", default="",
                    help="also write the token correspondences the Essential Matrix Module formed (rel_pose_amd/readout.py)")
    ap.add_argument("--eight_point", action="store_true",
                    help="also print the classical pose of the Essential Matrix Module's matches (rel_pose_amd/eightpoint.py)")
    ap.add_argument("--refine", type=int, default=0, metavar="N",
                    help="with --eight_point: also print that pose after N refinement iterations on the robust Sampson cost "
                         "(rel_pose_amd/refine.py) and the cost of the regressed, the eight-point and the refined pose")
    ap.add_argument("--consensus", type=int, default=0, metavar="M",
                    help="with --eight_point: also print the pose of the chain started from the best of M seeded minimal eight-point "
                         "hypotheses (rel_pose_amd/consensus.py); with --refine its cost joins the cost line")
    ap.add_argument("--seed", type=int, default=0, help="with --consensus: the seed of its sampler")
    ap.add_argument("--minimal", choices=("eight", "five"), default=None,
                    help="with --consensus: the minimal solver of its hypotheses -- eight matches (the default) or five, solved by the "
                         "calibrated five-point solver (rel_pose_amd/fivepoint.py)")
    ap.add_argument("--planar", action="store_true",
                    help="with --eight_point: also solve the scene as ONE PLANE (rel_pose_amd/homography.py) -- the homography's inlier share "
                         "next to the essential chain's, the candidates of its decomposition with visibility and Sampson cost, and which "
                         "one is picked and why; --consensus M and --seed S set its hypotheses (default 256) and its sampler")
    ap.add_argument("--rotation", action="store_true",
                    help="with --eight_point: also solve the pair as a PURE ROTATION (rel_pose_amd/rotation.py) -- the rotation-only pose "
                         "(t = 0), its robust cost and its inlier weight share, next to the inlier weight share of the eight-point consensus "
                         "chain.  The two shares count different distances at the same tau -- the one-sided transfer distance under R "
                         "against the Sampson distance to the epipolar line, which every match on the line passes -- so they are "
                         "labelled, not compared by a threshold; --consensus M and --seed S set the hypotheses (default 256) and the sampler")
    ap.add_argument("--auto", action="store_true",
                    help="with --eight_point: let the matches CHOOSE between the essential matrix, the plane and the pure rotation "
                         "(rel_pose_amd/select.py) -- the chosen model and its pose, one line per candidate with its criterion G, its "
                         "inlier count and its inlier gate, and the estimated noise scale; --consensus M and --seed S set the hypotheses "
                         "(default 1024 for the essential chain, 256 for the other two) and the sampler")
    ap.add_argument("--uncertainty", action="store_true",
                    help="with --eight_point: the pose of the chosen chain (the consensus chain with --consensus M, else the refined one) "
                         "with its standard deviations -- rotation +- x deg, translation direction +- y deg --, the least determined "
                         "direction and how many matches lie beyond tau (rel_pose_amd/covariance.py); 'not determined' where the "
                         "matches do not fix the pose")
    ap.add_argument("--subtoken", choices=("window", "quadratic"), default=None,
                    help="with --eight_point or --matches: localise every match between the token centres (rel_pose_amd/readout.py, "
                         "subtoken_correspondences) -- the poses are then computed from those positions, the .npz also carries them")
    ap.add_argument("--points", metavar="OUT.ply", default="",
                    help="with --eight_point: triangulate the matches under the classical pose (rel_pose_amd/triangulate.py; the refined "
                         "chain, or with --consensus M the consensus chain) -- an ASCII PLY of the points in front of both cameras whose "
                         "Cauchy weight is at least 0.5, coloured from image 1, and one line with the reprojection cost, the front share "
                         "and the mean parallax; OUT.npz writes the arrays instead")
    ap.add_argument("--guided", type=float, default=0.0, metavar="BAND",
                    help="with --eight_point: guided matching (rel_pose_amd/guided.py) -- every token's partner searched again within BAND "
                         "token pitches of the prior's epipolar lines, the pose refined on those matches; prints the guided pose and the "
                         "share of the attention's mass that the regressed, the consensus and the guided pose explain, on one scale")
    ap.add_argument("--third", metavar="IMG3", default="",
                    help="with --eight_point: the pose of a THIRD image against the structure of (img1, img2) (rel_pose_amd/resection.py) -- "
                         "its translation is in units of the baseline of (img1, img2), so the line 'baseline ratio' chains the two pairs; "
                         "the rotation and direction are compared with the two-view chain's for (img1, IMG3)")
    ap.add_argument("--prior", choices=("consensus", "regressed"), default=None, help="with --guided: the pose that guides (default consensus)")
    args = ap.parse_args(argv)
    if args.guided and not args.eight_point:
        ap.error("--guided needs --eight_point")
    if args.guided < 0:
        ap.error("--guided takes a positive band in token pitches")
    if args.prior and not args.guided:
        ap.error("--prior needs --guided")
    if args.third and not args.eight_point:
        ap.error("--third needs --eight_point")
    if args.points and not args.eight_point:
        ap.error("--points needs --eight_point")
    if args.subtoken and not (args.eight_point or args.matches):
        ap.error("--subtoken needs --eight_point or --matches")
    if args.consensus and not args.eight_point:
        ap.error("--consensus needs --eight_point")
    if args.planar and not args.eight_point:
        ap.error("--planar needs --eight_point")
    if args.rotation and not args.eight_point:
        ap.error("--rotation needs --eight_point")
    if args.auto and not args.eight_point:
        ap.error("--auto needs --eight_point")
    if args.uncertainty and not args.eight_point:
        ap.error("--uncertainty needs --eight_point")
    if args.minimal and not args.consensus:
        ap.error("--minimal needs --consensus")
    if args.consensus < 0:
        ap.error("--consensus takes a positive number of hypotheses")
    if args.refine and not args.eight_point:
        ap.error("--refine needs --eight_point")
    if args.refine < 0:
        ap.error("--refine takes a positive number of iterations")
    args.fusion_transformer = True
    args.noess = "1" if args.noess else ""
    print("predicting pose on %s and %s using model %s" % (args.img1, args.img2, args.ckpt or "<random init>"))
    matterport = "matterport" in args.ckpt or not args.ckpt
    intr = [[517.97, 517.97, 320, 240]] * 2 if matterport else [[128, 128, 128, 128]] * 2      # demo.py:52-55
    intrinsics = torch.tensor([intr], dtype=torch.float32).cuda()

    model = ViTEss(args)
    if args.ckpt:
        sd = OrderedDict((k.replace("module.", ""), v) for k, v in torch.load(args.ckpt, map_location="cpu", weights_only=False)["model"].items())
        model.load_state_dict(sd)
    model = model.cuda().eval()

    images = load_pair(args.img1, args.img2, matterport).cuda()
    Gs = SE3(torch.tensor([[[0, 0, 0, 0, 0, 0, 1.0]] * 2]).cuda())
    with torch.no_grad():
        est = model(images, Gs, intrinsics=intrinsics)
    preds = postprocess(est[0][0][1].data.cpu().numpy(), matterport)
    np.set_printoptions(suppress=True, precision=5)
    if matterport:
        print("predicted R&t, as quaternion, in format x,y,z,qx,qy,qz,qw:")
        print(preds)
    else:
        print("predicted R, as quaternion in format qx,qy,qz,qw")
        print(preds[3:])
    if args.matches:
        write_matches(model, images, args.matches, args.subtoken)
    if args.eight_point:
        print_eight_point(model, images, intr, png_size(args.img1), preds, args.refine, args.consensus, args.seed, args.subtoken, args.minimal or "eight")
        if args.planar:
            print_planar(model, images, intr, png_size(args.img1), args.consensus or 256, args.seed, args.subtoken)
        if args.rotation:
            print_rotation(model, images, intr, png_size(args.img1), preds, args.consensus or 256, args.seed, args.subtoken)
        if args.auto:
            print_auto(model, images, intr, png_size(args.img1), preds, args.consensus or (1024, 256, 256), args.seed, args.subtoken,
                       args.minimal or "eight")
        if args.uncertainty:
            print_uncertainty(model, images, intr, png_size(args.img1), preds, args.refine or 10, args.consensus, args.seed, args.subtoken,
                              args.minimal or "eight")
        if args.guided:
            print_guided(model, images, intr, png_size(args.img1), preds, est[0].data[:, 1], args.guided, args.prior or "consensus", args.subtoken)
        if args.third:
            third = load_pair(args.img1, args.third, matterport)[:, 1:].cuda()
            print_third(model, torch.cat([images, third], 1), intr, png_size(args.img1), args.consensus or 256, args.seed, args.refine or 10,
                        args.subtoken)
        if args.points:
            write_points(model, images, intr, png_size(args.img1), args.points, args.refine or 10, args.consensus, args.seed, args.subtoken,
                         args.minimal or "eight")
    return preds


def png_size(path):
    """(height, width) from the IHDR chunk"""
    with open(path, "rb") as f:
        head = f.read(24)
    w, h = struct.unpack(">II", head[16:24])
    return h, w


def _angles_line(name, p, r):
    dq = min(1.0, abs(float((p[3:] * r[3:]).sum()) / max(float(r[3:].norm()), 1e-30)))
    dt = max(-1.0, min(1.0, float((p[:3] * r[:3]).sum()) / max(float(r[:3].norm()), 1e-30)))
    print("%s pose x,y,z,qx,qy,qz,qw: %s ; rotation differs by %.3f deg, translation direction by %.3f deg"
          % (name, " ".join("%.5f" % v for v in p.tolist()), 2 * np.degrees(np.arccos(dq)), np.degrees(np.arccos(dt))))


def print_eight_point(model, images, intr, orig_hw, regressed, refine=0, consensus=0, seed=0, subtoken=None, minimal="eight"):
    """--eight_point: one line -- the pose (t unit, q xyzw) the weighted eight-point algorithm finds from the EMM's matches, the angle
    between its rotation and the regressed one, and the angle between the two translation directions, in degrees.  `regressed` is the
    [7] pose this script prints (t, q xyzw); the intrinsics follow the images' resize.  refine = N > 0 (--refine N): one more line of the same
    form for the pose after N refinement iterations, and one with the mean robust Sampson cost of the three poses.  consensus = M > 0
    (--consensus M): one more pose line, the chain started from the best of M hypotheses (refined N times, too); its cost joins the
    cost line; minimal = "five" (--minimal five): its hypotheses come from the five-point solver.  subtoken = "window" / "quadratic" (--subtoken): every chain and the cost line run on the localised matches."""
    H, W = images.shape[-2:]
    sy, sx = H / orig_hw[0], W / orig_hw[1]
    K = torch.tensor([intr], dtype=torch.float32).cuda() * torch.tensor([sx, sy, sx, sy]).cuda()
    r = torch.from_numpy(np.asarray(regressed, dtype=np.float64))
    cp = model.consensus_pose_from_matches(images, K, hypotheses=consensus, seed=seed, refine=refine, subtoken=subtoken,
                                           minimal=minimal) if consensus else None
    if not refine:
        _angles_line("eight-point", model.pose_from_matches(images, K, subtoken=subtoken).pose[0].double().cpu(), r)
        if cp is not None:
            _angles_line("consensus", cp.pose[0].double().cpu(), r)
        return
    # --refine N: one more line of the same form for the refined pose, then the mean robust Sampson cost (the iters = 0 scorer of
    # rel_pose_amd/refine.py) of the three poses against the same matches, base weights and tau
    from rel_pose_amd import eightpoint
    from rel_pose_amd import refine as refine_
    hw = (int(H), int(W))
    rp = model.refined_pose_from_matches(images, K, refine=refine, subtoken=subtoken)
    _angles_line("eight-point", rp.initial.pose[0].double().cpu(), r)
    _angles_line("refined", rp.pose[0].double().cpu(), r)
    if cp is not None:
        _angles_line("consensus", cp.pose[0].double().cpu(), r)
    if subtoken is None:
        x1, x2, w = eightpoint.assemble_matches(model.correspondences(images), K, hw)
    else:
        sub = model.subtoken_correspondences(images)
        x1, x2, w = eightpoint.assemble_matches(sub.corr, K, hw, sub=sub, subtoken=subtoken)
    tau = eightpoint.default_tau(K, hw).contiguous()
    poses = torch.cat([torch.from_numpy(np.asarray(regressed, dtype=np.float32))[None].cuda(), rp.initial.pose, rp.pose])
    cost = refine_.refine_pose(poses, x1.expand(3, -1, -1).contiguous(), x2.expand(3, -1, -1).contiguous(), w.expand(3, -1).contiguous(),
                               tau=tau.expand(3).contiguous(), iters=0).stat[:, 0].cpu().tolist()
    line = "mean robust Sampson cost of the matches: regressed %.6e, eight-point %.6e, refined %.6e" % tuple(cost)
    print(line if cp is None else line + ", consensus %.6e" % float(cp.stat[0, 1]))


def print_planar(model, images, intr, orig_hw, hypotheses=256, seed=0, subtoken=None):
    """--planar: the scene solved as one plane.  One line with the inlier weight share of the refined homography next to that of the
    essential chain (eight-point consensus, the same hypotheses and seed) -- no automatic choice between the two models is made: the
    caller decides --, one line per valid candidate of the decomposition (pose, plane normal, visibility share, robust Sampson cost,
    |t|/d), and one saying which candidate is picked and why."""
    H, W = images.shape[-2:]
    sy, sx = H / orig_hw[0], W / orig_hw[1]
    K = torch.tensor([intr], dtype=torch.float32).cuda() * torch.tensor([sx, sy, sx, sy]).cuda()
    pp = model.planar_pose_from_matches(images, K, hypotheses=hypotheses, seed=seed, subtoken=subtoken, prior="regressed")
    cp = model.consensus_pose_from_matches(images, K, hypotheses=hypotheses, seed=seed, refine=0, subtoken=subtoken)
    print("inlier weight share: homography %.4f (robust transfer cost %.6e), essential matrix %.4f"
          % (float(pp.stat[0, 1]), float(pp.stat[0, 0]), float(cp.consensus.stat[0, 1])))
    cs, pick = pp.candidates.cstat[0].cpu(), pp.pick[0].cpu().tolist()
    for k in range(4):
        if cs[k, 3] == 1:
            print("planar candidate %d pose x,y,z,qx,qy,qz,qw: %s ; normal %s ; visibility %.4f, Sampson cost %.6e, |t|/d %.4f"
                  % (k, " ".join("%.5f" % v for v in pp.candidates.pose[0, k].cpu().tolist()),
                     " ".join("%.4f" % v for v in pp.candidates.normal[0, k].cpu().tolist()), cs[k, 0], cs[k, 1], cs[k, 2]))
    if pick[0] < 0:
        print("planar: no candidate")
    elif cs[pick[0], 2] == 0:
        print("planar: candidate 0, a pure rotation (or a plane at infinity)")
    elif bool(pp.ambiguous[0]):
        print("planar: candidates %d and %d both see every match; %d is nearer the regressed pose" % (pick[0], pick[1], pick[0]))
    else:
        print("planar: candidate %d, %s" % (pick[0], "the only one that sees the plane from both cameras" if cs[pick[0], 0] >= 0.99
                                             else "by Sampson cost: none sees every match"))


def print_rotation(model, images, intr, orig_hw, regressed, hypotheses=256, seed=0, subtoken=None):
    """--rotation: the pair solved as a pure rotation.  One pose line of the usual form (t = 0: the translation angle is printed as 90
    degrees and means nothing), then one line with the robust cost and the inlier weight share of the refined rotation -- transfer
    distance -- next to the inlier weight share of the eight-point consensus chain (the same hypotheses and seed) -- Sampson distance.
    No threshold turns the share into a yes / no: the caller decides."""
    H, W = images.shape[-2:]
    sy, sx = H / orig_hw[0], W / orig_hw[1]
    K = torch.tensor([intr], dtype=torch.float32).cuda() * torch.tensor([sx, sy, sx, sy]).cuda()
    rp = model.rotation_from_matches(images, K, hypotheses=hypotheses, seed=seed, subtoken=subtoken)
    cp = model.consensus_pose_from_matches(images, K, hypotheses=hypotheses, seed=seed, refine=0, subtoken=subtoken)
    _angles_line("rotation-only", rp.pose[0].double().cpu(), torch.from_numpy(np.asarray(regressed, dtype=np.float64)))
    print("rotation-only: robust transfer cost %.6e, inlier weight share %.4f (transfer distance under R); eight-point consensus inlier "
          "weight share %.4f (Sampson distance)" % (float(rp.stat[0, 0]), float(rp.stat[0, 1]), float(cp.consensus.stat[0, 1])))


def print_third(model, images3, intr, orig_hw, hypotheses=256, seed=0, iters=10, subtoken=None):
    """--third IMG3: the third image against the structure of (img1, img2).  One pose line of the usual format for IMG3 (t in units of the
    baseline of (img1, img2), NOT normalised), the baseline ratio, the inlier weight share of the resection, and the angles between the
    resection's rotation / translation direction and those of the two-view consensus chain for (img1, IMG3); a degenerate result (too
    few usable points, or no valid hypothesis) says `not determined` instead."""
    H, W = images3.shape[-2:]
    sy, sx = H / orig_hw[0], W / orig_hw[1]
    K = torch.tensor([[intr[0], intr[1], intr[1]]], dtype=torch.float32).cuda() * torch.tensor([sx, sy, sx, sy]).cuda()
    kw = dict(subtoken=subtoken) if subtoken else {}
    tv = model.third_view_pose_from_matches(images3, K, hypotheses=hypotheses, seed=seed, iters=iters, **kw)
    pose, two = tv.pose_c[0].double().cpu(), tv.two_view_c.pose[0].double().cpu()
    scale = float(tv.scale[0])
    if not scale > 0 or not bool(torch.isfinite(pose).all()) or float(tv.stat[0, 3]) < 3:
        print("third view: not determined (%d usable points)" % int(tv.stat[0, 3]))
        return
    dq = min(1.0, abs(float((pose[3:] * two[3:]).sum())))
    dt = max(-1.0, min(1.0, float((pose[:3] * two[:3]).sum()) / max(scale * float(two[:3].norm()), 1e-30)))
    print("third view pose x,y,z,qx,qy,qz,qw: %s" % " ".join("%.5f" % v for v in pose.tolist()))
    print("third view: baseline ratio |t_c| / |t_a| = %.5f ; inlier weight share %.4f over %d points ; against the two-view chain for "
          "(img1, img3): rotation differs by %.3f deg, translation direction by %.3f deg"
          % (scale, float(tv.stat[0, 1]), int(tv.stat[0, 3]), 2 * np.degrees(np.arccos(dq)), np.degrees(np.arccos(dt))))


def print_auto(model, images, intr, orig_hw, regressed, hypotheses=(1024, 256, 256), seed=0, subtoken=None, minimal="eight"):
    """--auto: the model the matches support.  One line naming the chosen candidate and its kind, one pose line of the usual form for its
    pose, one line per candidate with the criterion G, the inlier count and the inlier gate on e^2 (an invalid candidate says so), and
    one with the noise scale and the candidate that supplied it."""
    from rel_pose_amd import select
    H, W = images.shape[-2:]
    sy, sx = H / orig_hw[0], W / orig_hw[1]
    K = torch.tensor([intr], dtype=torch.float32).cuda() * torch.tensor([sx, sy, sx, sy]).cuda()
    ap = model.auto_pose_from_matches(images, K, hypotheses=hypotheses, seed=seed, subtoken=subtoken, minimal=minimal)
    pick, kind = int(ap.selection.pick[0]), int(ap.kind[0])
    if pick < 0:
        print("auto: no model (too few matches, or no candidate fits any of them)")
    else:
        print("auto: %s (candidate %d, %s)" % (select.KIND_NAMES[kind], pick, select.AUTO_NAMES[pick]))
        _angles_line("auto", ap.pose[0].double().cpu(), torch.from_numpy(np.asarray(regressed, dtype=np.float64)))
    st = ap.selection.stat[0].cpu()
    for c, name in enumerate(select.AUTO_NAMES):
        if pick < 0 or st[c, 0] >= 3e38:
            print("auto candidate %d (%s): invalid" % (c, name))
        else:
            print("auto candidate %d (%s): G %.2f, %d inliers, gate %.6e" % (c, name, st[c, 0], int(st[c, 1]), st[c, 2]))
    print("auto: sigma %.6e (%s)" % (float(ap.selection.scale[0, 0]),
                                     "none" if pick < 0 else "given" if ap.selection.scale[0, 1] < 0 else "from candidate %d" % int(ap.selection.scale[0, 1])))


def print_uncertainty(model, images, intr, orig_hw, regressed, refine=10, consensus=0, seed=0, subtoken=None, minimal="eight"):
    """--uncertainty: the pose of the chosen chain -- the consensus chain with --consensus M, else the refined one -- in the usual form,
    then its standard deviations from the sandwich covariance of the robust fit (rel_pose_amd/covariance.py), the least determined
    direction of (omega_0, omega_1, omega_2, beta_1, beta_2), and one line with rho (the smallest pivot of the scaled A, near 0: a
    direction the matches do not fix), the rows beyond tau and the rows of positive weight.  Status -1 prints "not determined" in the
    place of the numbers, status 0 "degenerate"."""
    from rel_pose_amd import covariance
    H, W = images.shape[-2:]
    sy, sx = H / orig_hw[0], W / orig_hw[1]
    K = torch.tensor([intr], dtype=torch.float32).cuda() * torch.tensor([sx, sy, sx, sy]).cuda()
    kw = dict(hypotheses=consensus, seed=seed, minimal=minimal) if consensus else {}
    chain = "consensus" if consensus else "refined"
    res, pc = model.pose_uncertainty_from_matches(images, K, chain=chain, refine=refine, subtoken=subtoken, **kw)
    _angles_line("uncertainty (%s chain)" % chain, res.pose[0].double().cpu(), torch.from_numpy(np.asarray(regressed, dtype=np.float64)))
    st = pc.stat[0].cpu().tolist()
    if st[0] == covariance.OK:
        print("uncertainty: rotation +- %.4f deg, translation direction +- %.4f deg"
              % (float(covariance.rotation_sd_deg(pc)[0]), float(covariance.direction_sd_deg(pc)[0])))
        print("uncertainty: weak direction (w0 w1 w2 b1 b2) %s, +- %.4f deg along it"
              % (" ".join("%.4f" % v for v in pc.weak[0].cpu().tolist()), np.degrees(max(float(pc.eig[0, 0]), 0.0) ** 0.5)))
    else:
        print("uncertainty: %s" % ("not determined (the matches do not fix the pose at this tau)" if st[0] == covariance.NOT_DETERMINED
                                    else "degenerate (too few matches, or no pose)"))
    print("uncertainty: rho %.3e, %d of %d weighted matches beyond tau, robust cost %.6e" % (st[4], int(st[5]), int(st[1]), st[6]))


def print_guided(model, images, intr, orig_hw, regressed, regressed_raw, band, prior="consensus", subtoken=None):
    """--guided BAND: one pose line of the usual form for the guided chain (prior -> matches within BAND token pitches of its epipolar
    lines -> refinement from the prior), one with the share of its owners that found no partner in the band, and one with the in-band
    share of the attention's mass under the regressed, the consensus and the guided pose (mean over both images and the heads).  The
    guided matches lie near the prior's lines by construction, so the support, not the Sampson cost, is what says whether a pose holds."""
    H, W = images.shape[-2:]
    sy, sx = H / orig_hw[0], W / orig_hw[1]
    K = torch.tensor([intr], dtype=torch.float32).cuda() * torch.tensor([sx, sy, sx, sy]).cuda()
    g = model.guided_pose_from_matches(images, K, prior=prior, band=band, subtoken=subtoken)
    cons = g.prior if prior == "consensus" else model.consensus_pose_from_matches(images, K, subtoken=subtoken).pose
    _angles_line("guided", g.pose[0].double().cpu(), torch.from_numpy(np.asarray(regressed, dtype=np.float64)))
    print("guided: prior %s, band %g token pitches, %.4f of the owners without a partner in the band" % (prior, band, float(g.unmatched[0])))
    sup = [float(model.pose_support(images, K, p, band=band).mean()) for p in (regressed_raw, cons)] + [float(g.support_after.mean())]
    print("in-band share of the attention's mass: regressed %.4f, consensus %.4f, guided %.4f" % tuple(sup))


def write_points(model, images, intr, orig_hw, path, refine=10, consensus=0, seed=0, subtoken=None, minimal="eight"):
    """--points: the matches triangulated under the pose of the refined chain (consensus = M > 0: of the consensus chain).  Prints one
    line -- the robust reprojection cost, the share in front of both cameras, the mean parallax in degrees -- and writes the rows that are
    in front of both cameras with a Cauchy weight w / (1 + reproj / tau^2) of at least 0.5: an ASCII PLY (x y z in the frame of camera 1,
    units of the baseline; red green blue from image 1 at the match's pixel), or with a .npz suffix the arrays of every row (points,
    depth1, depth2, reproj, parallax, weight, keep, stat, pose)."""
    H, W = images.shape[-2:]
    sy, sx = H / orig_hw[0], W / orig_hw[1]
    K = torch.tensor([intr], dtype=torch.float32).cuda() * torch.tensor([sx, sy, sx, sy]).cuda()
    kw = dict(hypotheses=consensus, seed=seed, minimal=minimal) if consensus else {}
    ms = model.structure_from_matches(images, K, chain="consensus" if consensus else "refined", refine=refine, subtoken=subtoken, **kw)
    st = ms.structure
    print("structure: reprojection cost %.6e, in front of both cameras %.4f, mean parallax %.3f deg"
          % (float(st.stat[0, 0]), float(st.stat[0, 1]), np.degrees(float(st.stat[0, 2]))))
    weight = ms.weights[0].clamp(min=0).nan_to_num(0.0) / (1 + st.reproj[0] / ms.tau[0] ** 2)
    keep = (st.depth1[0] > 0) & (st.depth2[0] > 0) & (weight >= 0.5)
    if path.endswith(".npz"):
        np.savez(path, points=st.points[0].cpu().numpy(), depth1=st.depth1[0].cpu().numpy(), depth2=st.depth2[0].cpu().numpy(),
                 reproj=st.reproj[0].cpu().numpy(), parallax=st.parallax[0].cpu().numpy(), weight=weight.cpu().numpy(),
                 keep=keep.cpu().numpy(), stat=st.stat[0].cpu().numpy(), pose=ms.pose[0].cpu().numpy())
        return
    px = (ms.x1[0] * K[0, 0, :2] + K[0, 0, 2:]).round().long()                       # the match's pixel in image 1
    u, v = px[:, 0].clamp(0, W - 1), px[:, 1].clamp(0, H - 1)
    rgb = images[0, 0][:, v, u].t().flip(1).clamp(0, 255).round().long()             # the images are BGR
    pts, rgb = st.points[0][keep].cpu().tolist(), rgb[keep].cpu().tolist()
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment camera 1 frame, units of the baseline\nelement vertex %d\n" % len(pts))
        f.write("property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        for p_, c in zip(pts, rgb):
            f.write("%.6f %.6f %.6f %d %d %d\n" % (p_[0], p_[1], p_[2], c[0], c[1], c[2]))


def write_matches(model, images, path, subtoken=None):
    """--matches: the readout of the pair's EMM attention as an .npz -- row_idx / col_idx [2,3,576], row_stat / col_stat [2,3,576,4],
    mutual [2,3,576] (rel_pose_amd.readout.Correspondences) and, per head h, match_xy0_h<h> / match_xy1_h<h> [M,2] / match_conf_h<h> [M]:
    pixel centres (of the images as the model saw them) in image 0 / image 1 of the mutual matches of image 1's attention.
    subtoken = "window" / "quadratic" (--subtoken): also row_win / row_quad / col_win / col_quad [2,3,576,4]
    (rel_pose_amd.readout.SubtokenCorrespondences) and, per head, match_sub_xy1_h<h> [M,2]: the localised pixel position in image 1."""
    from rel_pose_amd import readout
    sub = model.subtoken_correspondences(images) if subtoken else None
    corr = sub.corr if subtoken else model.correspondences(images)
    out = {k: getattr(corr, k).cpu().numpy() for k in ("row_idx", "row_stat", "col_idx", "col_stat", "mutual")}
    if subtoken:
        out.update({k: getattr(sub, k).cpu().numpy() for k in ("row_win", "row_quad", "col_win", "col_quad")})
    counts = []
    for h in range(corr.row_idx.shape[1]):
        xy0, xy1, conf = readout.matches_xy(corr, 1, h, images.shape[-2:])
        out["match_xy0_h%d" % h], out["match_xy1_h%d" % h], out["match_conf_h%d" % h] = xy0.cpu().numpy(), xy1.cpu().numpy(), conf.cpu().numpy()
        if subtoken:
            pos = (sub.row_win if subtoken == "window" else sub.row_quad)[1, h][corr.mutual[1, h]]
            out["match_sub_xy1_h%d" % h] = readout.subtoken_xy(pos, images.shape[-2:]).cpu().numpy()
        counts.append(int(xy0.shape[0]))
    np.savez(path, **out)
    print("mutual matches per head: %s -> %s" % (" ".join(str(c) for c in counts), path))


if __name__ == "__main__":
    main()
