"""ViTEss -- drop-in for reference src/model.py (same constructor args, forward signature, attribute names and
state_dict keys), with the ViT + Essential-Matrix-Module hot path on hand-written gfx950 kernels.

forward(images, Gs, intrinsics=None, inference=False)      reference src/model.py:161-191
  images      [B,2,3,H,W] fp32 BGR 0..255
  Gs          SE3-like (.data [B,2,7]) or numpy [2,7]
  intrinsics  [B,2,4] (fx,fy,cx,cy) in pixels -- rescaled IN PLACE to the 24x24 grid like the reference (:100-109)
returns [SE3([B,2,7])]  (or numpy [2,7] of element 0 when inference=True)
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .modules.extractor import ResidualBlock
from .modules.resnet import resnet18
from .modules.vision_transformer import _create_vision_transformer
from .se3 import SE3


class ViTEss(nn.Module):
    def __init__(self, args):
        super().__init__()
        noess = getattr(args, "noess", None) or None            # src/model.py:15-17: '' and absent both mean "off"
        if not getattr(args, "fusion_transformer", False):
            # the reference's non-transformer head cannot run: pool_transformer_output leaves [2B,60,24,24], reshape([B,-1])
            # gives 69120 columns for a Linear(34560,.) (src/model.py:63-71,180-189); with noess pool_attn gets 120 of 384
            raise NotImplementedError("fusion_transformer=False crashes in the reference itself (src/model.py:63-71,189); "
                                      "every scripts/*.sh passes --fusion_transformer")
        self.noess = noess
        self.total_num_features = 192
        self.feature_resolution = (24, 24)
        self.num_images = 2
        self.pose_size = 7
        self.num_patches = 24 * 24
        self.H2 = args.fc_hidden_size

        self.flatten = nn.Flatten(0, 1)
        self.resnet = resnet18(pretrained=True)
        self.resnet_pretrained = bool(getattr(self.resnet, "pretrained_loaded", False))
        self.resnet.fc = nn.Identity()
        self.extractor_final_conv = ResidualBlock(128, self.total_num_features, "batch", kernel_size=5)

        self.num_heads = 3
        self.transformer_depth = args.transformer_depth
        self.fusion_transformer = _create_vision_transformer(
            "vit_tiny_patch16_384", patch_size=16, embed_dim=self.total_num_features, depth=args.transformer_depth,
            num_heads=self.num_heads, cross_features=args.cross_features, use_single_softmax=args.use_single_softmax,
            no_pos_encoding=args.no_pos_encoding, noess=noess, l1_pos_encoding=args.l1_pos_encoding)
        nn.init.xavier_uniform_(self.fusion_transformer.pos_embed)     # src/model.py:54-56
        self.pos_encoding = None

        hd = self.total_num_features // self.num_heads
        self.H = int(self.num_heads * 2 * (hd + 6) * hd)               # 26880, src/model.py:61
        if self.noess:                                                 # src/model.py:73-82
            self.pool_feat1, self.pool_feat2 = 96, 43
            self.H = 24 * 24 * self.pool_feat2
            self.pool_attn = nn.Sequential(
                nn.Conv2d(self.total_num_features * 2, self.pool_feat1, kernel_size=1, bias=True),
                nn.BatchNorm2d(self.pool_feat1), nn.ReLU(),
                nn.Conv2d(self.pool_feat1, self.pool_feat2, kernel_size=1, bias=True), nn.BatchNorm2d(self.pool_feat2))
            self.pool_attn.to(memory_format=torch.channels_last)
        self.pose_regressor = nn.Sequential(
            nn.Linear(self.H, self.H2), nn.ReLU(), nn.Linear(self.H2, self.H2), nn.ReLU(),
            nn.Linear(self.H2, self.num_images * self.pose_size), nn.Unflatten(1, (self.num_images, self.pose_size)))
        # CNN front-end in channels-last: MIOpen's fp32 kernels are NHWC (saves its NCHW<->NHWC transposes, measured
        # 24.1 -> 20.1 ms fwd+bwd at 128 images) and the [2B,24,24,192] map IS the token layout (src/model.py:136-141)
        self.resnet.to(memory_format=torch.channels_last)
        self.extractor_final_conv.to(memory_format=torch.channels_last)
        # ImageNet statistics as (non-persistent) buffers: no per-call host-to-device copies, state_dict unchanged
        self.register_buffer("_mean", torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1), persistent=False)
        self.register_buffer("_std", torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1), persistent=False)
        self._intr_scale = {}

    # -- src/model.py:100-109 ---------------------------------------------------------------------
    def update_intrinsics(self, input_shape, intrinsics):
        sizey, sizex = self.feature_resolution
        key = (int(input_shape[-2]), int(input_shape[-1]), str(intrinsics.device), intrinsics.dtype)
        sc = self._intr_scale.get(key)
        if sc is None:          # (sx, sy, sx, sy): same fp32 products as the reference's two index_put_ lines, no index tensors
            scalex, scaley = sizex / input_shape[-1], sizey / input_shape[-2]
            sc = torch.tensor([scalex, scaley, scalex, scaley], dtype=intrinsics.dtype, device=intrinsics.device)
            self._intr_scale[key] = sc
        intrinsics.mul_(sc)     # in place on the CALLER's tensor, like the reference
        return intrinsics

    # -- src/model.py:111-143 ---------------------------------------------------------------------
    def cnn_map(self, images, intrinsics=None):
        """preprocessing + CNN front-end -> [2B,192,24,24] (PyTorch-ROCm / MIOpen: 'next' row 8f-1)."""
        if intrinsics is not None:
            intrinsics = self.update_intrinsics(images.shape, intrinsics)
        with ops.batches_tracked_batch(), ops.conv_params_bf16(self.resnet.layer1, self.resnet.layer2, self.extractor_final_conv):
            return self._cnn_layers(images), intrinsics

    def _cnn_layers(self, images):
        r = self.resnet
        if ops.stem_conv_ok(r.conv1, images):
            # BGR->RGB, /255, mean/std, nearest 224 (one bit-exact HIP kernel) written inside the stem's zero padding; hand-written conv1
            # (in training also bn1's batch statistics, from the convolution's epilogue)
            stats = None
            fn = ops.StemConvBf16Fn if ops.CNN_PRECISION == 1 else ops.StemConvFn      # (bf16 configuration: csrc/conv_stem_bf16.hip)
            if r.bn1.training and ops.STEM_STATS and ops.FUSE_STEM_POOL:
                c1, stats = fn.apply(ops.preprocess(images, pad=3), r.conv1.weight, True)
            else:
                c1 = fn.apply(ops.preprocess(images, pad=3), r.conv1.weight)
        else:
            c1, stats = ops.conv2d(r.conv1, ops.preprocess(images)), None
        x = ops.bn_relu_maxpool(r.bn1, r.maxpool, c1, stats)                    # stem: BatchNorm + ReLU + pool, one pass each way
        x = r.layer2(r.layer1(x))
        return self.extractor_final_conv(x)

    def extract_features(self, images, intrinsics=None):
        """tokens [2B,576,192] WITHOUT pos_embed (reference return value, src/model.py:136-143)."""
        fmap, intrinsics = self.cnn_map(images, intrinsics)
        if fmap.dtype != torch.float32:
            fmap = fmap.float()
        zero_pe = torch.zeros_like(self.fusion_transformer.pos_embed[0])
        return ops.TokensFn.apply(fmap, zero_pe), intrinsics

    def forward_tokens(self, fmap, Gs_data, intrinsics=None):
        """hot path: CNN map [2B,192,24,24] (or [2B,192,576]) -> normalised poses [B,2,7]."""
        ft = self.fusion_transformer
        if fmap.dtype != torch.float32:            # bf16 CNN front-end (the bf16 configuration): the token stream is fp32
            fmap = fmap.float()
        x = ops.TokensFn.apply(fmap, ft.pos_embed[0])
        for layer in range(self.transformer_depth):
            x = ft.blocks[layer](x, intrinsics=intrinsics)
        pr = self.pose_regressor
        if self.noess:
            # src/model.py:178,183-188.  features.reshape([B,24,24,-1]).permute(0,3,1,2) on the contiguous [2B,576,192] norm
            # output: "pixel" m of pair b holds tokens 2m, 2m+1 of the concatenated (image 0, image 1) token list -- in
            # channels-last memory that NCHW tensor IS the buffer, so the 1x1-conv/BN head (MIOpen, like the CNN front
            # end) runs on a view; only its [B,43,24,24] output is re-laid out (c-major) for the regressor.
            B = x.shape[0] // 2
            f = ops.LayerNormFn.apply(x, ft.norm.weight, ft.norm.bias)
            pooled = self.pool_attn(f.view(B, 24, 24, 2 * self.total_num_features).permute(0, 3, 1, 2))
            feats = pooled.contiguous(memory_format=torch.contiguous_format).reshape(B, -1)
            return ops.RegressFn.apply(feats, Gs_data, pr[0].weight, pr[0].bias, pr[2].weight, pr[2].bias, pr[4].weight,
                                       pr[4].bias)
        return ops.HeadFn.apply(x, Gs_data, ft.norm.weight, ft.norm.bias, pr[0].weight, pr[0].bias, pr[2].weight,
                                pr[2].bias, pr[4].weight, pr[4].bias)

    # -- readout of the EMM's attention (rel_pose_amd/readout.py; no counterpart in the reference) ----
    def correspondences_from_map(self, fmap, dense=False):
        """CNN map [2B,192,24,24] -> readout.Correspondences: per image and head the argmax / weight / mass / soft-argmax of every
        row and column of the EMM attention, the mutual matches and (dense=True) the attention itself.  eval() mode only."""
        from . import readout
        return readout.correspondences_from_map(self, fmap, dense)

    def correspondences(self, images, dense=False):
        """images [B,2,3,H,W] -> readout.Correspondences (see correspondences_from_map); changes no module state"""
        from . import readout
        return readout.correspondences(self, images, dense)

    def subtoken_correspondences_from_map(self, fmap, radius=2):
        """CNN map [2B,192,24,24] -> readout.SubtokenCorrespondences: correspondences_from_map and, around every row and column match, the
        position between the token centres -- a soft-argmax over the (2 radius + 1)^2 window and a parabola vertex.  eval() mode only."""
        from . import readout
        return readout.subtoken_correspondences_from_map(self, fmap, radius)

    def subtoken_correspondences(self, images, radius=2):
        """images [B,2,3,H,W] -> readout.SubtokenCorrespondences (see subtoken_correspondences_from_map); changes no module state"""
        from . import readout
        return readout.subtoken_correspondences(self, images, radius)

    def pose_from_matches(self, images, intrinsics, heads=(0, 1, 2), iters=4, tau=None, subtoken=None, radius=2):
        """images [B,2,3,H,W], intrinsics [B,2,4] = (fx, fy, cx, cy) in pixels of (H, W) -> eightpoint.MatchPose: the CLASSICAL pose of
        the matches the Essential Matrix Module formed -- correspondences -> weighted eight-point with `iters` rounds of robust
        re-weighting (tau: its scale; None = half a token pitch) -> E -> (R, t) by the cheirality vote.  subtoken = "window" / "quadratic":
        the matches are localised between the token centres first (subtoken_correspondences with `radius`; pass a smaller tau then).
        eval() mode only; changes no module state and does not write to `intrinsics`."""
        from . import eightpoint
        return eightpoint.pose_from_matches(self, images, intrinsics, heads, iters, tau, subtoken, radius)

    def refined_pose_from_matches(self, images, intrinsics, heads=(0, 1, 2), iters=4, tau=None, refine=10, subtoken=None, radius=2):
        """pose_from_matches followed by `refine` Levenberg-Marquardt iterations on the robust Sampson cost of the same matches (their base
        weights, the same tau) over the five degrees of freedom of (R, t) -> refine.RefinedMatchPose; its `initial` is what
        pose_from_matches returns; subtoken, radius as there.  eval() mode only; changes no module state and does not write to `intrinsics`."""
        from . import refine as refine_
        return refine_.refined_pose_from_matches(self, images, intrinsics, heads, iters, tau, refine, subtoken, radius)

    def consensus_pose_from_matches(self, images, intrinsics, heads=(0, 1, 2), hypotheses=1024, seed=0, iters=4, tau=None, refine=10,
                                    subtoken=None, radius=2, minimal="eight"):
        """refined_pose_from_matches started from a consensus instead of the all-data solve: `hypotheses` minimal eight-point samples drawn
        from `seed`, each scored on all matches; the best one's Cauchy weights are the base weights of the eight-point solve that the
        refinement (on the matches' own base weights) then starts from -> consensus.ConsensusMatchPose.  The same seed gives the same
        bits.  subtoken, radius as for pose_from_matches.  minimal = "five": samples of five matches solved by the calibrated five-point
        solver (rel_pose_amd/fivepoint.py), which holds up to 60 % of outliers.  eval() mode only; changes no module state and does not
        write to `intrinsics`."""
        from . import consensus
        return consensus.consensus_pose_from_matches(self, images, intrinsics, heads, hypotheses, seed, iters, tau, refine, subtoken, radius,
                                                     minimal)

    def planar_pose_from_matches(self, images, intrinsics, heads=(0, 1, 2), hypotheses=256, seed=0, refine=10, tau=None, subtoken=None,
                                 radius=2, vis_min=0.99, prior=None):
        """The pose of a PLANAR scene from the matches, where every essential-matrix chain above fails (two essential matrices fit one
        plane): `hypotheses` four-point homography samples drawn from `seed`, each scored on all matches; the best one polished by
        `refine` Levenberg-Marquardt iterations on the robust transfer cost; the closed-form decomposition into at most two physically
        possible (R, t, n), ranked by visibility (share >= vis_min) and robust Sampson cost -> homography.PlanarMatchPose, whose
        `ambiguous` says that a second candidate also passes.  prior = "regressed" orders such a pair by distance to the regressed pose.
        The same seed gives the same bits.  eval() mode only; changes no module state and does not write to `intrinsics`."""
        from . import homography
        return homography.planar_pose_from_matches(self, images, intrinsics, heads, hypotheses, seed, refine, tau, subtoken, radius, vis_min,
                                                   prior)

    def rotation_from_matches(self, images, intrinsics, heads=(0, 1, 2), hypotheses=256, seed=0, refine=10, tau=None, subtoken=None,
                              radius=2):
        """The rotation of a pair that ONLY ROTATES (a panorama crop), from the matches: with t = 0 every essential matrix fits, so the
        chains above return a translation that means nothing.  `hypotheses` two-point rotation samples drawn from `seed`, each scored on
        all matches; the best one polished by `refine` Levenberg-Marquardt iterations over its three parameters ->
        rotation.RotationMatchPose, pose = (0, 0, 0, q).  Its stat[:, 1], the inlier weight share, is the evidence for "this pair only
        rotates": near the share of good matches on a rotating pair, a few percent on a translating one.  The same seed gives the same
        bits.  eval() mode only; changes no module state and does not write to `intrinsics`."""
        from . import rotation
        return rotation.rotation_from_matches(self, images, intrinsics, heads, hypotheses, seed, refine, tau, subtoken, radius)

    def auto_pose_from_matches(self, images, intrinsics, heads=(0, 1, 2), hypotheses=(1024, 256, 256), seed=0, refine=10, tau=None,
                               sigma=None, subtoken=None, radius=2, minimal="eight"):
        """WHICH of the three chains above to believe, decided from the matches themselves: the consensus chain, the planar chain and the
        rotation chain run on the same matches, and an information criterion (select.model_select) compares five
        candidates -- the E of the refined consensus pose, the E of the planar chain's two picks after `refine` iterations, H and R -- on
        one scale: the Sampson residuals under each, a noise scale estimated from the residuals (sigma: given instead), and an outlier
        that costs the same under every model -> select.AutoMatchPose: `kind` 0 essential, 1 homography, 2 rotation (-1: none) and the
        `pose` of the chosen model -- for H the planar chain's first pick, for R (0, 0, 0, q).  hypotheses: one number, or (consensus,
        planar, rotation).  The same seed gives the same bits.  eval() mode only; changes no module state and does not write to
        `intrinsics`."""
        from . import select
        return select.auto_pose_from_matches(self, images, intrinsics, heads, hypotheses, seed, refine, tau, sigma, subtoken, radius, minimal)

    def structure_from_matches(self, images, intrinsics, pose=None, chain="refined", **chain_kwargs):
        """Where the POINTS are: the matches triangulated under a pose -> triangulate.MatchStructure, whose `structure` holds per match the
        point (frame of camera 1, units of the baseline), its depth in both cameras, the squared reprojection error and the parallax, and
        per pair the robust reprojection cost, the share in front of both cameras and the mean parallax.  The pose is that of the chain
        `chain` -- "eight" (pose_from_matches), "refined", "consensus" or "planar" (its first pick), run with `chain_kwargs` -- or the given
        `pose` [B,7] as it is, e.g. the regressed one.  eval() mode only; changes no module state and does not write to `intrinsics`."""
        from . import triangulate
        return triangulate.structure_from_matches(self, images, intrinsics, pose, chain, **chain_kwargs)

    def pose_uncertainty_from_matches(self, images, intrinsics, pose=None, chain="consensus", **chain_kwargs):
        """HOW WELL the matches determine the pose: the covariance of the refined pose's five parameters (three rotation angles, two
        angles of the direction of t) as the sandwich estimate of the robust fit (covariance.pose_covariance), on the
        same matches, base weights and tau the chain's refinement used -> (what the chain returned, covariance.PoseCovariance): the
        standard deviations of the rotation and of the direction, the least determined direction, and a status that says "not
        determined" instead of a number where the matches do not fix the pose.  The pose is that of the chain `chain` -- "eight",
        "refined", "consensus" or "planar" (its first pick), run with `chain_kwargs` -- or the given `pose` [B,7] as it is.  eval() mode
        only; changes no module state and does not write to `intrinsics`."""
        from . import covariance
        return covariance.pose_uncertainty_from_matches(self, images, intrinsics, pose, chain, **chain_kwargs)

    def third_view_pose_from_matches(self, images, intrinsics, chain="consensus", hypotheses=256, seed=0, iters=10, min_parallax=None,
                                     **chain_kwargs):
        """WHERE a THIRD camera is, in units of the first pair's baseline: images [B,3,3,H,W] = (hub, a, c), intrinsics [B,3,4].  The
        matches of (hub, a) are triangulated under the pose of the chain `chain`, and the pose of c is fitted to those points and to the
        matches of (hub, c) -- row p of both pairs is the same token of the hub -- by three-point consensus and a six-parameter polish
        (resection.third_view_pose) -> resection.ThirdView, whose `scale` = |t_c| is the ratio of the two baselines.
        eval() mode only; changes no module state and does not write to `intrinsics`."""
        from . import resection
        return resection.third_view_pose(self, images, intrinsics, chain, hypotheses, seed, iters, min_parallax, **chain_kwargs)

    # -- guided matching (rel_pose_amd/guided.py; no counterpart in the reference) ----
    def guided_correspondences(self, images, intrinsics, pose, band=1.5):
        """The EMM's matches read again under `pose` [B,7]: per row and column the argmax over the tokens within `band` token pitches
        of the pose's epipolar line (-1 where none is), its weight, the mass inside the band and the total mass, the mutual matches and
        the in-band mass share per image and head -> guided.GuidedCorrespondences, usable by eightpoint.assemble_matches as it is.
        eval() mode only; changes no module state and does not write to `intrinsics`."""
        from . import guided
        return guided.guided_correspondences(self, images, intrinsics, pose, band)

    def pose_support(self, images, intrinsics, pose, band=1.5):
        """[2B,3]: how much of what the EMM attends to `pose` explains -- the share of the attention's mass within `band` token pitches
        of the pose's epipolar lines, per image and head.  Any two poses can be ranked by it.  eval() mode only."""
        from . import guided
        return guided.pose_support(self, images, intrinsics, pose, band)

    def guided_pose_from_matches(self, images, intrinsics, prior="consensus", band=1.5, rounds=1, iters=10, heads=(0, 1, 2), tau=None,
                                 subtoken=None, radius=2):
        """Guided matching: prior ("consensus", "regressed" or a pose [B,7]) -> guided_correspondences -> assemble_matches ->
        `iters` Levenberg-Marquardt iterations from the prior, `rounds` times -> guided.GuidedMatchPose with the support before and
        after.  Guided matches lie near the prior's lines by construction: judge the result by its support, not by its Sampson cost.
        eval() mode only; changes no module state and does not write to `intrinsics`."""
        from . import guided
        return guided.guided_pose_from_matches(self, images, intrinsics, prior, band, rounds, iters, heads, tau, subtoken, radius)

    def forward(self, images, Gs, intrinsics=None, inference=False):
        if not hasattr(Gs, "data") or isinstance(Gs, np.ndarray):
            Gs = SE3(torch.from_numpy(np.asarray(Gs)).unsqueeze(0).to(images.device).float())
        fmap, intrinsics = self.cnn_map(images, intrinsics)
        out = self.forward_tokens(fmap, Gs.data.to(torch.float32), intrinsics)
        if inference:
            return out[0].detach().cpu().numpy()
        return [SE3(out)]
