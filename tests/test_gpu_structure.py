"""ViTEss.structure_from_matches (rel_pose_amd/triangulate.py) and demo.py --points on a real MI355X: the structure of the matches is the
composition of the public pieces -- eightpoint._matches_of, the named chain, triangulate on the same matches, base weights and tau --
bit for bit, for each chain and for a passed pose; a randomly initialised model on the synthetic input of tests/test_gpu_consensus.py."""
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = {"eight": ("pose_from_matches", dict(iters=2)), "refined": ("refined_pose_from_matches", dict(refine=3)),
          "consensus": ("consensus_pose_from_matches", dict(hypotheses=128, seed=5, refine=2)),
          "planar": ("planar_pose_from_matches", dict(hypotheses=128, seed=5, refine=3))}


@pytest.fixture(scope="module")
def setup():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from oracle import relpose_oracle as O
    from rel_pose_amd import _lib
    from tests.test_gpu_memory_contract import _model
    _lib.load()
    _lib.load_triangulate()
    m = _model().eval()
    B = 2
    images = O.synthetic_images(B, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(B, 2, 1).contiguous().cuda()
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    m.correspondences(images)                                    # (warm-up)
    yield m, images, intr
    torch.backends.cudnn.deterministic = keep


def same(p, q):
    return all((a is None and b is None) or (torch.equal(a, b) if torch.is_tensor(a) else a == b if not isinstance(a, tuple) else same(a, b))
               for a, b in zip(p, q))


@pytest.mark.parametrize("chain", list(CHAINS) + ["pose"])
def test_structure_from_matches_is_the_composition_of_the_public_pieces(setup, chain):
    from rel_pose_amd import eightpoint, triangulate
    m, images, intr = setup
    B = images.shape[0]
    before = intr.clone()
    x1, x2, w, hw = eightpoint._matches_of(m, images, intr, (0, 1, 2), None, 2)
    tau = eightpoint.default_tau(intr, hw).to(x1.device).contiguous()
    if chain == "pose":                                          # the regressed pose, as a caller would pass it
        Gs = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device="cuda").repeat(B, 2, 1)
        with torch.no_grad():
            pose = m(images, Gs, intrinsics=intr.clone())[0].data[:, 1].contiguous()
        ms = m.structure_from_matches(images, intr, pose=pose)
        assert ms.chain is None
    else:
        name, kw = CHAINS[chain]
        result = getattr(m, name)(images, intr, **kw)
        pose = result.pose
        ms = m.structure_from_matches(images, intr, chain=chain, **kw)
        assert type(ms.chain) is type(result) and torch.equal(ms.chain.pose, pose)
    want = triangulate.triangulate(pose, x1, x2, w, tau=tau, return_corrected=True)
    assert torch.equal(intr, before) and not m.training
    assert torch.equal(ms.pose, pose) and torch.equal(ms.x1, x1) and torch.equal(ms.x2, x2) and torch.equal(ms.weights, w) and torch.equal(ms.tau, tau)
    assert same(ms.structure, want)
    s = ms.structure
    P = x1.shape[1]
    assert s.points.shape == (B, P, 3) and s.stat.shape == (B, 4) and s.corrected.shape == (B, P, 4)
    assert all(bool(torch.isfinite(t).all()) for t in s)
    assert torch.equal(s.stat[:, 3], (w > 0).sum(-1).float())
    live = pose[:, :3].norm(dim=-1) > 0                           # (the planar chain may have no candidate: a zero pose, a degenerate problem)
    assert bool((s.parallax[live].abs().sum(-1) > 0).all()) and not s.points[~live].any()


def test_structure_from_matches_raises_in_train_mode(setup):
    m, images, intr = setup
    m.train()
    try:
        for kw in ({}, dict(pose=torch.zeros(images.shape[0], 7, device="cuda")), dict(chain="eight")):
            with pytest.raises(RuntimeError, match="eval"):
                m.structure_from_matches(images, intr, **kw)
    finally:
        m.eval()


def test_demo_points_flag(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png"), "--eight_point"]
    ply, npz = str(tmp_path / "points.ply"), str(tmp_path / "points.npz")
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        torch.manual_seed(5)
        demo.main(argv + ["--points", ply])
        out = capsys.readouterr().out.splitlines()
        torch.manual_seed(5)
        demo.main(argv + ["--points", npz])
        again = capsys.readouterr().out.splitlines()
    finally:
        torch.backends.cudnn.deterministic = keep
    assert out == again and out[-1].startswith("structure: reprojection cost ")
    cost, front, par = (float(t) for t in re.findall(r"-?\d+\.\d+(?:e[-+]\d+)?", out[-1]))
    assert np.isfinite([cost, front, par]).all() and cost >= 0 and 0 <= front <= 1 and 0 <= par <= 180
    lines = open(ply).read().splitlines()
    end = lines.index("end_header")
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0"
    count = int([l for l in lines[:end] if l.startswith("element vertex ")][0].split()[2])
    vertices = lines[end + 1:]
    assert count == len(vertices)
    assert [l for l in lines[:end] if l.startswith("property ")] == ["property float x", "property float y", "property float z",
                                                                      "property uchar red", "property uchar green", "property uchar blue"]
    a = np.load(npz)
    assert int(a["keep"].sum()) == count and a["points"].shape == (1728, 3) and a["stat"].shape == (4,)
    assert bool(((a["depth1"] > 0) & (a["depth2"] > 0) & (a["weight"] >= 0.5) == a["keep"]).all())
    for l, p in zip(vertices, a["points"][a["keep"]]):
        t = l.split()
        assert len(t) == 6 and np.allclose([float(v) for v in t[:3]], p, atol=1e-6 * max(1.0, float(np.abs(p).max())))
        assert all(0 <= int(v) <= 255 for v in t[3:]) and float(t[2]) > 0
    assert abs(float(a["stat"][0]) / max(cost, 1e-30) - 1) < 1e-5 or cost == 0
    with pytest.raises(SystemExit):
        demo.main(argv[:4] + ["--points", ply])
