"""Entry points on the GPU: train.py (synthetic data, few steps, checkpoint + auto-resume) and demo.py (reference's demo
images, random-init weights => plumbing only; the pretrained checkpoints are not obtainable offline)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)


def test_train_steps_checkpoint_and_resume(tmp_path):
    args = [os.path.join(ROOT, "train.py"), "--name", "t0", "--batch", "4", "--steps", "6", "--warmup", "2", "--fusion_transformer",
            "--image_size", "256", "320", "--num_workers", "0", "--dataset", "synthetic"]
    # (--gpus is left at the reference's default of 4: train.py clamps it to the one visible GPU and says so)
    r = run(args, str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "finished training!" in r.stdout and "GPU(s) visible" in r.stdout
    ck = tmp_path / "output" / "t0" / "checkpoints" / "000006.pth"
    assert ck.exists()
    import torch
    sd = torch.load(str(ck), map_location="cpu")
    assert set(sd) == {"model", "optimizer", "scheduler"} and len(sd["model"]) == 227
    # second invocation auto-resumes from the newest checkpoint (reference train.py:255-275)
    r2 = run(args[:6] + ["8"] + args[7:], str(tmp_path))
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert "resumed from" in r2.stdout


def test_train_in_the_bf16_configuration(tmp_path):
    """train.py --precision bf16 (BASELINE.json configs[4]: bf16 data path of the ViT / EMM + the hand-written bf16 convolutions of the CNN
    front-end): a few steps on synthetic 384 x 384 pairs run to the end with finite losses and write the reference's checkpoint layout."""
    args = [os.path.join(ROOT, "train.py"), "--name", "tb", "--batch", "4", "--steps", "5", "--warmup", "2", "--fusion_transformer",
            "--image_size", "384", "384", "--num_workers", "0", "--dataset", "synthetic", "--precision", "bf16"]
    r = run(args, str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "finished training!" in r.stdout and "nan" not in r.stdout.lower()
    import torch
    sd = torch.load(str(tmp_path / "output" / "tb" / "checkpoints" / "000005.pth"), map_location="cpu")
    assert len(sd["model"]) == 227 and all(torch.isfinite(v).all() for v in sd["model"].values() if v.is_floating_point())


def test_demo_runs_on_png_pair(tmp_path):
    import numpy as np
    import zlib, struct

    def write_png(path, arr):                       # 8-bit RGB, filter 0
        h, w, _ = arr.shape
        raw = b"".join(b"\x00" + arr[y].tobytes() for y in range(h))
        def chunk(t, d):
            return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
        with open(path, "wb") as f:
            f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                    chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))
    rng = np.random.default_rng(0)
    for n in ("a.png", "b.png"):
        write_png(str(tmp_path / n), rng.integers(0, 255, size=(480, 640, 3), dtype=np.uint8))
    r = run([os.path.join(ROOT, "demo.py"), "--img1", str(tmp_path / "a.png"), "--img2", str(tmp_path / "b.png")], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "predicted R&t" in r.stdout


def _fixed_batch(B=4, size=256):
    import torch
    g = torch.Generator().manual_seed(1)
    images = torch.floor(torch.rand(B, 2, 3, size, size, generator=g) * 255).cuda()
    q = torch.randn(B, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True) * torch.where(q[:, 3:] < 0, -1.0, 1.0)
    poses = torch.zeros(B, 2, 7)
    poses[:, :, 6] = 1
    poses[:, 1] = torch.cat([torch.rand(B, 3, generator=g) - 0.5, q], -1)
    intr = torch.tensor([[200.0, 200.0, size / 2.0, size / 2.0]]).repeat(B, 2, 1).cuda()
    return images, poses.cuda(), intr


def _model_args():
    import types
    return types.SimpleNamespace(noess="", pool_size=60, fc_hidden_size=512, fusion_transformer=True, transformer_depth=6,
                                 cross_features=False, use_single_softmax=False, no_pos_encoding=False, l1_pos_encoding=False)


class _precision:
    """the bf16 configuration of BASELINE.json configs[4] exactly as bench.py --precision bf16 sets it, restored on exit"""

    def __init__(self, name):
        self.bf = name == "bf16"

    def __enter__(self):
        from rel_pose_amd import ops
        if self.bf:
            ops.set_gemm_precision(1)
            ops.set_attention_precision(1)
            ops.set_cnn_precision(1)

    def __exit__(self, *a):
        from rel_pose_amd import ops
        ops.set_gemm_precision(0)
        ops.set_attention_precision(0)
        ops.set_cnn_precision(0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_overfits_a_fixed_batch(precision):
    """End-to-end sanity of forward + loss + backward + optimiser on the HIP path: a fixed batch of 4 pairs is memorised -- in the
    exact-fp32 configuration and, to the SAME criterion (loss below 0.35 x its initial value within 80 Adam steps), in the bf16
    configuration (bf16 data path of the ViT, bf16 convolutions): the bf16 configuration trains."""
    import torch
    from rel_pose_amd.losses import geodesic_loss_tensors
    from rel_pose_amd.model import ViTEss
    from rel_pose_amd.se3 import SE3
    torch.manual_seed(0)
    model = ViTEss(_model_args()).cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=2e-4)
    images, poses, intr = _fixed_batch()
    Ps = SE3(poses)
    Gs = SE3.IdentityLike(Ps)
    losses = []
    with _precision(precision):
        for _ in range(80):
            opt.zero_grad(set_to_none=True)
            est = model(images, Gs, intrinsics=intr.clone())
            ltr, lrot = geodesic_loss_tensors(Ps, est)
            loss = 10 * ltr + 10 * lrot
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 2.5)
            opt.step()
            losses.append(float(loss.detach()))
    with open(os.path.join(ROOT, "gpurun_out", "test_report.txt"), "a") as f:
        f.write("overfit_fixed_batch[%s]: first=%.4f last10_min=%.4f ratio=%.3f\n" % (precision, losses[0], min(losses[-10:]), min(losses[-10:]) / losses[0]))
    assert all(l == l for l in losses), "NaN in the loss"
    assert min(losses[-10:]) < 0.35 * losses[0], (losses[0], losses[-10:])


def test_bf16_configuration_gradients_point_where_the_fp32_gradients_point():
    """Every parameter gradient of one training step in the bf16 configuration against the exact-fp32 configuration on the same batch
    and weights (eval-mode BatchNorm, so that both see the same normalisation): cosine similarity and norm ratio PER TENSOR.  The
    max-norm bound of test_bf16_configuration_at_128_pairs_per_gpu (2e-1 of max|ref| on the token gradients) says little about
    direction; this does.  Stated: hot-path tensors (ViT / EMM / regressor) cosine > 0.98 and norm within 10 %; CNN trunk tensors
    (12 bf16 convolutions deep) cosine > 0.9 and norm within 25 %; bias / LayerNorm vectors whose fp32 gradient is below 1e-3 of
    the largest gradient norm are skipped (pure rounding noise in both)."""
    import torch
    from rel_pose_amd.losses import geodesic_loss_tensors
    from rel_pose_amd.model import ViTEss
    from rel_pose_amd.se3 import SE3
    torch.manual_seed(0)
    model = ViTEss(_model_args()).cuda().eval()
    images, poses, intr = _fixed_batch(B=8, size=384)
    Ps = SE3(poses)
    Gs = SE3.IdentityLike(Ps)
    grads = {}
    for prec in ("fp32", "bf16"):
        for p_ in model.parameters():
            p_.grad = None
        with _precision(prec):
            est = model(images, Gs, intrinsics=intr.clone())
            ltr, lrot = geodesic_loss_tensors(Ps, est)
            (10 * ltr + 10 * lrot).backward()
        grads[prec] = {n: p_.grad.detach().double().flatten().clone() for n, p_ in model.named_parameters() if p_.grad is not None}
    gmax = max(float(g.norm()) for g in grads["fp32"].values())
    worst_hot, worst_cnn, n_checked = (1.0, "", 1.0), (1.0, "", 1.0), 0
    for n, g32 in grads["fp32"].items():
        g16 = grads["bf16"][n]
        if float(g32.norm()) < 1e-3 * gmax:
            continue
        n_checked += 1
        cos = float(torch.dot(g32, g16) / (g32.norm() * g16.norm()))
        ratio = float(g16.norm() / g32.norm())
        cnn = n.startswith("resnet.") or n.startswith("extractor_final_conv.")
        if cnn and cos < worst_cnn[0]:
            worst_cnn = (cos, n, ratio)
        if not cnn and cos < worst_hot[0]:
            worst_hot = (cos, n, ratio)
        assert cos > (0.9 if cnn else 0.98), (n, cos, ratio)
        assert abs(ratio - 1.0) < (0.25 if cnn else 0.10), (n, cos, ratio)
    with open(os.path.join(ROOT, "gpurun_out", "test_report.txt"), "a") as f:
        f.write("bf16_vs_fp32_parameter_gradients: tensors=%d worst_hot cos=%.4f ratio=%.3f (%s) worst_cnn cos=%.4f ratio=%.3f (%s)\n"
                % (n_checked, worst_hot[0], worst_hot[2], worst_hot[1], worst_cnn[0], worst_cnn[2], worst_cnn[1]))
    assert n_checked >= 30                      # (36 of the 123 trainable tensors carry a gradient above the noise floor on this batch)


def _fake_matterport(root, n=6):
    import json
    import numpy as np
    from PIL import Image
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0)
    data = []
    for i in range(n):
        names = []
        for k in range(2):
            rel = "rgb/h%d/i_%d_%d.png" % (i, i, k)
            os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
            Image.fromarray(rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)).save(os.path.join(root, rel))
            names.append("/a/b/c/d/e/" + rel)
        q = Rotation.from_euler("xyz", [5 * i, -10, 3], degrees=True).as_quat()
        data.append({"0": {"file_name": names[0]}, "1": {"file_name": names[1]},
                     "rel_pose": {"position": [0.5 * i, -1.0, 0.25], "rotation": [float(q[3]), float(q[0]), float(q[1]), float(q[2])]}})
    os.makedirs(os.path.join(root, "mp3d_planercnn_json"), exist_ok=True)
    for split in ("train", "val", "test"):
        with open(os.path.join(root, "mp3d_planercnn_json", "cached_set_%s.json" % split), "w") as f:
            json.dump({"data": data}, f)


def test_train_and_evaluate_on_a_fake_matterport_dataset(tmp_path):
    """train.py --dataset matterport through rel_pose_amd/data_readers (PIL decode, colour jitter, resize, DataLoader workers),
    then test_matterport.py on the checkpoint it wrote: the reference's two entry points around the dataset layout."""
    root = str(tmp_path / "matterport_fake")
    _fake_matterport(root)
    r = run([os.path.join(ROOT, "train.py"), "--name", "m0", "--batch", "2", "--steps", "4", "--warmup", "2", "--fusion_transformer",
             "--dataset", "matterport", "--datapath", root, "--image_size", "192", "256", "--num_workers", "2"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "finished training!" in r.stdout
    ck = tmp_path / "output" / "m0" / "checkpoints" / "000004.pth"
    assert ck.exists()
    r = run([os.path.join(ROOT, "test_matterport.py"), "--datapath", root, "--exp", "e0", "--ckpt", str(ck), "--fusion_transformer"],
            str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    res = (tmp_path / "output" / "e0" / "matterport_test" / "results.txt").read_text()
    assert "R mean err" in res and "top1 T err < 1.0" in res


def test_bench_two_ranks_on_one_gpu():
    """bench.py's N>1 path (one process per rank, DDP gradient all-reduce, barrier + max-over-ranks timing) launched exactly as
    the driver launches it, but with both ranks sharing cuda:0 over gloo (RP_BENCH_SHARE_GPU: a 1-GPU box cannot run RCCL)."""
    import json
    env = dict(os.environ, PYTHONPATH=ROOT, RP_BENCH_SHARE_GPU="1", RP_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "8",
           "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 2 and rec["config"]["global_batch_pairs"] == 16 and rec["config"]["finite"] and rec["scaling"] == "weak"
    assert "cpu_baseline" not in rec and rec["roofline"]["launches_timed"] > 0
    assert len(rec["distributed"]["per_rank_ms_per_step"]) == 2 and rec["distributed"]["ms_per_step_no_allreduce"] > 0


def test_product_model_ddp_gradients_equal_full_batch(tmp_path):
    """The reference's only parallelism (train.py:28-36,66-67,128-130) on the PRODUCT model: two ranks, each with a full
    ViTEss replica under DistributedDataParallel and pairs r::2 of an 8-pair batch, must end up with the gradients of the
    single-process full batch after DDP's all-reduce(mean).  Both ranks share cuda:0 over gloo (one-GPU test box; on a node
    the same code runs over RCCL).  BatchNorm is in eval mode so that shard and full batch normalise identically
    ("BatchNorm under DDP"); tolerance = fp32 summation-order noise between 4- and 8-pair launches."""
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    out = tmp_path / "ddp.txt"
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(ROOT, "tests", "_ddp_product_worker.py"), str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    n, worst, name, worst_hot = out.read_text().split()[:4]
    with open(os.path.join(ROOT, "gpurun_out", "test_report.txt"), "a") as f:
        f.write("ddp_product_2ranks: tensors=%s worst=%s (%s) worst_hot_path=%s\n" % (n, worst, name, worst_hot))
    assert int(n) >= 120                                  # every trainable tensor (123: 227 state tensors minus buffers, layer3/4)
    assert float(worst_hot) < 2e-4, worst_hot             # ViT / EMM / regressor tensors (the HIP kernels)
    assert float(worst) < 1e-3, (worst, name)             # CNN trunk on MIOpen: 8- vs 16-image launches pick different split orders


def test_demo_reproduces_reference_demo_output(tmp_path):
    """BASELINE configs[0] / SURVEY 8c: this repo's demo.py on the reference's own demo/matterport_{1,2}.png (640x480 RGBA,
    committed as data under tests/golden/demo) with the closed-form checkpoint prints the [7] vector the reference's demo.py
    produced on the same files and weights (tests/golden/reference_demo.npz, generated by executing the reference's script)."""
    import numpy as np
    import torch
    from oracle import relpose_oracle as O
    sys.path.insert(0, ROOT)
    import demo
    shapes = dict(O.vit_param_shapes())
    shapes.update(O.cnn_param_shapes())
    sd32 = O.make_state(shapes, torch.float32)
    from rel_pose_amd.model import ViTEss
    import types
    args = types.SimpleNamespace(noess="", pool_size=60, fc_hidden_size=512, fusion_transformer=True, transformer_depth=6,
                                 cross_features=False, use_single_softmax=False, no_pos_encoding=False, l1_pos_encoding=False)
    full = ViTEss(args).state_dict()
    full.update(sd32)
    ck = str(tmp_path / "matterport_closed_form.pth")
    torch.save({"model": {"module." + k: v for k, v in full.items()}, "optimizer": {}, "scheduler": {}}, ck)
    g = os.path.join(ROOT, "tests", "golden")
    preds = demo.main(["--img1", os.path.join(g, "demo", "matterport_1.png"), "--img2", os.path.join(g, "demo", "matterport_2.png"),
                       "--ckpt", ck])
    ref = np.load(os.path.join(g, "reference_demo.npz"))["demo_matterport_pred7_f32"]
    err = float(np.abs(preds - ref).max() / np.abs(ref).max())
    with open(os.path.join(ROOT, "gpurun_out", "test_report.txt"), "a") as f:
        f.write("demo_vs_reference_demo: rel=%.3e pred=%s\n" % (err, np.array2string(preds, precision=5)))
    assert err < 1e-4


def test_bench_distributed_path_on_rccl_single_rank():
    """The N>1 code path of bench.py -- process group on backend "nccl" (= RCCL), DistributedDataParallel around the product
    model with its bucketed gradient all-reduce overlapping the backward, barrier + max-over-ranks timing -- run with ONE rank
    (RP_BENCH_FORCE_DIST), which is all a 1-GPU box can give RCCL.  Multi-rank RCCL remains unexercised."""
    import json
    env = dict(os.environ, PYTHONPATH=ROOT, RP_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29543",
               HSA_ENABLE_IPC_MODE_LEGACY="0", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
           "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["n_gpus"] == 1 and rec["config"]["finite"] and rec["roofline"]["launches_timed"] > 0
    # the scaling record diagnoses itself: per-rank step times and the step without the gradient exchange (timed after the judged region)
    d = rec["distributed"]
    assert len(d["per_rank_ms_per_step"]) == 1 and abs(d["per_rank_ms_per_step"][0] - rec["ms_per_step"]) < 1e-2
    assert d["ms_per_step_no_allreduce"] > 0 and d["gradient_bytes"] == 4 * 19258510
    assert abs(d["exposed_allreduce_ms"] - (rec["ms_per_step"] - d["ms_per_step_no_allreduce"])) < 1e-2


def test_bench_plain_run_prints_the_headline_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain bench.py run (no --full) times exactly --steps steps and prints the headline line without the --full records;
    --dump-outputs writes what its last timed step computed (here on the graph-replay path, the default at 8 pairs).  With the
    weights held at the seeded ones, two runs of the same command agree to rounding however many steps they time."""
    import json
    import numpy as np
    outs = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
               "--dump-outputs", str(tmp_path / run)]
        r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["config"]["finite"] and rec["config"]["launch"].startswith("HIP graph")
        assert abs(rec["value"] - 8 * 1e3 / rec["ms_per_step"]) < 1e-2 * rec["value"]
        assert not {"roofline", "supplementary", "cpu_baseline"} & set(rec)
        outs.append({f[:-len(".npy")]: np.load(str(tmp_path / run / f)) for f in os.listdir(str(tmp_path / run))})
    a, b = outs
    assert set(a) == {"poses", "loss", "grad_sample"}
    assert a["poses"].shape == (8, 2, 7) and a["loss"].shape == () and a["grad_sample"].shape == (1 << 22,)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert np.abs(a["grad_sample"]).max() > 0 and np.abs(a["poses"]).max() > 0
    assert abs(float(a["loss"]) - float(b["loss"])) < 1e-5 * abs(float(a["loss"]))
    assert np.abs(a["poses"] - b["poses"]).max() < 1e-4
    assert np.abs(a["grad_sample"] - b["grad_sample"]).max() < 1e-4 * np.abs(a["grad_sample"]).max()


def test_graphed_train_step_matches_the_eager_step():
    """rel_pose_amd/graph.py (bench.py --graph): the HIP-graph replay of forward + loss + backward | clip + Adam takes the same
    optimisation steps as the same functions run eagerly from the same initial state -- the losses of 4 consecutive steps agree to
    2e-4 / 1e-3 / 5e-3 / 1e-2 (measured 5e-6, 5e-6, 2e-5, 1.2e-4: the kernels are the same and deterministic, Adam on a random-init net amplifies the
    last-bit differences of MIOpen's solver choice under capture from step to step)."""
    import copy
    import types
    import torch
    from rel_pose_amd.graph import GraphedTrainStep
    from rel_pose_amd.model import ViTEss
    torch.manual_seed(0)
    args = types.SimpleNamespace(fusion_transformer=True, transformer_depth=6, fc_hidden_size=512, cross_features=False,
                                 use_single_softmax=False, no_pos_encoding=False, l1_pos_encoding=False, noess=False,
                                 feature_resolution=(24, 24), num_heads=3, total_num_features=192, pool_size=60)
    net0 = ViTEss(args).cuda().train()
    B = 2
    images = torch.floor(torch.rand(B, 2, 3, 384, 384, device="cuda") * 255.0)
    q = torch.nn.functional.normalize(torch.randn(B, 4, device="cuda"), dim=1)
    poses = torch.zeros(B, 2, 7, device="cuda")
    poses[:, 0, 6] = 1.0
    poses[:, 1, :3] = torch.rand(B, 3, device="cuda") - 0.5
    poses[:, 1, 3:] = q * torch.sign(q[:, 3:4])
    intr = torch.tensor([[192.0, 192.0, 192.0, 192.0]], device="cuda").repeat(B, 2, 1)
    losses = {}
    for mode in ("eager", "graph"):
        net = copy.deepcopy(net0)
        opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4, capturable=True)      # (non-fused: torch's fused capturable Adam is itself only reproducible to ~2e-3 of the loss after two
        # steps between two processes' orderings, tools/lab/graph_probe.py; bench.py --graph uses the fused one for speed)
        gs = GraphedTrainStep(net, opt, images, poses, intr)
        out = []
        if mode == "graph":
            gs.capture(warmup=2)                                        # 2 eager steps (lazy initialisation) + 4 replayed ones
            for _ in range(4):
                out.append(float(gs.step()))
            # replay, then an EAGER forward: the cached alignment pads of the CrossBlock / regressor weights (ops._padded) must follow
            # the parameters the replayed Adam step rewrote without bumping Tensor._version -- compare with a fresh
            # model that loads the same state and has no cache at all
            from rel_pose_amd.se3 import SE3
            Gs = SE3.IdentityLike(SE3(poses))
            with torch.no_grad():
                a = net(images, Gs, intrinsics=intr.clone())[0].data.clone()
                fresh = ViTEss(args).cuda().train()
                fresh.load_state_dict(net.state_dict())
                b = fresh(images, Gs, intrinsics=intr.clone())[0].data
            # (a stale pad would show up at the size of the weight updates, >= 1e-4; rounding-level differences between two model
            # instances come from MIOpen's workspace-dependent solver paths)
            assert float((a - b).abs().max()) < 5e-6, float((a - b).abs().max())
        else:
            for _ in range(6):
                gs._fwd_bwd()
                gs._exchange()
                gs._update()
                out.append(float(gs.loss))
        losses[mode] = out
    assert all(l == l and l > 0 for l in losses["graph"])
    assert losses["graph"][-1] != losses["graph"][0]                      # the replayed optimiser really moves the weights
    # Adam's first updates are ~lr * sign(g): a gradient whose sign flips with the rounding noise of MIOpen's atomically accumulated
    # weight gradients moves its parameter by 2 lr, and the difference compounds step by step (one full-suite run in ~17 exceeded a flat
    # 2e-3 on a later step).  The first replayed step is the check on the capture itself; the later ones bound the drift.
    for k, (a, b) in enumerate(zip(losses["eager"][2:], losses["graph"])):
        assert abs(a - b) <= (2e-4, 1e-3, 5e-3, 1e-2)[k] * abs(a), (k, losses)


def _closed_form_checkpoint(path):
    import types
    import torch
    from oracle import relpose_oracle as O
    from rel_pose_amd.model import ViTEss
    shapes = dict(O.vit_param_shapes())
    shapes.update(O.cnn_param_shapes())
    sd32 = O.make_state(shapes, torch.float32)
    args = types.SimpleNamespace(noess="", pool_size=60, fc_hidden_size=512, fusion_transformer=True, transformer_depth=6,
                                 cross_features=False, use_single_softmax=False, no_pos_encoding=False, l1_pos_encoding=False)
    full = ViTEss(args).state_dict()
    full.update(sd32)
    torch.save({"model": {"module." + k: v for k, v in full.items()}, "optimizer": {}, "scheduler": {}}, path)


def _metrics_close(got, ref, prefix, tol):
    import numpy as np
    names = ref[prefix + "_metric_names"].tolist()
    assert list(got.keys()) == names
    worst = 0.0
    for n, v in zip(names, ref[prefix + "_metric_values"]):
        worst = max(worst, abs(float(got[n]) - v) / max(1.0, abs(v)))
    assert worst <= tol, (prefix, worst)
    return worst


def test_evaluation_scripts_reproduce_the_references_runs(tmp_path, monkeypatch):
    """SURVEY 8f row 4 end to end: this repo's test_matterport.py / test_streetlearn_interiornet.py on the closed-form fake datasets
    (tests/_eval_cases.py) with the closed-form checkpoint, HIP model, against what the REFERENCE's scripts produced on the same
    files with the reference model on the CPU (tests/golden/reference_metrics.npz): raw model outputs (<= 1e-4 of max|ref|, the
    north_star R,t bound), converted predictions, ground truths (bit-identical: host arithmetic), every metric (<= 1e-4)."""
    import numpy as np
    from tests import _eval_cases as EC
    sys.path.insert(0, ROOT)
    import test_matterport
    import test_streetlearn_interiornet
    ref = np.load(os.path.join(ROOT, "tests", "golden", "reference_metrics.npz"))
    ck = str(tmp_path / "closed_form.pth")
    _closed_form_checkpoint(ck)
    monkeypatch.chdir(tmp_path)
    root = str(tmp_path / "matterport_fake")
    EC.write_matterport(root)
    m, p = test_matterport.main(["--datapath", root, "--exp", "e0", "--ckpt", ck, "--fusion_transformer"])
    raw_ref = ref["mp_script_raw_outputs_f32"]
    e_raw = float(np.abs(np.stack(p["raw"]) - raw_ref).max() / np.abs(raw_ref).max())
    assert np.array_equal(np.vstack(p["gt_rot"]), ref["mp_script_gt_rot"]) and np.array_equal(np.vstack(p["gt_tran"]), ref["mp_script_gt_tran"])
    e_pt = float(np.abs(np.vstack(p["pred_tran"]) - ref["mp_script_pred_tran"]).max())
    e_m = _metrics_close(m, ref, "mp_script", 1e-4)
    assert e_raw < 1e-4 and e_pt < 5e-4 and np.vstack(p["pred_tran"]).dtype == np.float32
    proot = str(tmp_path / "pano_fake")
    EC.write_panorama(proot, "interiornet")
    m2, p2 = test_streetlearn_interiornet.main(["--datapath", proot, "--exp", "e1", "--ckpt", ck, "--dataset", "interiornet", "--fusion_transformer"])
    raw_ref2 = ref["pano_script_raw_outputs_f32"]
    e_raw2 = float(np.abs(np.stack(p2["raw"]) - raw_ref2).max() / np.abs(raw_ref2).max())
    assert np.array_equal(np.vstack(p2["gt_rot"]), ref["pano_script_gt_rot"])
    e_m2 = _metrics_close(m2, ref, "pano_script", 1e-4)
    assert e_raw2 < 1e-4
    for f in ("results.txt", "all_rotation_err_degrees.csv", "all_gt_rot_degrees.csv"):
        assert os.path.exists(os.path.join(p2["out_dir"], f))
    assert open(os.path.join(p2["out_dir"], "all_gt_rot_degrees.csv")).read() == str(ref["pano_script_file_all_gt_rot_degrees.csv"])
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "test_report.txt"), "a") as f:
        f.write("eval_scripts_vs_reference_runs: matterport raw=%.2e pred_t=%.2e metrics=%.2e | interiornet raw=%.2e metrics=%.2e\n"
                % (e_raw, e_pt, e_m, e_raw2, e_m2))


FP32_SWITCHES = ["SPLITK_BATCHING", "ROWS_LINEAR", "ROWS_DX", "FUSE_LN_BWD", "DW192_F32", "COLSUM_BATCHING", "ATTN_BWD_STORE_DS",
                 "EMM_BWD_STORE_DS", "QKV_BIAS_FROM_PRODUCERS", "EMM_STATS_ONE_PASS", "FUSE_MLP", "FUSE_MLP_TRAIN", "FUSE_MLP_BWD", "MLP_BWD_LN",
                 "USE_SIDE_STREAM", "STEM_CONV", "STEM_STATS", "FUSE_STEM_POOL", "CONV3X3_WGRAD_F32_MIN_N", "STEM_WGRAD", "ATTN_STORE_P",
                 "EMM_STORE_S", "CONV3X3_F32_MIN_N", "CONV3X3_C128_F32_MIN_N", "CONV_F32_STATS", "CONV_F32_SHARE_INPUT", "CONV_F32_BN_BWD"]
BF16_SWITCHES = ["ACT_BF16", "BF16_PATH", "DX_LNBWD_BF16", "DW192", "MLP_W2_CHUNK_MAJOR", "MLP_BWD_LN", "CONV3X3_OWN", "CONV3X3_OWN_WGRAD", "STEM_CONV",
                 "STEM_WGRAD", "STEM_STATS", "CONV_BWD_AS_FWD_MIN_K"]


def _step_outputs(model, images, Gs, intr):
    import torch
    for p in model.parameters():
        p.grad = None
    out = model(images, Gs, intrinsics=intr.clone())[0].data
    out[:, 1].square().sum().backward()
    keys = ("resnet.conv1.weight", "resnet.layer1.0.conv1.weight", "resnet.layer1.1.conv2.weight", "extractor_final_conv.conv2.weight",
            "fusion_transformer.blocks.0.attn.qkv.weight", "fusion_transformer.blocks.2.mlp.fc1.weight", "fusion_transformer.blocks.2.mlp.fc2.weight",
            "fusion_transformer.blocks.5.cross_attn.qkv.weight", "fusion_transformer.blocks.4.norm2.weight", "pose_regressor.0.weight")
    named = dict(model.named_parameters())
    return out.detach().clone(), {k: named[k].grad.detach().double().flatten().clone() for k in keys}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_every_kernel_path_switch_has_a_working_alternative(precision):
    """every `RP_*` switch of rel_pose_amd/ops.py that selects an alternative kernel path is flipped, one at a
    time, on a whole training step of the product model (2 pairs, images in, train-mode BatchNorm): the alternative must run and give
    the default path's pose and gradients -- fp32: pose within 2e-4, every checked gradient cosine >= 0.9999 (the alternatives are the
    same arithmetic in another summation order or kernel); bf16 configuration: pose within 5e-2, cosine >= 0.97 (another rounding
    schedule) -- except the CNN front-end's own weight gradients, which at 2 pairs sit behind 12 layers of ReLU / max-pool masks that a
    bf16 rounding flips (test_bf16_convolution_front_end...: 0.958 between fp32 and bf16): >= 0.85.  A switch whose alternative no longer
    works fails here instead of rotting."""
    import types
    import torch
    from rel_pose_amd import ops
    from rel_pose_amd.model import ViTEss
    torch.manual_seed(0)
    args = types.SimpleNamespace(noess="", pool_size=60, fc_hidden_size=512, fusion_transformer=True, transformer_depth=6,
                                 cross_features=False, use_single_softmax=False, no_pos_encoding=False, l1_pos_encoding=False)
    model = ViTEss(args).cuda().train()
    images = torch.floor(torch.rand(2, 2, 3, 384, 384, device="cuda") * 255.0)
    Gs = torch.tensor([0, 0, 0, 0, 0, 0, 1.0]).repeat(2, 2, 1).cuda()
    intr = torch.tensor([[192.0, 192.0, 192.0, 192.0]]).repeat(2, 2, 1).cuda()
    bn = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    bf = precision == "bf16"
    ops.set_gemm_precision(1 if bf else 0)
    ops.set_attention_precision(1 if bf else 0)
    ops.set_cnn_precision(1 if bf else 0)
    tol_pose, tol_cos = (5e-2, 0.97) if bf else (2e-4, 0.9999)
    try:
        base_out, base_g = _step_outputs(model, images, Gs, intr)
        model.load_state_dict(bn, strict=False)
        bad = {}
        for name in (BF16_SWITCHES if bf else FP32_SWITCHES):
            old = getattr(ops, name)
            setattr(ops, name, (99 if name == "CONV_BWD_AS_FWD_MIN_K" else 0 if name in ("CONV3X3_WGRAD_F32_MIN_N", "CONV3X3_F32_MIN_N", "CONV3X3_C128_F32_MIN_N") else 2 if (name == "MLP_BWD_LN" and not bf) else (not old)))      # (MLP_BWD_LN = 2: the fold with fp32 operands too; CONV3X3_WGRAD_F32_MIN_N / CONV3X3_F32_MIN_N = 0: the own fp32 layer1 kernels at this 4-image batch)
            try:
                out, g = _step_outputs(model, images, Gs, intr)
            finally:
                setattr(ops, name, old)
                model.load_state_dict(bn, strict=False)
            e_pose = float((out - base_out).abs().max() / base_out.abs().max())
            cs = {k: float(torch.dot(g[k], base_g[k]) / (g[k].norm() * base_g[k].norm()).clamp_min(1e-300)) for k in g}
            # (a switch that changes the FIRST layers' rounding schedule in bf16 perturbs every activation behind it: at 2 pairs and
            # random init the late gradients move with it -- the kernels themselves are pinned against fp64 in test_gpu_kernels.py)
            front = bf and name in ("STEM_CONV", "CONV3X3_OWN")
            ok = all(c >= (0.85 if (front or (bf and k.startswith(("resnet", "extractor")))) else tol_cos) for k, c in cs.items())
            if not (torch.isfinite(out).all() and e_pose < tol_pose and ok):
                bad[name] = (e_pose, min(cs.values()))
        assert not bad, bad
    finally:
        ops.set_gemm_precision(0)
        ops.set_attention_precision(0)
        ops.set_cnn_precision(0)
