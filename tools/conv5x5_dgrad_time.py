"""rp_conv5x5_dgrad_f32 against MIOpen's fp32 backward-data at the tail's two valid 5x5 convolutions (conv2 192 -> 192, downsample.0
128 -> 192; 28 x 28 -> 24 x 24) at 12, 48, 64 and 128 images: sustained launches, the two interleaved in one process, three rounds.
FLOP = the convolution's 2 N 576 192 CI 25 (the own kernel forms exactly these products); fraction of the 157.3 TF fp32 matrix peak.
Usage: python tools/conv5x5_dgrad_time.py [N ...]  (output: profiles/conv5x5_dgrad_time.txt)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rel_pose_amd import ops
CL = torch.channels_last
SIZES = [int(a) for a in sys.argv[1:]] or [12, 48, 64, 128]


def timeit(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


print(torch.cuda.get_device_name(0), flush=True)
for CI, layer in ((192, "conv2"), (128, "downsample.0")):
    for N in SIZES:
        x = torch.empty(N, CI, 28, 28, device="cuda").contiguous(memory_format=CL)
        w = (torch.randn(192, CI, 5, 5, device="cuda") * (192 * 25) ** -0.5).contiguous(memory_format=CL)
        dy = torch.randn(N, 192, 24, 24, device="cuda").contiguous(memory_format=CL)
        wr, dyr = w.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
        assert wr.is_contiguous() and dyr.is_contiguous()
        gf = 2.0 * N * 576 * 192 * CI * 25
        own = lambda: ops.conv5x5_dgrad_f32(dyr, wr)
        mi = lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [True, False, False])
        t_own, t_mi = [], []
        for _ in range(3):
            t_own.append(timeit(own))
            t_mi.append(timeit(mi))
        o, m = sorted(t_own)[1], sorted(t_mi)[1]
        print("%-12s CI=%d N=%3d  own %7.1f us (%5.1f TF = %.2f) [%s]   MIOpen %7.1f us (%5.1f TF = %.2f) [%s]   own/MIOpen %.2f"
              % (layer, CI, N, o, gf / o * 1e-6, gf / o * 1e-6 / 157.3, " ".join("%.0f" % t for t in t_own), m, gf / m * 1e-6,
                 gf / m * 1e-6 / 157.3, " ".join("%.0f" % t for t in t_mi), o / m), flush=True)
