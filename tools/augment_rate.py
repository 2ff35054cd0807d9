"""Per-call time of the RAD translate augmentation (tactile_gym_amd.augment: RandomAffine(degrees=0, translate=[0.05, 0.05], scale=[1, 1], p=0.5)
on device tensors; csrc/tg_augment.hip) against the same operation written as torch ops on the GPU - kornia's path in float32: draws with torch
generators, the translation matrices, affine_grid, grid_sample(bilinear, zeros, align_corners=False) and the pass-through of unapplied samples.
Device events around `--iters` calls after `--warmup`, one line per (batch, image shape, input dtype).

Bytes moved = the input read once and the float32 output written once (from the shapes); GB/s = bytes over the per-call time, and the share of
the 6.29 TB/s float4 copy rate measured on MI355X.  Kernel time: a separate run under rocprofv3 --kernel-trace --stats.

    python tools/augment_rate.py [--iters 20] [--warmup 3] [--only-device]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29
BATCHES = (64, 4096, 16384)
SHAPES = ((2, 128, 128), (6, 128, 128))      # tactile frame_stack=2; visual frame_stack=2 (3 colours x 2), channels first


def torch_ops_path(x, ax=0.05, ay=0.05, p=0.5):
    import torch
    import torch.nn.functional as F
    B, _, H, W = x.shape
    xf = x.float()
    apply = torch.rand(B, device=x.device) < p
    tx = (torch.rand(B, device=x.device) * 2 - 1) * (ax * W)
    ty = (torch.rand(B, device=x.device) * 2 - 1) * (ay * H)
    theta = torch.zeros((B, 2, 3), device=x.device)
    theta[:, 0, 0] = 1.0
    theta[:, 1, 1] = 1.0
    theta[:, 0, 2] = -2.0 * tx / (W - 1)
    theta[:, 1, 2] = -2.0 * ty / (H - 1)
    grid = F.affine_grid(theta, list(xf.shape), align_corners=False)
    out = F.grid_sample(xf, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return torch.where(apply.view(B, 1, 1, 1), out, xf)


def time_calls(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-device", action="store_true", help="skip the torch-ops path (the profiler run)")
    args = ap.parse_args()
    import torch
    import tactile_gym_amd.augment as K
    dev = torch.device("cuda", 0)
    print(f"# {'path':9s} {'B':>6s} {'shape':>12s} {'in':>7s} {'us/call':>10s} {'MB moved':>9s} {'GB/s':>8s} {'of copy':>8s}", flush=True)
    for B in BATCHES:
        for shape in SHAPES:
            g = torch.Generator(device=dev).manual_seed(B)
            x8 = torch.randint(0, 256, (B,) + shape, dtype=torch.uint8, device=dev, generator=g)
            for name, x in (("uint8", x8), ("float32", x8.float())):
                n = x.numel()
                mb = n * (x.element_size() + 4) / 1e6
                m = K.RandomAffine(degrees=0, translate=[0.05, 0.05], scale=[1.0, 1.0], p=0.5, seed=1)
                paths = [("device", lambda: m(x))]
                if not args.only_device:
                    paths.append(("torch-ops", lambda: torch_ops_path(x)))
                for path, fn in paths:
                    us = time_calls(fn, args.iters, args.warmup)
                    gbs = mb * 1e6 / (us * 1e-6) / 1e9
                    print(f"  {path:9s} {B:6d} {'x'.join(map(str, shape)):>12s} {name:>7s} {us:10.1f} {mb:9.1f} {gbs:8.0f} {gbs / (COPY_TBS * 1000):8.2f}",
                          flush=True)
                del x
            del x8
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
