"""Per-call time of the general affine augmentation (tactile_gym_amd.augment.RandomWarp: degrees 10, translate 0.05, scale (0.9, 1.1), p = 0.5 on
device tensors; csrc/tg_affine.hip) against the only way to do it without the kernel: the same operation written as torch ops on the GPU -
draws with torch generators, the 3 x 3 matrices and their inverse, affine_grid, grid_sample(bilinear, zeros, align_corners=False) and the
pass-through of unapplied samples, in float32.  Device events around `--iters` calls after `--warmup`, the candidates alternated.

  1. fused call / torch ops / the translate kernel (the memory-rate yardstick) per (batch, input dtype) at [2, 128, 128], channels first.
  2. the two tap sources of k_random_affine at the same shapes, at p = 1 and p = 0.5: an aligned input takes the path affine_plan picks (source
     rows staged through LDS for planes up to 32 KiB: uint8 here; float32 128 x 128 planes are gathered), an input that starts one element past
     a 16-byte boundary always has its taps gathered from global memory.
  3. DeviceReplayBuffer.sample(B) with a RandomWarp against the same minibatch with a RandomTranslate.

Bytes moved = the input read once and the float32 output written once (from the shapes); GB/s = bytes over the per-call time, and the share of
the 6.29 TB/s float4 copy rate measured on MI355X.  Kernel time: a separate run under rocprofv3 --kernel-trace --stats.

    python tools/affine_rate.py [--iters 20] [--warmup 3] [--only-device]
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29
BATCHES = (64, 4096)
SHAPE = (2, 128, 128)
CFG = dict(degrees=10.0, translate=(0.05, 0.05), scale=(0.9, 1.1), p=0.5)


def torch_ops_path(x, degrees=10.0, ax=0.05, ay=0.05, s0=0.9, s1=1.1, p=0.5):
    import torch
    import torch.nn.functional as F
    B, _, H, W = x.shape
    dev = x.device
    xf = x.float()
    apply = torch.rand(B, device=dev) < p
    tx = (torch.rand(B, device=dev) * 2 - 1) * (ax * W)
    ty = (torch.rand(B, device=dev) * 2 - 1) * (ay * H)
    ang = (torch.rand(B, device=dev) * 2 - 1) * math.radians(degrees)
    sc = s0 + (s1 - s0) * torch.rand(B, device=dev)
    c, s = torch.cos(ang) * sc, torch.sin(ang) * sc
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    M = torch.zeros((B, 3, 3), device=dev)
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1], M[:, 2, 2] = c, -s, s, c, 1.0
    M[:, 0, 2] = cx + tx - (c * cx - s * cy)
    M[:, 1, 2] = cy + ty - (s * cx + c * cy)
    N = torch.tensor([[2.0 / (W - 1), 0.0, -1.0], [0.0, 2.0 / (H - 1), -1.0], [0.0, 0.0, 1.0]], device=dev)
    theta = (N @ torch.linalg.inv(M) @ torch.linalg.inv(N))[:, :2, :]
    grid = F.affine_grid(theta, list(xf.shape), align_corners=False)
    out = F.grid_sample(xf, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return torch.where(apply.view(B, 1, 1, 1), out, xf)


def time_alternated(fns, iters, warmup, rounds=4):
    """us per call of each fn: `rounds` windows of iters / rounds calls each, the candidates taking turns; the median window."""
    import torch
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    per = max(1, iters // rounds)
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) * 1000.0 / per)
    return [sorted(t)[len(t) // 2] for t in times], [(min(t), max(t)) for t in times]


def line(path, B, name, us, spread, mb):
    gbs = mb * 1e6 / (us * 1e-6) / 1e9
    print(f"  {path:18s} {B:6d} {'x'.join(map(str, SHAPE)):>10s} {name:>7s} {us:10.1f} {spread[0]:9.1f} {spread[1]:9.1f} {mb:9.1f} {gbs:8.0f} "
          f"{gbs / (COPY_TBS * 1000):8.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-device", action="store_true", help="skip the torch-ops path and the buffers (the profiler run)")
    args = ap.parse_args()
    import torch
    import tactile_gym_amd as tg
    import tactile_gym_amd.augment as K
    from tactile_gym_amd import spaces as sp
    dev = torch.device("cuda", 0)
    head = f"# {'path':18s} {'B':>6s} {'shape':>10s} {'in':>7s} {'us/call':>10s} {'min':>9s} {'max':>9s} {'MB moved':>9s} {'GB/s':>8s} {'of copy':>8s}"
    print("# 1. fused call, torch ops, translate yardstick\n" + head, flush=True)
    for B in BATCHES:
        g = torch.Generator(device=dev).manual_seed(B)
        x8 = torch.randint(0, 256, (B,) + SHAPE, dtype=torch.uint8, device=dev, generator=g)
        for name, x in (("uint8", x8), ("float32", x8.float())):
            mb = x.numel() * (x.element_size() + 4) / 1e6
            warp = K.RandomWarp(CFG["degrees"], translate=CFG["translate"], scale=CFG["scale"], p=CFG["p"], seed=1)
            tr = K.RandomTranslate(CFG["translate"], CFG["p"], seed=1)
            paths = [("affine", lambda: warp(x)), ("translate", lambda: tr(x))]
            if not args.only_device:
                paths.append(("torch-ops affine", lambda: torch_ops_path(x)))
            us, spread = time_alternated([f for _, f in paths], args.iters, args.warmup)
            for (path, _), u, s in zip(paths, us, spread):
                line(path, B, name, u, s, mb)
            if not args.only_device:
                print(f"    torch ops / fused call: {us[2] / us[0]:.1f}x; fused affine / translate: {us[0] / us[1]:.2f}x", flush=True)
            del x
        del x8
        torch.cuda.empty_cache()

    print("# 2. tap source: aligned input (staged through LDS up to 32 KiB planes, else gathered) against an input one element off (always gathered)\n" + head, flush=True)
    for B in BATCHES:
        for dtype, name in ((torch.uint8, "uint8"), (torch.float32, "float32")):
            n = B * SHAPE[0] * SHAPE[1] * SHAPE[2]
            flat = (torch.rand(n + 16, device=dev) * 255).to(dtype)
            xa, xo = flat[:n].view((B,) + SHAPE), flat[1:n + 1].view((B,) + SHAPE)
            assert xa.data_ptr() % 16 == 0 and xo.data_ptr() % 16 == flat.element_size()
            out = torch.empty((B,) + SHAPE, dtype=torch.float32, device=dev)
            mb = n * (flat.element_size() + 4) / 1e6
            for p in (1.0, 0.5):
                kw = dict(degrees=CFG["degrees"], translate=CFG["translate"], scale=CFG["scale"], p=p, seed=3, counter=0, out=out)
                us, spread = time_alternated([lambda: K.random_affine(xa, **kw), lambda: K.random_affine(xo, **kw)], args.iters, args.warmup)
                line(f"aligned p={p}", B, name, us[0], spread[0], mb)
                line(f"offset p={p}", B, name, us[1], spread[1], mb)
            del flat, xa, xo, out
            torch.cuda.empty_cache()
    if args.only_device:
        return

    print("# 3. DeviceReplayBuffer.sample(B, augment=...): one tactile key [2, 128, 128], 8192 stored transitions", flush=True)
    N, T = 256, 32
    space = sp.Dict({"tactile": sp.Box(low=0, high=255, shape=SHAPE, dtype=np.uint8)})
    buf = tg.DeviceReplayBuffer(T * N, space, sp.Box(low=-1.0, high=1.0, shape=(3,), dtype=np.float32), "cuda", n_envs=N, seed=0)
    for _ in range(T):
        img = lambda: {"tactile": torch.randint(0, 256, (N,) + SHAPE, dtype=torch.uint8, device=dev)}   # noqa: E731
        buf.add(img(), img(), torch.zeros((N, 3), device=dev), torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev))
    for B in BATCHES:
        warp = K.RandomWarp(CFG["degrees"], translate=CFG["translate"], scale=CFG["scale"], p=CFG["p"], seed=1)
        tr = K.RandomTranslate(CFG["translate"], CFG["p"], seed=1)
        us, spread = time_alternated([lambda: buf.sample(B, augment=warp), lambda: buf.sample(B, augment=tr)], args.iters, args.warmup)
        print(f"  sample({B:4d})  RandomWarp {us[0]:8.1f} us ({spread[0][0]:.1f} .. {spread[0][1]:.1f})   RandomTranslate {us[1]:8.1f} us "
              f"({spread[1][0]:.1f} .. {spread[1][1]:.1f})   ratio {us[0] / us[1]:.2f}", flush=True)


if __name__ == "__main__":
    main()
