"""Times of the device conv stem (tactile_gym_amd.torch_layers.conv_stem; csrc/tg_conv_stem.hip) against torch on the same tensors and device,
F.relu(F.conv2d(x.float() / 255, w, b, stride=4)) as it comes (nothing about it is tuned), with torch autograd for forward plus backward.
Writes profiles/conv_stem_rate.txt.

  forward             1024 x 1 x 128 x 128 and 1024 x 2 x 256 x 256 uint8, under torch.no_grad()
  forward + backward  64 x 1 x 128 x 128 uint8: the layer, sum of y * dy as the loss, gradients of weight and bias

Each figure is the median over `--runs` runs (at least 20) of the device-event time of `--iters` back-to-back calls, divided by iters; the two
candidates of a shape take turns run by run after `--warmup` calls each.  The bytes are the ones the shapes need: the input read once and the
output written once.

    python tools/conv_stem_rate.py [--runs 30] [--iters 20] [--warmup 10] [--out profiles/conv_stem_rate.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters        # us per call


def compare(cands, args):
    """{name: (median, min, max) us per call}: warm-up, then the candidates alternated run by run."""
    import torch
    for _, fn in cands:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cands}
    for _ in range(args.runs):
        for name, fn in cands:
            times[name].append(timed(fn, args.iters))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_stem_rate.txt"))
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("--runs must be at least 20")
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("tools/conv_stem_rate.py measures on the GPU: no device found")
    import tactile_gym_amd as tg
    torch.manual_seed(0)
    lines = [f"# conv stem: us per call, median (min .. max) over {args.runs} alternated runs of {args.iters} calls each after {args.warmup} warm-up "
             f"calls; device events; {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "# torch baseline: F.relu(F.conv2d(x.float() / 255, w, b, stride=4)) on the same tensors, untuned; autograd for the backward"]
    verdict = None
    for B, Cn, H in ((1024, 1, 128), (1024, 2, 256)):
        x = torch.randint(0, 256, (B, Cn, H, H), dtype=torch.uint8, device="cuda")
        w, b = 0.05 * torch.randn(32, Cn, 8, 8, device="cuda"), 0.05 * torch.randn(32, device="cuda")

        def ours():
            with torch.no_grad():
                return tg.conv_stem(x, w, b)

        def theirs():
            with torch.no_grad():
                return F.relu(F.conv2d(x.float() / 255, w, b, stride=4))
        err = float((ours() - theirs()).abs().max())
        r = compare([("conv_stem  [1 launch]", ours), ("torch: float, div, conv2d, relu", theirs)], args)
        OH = (H - 8) // 4 + 1
        nbytes = x.numel() + 4 * B * 32 * OH * OH
        lines.append(f"forward {B} x {Cn} x {H} x {H} uint8 -> {B} x 32 x {OH} x {OH} float32 ({nbytes / 1e6:.1f} MB read once + written once; "
                     f"max |ours - torch| {err:.2e})")
        for name, (med, lo, hi) in r.items():
            lines.append(f"    {name:34s} {med:9.1f} us ({lo:.1f} .. {hi:.1f})   {nbytes / med / 1e3:7.1f} GB/s of those bytes")
        if (B, Cn, H) == (1024, 1, 128):
            a, t = r["conv_stem  [1 launch]"][0], r["torch: float, div, conv2d, relu"][0]
            verdict = (f"forward at 1024 x 1 x 128 x 128: conv_stem {a:.1f} us, torch {t:.1f} us: "
                       + ("not slower than the torch baseline" if a <= t else "SLOWER than the torch baseline"))
        del x
    B, Cn, H = 64, 1, 128
    x = torch.randint(0, 256, (B, Cn, H, H), dtype=torch.uint8, device="cuda")
    w = (0.05 * torch.randn(32, Cn, 8, 8, device="cuda")).requires_grad_()
    b = (0.05 * torch.randn(32, device="cuda")).requires_grad_()
    dy = torch.randn(B, 32, 31, 31, device="cuda")

    def ours_fb():
        w.grad = b.grad = None
        tg.conv_stem(x, w, b).backward(dy)

    def theirs_fb():
        w.grad = b.grad = None
        F.relu(F.conv2d(x.float() / 255, w, b, stride=4)).backward(dy)
    ours_fb()
    gw = w.grad.clone()
    theirs_fb()
    err = float((gw - w.grad).abs().max() / w.grad.abs().max())
    r = compare([("conv_stem  [1 + 2 launches]", ours_fb), ("torch autograd", theirs_fb)], args)
    lines.append(f"forward + backward {B} x {Cn} x {H} x {H} uint8 (dweight, dbias; max |ours - torch| / max |torch| of dweight {err:.2e})")
    for name, (med, lo, hi) in r.items():
        lines.append(f"    {name:34s} {med:9.1f} us ({lo:.1f} .. {hi:.1f})")
    lines.insert(0, "# " + verdict)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
