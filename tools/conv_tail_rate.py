"""Times and launch counts of tg.NatureCNN(device_tail=True) - conv2, conv3 and the linear layer on csrc/tg_conv.hip - against
tg.NatureCNN(device_tail=False), the module as it was before the device tail (the same stem, torch's conv2d / linear / relu behind it), with
the same weights on the same tensors and device.  Writes profiles/conv_tail_rate.txt.

  forward             1024 x 1 x 128 x 128 uint8 under torch.no_grad(): the whole module, and each tail layer on its own input
  forward + backward  64 x 1 x 128 x 128 uint8: the whole module (gradients of all eight parameters), and each tail layer (gradients of its
                      input, weight and bias)

Each figure is the median over `--runs` runs (at least 20) of the device-event time of `--iters` back-to-back calls, divided by iters; the two
candidates of a shape take turns run by run after `--warmup` calls each.  Launch counts: on the device tail's side the library's entries
called times the launches each one documents (include/tactile_gym_hip.h) plus the aten operators torch dispatches around them; on torch's side
the aten operators dispatched (allocations, views and detach left out: every one counted is at least one kernel launch, a convolution's
backward is several).

    python tools/conv_tail_rate.py [--runs 20] [--iters 10] [--warmup 5] [--out profiles/conv_tail_rate.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENTRY_LAUNCHES = {"tg_conv_stem": 1, "tg_conv_stem_bwd": 2, "tg_conv_relu": 1}          # tg_conv_relu_bwd: 2, 3 with dx
NO_LAUNCH = ("empty", "view", "detach", "alias", "as_strided", "reshape", "expand", "permute", "transpose", "t.", "squeeze", "unsqueeze",
             "_unsafe_view", "flatten", "select", "slice", "is_", "sym_", "stride", "size", "numel", "_local_scalar", "lift")


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


def launches(fn):
    """(library launches, aten operators) of one call of fn."""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from tactile_gym_amd import _device
    counts = [0, 0]

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func).replace("aten.", "")
            if not any(name.startswith(p) for p in NO_LAUNCH):
                counts[1] += 1
            return func(*args, **(kwargs or {}))
    real = _device.call

    def spy(entry, *a):
        counts[0] += ENTRY_LAUNCHES.get(entry, 0)
        if entry == "tg_conv_relu_bwd":
            counts[0] += 2 + (a[14].value is not None)
        return real(entry, *a)
    _device.call = spy
    try:
        with Count():
            fn()
    finally:
        _device.call = real
    torch.cuda.synchronize()
    return tuple(counts)


def report(lines, title, cands, args):
    r = compare(cands, args)
    lines.append(title)
    for name, fn in cands:
        med, lo, hi = r[name]
        lib, aten = launches(fn)
        lines.append(f"    {name:30s} {med:10.1f} us ({lo:.1f} .. {hi:.1f})   launches: {lib} of the library + {aten} aten operators")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_tail_rate.txt"))
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("--runs must be at least 20")
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("tools/conv_tail_rate.py measures on the GPU: no device found")
    import tactile_gym_amd as tg

    class Space:
        shape = (1, 128, 128)
    torch.manual_seed(0)
    tail = tg.NatureCNN(Space(), features_dim=512, device_tail=True).cuda()
    plain = tg.NatureCNN(Space(), features_dim=512, device_tail=False).cuda()
    plain.load_state_dict(tail.state_dict(), strict=True)
    lines = [f"# NatureCNN tail (conv2, conv3, linear; 1 x 128 x 128 uint8, features_dim 512): us per call, median (min .. max) over {args.runs} "
             f"alternated runs of {args.iters} calls each after {args.warmup} warm-up calls; device events; {torch.cuda.get_device_name(0)}, "
             f"torch {torch.__version__}",
             "# device_tail=False is the module as it was: the same device stem, then torch's conv2d, relu, conv2d, relu, flatten, linear, relu"]
    layers = [("conv2", (32, 31, 31), tail.cnn[2], lambda x, m: F.relu(F.conv2d(x, m.weight, m.bias, stride=2))),
              ("conv3", (64, 14, 14), tail.cnn[4], lambda x, m: F.relu(F.conv2d(x, m.weight, m.bias, stride=1))),
              ("linear", (64, 12, 12), tail.linear[0], lambda x, m: F.relu(F.linear(x.flatten(1), m.weight, m.bias)))]
    summary = []
    # ---- forward under no_grad at B = 1024
    B = 1024
    x8 = torch.randint(0, 256, (B, 1, 128, 128), dtype=torch.uint8, device="cuda")
    with torch.no_grad():
        err = float((tail(x8) - plain(x8)).abs().max())

    def fwd(m):
        def run():
            with torch.no_grad():
                return m(x8)
        return run
    r = report(lines, f"forward, no_grad, {B} x 1 x 128 x 128 uint8 -> {B} x 512 (max |tail - torch| {err:.2e})",
               [("device_tail=True", fwd(tail)), ("device_tail=False", fwd(plain))], args)
    summary.append(f"forward at B = {B}: device tail {r['device_tail=True'][0]:.0f} us, torch tail {r['device_tail=False'][0]:.0f} us")
    for name, shape, mod, theirs in layers:
        x = torch.randn((B,) + shape, device="cuda").abs_()

        def ours_l(x=x, mod=mod):
            with torch.no_grad():
                return mod(x)

        def theirs_l(x=x, mod=mod, theirs=theirs):
            with torch.no_grad():
                return theirs(x, mod)
        report(lines, f"  {name} alone, forward, no_grad, input {B} x {' x '.join(map(str, shape))}", [("tg", ours_l), ("torch", theirs_l)], args)
        del x
    del x8
    # ---- forward + backward at B = 64
    B = 64
    x8 = torch.randint(0, 256, (B, 1, 128, 128), dtype=torch.uint8, device="cuda")
    dy = torch.randn(B, 512, device="cuda")

    def fb(m):
        def run():
            for p in m.parameters():
                p.grad = None
            m(x8).backward(dy)
        return run
    fb(tail)()
    g_tail = tail.linear[0].weight.grad.clone()
    fb(plain)()
    g_plain = plain.linear[0].weight.grad
    err = float((g_tail - g_plain).abs().max() / g_plain.abs().max())
    with torch.no_grad():                                                     # an output within rounding of zero may be clamped on one side only:
        flips = int(((tail(x8) > 0) != (plain(x8) > 0)).sum())                # one such element moves a whole row of the linear's dweight
    r = report(lines, f"forward + backward, {B} x 1 x 128 x 128 uint8, all eight parameters (max |tail - torch| / max |torch| of the linear's "
               f"dweight {err:.2e}; {flips} of {B * 512} outputs clamped on one side only)", [("device_tail=True", fb(tail)), ("device_tail=False", fb(plain))], args)
    summary.append(f"forward + backward at B = {B}: device tail {r['device_tail=True'][0]:.0f} us, torch tail {r['device_tail=False'][0]:.0f} us")
    for name, shape, mod, theirs in layers:
        x = torch.randn((B,) + shape, device="cuda").abs_().requires_grad_()
        with torch.no_grad():
            dyl = torch.randn_like(mod(x))

        def ours_l(x=x, mod=mod, dyl=dyl):
            x.grad = mod.weight.grad = mod.bias.grad = None
            mod(x).backward(dyl)

        def theirs_l(x=x, mod=mod, theirs=theirs, dyl=dyl):
            x.grad = mod.weight.grad = mod.bias.grad = None
            theirs(x, mod).backward(dyl)
        report(lines, f"  {name} alone, forward + backward (dx, dweight, dbias), input {B} x {' x '.join(map(str, shape))}",
               [("tg", ours_l), ("torch", theirs_l)], args)
    lines[0:0] = ["# " + s for s in summary]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
