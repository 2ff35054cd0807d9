"""Times of the device MLP towers (tactile_gym_amd.mlp; csrc/tg_mlp.hip) against torch nn modules of the same shapes and weights on the same
device, as they come (nothing about them is tuned), with torch autograd for forward plus backward.  Writes profiles/mlp_rate.txt (DESIGN.md
4.17).

  PPO heads   256 -> 256 -> 256 -> {2, 1} (Tanh), B = 1024: forward under torch.no_grad();  B = 64: forward + backward
  SAC critic  258 (256 + 2) -> 256 -> 256 -> 1, twice (ReLU), B = 64: forward + backward
  SAC actor   256 -> 256 -> 256 -> {2, 2} (ReLU), B = 64: forward + backward

Each figure is the median (and the minimum) over `--runs` runs (at least 20) of the device-event time of `--iters` back-to-back calls, divided
by iters; the two candidates of a shape take turns run by run after `--warmup` calls each.  The launches per call are counted with torch's
profiler on one call of each candidate.

    python tools/mlp_rate.py [--runs 30] [--iters 20] [--warmup 10] [--out profiles/mlp_rate.txt]
"""
import argparse
import copy
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


def launches(fn):
    """Device kernels of one call, counted by torch's profiler (memcpy / memset nodes are not kernels and are not counted)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len([n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()])


def torch_twin(module, kind):
    """The same parameters behind torch's own ops: nn.Sequential / nn.Linear calls, torch.cat for the critic's input."""
    import torch
    m = copy.deepcopy(module)
    if kind == "ppo":
        return lambda f: (m.action_net(m.mlp_extractor.policy_net(f)), m.log_std, m.value_net(m.mlp_extractor.value_net(f)).flatten()), m
    if kind == "actor":
        def run(f):
            z = m.latent_pi(f)
            return m.mu(z), m.log_std(z)
        return run, m

    def run(f, a):
        x = torch.cat([f, a], dim=1)
        return tuple(getattr(m, f"qf{i}")(x) for i in range(m.n_critics))
    return run, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_rate.txt"))
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("--runs must be at least 20")
    import torch
    from torch import nn
    if not torch.cuda.is_available():
        raise SystemExit("tools/mlp_rate.py measures on the GPU: no device found")
    import tactile_gym_amd as tg
    torch.manual_seed(0)
    lines = [f"# MLP towers: us per call, median (min .. max) over {args.runs} alternated runs of {args.iters} calls each after {args.warmup} warm-up "
             f"calls; device events; {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "# torch baseline: nn.Sequential / nn.Linear modules of the same shapes and weights, untuned; autograd for the backward; "
             "launches per call from torch's profiler"]
    verdicts = []
    shapes = [("PPO heads 256 -> 256 -> 256 -> {2, 1}, Tanh", "ppo", tg.ActorCriticHeads(256, 2, dict(pi=[256, 256], vf=[256, 256])), (1024, 64)),
              ("SAC critic 256 + 2 -> 256 -> 256 -> 1, x 2, ReLU", "critic", tg.ContinuousCriticHeads(256, 2, [256, 256]), (64,)),
              ("SAC actor 256 -> 256 -> 256 -> {2, 2}, ReLU", "actor", tg.SacActorHeads(256, 2, [256, 256]), (64,))]
    for title, kind, module, batches in shapes:
        module = module.cuda()
        theirs_fn, twin = torch_twin(module, kind)
        for B in batches:
            inputs = [torch.randn(B, 256, device="cuda")] + ([torch.rand(B, 2, device="cuda") * 2 - 1] if kind == "critic" else [])
            backward = not (kind == "ppo" and B == 1024)

            def outputs(out):
                return [out[0], out[2]] if kind == "ppo" else list(out)      # PPO: mean and values (log_std is the parameter itself)
            with torch.no_grad():
                a, b = outputs(module(*inputs)), outputs(theirs_fn(*inputs))
            err = max(float((x - y).abs().max()) for x, y in zip(a, b))
            dys = [torch.randn_like(t) for t in a]

            def make(fn, params):
                if not backward:
                    def run():
                        with torch.no_grad():
                            return fn(*inputs)
                    return run

                def run():
                    for p in params:
                        p.grad = None
                    outs = outputs(fn(*inputs))
                    torch.autograd.backward(outs, dys)
                return run
            ours, theirs = make(module, list(module.parameters())), make(theirs_fn, list(twin.parameters()))
            n_ours, n_theirs = launches(ours), launches(theirs)
            r = compare([("tg", ours), ("torch", theirs)], args)
            what = "forward + backward" if backward else "forward under no_grad"
            lines.append(f"{title}, B = {B}, {what} (max |ours - torch| of the outputs {err:.2e})")
            lines.append(f"    {'tg.mlp':12s} [{n_ours:3d} launches] {r['tg'][0]:9.1f} us ({r['tg'][1]:.1f} .. {r['tg'][2]:.1f})")
            lines.append(f"    {'torch nn':12s} [{n_theirs:3d} launches] {r['torch'][0]:9.1f} us ({r['torch'][1]:.1f} .. {r['torch'][2]:.1f})")
            ratio = r["torch"][0] / r["tg"][0]
            verdicts.append(f"{title.split(',')[0].split(' 2')[0]} B = {B} {what}: tg {r['tg'][0]:.1f} us, torch {r['torch'][0]:.1f} us, x{ratio:.2f}"
                            + ("" if ratio >= 1 else "  SLOWER than the torch baseline"))
    lines[0:0] = ["# " + v for v in verdicts]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
