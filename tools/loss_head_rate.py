"""Times of the device loss heads (tactile_gym_amd.loss_head; csrc/tg_loss_head.hip) against the same lines written with torch's own ops on the
same tensors and device, forward plus backward under torch autograd on both sides.  Writes profiles/loss_head_rate.txt.

  ppo_loss   B = 64 and 8192, A = 2 and 6, log_std [A]: PPO.train from evaluate_actions to loss.backward(), gradients at mean, log_std, values
  rsample    B = 64 and 256, A = 2: SAC's actor.action_log_prob and the backward from given gradients of actions and log_prob

Both are latency-bound chains of small launches, so two times are given per candidate: the device-event time of `--iters` back-to-back calls
divided by iters (the queue never drains: what a training loop sees), and the host wall time of the same calls up to a final synchronize.
Each figure is the median over `--runs` runs (at least 20); the two candidates of a shape take turns run by run after `--warmup` calls each.
The kernel count is what torch's profiler sees on the device for ONE call (forward + backward) of each side.

    python tools/loss_head_rate.py [--runs 30] [--iters 50] [--warmup 20] [--out profiles/loss_head_rate.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    """(device-event us per call, host wall us per call) of iters back-to-back calls."""
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    wall = time.perf_counter() - t0
    return start.elapsed_time(end) * 1e3 / iters, wall * 1e6 / iters


def compare(cands, args):
    """{name: ((median, min, max) device us, (median, min, max) wall us)}: warm-up, then the candidates alternated run by run."""
    import torch
    for _, fn in cands:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cands}
    for _ in range(args.runs):
        for name, fn in cands:
            times[name].append(timed(fn, args.iters))
    spread = lambda v: (statistics.median(v), min(v), max(v))   # noqa: E731
    return {name: (spread([d for d, _ in t]), spread([w for _, w in t])) for name, t in times.items()}


def kernels(fn):
    """Device kernels of one call, by torch's profiler; None where it cannot trace the device."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:   # noqa: BLE001
        return None


def torch_ppo(mean, log_std, values, actions, old_log_prob, advantages, returns, old_values, clip_range, clip_range_vf, ent_coef, vf_coef):
    """PPO.train's lines as stable_baselines3 writes them."""
    import torch
    import torch.nn.functional as F
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp())
    log_prob, entropy = dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)
    adv = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    ratio = torch.exp(log_prob - old_log_prob)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    values_pred = old_values + torch.clamp(values - old_values, -clip_range_vf, clip_range_vf)
    value_loss = F.mse_loss(returns, values_pred)
    loss = policy_loss + ent_coef * -torch.mean(entropy) + vf_coef * value_loss
    with torch.no_grad():                             # SB3 logs these per minibatch
        log_ratio = log_prob - old_log_prob
        torch.mean((torch.exp(log_ratio) - 1) - log_ratio)
        torch.mean((torch.abs(ratio - 1) > clip_range).float())
    return loss


def torch_rsample(mean, log_std, noise):
    import torch
    log_std = torch.clamp(log_std, -20, 2)
    dist = torch.distributions.Normal(mean, log_std.exp())
    x = mean + dist.scale * noise
    a = torch.tanh(x)
    return a, dist.log_prob(x).sum(dim=1) - torch.log(1 - a ** 2 + 1e-6).sum(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_head_rate.txt"))
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("--runs must be at least 20")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/loss_head_rate.py measures on the GPU: no device found")
    import tactile_gym_amd as tg
    from tactile_gym_amd import spaces
    torch.manual_seed(0)
    lines = [f"# loss heads, forward + backward: us per call, median (min .. max) over {args.runs} alternated runs of {args.iters} back-to-back calls "
             f"each after {args.warmup} warm-up calls; device events | host wall; {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "# torch baseline: stable_baselines3's lines with torch's own ops on the same tensors, torch autograd; kernels: of one call, by "
             "torch's profiler"]
    verdicts = []

    def report(title, r, counts):
        lines.append(title)
        for name, ((med, lo, hi), (wmed, wlo, whi)) in r.items():
            n = counts[name]
            lines.append(f"    {name:28s} {med:8.1f} us ({lo:.1f} .. {hi:.1f}) | wall {wmed:8.1f} us ({wlo:.1f} .. {whi:.1f})   "
                         f"{'kernels not counted' if n is None else f'{n} kernels'}")

    for B, A in ((64, 2), (64, 6), (8192, 2), (8192, 6)):
        f32 = dict(dtype=torch.float32, device="cuda")
        mean, log_std, values = (torch.randn(B, A, **f32).requires_grad_(), torch.full((A,), -1.0, **f32).requires_grad_(),
                                 torch.randn(B, **f32).requires_grad_())
        actions = (mean + log_std.exp() * torch.randn(B, A, **f32)).detach()
        with torch.no_grad():
            old_lp = torch.distributions.Normal(mean, log_std.exp()).log_prob(actions).sum(dim=1) + 0.1 * torch.randn(B, **f32)
        adv, ret, old_values = torch.randn(B, **f32), torch.randn(B, **f32), (values + 0.2 * torch.randn(B, **f32)).detach()
        kw = dict(clip_range=0.2, clip_range_vf=0.2, ent_coef=0.01, vf_coef=0.5)
        leaves = (mean, log_std, values)

        def ours():
            for t in leaves:
                t.grad = None
            tg.ppo_loss(mean, log_std, values, actions, old_lp, adv, ret, old_values=old_values, **kw)[0].backward()

        def theirs():
            for t in leaves:
                t.grad = None
            torch_ppo(mean, log_std, values, actions, old_lp, adv, ret, old_values, **kw).backward()
        ours()
        g = mean.grad.clone()
        theirs()
        err = float((g - mean.grad).abs().max() / mean.grad.abs().max())
        names = ("tg.ppo_loss", "torch ops + autograd")
        r = compare(list(zip(names, (ours, theirs))), args)
        report(f"ppo_loss B = {B}, A = {A}, log_std [A] (max |ours - torch| / max |torch| of dmean {err:.2e})", r,
               dict(zip(names, (kernels(ours), kernels(theirs)))))
        if B == 64:
            a, t = r[names[0]][0][0], r[names[1]][0][0]
            verdicts.append(f"ppo_loss B = 64, A = {A}: fused {a:.1f} us, torch {t:.1f} us: " + ("not slower" if a <= t else "SLOWER") + " than the composition")
    box = spaces.Box(low=-1.0, high=1.0, shape=(2,), dtype=np.float32)
    for B in (64, 256):
        head = tg.DeviceSquashedDiagGaussian(box, seed=1)
        mean, log_std = torch.randn(B, 2, device="cuda").requires_grad_(), (-1.0 + torch.randn(B, 2, device="cuda")).requires_grad_()
        noise, g_a, g_lp = torch.randn(B, 2, device="cuda"), torch.randn(B, 2, device="cuda"), torch.randn(B, device="cuda")

        def ours():
            mean.grad = log_std.grad = None
            torch.autograd.backward(head.rsample(mean, log_std, noise=noise), (g_a, g_lp))

        def theirs():
            mean.grad = log_std.grad = None
            torch.autograd.backward(torch_rsample(mean, log_std, noise), (g_a, g_lp))
        ours()
        g = log_std.grad.clone()
        theirs()
        err = float((g - log_std.grad).abs().max() / log_std.grad.abs().max())
        names = ("head.rsample", "torch ops + autograd")
        r = compare(list(zip(names, (ours, theirs))), args)
        report(f"rsample B = {B}, A = 2 (max |ours - torch| / max |torch| of dlog_std {err:.2e})", r, dict(zip(names, (kernels(ours), kernels(theirs)))))
        if B == 64:
            a, t = r[names[0]][0][0], r[names[1]][0][0]
            verdicts.append(f"rsample B = 64: fused {a:.1f} us, torch {t:.1f} us: " + ("not slower" if a <= t else "SLOWER") + " than the composition")
    text = "\n".join(["# " + v for v in verdicts] + lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
