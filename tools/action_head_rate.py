"""Times of the device action heads (tactile_gym_amd.action_head; csrc/tg_action_head.hip) against the same outputs composed from torch ops, by
device events around `--iters` calls after `--warmup`, the candidates alternated `--rounds` times; its output belongs in
profiles/action_head_rate.txt.

  call    head.sample at N = 1024 and 16 384, A = 2 and 6, both heads, against torch's Normal(...).rsample, log_prob().sum(1), clamp (and the
          tanh variant with its correction and unscale_action): device time per call, and the host clock around the same calls when they are
          not waited for
  loop    edge_follow-v0, 128 x 128, 1024 envs, per iteration: step + head + DeviceRolloutBuffer.add, and step + head +
          DeviceReplayBuffer.add_from_env, against the same loops with the torch-op stage

    python tools/action_head_rate.py [--section call|loop|all] [--iters 200] [--warmup 20] [--rounds 3]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from replay_rate import EDGE, alternate  # noqa: E402


def torch_gaussian(mean, log_std, lo, hi):
    """What SB3's collect_rollouts runs: the distribution, its sample, the summed log-prob, the clip for the env."""
    import torch
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp())
    actions = dist.rsample()
    return actions, torch.clamp(actions, lo, hi), dist.log_prob(actions).sum(dim=1)


def torch_squashed(mean, log_std, lo, hi):
    """SAC's actor head and _sample_action: the clamp of log_std, the tanh sample with its corrected log-prob, unscale_action."""
    import torch
    dist = torch.distributions.Normal(mean, torch.clamp(log_std, -20.0, 2.0).exp())
    gaussian = dist.rsample()
    actions = torch.tanh(gaussian)
    log_prob = dist.log_prob(gaussian).sum(dim=1) - torch.log(1 - actions ** 2 + 1e-6).sum(dim=1)
    return actions, lo + (0.5 * (actions + 1.0) * (hi - lo)), log_prob


def _report(label, cands, args):
    dev, host = alternate(cands, args.iters, args.warmup, args.rounds)
    for name, _ in cands:
        print(f"  {label}  {name:40s} device {min(dev[name]):8.2f} us (rounds: {' '.join(f'{x:.2f}' for x in dev[name])})   "
              f"host enqueue {min(host[name]):8.2f} us (rounds: {' '.join(f'{x:.2f}' for x in host[name])})", flush=True)


def section_call(args):
    import numpy as np
    import torch
    import tactile_gym_amd as tg
    from tactile_gym_amd import spaces
    print(f"# call: us per call, {args.rounds} alternated rounds of {args.iters} calls (device events; host: the clock round the unwaited calls)")
    for N in (1024, 16384):
        for A in (2, 6):
            space = spaces.Box(low=-0.25, high=0.25, shape=(A,), dtype=np.float32)
            lo, hi = torch.full((A,), -0.25, device="cuda:0"), torch.full((A,), 0.25, device="cuda:0")
            mean = torch.rand((N, A), device="cuda:0") - 0.5
            ls_a, ls_na = torch.full((A,), -1.5, device="cuda:0"), torch.rand((N, A), device="cuda:0") - 2.0
            g = tg.DeviceDiagGaussian(space, seed=1, num_envs=N, device="cuda:0")
            s = tg.DeviceSquashedDiagGaussian(space, seed=1, num_envs=N, device="cuda:0")
            cands = [("DeviceDiagGaussian.sample  [1 launch]", lambda: g.sample(mean, ls_a)),
                     ("torch ops, Gaussian", lambda: torch_gaussian(mean, ls_a, lo, hi)),
                     ("DeviceSquashedDiagGaussian.sample  [1]", lambda: s.sample(mean, ls_na)),
                     ("torch ops, squashed", lambda: torch_squashed(mean, ls_na, lo, hi)),
                     ("sample_uniform  [1 launch]", lambda: s.sample_uniform())]
            _report(f"N {N:6d} A {A}", cands, args)


def section_loop(args, N=1024, T=16):
    import torch
    import tactile_gym_amd as tg
    print(f"# loop: edge_follow-v0, 128 x 128, {N} envs, obs_mode torch; us per iteration, {args.rounds} alternated rounds of {args.iters} "
          f"iterations (every step waits for its rewards, so host and device times nearly coincide)")
    envs = [tg.make_vec("edge_follow-v0", num_envs=N, max_steps=200, image_size=[128, 128], env_modes=EDGE, seed=1 + i, obs_mode="torch")
            for i in range(4)]
    try:
        lo, hi = torch.full((2,), -0.25, device="cuda:0"), torch.full((2,), 0.25, device="cuda:0")
        mean, values = (torch.rand((N, 2), device="cuda:0") - 0.5) * 0.4, torch.zeros(N, device="cuda:0")
        ls_a, ls_na = torch.full((2,), -1.5, device="cuda:0"), torch.rand((N, 2), device="cuda:0") - 2.0
        zeros = torch.zeros(N, device="cuda:0")
        obs = [e.reset() for e in envs]
        bufs = [tg.DeviceRolloutBuffer.for_env(e, T) for e in envs[:2]]
        rbs = [tg.DeviceReplayBuffer.for_env(e, T * N) for e in envs[2:]]
        for rb, o in zip(rbs, obs[2:]):
            rb.start(o)
        g, s = tg.DeviceDiagGaussian.for_env(envs[0], seed=1), tg.DeviceSquashedDiagGaussian.for_env(envs[2], seed=1)

        def rollout(i, head):
            env, buf = envs[i], bufs[i]
            rd = env.reward_done_torch()

            def it():
                if buf.full:
                    buf.reset()
                a, e, lp = head()
                t = buf.pos
                buf.add(obs[i], a, zeros, rd[1], values, lp)
                obs[i], _, _, _ = env.step(e)
                buf.rewards[t].copy_(rd[0])
            return it

        def replay(i, head):
            env, rb = envs[i], rbs[i - 2]

            def it():
                a, e, _ = head()
                env.step(e)
                rb.add_from_env(a)
            return it
        cands = [("step + DeviceDiagGaussian + add", rollout(0, lambda: g.sample(mean, ls_a))),
                 ("step + torch ops + add", rollout(1, lambda: torch_gaussian(mean, ls_a, lo, hi))),
                 ("step + DeviceSquashed + add_from_env", replay(2, lambda: s.sample(mean, ls_na))),
                 ("step + torch ops + add_from_env", replay(3, lambda: torch_squashed(mean, ls_na, lo, hi)))]
        _report(f"N {N:6d}", cands, args)
    finally:
        for e in envs:
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default="all", choices=["call", "loop", "all"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/action_head_rate.py measures on the GPU: no device found")
    for name, fn in (("call", section_call), ("loop", section_loop)):
        if args.section in (name, "all"):
            fn(args)


if __name__ == "__main__":
    main()
