"""Times of the device VecNormalize (tactile_gym_amd.vecnorm; csrc/tg_vecnorm.hip) against the same maths composed from torch ops, by device
events around `--iters` calls after `--warmup`, the candidates alternated `--rounds` times; its output belongs in profiles/vecnorm_rate.txt
(DESIGN.md 4.12).  Kernel times come from a separate run of `--section kernels` under rocprofv3 --kernel-trace --stats.

  step    edge_follow-v0 in oracle mode, 64 x 64, 1024 and 16 384 envs: venv.step(), DeviceVecNormalize.step(), and venv.step() followed by
          the torch-op composition (f64 mean / var / moment merge, clamp, the returns recurrence and its masked reset); the host time of an
          iteration is the host clock around the loop (every step waits for its rewards, so host and device times nearly coincide)
  sample  sample(B, env=vn) against sample(B) followed by torch-op normalisation, B = 64 and 4096, object_roll-v0 tactile_and_feature

    python tools/vecnorm_rate.py [--section step|sample|kernels|all] [--iters 200] [--warmup 20] [--rounds 3]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from replay_rate import alternate  # noqa: E402

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="oracle", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")
ROLL = dict(movement_mode="xy", control_mode="TCP_velocity_control", rand_init_obj_pos=True, rand_obj_size=True, rand_embed_dist=True,
            observation_mode="tactile_and_feature", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")


class TorchOps:
    """VecNormalize's step over one vector key from torch ops, float64 statistics on the device."""

    def __init__(self, N, d, dev, gamma=0.99, clip=10.0, eps=1e-8):
        import torch
        f = dict(dtype=torch.float64, device=dev)
        self.mean, self.var, self.count = torch.zeros(d, **f), torch.ones(d, **f), torch.full((), 1e-4, **f)
        self.rmean, self.rvar, self.rcount = torch.zeros((), **f), torch.ones((), **f), torch.full((), 1e-4, **f)
        self.returns, self.gamma, self.clip, self.eps = torch.zeros(N, **f), gamma, clip, eps

    @staticmethod
    def _merge(mean, var, count, x):
        n = x.shape[0]
        bm, bv = x.mean(0), x.var(0, unbiased=False)
        delta, tot = bm - mean, count + n
        m2 = var * count + bv * n + delta * delta * count * n / tot
        return mean + delta * n / tot, m2 / tot, tot

    def step(self, x, reward, done):
        import torch
        x64 = x.double()
        self.mean, self.var, self.count = self._merge(self.mean, self.var, self.count, x64)
        out = torch.clamp((x64 - self.mean) / torch.sqrt(self.var + self.eps), -self.clip, self.clip).float()
        self.returns = self.returns * self.gamma + reward.double()
        self.rmean, self.rvar, self.rcount = self._merge(self.rmean, self.rvar, self.rcount, self.returns)
        rew = torch.clamp(reward.double() / torch.sqrt(self.rvar + self.eps), -self.clip, self.clip).float()
        self.returns = torch.where(done != 0, torch.zeros_like(self.returns), self.returns)
        return out, rew.cpu().numpy()

    def normalize(self, x, reward):
        import torch
        return (torch.clamp((x.double() - self.mean) / torch.sqrt(self.var + self.eps), -self.clip, self.clip).float(),
                torch.clamp(reward.double() / torch.sqrt(self.rvar + self.eps), -self.clip, self.clip).float())


def section_step(args, sizes=(1024, 16384)):
    import torch
    import tactile_gym_amd as tg
    print(f"# step: edge_follow-v0, oracle mode, 64 x 64, obs_mode torch; us per step, {args.rounds} alternated rounds of {args.iters} steps "
          f"(device events; host: the loop's own clock)")
    for N in sizes:
        envs = [tg.make_vec("edge_follow-v0", num_envs=N, max_steps=200, image_size=[64, 64], env_modes=EDGE, seed=1 + i, obs_mode="torch")
                for i in range(3)]
        try:
            bare, wrapped, composed = envs
            vn = tg.DeviceVecNormalize(wrapped)
            d = bare.observation_space.spaces["oracle"].shape[0]
            ops = TorchOps(N, d, "cuda:0")
            for e in (bare, vn, composed):
                e.reset()
            a = (torch.rand((N, 2), device="cuda:0") - 0.5) * 0.5
            rd = composed.reward_done_torch()

            def torch_step():
                obs, _, _, _ = composed.step(a)
                ops.step(obs["oracle"], rd[0], rd[1])
            cands = [("venv.step()", lambda: bare.step(a)), ("DeviceVecNormalize.step()  [+3 launches]", lambda: vn.step(a)),
                     ("venv.step() + torch ops", torch_step)]
            dev, host = alternate(cands, args.iters, args.warmup, args.rounds)
            for name, _ in cands:
                print(f"  N {N:6d}  {name:44s} device {min(dev[name]):8.2f} us (rounds: {' '.join(f'{x:.2f}' for x in dev[name])})   "
                      f"host {min(host[name]):8.2f} us", flush=True)
            b = min(dev[cands[0][0]])
            print(f"  N {N:6d}  wrapper - bare = {min(dev[cands[1][0]]) - b:.2f} us   torch ops - bare = {min(dev[cands[2][0]]) - b:.2f} us", flush=True)
        finally:
            for e in envs:
                e.close()


def _filled(N=1024, steps=16):
    import torch
    import tactile_gym_amd as tg
    venv = tg.make_vec("object_roll-v0", num_envs=N, max_steps=200, image_size=[64, 64], env_modes=ROLL, seed=1, obs_mode="torch")
    vn = tg.DeviceVecNormalize(venv)
    buf = tg.DeviceReplayBuffer.for_env(vn, steps * N, seed=1)
    vn.reset()
    buf.start(vn.get_original_obs())
    a = (torch.rand((N, venv.action_space.shape[0]), device="cuda:0") - 0.5) * 0.5
    for _ in range(steps):
        vn.step(a)
        buf.add_from_env(a)
    return venv, vn, buf


def section_sample(args, batches=(64, 4096)):
    venv, vn, buf = _filled()
    try:
        ops = TorchOps(venv.num_envs, venv.feature_dim, "cuda:0")
        ops.mean, ops.var = vn.obs_rms["extended_feature"].mean.clone(), vn.obs_rms["extended_feature"].var.clone()
        print(f"# sample: object_roll-v0 tactile_and_feature, 64 x 64, ring of 16 x 1024; us per call, {args.rounds} alternated rounds of "
              f"{args.iters} calls")

        def composed(B):
            s = buf.sample(B)
            ops.normalize(s.observations["extended_feature"], s.rewards)
            ops.normalize(s.next_observations["extended_feature"], s.rewards)
        for B in batches:
            cands = [("sample(B, env=vn)  [+1 launch]", lambda: buf.sample(B, env=vn)), ("sample(B)", lambda: buf.sample(B)),
                     ("sample(B) + torch ops", lambda: composed(B))]
            dev, host = alternate(cands, args.iters, args.warmup, args.rounds)
            for name, _ in cands:
                print(f"  B {B:5d}  {name:34s} device {min(dev[name]):8.2f} us (rounds: {' '.join(f'{x:.2f}' for x in dev[name])})   "
                      f"host enqueue {min(host[name]):8.2f} us", flush=True)
    finally:
        venv.close()


def section_kernels(args):
    """A few dispatches of every kernel at the measured shapes, for the profiler run."""
    import torch
    import tactile_gym_amd as tg
    for N in (1024, 16384):
        venv = tg.make_vec("edge_follow-v0", num_envs=N, max_steps=200, image_size=[64, 64], env_modes=EDGE, seed=1, obs_mode="torch")
        try:
            vn = tg.DeviceVecNormalize(venv)
            vn.reset()
            a = (torch.rand((N, 2), device="cuda:0") - 0.5) * 0.5
            for _ in range(8):
                vn.step(a)
            torch.cuda.synchronize()
        finally:
            venv.close()
    venv, vn, buf = _filled()
    try:
        for B in (64, 4096):
            for _ in range(6):
                buf.sample(B, env=vn)
        torch.cuda.synchronize()
    finally:
        venv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default="all", choices=["step", "sample", "kernels", "all"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/vecnorm_rate.py measures on the GPU: no device found")
    if args.section == "kernels":
        return section_kernels(args)
    for name, fn in (("step", section_step), ("sample", section_sample)):
        if args.section in (name, "all"):
            fn(args)


if __name__ == "__main__":
    main()
