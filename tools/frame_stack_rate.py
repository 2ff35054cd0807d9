"""Per-step time of the device frame stack (frame_stack=n) at 1024 envs, by device events around K random-action steps (step_random_async, obs_mode
"torch"), against the same env without a stack and with the stacking written as torch ops on the zero-copy tensors (roll, terminal concat,
masked zero, newest slot).  Prints one line per configuration.

    python tools/frame_stack_rate.py [--envs 1024] [--steps 200] [--warmup 20]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")
BAL = dict(movement_mode="xy", control_mode="TCP_velocity_control", object_mode="pole", rand_gravity=True, rand_embed_dist=True,
           observation_mode="tactile", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")


def measure(env_id, modes, n, envs, steps, warmup, torch_ops=False):
    import torch
    import tactile_gym_amd as tg
    v = tg.make_vec(env_id, num_envs=envs, max_steps=200 if env_id.startswith("edge") else 1000, image_size=[128, 128], env_modes=modes, seed=1,
                    obs_mode="torch", frame_stack=1 if torch_ops else n)
    v.reset()
    obs = v.tactile_torch()
    term = v.tactile_torch(terminal=True)
    _, done = v.reward_done_torch()
    stack = torch.zeros(obs.shape[:-1] + (n,), dtype=torch.uint8, device=obs.device) if torch_ops else None
    tstack = torch.zeros_like(stack) if torch_ops else None

    def one(k):
        nonlocal stack
        v.step_random_async(7, first_draw=0, restart=(k == 0))
        if torch_ops:
            stack = torch.roll(stack, -1, dims=-1)
            d = done.bool()
            tstack.copy_(torch.cat([stack[..., :-1], term], dim=-1))         # rows valid where done
            stack.masked_fill_(d.view(-1, 1, 1, 1), 0)
            stack[..., -1:] = obs
    for k in range(warmup):
        one(k)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(steps):
        one(warmup + k)
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1000.0 / steps
    v.close()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    cases = [("edge_follow-v0", EDGE, 1, False), ("edge_follow-v0", EDGE, 2, False), ("edge_follow-v0", EDGE, 4, False),
             ("edge_follow-v0", EDGE, 2, True), ("object_balance-v0", BAL, 1, False), ("object_balance-v0", BAL, 2, False),
             ("object_balance-v0", BAL, 2, True)]
    for env_id, modes, n, ops in cases:
        if args.only and args.only not in env_id:
            continue
        us = measure(env_id, modes, n, args.envs, args.steps, args.warmup, ops)
        print(f"{env_id:18s} envs {args.envs} n {n} {'torch-ops' if ops else 'device  '}  {us:8.2f} us/step", flush=True)


if __name__ == "__main__":
    main()
