"""Per-step time of channels_first (tg_set_obs_layout) and of the visual frame stacks at 1024 envs, by device events around K random-action steps
(step_random_async, obs_mode "torch"), as tools/frame_stack_rate.py measures frame_stack.  Prints one line per configuration:

- edge_follow tactile n = 2: (a) the channels-last stack, (b) channels_first=True, (c) (a) plus the caller's permute(0, 3, 1, 2).contiguous();
- edge_follow visuotactile: n = 1, and n = 2 in both layouts (the scene camera's images stacked as well).

    python tools/obs_layout_rate.py [--envs 1024] [--steps 200] [--warmup 20] [--only tactile|visual]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")


def measure(modes, n, channels_first, envs, steps, warmup, permute=False):
    import torch
    import tactile_gym_amd as tg
    v = tg.make_vec("edge_follow-v0", num_envs=envs, max_steps=200, image_size=[128, 128], env_modes=modes, seed=1, obs_mode="torch",
                    frame_stack=n, channels_first=channels_first)
    obs = v.reset()
    keys = [k for k in ("tactile", "visual") if k in obs]

    def one(k):
        v.step_random_async(7, first_draw=0, restart=(k == 0))
        if permute:
            for key in keys:
                v._stack_torch(key).permute(0, 3, 1, 2).contiguous()
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
    vis = dict(EDGE, observation_mode="visuotactile")
    cases = [("tactile", EDGE, 2, False, False, "(a) channels last"), ("tactile", EDGE, 2, True, False, "(b) channels_first"),
             ("tactile", EDGE, 2, False, True, "(c) (a) + permute().contiguous()"),
             ("visual", vis, 1, False, False, "no stack"), ("visual", vis, 2, False, False, "channels last"), ("visual", vis, 2, True, False, "channels_first")]
    for what, modes, n, cf, perm, label in cases:
        if args.only and args.only != what:
            continue
        us = measure(modes, n, cf, args.envs, args.steps, args.warmup, perm)
        print(f"edge_follow-v0 {modes['observation_mode']:12s} envs {args.envs} n {n}  {label:34s} {us:9.2f} us/step", flush=True)


if __name__ == "__main__":
    main()
