"""Times of the device rollout buffer (tactile_gym_amd.rollout; csrc/tg_rollout.hip) against what the package offered before it, by device
events around `--iters` calls after `--warmup`; profiles/rollout_rate.txt holds the output.  Kernel times come from a separate run of
`--section kernels` under rocprofv3 --kernel-trace --stats (a few dispatches of each kernel at the same shapes, nothing else).

  minibatch  B x [2, 128, 128] uint8 rows drawn from a T N = 65 536 buffer: the fused row-indexed translate launch against
             (a) random_translate on a contiguous batch of the same shape and (b) index_select + random_translate; and a whole get() minibatch
  add        1024 envs, edge_follow n = 2 channels first (2 x 33.5 MB per slot): one k_rollout_add launch against the per-key copy_ chain,
             and the env step with add in the loop against the bare step
  gae        T = 2048, N = 1024 and 16 384: k_rollout_gae against the loop over t written with torch ops

    python tools/rollout_rate.py [--section minibatch|add|gae|kernels|all] [--iters 20] [--warmup 3]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29      # the float4 copy rate measured on MI355X
EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")


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


def _spaces(shape=(2, 128, 128), A=2):
    import numpy as np
    from tactile_gym_amd import spaces
    return (spaces.Dict({"tactile": spaces.Box(low=0, high=255, shape=shape, dtype=np.uint8)}),
            spaces.Box(low=-1.0, high=1.0, shape=(A,), dtype=np.float32))


def _image_buffer(T, N):
    import torch
    import tactile_gym_amd as tg
    obs, act = _spaces()
    buf = tg.DeviceRolloutBuffer(T, obs, act, "cuda:0", gae_lambda=0.9, gamma=0.95, n_envs=N, channels_first=True)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    for t in range(T):                                                  # random bytes slot by slot: no second copy of the storage
        buf.observations["tactile"][t].copy_(torch.randint(0, 256, (N, 2, 128, 128), dtype=torch.uint8, device="cuda:0", generator=g))
    buf.pos, buf.full = T, True
    return buf


def _fused_call(buf, rows, out, module):
    """The image launch of get(augment=module) alone, into a preallocated output (tg_random_translate_rows)."""
    import torch
    from tactile_gym_amd import _capi as capi
    L, src = capi.lib(), buf.observations["tactile"]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    prm = torch.empty((rows.numel(), 3), dtype=torch.float32, device=rows.device)

    def call():
        capi.check(L.tg_random_translate_rows(C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), 0, 1, rows.numel(), 2, 128, 128,
                                              module.translate[0], module.translate[1], module.p, C.c_uint64(module.seed),
                                              C.c_uint64(module.counter), None, C.c_void_p(prm.data_ptr()), C.c_void_p(rows.data_ptr()), stream))
        module.counter += 1
    return call


def section_minibatch(args, batches=(4096, 64)):
    import torch
    import tactile_gym_amd.augment as K
    from tactile_gym_amd.rollout import flat_rows
    T, N = 64, 1024
    buf = _image_buffer(T, N)
    flat = buf.observations["tactile"].view(T * N, 2, 128, 128)
    print(f"# minibatch: B x [2, 128, 128] uint8 rows of a T = {T}, N = {N} buffer ({flat.numel() / 1e9:.2f} GB), p = 0.5, us per call")
    for B in batches:
        g = torch.Generator(device="cuda:0").manual_seed(B)
        rows = flat_rows(torch.randperm(T * N, device="cuda:0", generator=g)[:B], T, N).contiguous()
        out = torch.empty((B, 2, 128, 128), dtype=torch.float32, device="cuda:0")
        contiguous = flat[:B].clone()
        m = K.RandomTranslate((0.05, 0.05), 0.5, seed=1)
        mb = B * 2 * 128 * 128 * 5 / 1e6
        res = {}
        res["fused rows launch (preallocated out)"] = time_calls(_fused_call(buf, rows, out, m), args.iters, args.warmup)
        res["(a) random_translate, contiguous batch (out=)"] = time_calls(
            lambda: K.random_translate(contiguous, (0.05, 0.05), 0.5, seed=1, counter=0, out=out), args.iters, args.warmup)
        res["(b) index_select + random_translate (out=)"] = time_calls(
            lambda: K.random_translate(flat.index_select(0, rows), (0.05, 0.05), 0.5, seed=1, counter=0, out=out), args.iters, args.warmup)
        aug = torch.nn.Sequential(m)
        res["get(augment=) whole minibatch (allocating)"] = time_calls(lambda: buf._gather(rows, m, torch.float32), args.iters, args.warmup)
        res["index_select + module(x) + 5 index_select"] = time_calls(
            lambda: (aug(flat.index_select(0, rows)), [getattr(buf, n).view(T * N, -1).index_select(0, rows)
                                                        for n in ("actions", "values", "log_probs", "advantages", "returns")]),
            args.iters, args.warmup)
        for name, us in res.items():
            gbs = mb / us                                                # MB per us = TB/s
            print(f"  B {B:5d}  {name:48s} {us:9.1f} us  {mb:7.1f} MB  {gbs:6.2f} TB/s  {gbs / COPY_TBS:5.2f} of copy", flush=True)
        f = res["fused rows launch (preallocated out)"]
        print(f"  B {B:5d}  fused / (a) = {f / res['(a) random_translate, contiguous batch (out=)']:.3f}   "
              f"(b) / fused = {res['(b) index_select + random_translate (out=)'] / f:.3f}", flush=True)


def section_add(args):
    import torch
    import tactile_gym_amd as tg
    N, T = 1024, 8
    obs_space, act = _spaces()
    buf = tg.DeviceRolloutBuffer(T, obs_space, act, "cuda:0", n_envs=N, channels_first=True)
    g = torch.Generator(device="cuda:0").manual_seed(2)
    obs = {"tactile": torch.randint(0, 256, (N, 2, 128, 128), dtype=torch.uint8, device="cuda:0", generator=g)}
    a, r, s, v, lp = (torch.rand((N, 2), device="cuda:0"), torch.rand(N, device="cuda:0"), torch.zeros(N, dtype=torch.uint8, device="cuda:0"),
                      torch.rand(N, device="cuda:0"), torch.rand(N, device="cuda:0"))

    def one_launch():
        if buf.full:
            buf.reset()
        buf.add(obs, a, r, s, v, lp)

    state = {"t": 0}

    def copy_chain():
        t = state["t"] = (state["t"] + 1) % T
        buf.observations["tactile"][t].copy_(obs["tactile"])
        buf.actions[t].copy_(a)
        buf.rewards[t].copy_(r)
        buf.episode_starts[t].copy_(s)
        buf.values[t].copy_(v)
        buf.log_probs[t].copy_(lp)
    mb = 2 * N * 2 * 128 * 128 / 1e6
    print(f"# add: {N} envs x [2, 128, 128] uint8 + 5 rows per slot, {mb:.1f} MB read + written, us per call")
    for name, fn in (("one k_rollout_add launch (add())", one_launch), ("per-key copy_ chain (6 launches)", copy_chain)):
        us = time_calls(fn, max(args.iters, 50), args.warmup)
        print(f"  {name:40s} {us:8.1f} us  {mb / us:5.2f} TB/s  {mb / us / COPY_TBS:5.2f} of copy", flush=True)
    del buf
    venv = tg.make_vec("edge_follow-v0", num_envs=N, max_steps=200, image_size=[128, 128], env_modes=EDGE, seed=1, obs_mode="torch", frame_stack=2,
                       channels_first=True)
    try:
        o = venv.reset()
        buf = tg.DeviceRolloutBuffer.for_env(venv, 16)
        rew, done = venv.reward_done_torch()
        k = {"k": 0}

        def bare():
            venv.step_random_async(7, first_draw=0, restart=(k["k"] == 0))
            k["k"] += 1

        def with_add():
            if buf.full:
                buf.reset()
            buf.add(o, venv.actions_torch(), rew, done, v, lp)
            bare()
        steps = max(args.iters, 200)
        for name, fn in (("bare step (step_random_async)", bare), ("add() + step", with_add), ("bare step, again", bare)):
            k["k"] = 0
            us = time_calls(fn, steps, 20)
            print(f"  edge_follow-v0 n 2 channels_first {N} envs  {name:32s} {us:8.2f} us/step", flush=True)
    finally:
        venv.close()


def _torch_gae(r, v, es, lv, d, gamma, lam):
    """The recurrence written the obvious way with torch ops: a Python loop over t."""
    import torch
    T = r.shape[0]
    adv = torch.empty_like(r)
    last = torch.zeros_like(lv)
    for t in reversed(range(T)):
        nnt = 1.0 - (d if t == T - 1 else es[t + 1])
        nv = lv if t == T - 1 else v[t + 1]
        delta = r[t] + gamma * nv * nnt - v[t]
        last = delta + gamma * lam * nnt * last
        adv[t] = last
    return adv, adv + v


def section_gae(args, sizes=((2048, 1024), (2048, 16384)), torch_loop=True):
    import numpy as np
    import torch
    import tactile_gym_amd as tg
    from tactile_gym_amd import spaces
    print("# gae: gamma 0.95, lambda 0.9, us per call")
    for T, N in sizes:
        buf = tg.DeviceRolloutBuffer(T, spaces.Dict({"oracle": spaces.Box(low=-1, high=1, shape=(1,), dtype=np.float32)}), _spaces()[1], "cuda:0",
                                     gae_lambda=0.9, gamma=0.95, n_envs=N)
        buf.rewards.normal_()
        buf.values.normal_()
        buf.episode_starts.copy_((torch.rand((T, N), device="cuda:0") < 0.01).float())
        lv, d = torch.randn(N, device="cuda:0"), (torch.rand(N, device="cuda:0") < 0.1).float()
        us = time_calls(lambda: buf.compute_returns_and_advantage(lv, d), args.iters, args.warmup)
        mb = T * N * 4 * 5 / 1e6
        print(f"  T {T} N {N:6d}  k_rollout_gae (compute_returns_and_advantage) {us:10.1f} us  {us * 1000 / T:7.1f} ns per step of the chain  "
              f"{mb:6.1f} MB  {mb / us:5.2f} TB/s", flush=True)
        if torch_loop:
            us_t = time_calls(lambda: _torch_gae(buf.rewards, buf.values, buf.episode_starts, lv, d, 0.95, 0.9), 2, 1)
            print(f"  T {T} N {N:6d}  torch-op loop over t ({T} x 9 launches)              {us_t:10.1f} us  ratio {us_t / us:7.1f}", flush=True)
            a, _ = _torch_gae(buf.rewards, buf.values, buf.episode_starts, lv, d, 0.95, 0.9)
            print(f"  T {T} N {N:6d}  max |kernel - torch loop| = {float((a - buf.advantages).abs().max()):.3e}", flush=True)
        del buf


def section_kernels(args):
    """A few dispatches of every kernel at the measured shapes, for the profiler run."""
    import torch
    import tactile_gym_amd.augment as K
    a = argparse.Namespace(iters=5, warmup=1)
    section_gae(a, torch_loop=False)
    from tactile_gym_amd.rollout import flat_rows
    T, N = 64, 1024
    buf = _image_buffer(T, N)
    flat = buf.observations["tactile"].view(T * N, 2, 128, 128)
    for B in (4096, 64):
        rows = flat_rows(torch.randperm(T * N, device="cuda:0")[:B], T, N).contiguous()
        out = torch.empty((B, 2, 128, 128), dtype=torch.float32, device="cuda:0")
        m = K.RandomTranslate((0.05, 0.05), 0.5, seed=1)
        contiguous = flat[:B].clone()
        for _ in range(6):
            K.random_translate(contiguous, (0.05, 0.05), 0.5, seed=1, counter=0, out=out)      # dispatches 1 - 6 of this B: contiguous
        torch.cuda.synchronize()
        call = _fused_call(buf, rows, out, m)
        for _ in range(6):
            call()                                                                             # dispatches 7 - 12: row indexed
        torch.cuda.synchronize()
        for _ in range(6):
            buf._gather(rows, None, torch.uint8)                                               # k_rollout_gather with the uint8 image rows
        torch.cuda.synchronize()
    del buf
    obs_space, act = _spaces()
    import tactile_gym_amd as tg
    buf = tg.DeviceRolloutBuffer(8, obs_space, act, "cuda:0", n_envs=1024, channels_first=True)
    obs = {"tactile": torch.randint(0, 256, (1024, 2, 128, 128), dtype=torch.uint8, device="cuda:0")}
    z, s = torch.zeros(1024, device="cuda:0"), torch.zeros(1024, dtype=torch.uint8, device="cuda:0")
    for _ in range(8):
        buf.add(obs, torch.zeros((1024, 2), device="cuda:0"), z, s, z, z)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default="all", choices=["minibatch", "add", "gae", "kernels", "all"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/rollout_rate.py measures on the GPU: no device found")
    if args.section == "kernels":
        return section_kernels(args)
    for name, fn in (("minibatch", section_minibatch), ("add", section_add), ("gae", section_gae)):
        if args.section in (name, "all"):
            fn(args)


if __name__ == "__main__":
    main()
