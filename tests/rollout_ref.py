"""Reference of tactile_gym_amd.rollout (csrc/tg_rollout.hip): stable_baselines3's RolloutBuffer / DictRolloutBuffer semantics restated in numpy.

SB3 (common/buffers.py) stores [T, N, ...] arrays, computes GAE(lambda) in compute_returns_and_advantage

    for step in reversed(range(T)):
        next_non_terminal = 1 - (dones if step == T - 1 else episode_starts[step + 1])
        next_values       =      last_values if step == T - 1 else values[step + 1]
        delta        = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    returns = advantages + values

and hands out minibatches of swap_and_flatten(arr) = arr.swapaxes(0, 1).reshape(T * N, ...) indexed by a permutation: flat sample i = n T + t.

gae_f64: that recurrence in float64 (what SB3 computes up to its mixed float32 / float64 intermediates).  gae_f32: the device arithmetic, every
operation one float32 rounding, no fused multiply-add, g = float32(gamma), gl = float32(gamma * gae_lambda) with the product formed in double;
the device output must equal it bit for bit.
"""
import numpy as np


def _flags(x):
    return (np.asarray(x) != 0)


def gae_f64(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda, dtype=np.float64):
    """(advantages, returns), float64 [T, N]: SB3's recurrence.  dtype=np.float32: the same lines on float32 arrays (SB3's own storage)."""
    with np.errstate(all="ignore"):                      # infinities and NaNs go through as they do in SB3
        r, v, es = (np.asarray(a, dtype=dtype) for a in (rewards, values, episode_starts))
        T, N = r.shape
        lv, d = np.asarray(last_values, dtype=dtype).reshape(N), _flags(dones).reshape(N).astype(dtype)
        gamma, gae_lambda, one = dtype(gamma), dtype(gae_lambda), dtype(1.0)
        adv = np.zeros((T, N), dtype)
        last = np.zeros(N, dtype)
        for t in reversed(range(T)):
            nnt = one - (d if t == T - 1 else es[t + 1])
            nv = lv if t == T - 1 else v[t + 1]
            delta = r[t] + gamma * nv * nnt - v[t]
            last = delta + gamma * gae_lambda * nnt * last
            adv[t] = last
        return adv, adv + v


def gae_f32(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda, starts_offset=1):
    """(advantages, returns), float32 [T, N]: the device arithmetic.  starts_offset=0 is a deliberately wrong recurrence (episode_starts[t] in
    place of [t + 1]) for the test that shows the error bound is not vacuous."""
    with np.errstate(all="ignore"):
        return _gae_f32(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda, starts_offset)


def _gae_f32(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda, starts_offset):
    f = np.float32
    r, v, es = (np.ascontiguousarray(a, dtype=f) for a in (rewards, values, episode_starts))
    T, N = r.shape
    lv, d = np.asarray(last_values, dtype=f).reshape(N), _flags(dones).reshape(N).astype(f)
    g, gl, one = f(gamma), f(float(gamma) * float(gae_lambda)), f(1)
    adv, ret = np.zeros((T, N), f), np.zeros((T, N), f)
    last = np.zeros(N, f)
    for t in reversed(range(T)):
        if starts_offset == 1:
            nnt = one - (d if t == T - 1 else es[t + 1])
        else:
            nnt = one - es[t]
        nv = lv if t == T - 1 else v[t + 1]
        delta = (r[t] + (g * nv) * nnt) - v[t]
        last = delta + (gl * nnt) * last
        adv[t] = last
        ret[t] = last + v[t]
    assert adv.dtype == f and ret.dtype == f and last.dtype == f
    return adv, ret


def gae_bound(rewards, values, last_values, adv_f64, gamma, gae_lambda):
    """Bound of max |gae_f32 - gae_f64|: six float32 roundings per step (8 with slack), each at most 2^-24 of a term bounded by
    A = max|r| + (1 + gamma) max|v| + gamma lambda max|adv|, summed over the steps with the damping gamma lambda: A / (1 - gamma lambda), or
    A T when gamma lambda = 1."""
    T = np.asarray(rewards).shape[0]
    vmax = max(np.abs(values).max(), np.abs(last_values).max())
    A = np.abs(rewards).max() + (1 + gamma) * vmax + gamma * gae_lambda * np.abs(adv_f64).max()
    gl = gamma * gae_lambda
    return 8 * 2.0 ** -24 * A * (T if gl >= 1 else 1 / (1 - gl))


def gae_error(adv32, ret32, adv64, ret64):
    """The figure gae_bound bounds: max |adv32 - adv64|, and max |ret32 - ret64| less the one rounding of the final last + v."""
    return max(np.abs(adv32 - adv64).max(), np.abs(ret32 - ret64).max() - 2.0 ** -24 * np.abs(ret64).max())


# The shapes and inputs of the GAE kernel's edge tests (tests/test_gpu_rollout_abi.py; tests/test_rollout_cpu.py holds gae_f32 to gae_bound on
# them): T on both sides of the kernel's blocks of 8 prefetched steps, N on both sides of its workgroups of 64 envs.
GAE_T = (1, 2, 7, 8, 9, 15, 16, 17, 64, 65)
GAE_N = (1, 2, 63, 64, 65, 127, 128, 129, 1000)
GAE_PARAMS = ((0.95, 0.9), (0.99, 0.95), (0.999, 1.0), (0.99, 0.0), (1.0, 0.95))       # (gamma, lambda)
GAE_STARTS = ("none", "all", "alternating", "first", "last")


def gae_edge_inputs(T, N, starts):
    """(rewards, values, episode_starts, last_values, dones) float32 for one edge case; dones 0 / 1."""
    rng = np.random.default_rng(1000 * T + N)
    r = rng.standard_normal((T, N)).astype(np.float32)
    v = (rng.standard_normal((T, N)) * 5).astype(np.float32)
    lv = (rng.standard_normal(N) * 5).astype(np.float32)
    es = np.zeros((T, N), np.float32)
    d = (rng.random(N) < 0.3).astype(np.float32)
    if starts == "all":
        es[:], d[:] = 1.0, 1.0
    elif starts == "alternating":
        es[:] = (np.arange(T)[:, None] + np.arange(N)[None, :]) % 2
    elif starts == "first":
        es[0] = 1.0
    elif starts == "last":
        es[T - 1] = 1.0
    else:
        assert starts == "none"
        d[:] = 0.0
    return r, v, es, lv, d


def flat_rows(indices, T, N):
    """Storage rows t N + n of SB3's flat sample indices i = n T + t."""
    i = np.asarray(indices, dtype=np.int64)
    return (i % T) * N + i // T


def swap_and_flatten(arr):
    """SB3's swap_and_flatten: [T, N, ...] -> [T N, ...] with sample i = n T + t."""
    a = np.asarray(arr)
    T, N = a.shape[:2]
    return a.swapaxes(0, 1).reshape((T * N,) + a.shape[2:])


def minibatches(storage, indices, batch_size):
    """SB3's get(): `storage` {name: [T, N, ...]}; yields {name: swap_and_flatten(array)[indices[start:start + batch_size]]}."""
    flat = {k: swap_and_flatten(v) for k, v in storage.items()}
    idx = np.asarray(indices, dtype=np.int64)
    for start in range(0, len(idx), batch_size):
        sel = idx[start:start + batch_size]
        yield {k: v[sel] for k, v in flat.items()}
