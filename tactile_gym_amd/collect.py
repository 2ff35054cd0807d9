"""stable_baselines3's two collection loops over the device pieces, for an env made with obs_mode="torch" (or a DeviceVecNormalize over one):
nothing in a step touches the host but the env's own reward / done copy.

    buf = tg.DeviceRolloutBuffer.for_env(venv, n_steps, gamma=0.95, gae_lambda=0.9)              # PPO / RAD_PPO
    head = tg.DeviceDiagGaussian.for_env(venv, seed=0)
    obs, starts = venv.reset(), torch.ones(venv.num_envs, dtype=torch.uint8, device=buf.device)
    obs, starts = collect_rollouts(venv, policy, buf, head, n_steps, obs, starts)                 # policy(obs) -> mean, log_std, values

    rb = tg.DeviceReplayBuffer.for_env(venv, 100_000)                                             # SAC / RAD_SAC
    head = tg.DeviceSquashedDiagGaussian.for_env(venv, seed=0)
    obs = venv.reset(); rb.start(obs)
    obs, num_timesteps = collect_transitions(venv, actor, rb, head, n_steps, num_timesteps, learning_starts, obs)   # actor(obs) -> mean, log_std

`policy` and `actor` are any callables on the observation dict that return float32 device tensors; they are called under torch.no_grad().  The
orderings are the ones the zero-copy observation views force: the rollout buffer's add comes BEFORE the step (the step rewrites the views it
reads), the replay buffer's add_from_env AFTER it (it reads the env's own next and terminal observations).

Bootstrapping on info["TimeLimit.truncated"] (SB3 adds gamma V(terminal_observation) to the reward of a truncated episode's last step) is left
out: this library's envs report TimeLimit.truncated = False, an episode that reaches max_steps is a termination as in the reference.
"""
import torch

__all__ = ["collect_rollouts", "collect_transitions"]


def collect_rollouts(venv, policy, buf, head, n_steps, last_obs, last_starts):
    """SB3's OnPolicyAlgorithm.collect_rollouts: fills `buf` (a DeviceRolloutBuffer of n_steps slots, reset first) with n_steps steps of `venv`
    and computes returns and advantages.  Per step: mean, log_std, values = policy(obs); head.sample; buf.add(obs, actions, 0, starts, values,
    log_prob) before the step; venv.step(env_actions); the step's reward into buf.rewards[t].  last_obs: the env's current observation;
    last_starts: uint8, bool or float32 [N], whether it begins an episode.  Returns (last_obs, last_starts) for the next call."""
    if n_steps != buf.buffer_size:
        raise ValueError(f"n_steps={n_steps} must be the rollout buffer's size {buf.buffer_size}")
    buf.reset()
    rewards, dones = venv.reward_done_torch()            # the env's (or the normaliser's) own buffers: they never move
    zeros = torch.zeros(buf.n_envs, dtype=torch.float32, device=rewards.device)
    for t in range(n_steps):
        with torch.no_grad():
            mean, log_std, values = policy(last_obs)
        actions, env_actions, log_prob = head.sample(mean, log_std)
        buf.add(last_obs, actions, zeros, last_starts, values, log_prob)
        last_obs, _, _, _ = venv.step(env_actions)
        buf.rewards[t].copy_(rewards)
        last_starts = dones                               # read by the next add before the next step rewrites it
    with torch.no_grad():
        _, _, last_values = policy(last_obs)
    buf.compute_returns_and_advantage(last_values, dones)
    return last_obs, dones.clone()


def collect_transitions(venv, actor, rb, head, n_steps, num_timesteps, learning_starts, last_obs=None):
    """SB3's OffPolicyAlgorithm.collect_rollouts with _sample_action and _store_transition: n_steps steps of `venv` into `rb` (a
    DeviceReplayBuffer made by for_env, with rb.start(obs) called once after the reset).  While num_timesteps < learning_starts the actions are
    head.sample_uniform(), afterwards mean, log_std = actor(obs); head.sample.  Each step is venv.step(env_actions) followed by
    rb.add_from_env(actions); num_timesteps grows by num_envs per step.  last_obs: the env's current observation (only read once the warm-up
    is over).  Returns (last_obs, num_timesteps)."""
    for _ in range(n_steps):
        if num_timesteps < learning_starts:
            actions, env_actions = head.sample_uniform()
        else:
            if last_obs is None:
                raise ValueError("collect_transitions needs last_obs (the env's current observation) once num_timesteps >= learning_starts")
            with torch.no_grad():
                mean, log_std = actor(last_obs)
            actions, env_actions, _ = head.sample(mean, log_std)
        last_obs, _, _, _ = venv.step(env_actions)
        rb.add_from_env(actions)
        num_timesteps += venv.num_envs
    return last_obs, num_timesteps
