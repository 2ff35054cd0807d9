"""stable_baselines3's PPO.train and SAC.train over the device pieces.  PPO.train: DeviceRolloutBuffer.get's minibatches, the policy, tg.ppo_loss (one launch for the loss
and its gradients at the head's inputs), clip_grad_norm_ and the optimiser.

    buf = tg.DeviceRolloutBuffer.for_env(venv, n_steps, gamma=0.95, gae_lambda=0.9)
    obs, starts = tg.collect.collect_rollouts(venv, policy, buf, head, n_steps, obs, starts)
    stats = tg.train.ppo_train(policy, optimizer, buf, n_epochs=10, batch_size=64, clip_range=0.2, clip_range_vf=None, ent_coef=0.0,
                               vf_coef=0.5, max_grad_norm=0.5, target_kl=None, augment=aug)

`policy` is any callable on the observations that returns float32 device tensors mean [B, A], log_std [A] or [B, A] and values [B], with
gradients to the optimiser's parameters.

SAC.train: DeviceReplayBuffer.sample's minibatch, the actor and the critics, head.rsample, tg.sac_critic_loss and tg.sac_actor_loss (one launch
each for the TD target with the critic loss, and for the actor loss with the entropy-coefficient loss, gradients included),
the optimisers and polyak_update (two multi-tensor launches of torch's own for all of the target's tensors).

    rb = tg.DeviceReplayBuffer.for_env(venv, 100_000)
    log_ent_coef = torch.zeros(1, device="cuda", requires_grad=True)                     # ent_coef="auto": log(1.0), with an Adam of its own
    critic_stats, actor_stats, n_updates = tg.train.sac_train(actor, critic, critic_target, actor_opt, critic_opt, rb, head, gradient_steps=1,
                                                              batch_size=64, gamma=0.95, tau=0.005, log_ent_coef=log_ent_coef,
                                                              ent_coef_optimizer=ent_opt, target_entropy=-A, n_updates=n_updates, augment=aug)

`actor(obs) -> (mean, log_std)`; `critic(obs, actions)` and `critic_target(obs, actions)` return a tuple of q tensors [B] or [B, 1], as
SB3's ContinuousCritic does.
"""
import torch

from .loss_head import ppo_loss, sac_actor_loss, sac_critic_loss
from .optim import DeviceAdam

__all__ = ["ppo_train", "sac_train", "polyak_update"]


def ppo_train(policy, optimizer, buf, n_epochs, batch_size, clip_range, clip_range_vf, ent_coef, vf_coef, max_grad_norm, target_kl, augment=None,
              out_dtype=None):
    """SB3's PPO.train: n_epochs passes over `buf` (a full DeviceRolloutBuffer) in minibatches of batch_size (the last one shorter), the
    advantages normalised per minibatch.  Per minibatch: mean, log_std, values = policy(observations); tg.ppo_loss; optimizer.zero_grad();
    loss.backward(); clip_grad_norm_ over the optimiser's parameters (max_grad_norm=None: none); optimizer.step().  target_kl: training stops
    before the step of the first minibatch whose approx_kl exceeds 1.5 target_kl, as in SB3 - that 4-byte read per minibatch is the only host
    read; None reads nothing.  With a tg.DeviceAdam the clip and the step are optimizer.step(max_grad_norm=max_grad_norm): two launches, and
    p.grad keeps backward's values (max_grad_norm=None then means the optimiser's own max_grad_norm).  Returns the last minibatch's stats (float32 [8], on the device; loss_head.STATS), None when there was none."""
    params = [p for group in optimizer.param_groups for p in group["params"]]
    device_adam = isinstance(optimizer, DeviceAdam)
    stats = None
    for _ in range(n_epochs):
        for batch in buf.get(batch_size, augment=augment, out_dtype=torch.float32 if out_dtype is None else out_dtype):
            mean, log_std, values = policy(batch.observations)
            loss, stats = ppo_loss(mean, log_std, values, batch.actions, batch.old_log_prob, batch.advantages, batch.returns,
                                   old_values=batch.old_values, clip_range=clip_range, clip_range_vf=clip_range_vf, ent_coef=ent_coef,
                                   vf_coef=vf_coef, normalize_advantage=True)
            if target_kl is not None and float(stats[4]) > 1.5 * target_kl:
                return stats
            optimizer.zero_grad()
            loss.backward()
            if device_adam:                           # the clip and the step in two launches
                optimizer.step(max_grad_norm=max_grad_norm)
                continue
            if max_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
            optimizer.step()
    return stats


def polyak_update(params, target_params, tau):
    """SB3's polyak_update on two lists of tensors: target = (1 - tau) * target + tau * param, in place and under no_grad, as
    torch._foreach_mul_(targets, 1 - tau) and torch._foreach_add_(targets, params, alpha=tau): SB3's own two operations per tensor with
    SB3's bits, in two launches for the whole list where SB3's loop takes two per tensor.  `params` is unchanged; lists of different
    lengths are refused (SB3's zip_strict)."""
    params, target_params = list(params), list(target_params)
    if len(params) != len(target_params):
        raise ValueError(f"polyak_update: {len(params)} params against {len(target_params)} target params")
    if not params:
        return
    with torch.no_grad():
        torch._foreach_mul_(target_params, 1 - tau)
        torch._foreach_add_(target_params, params, alpha=tau)


def _batch_norm_stats(module):
    """SB3's get_parameters_by_name(module, ["running_"]) over the buffers: batch-norm running statistics, copied to the target with tau = 1."""
    return [b for name, b in module.named_buffers() if "running_" in name] if hasattr(module, "named_buffers") else []


def sac_train(actor, critic, critic_target, actor_optimizer, critic_optimizer, rb, head, gradient_steps, batch_size, gamma, tau, log_ent_coef=None,
              ent_coef_optimizer=None, ent_coef=None, target_entropy=None, target_update_interval=1, n_updates=0, augment=None, env=None,
              out_dtype=None):
    """SB3's SAC.train: gradient_steps updates on minibatches of batch_size from `rb` (a DeviceReplayBuffer).  Per step:
      batch = rb.sample(batch_size, env=env, augment=augment)
      actions_pi, log_prob = head.rsample(*actor(batch.observations))                    # SB3's draw order: actions_pi first
      under no_grad: next_actions, next_log_prob = head.rsample(*actor(batch.next_observations)); q_next = critic_target(next_observations, next_actions)
      tg.sac_critic_loss on critic(batch.observations, batch.actions); the critic's zero_grad / backward / step
      tg.sac_actor_loss on critic(batch.observations, actions_pi); the actor's and the entropy optimiser's zero_grad; ONE backward of
      actor_loss + ent_coef_loss; both steps
      n_updates += 1; every target_update_interval updates polyak_update(critic.parameters(), critic_target.parameters(), tau) and the
      batch-norm running statistics with tau = 1.
    The entropy coefficient: log_ent_coef (a float32 device scalar, never read on the host) with ent_coef_optimizer and target_entropy - SB3's
    ent_coef="auto" - or the float ent_coef.  SB3 steps the entropy optimiser BEFORE it forms the target; stepping it last is the same
    update: SB3's target and actor loss use the ent_coef computed before that step, which is what both launches here read, and the gradient
    of ent_coef_loss, -mean(log_prob + target_entropy), does not depend on log_ent_coef.  The two losses' leaves are disjoint except through
    alpha, which both detach, so one backward of their sum gives every leaf SB3's gradient.
    Returns (critic_stats, actor_stats, n_updates): the last step's float32 [8] device tensors (loss_head.SAC_CRITIC_STATS, SAC_ACTOR_STATS;
    None without a step) and the update count.  Nothing is read on the host."""
    if (log_ent_coef is None) == (ent_coef is None):
        raise ValueError("give exactly one of log_ent_coef (a device tensor) and ent_coef (a float)")
    learn_ent = ent_coef_optimizer is not None
    if learn_ent and (log_ent_coef is None or target_entropy is None):
        raise ValueError("ent_coef_optimizer needs log_ent_coef and target_entropy")
    alpha = dict(log_ent_coef=log_ent_coef) if log_ent_coef is not None else dict(ent_coef=ent_coef)
    critic_stats = actor_stats = None
    for _ in range(gradient_steps):
        batch = rb.sample(batch_size, env=env, augment=augment, out_dtype=torch.float32 if out_dtype is None else out_dtype)
        actions_pi, log_prob = head.rsample(*actor(batch.observations))
        with torch.no_grad():
            next_actions, next_log_prob = head.rsample(*actor(batch.next_observations))
            q_next = critic_target(batch.next_observations, next_actions)
        critic_loss, critic_stats = sac_critic_loss(critic(batch.observations, batch.actions), q_next, next_log_prob, batch.rewards, batch.dones,
                                                    gamma, **alpha)
        critic_optimizer.zero_grad()
        critic_loss.backward()
        critic_optimizer.step()
        actor_loss, ent_coef_loss, actor_stats = sac_actor_loss(log_prob, critic(batch.observations, actions_pi),
                                                                target_entropy=target_entropy if learn_ent else None, **alpha)
        actor_optimizer.zero_grad()
        if learn_ent:
            ent_coef_optimizer.zero_grad()
            (actor_loss + ent_coef_loss).backward()
        else:
            actor_loss.backward()
        actor_optimizer.step()
        if learn_ent:
            ent_coef_optimizer.step()
        n_updates += 1
        if n_updates % target_update_interval == 0:
            polyak_update(list(critic.parameters()), list(critic_target.parameters()), tau)
            polyak_update(_batch_norm_stats(critic), _batch_norm_stats(critic_target), 1.0)
    return critic_stats, actor_stats, n_updates
