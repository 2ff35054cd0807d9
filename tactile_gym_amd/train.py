"""stable_baselines3's PPO.train over the device pieces: DeviceRolloutBuffer.get's minibatches, the policy, tg.ppo_loss (one launch for the loss
and its gradients at the head's inputs), clip_grad_norm_ and the optimiser.

    buf = tg.DeviceRolloutBuffer.for_env(venv, n_steps, gamma=0.95, gae_lambda=0.9)
    obs, starts = tg.collect.collect_rollouts(venv, policy, buf, head, n_steps, obs, starts)
    stats = tg.train.ppo_train(policy, optimizer, buf, n_epochs=10, batch_size=64, clip_range=0.2, clip_range_vf=None, ent_coef=0.0,
                               vf_coef=0.5, max_grad_norm=0.5, target_kl=None, augment=aug)

`policy` is any callable on the observations that returns float32 device tensors mean [B, A], log_std [A] or [B, A] and values [B], with
gradients to the optimiser's parameters.  SAC.train is not spelled here: its actor loss and next actions take head.rsample, the
critics, the entropy coefficient and the polyak update stay on torch.
"""
import torch

from .loss_head import ppo_loss

__all__ = ["ppo_train"]


def ppo_train(policy, optimizer, buf, n_epochs, batch_size, clip_range, clip_range_vf, ent_coef, vf_coef, max_grad_norm, target_kl, augment=None,
              out_dtype=None):
    """SB3's PPO.train: n_epochs passes over `buf` (a full DeviceRolloutBuffer) in minibatches of batch_size (the last one shorter), the
    advantages normalised per minibatch.  Per minibatch: mean, log_std, values = policy(observations); tg.ppo_loss; optimizer.zero_grad();
    loss.backward(); clip_grad_norm_ over the optimiser's parameters (max_grad_norm=None: none); optimizer.step().  target_kl: training stops
    before the step of the first minibatch whose approx_kl exceeds 1.5 target_kl, as in SB3 - that 4-byte read per minibatch is the only host
    read; None reads nothing.  Returns the last minibatch's stats (float32 [8], on the device; loss_head.STATS), None when there was none."""
    params = [p for group in optimizer.param_groups for p in group["params"]]
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
            if max_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
            optimizer.step()
    return stats
