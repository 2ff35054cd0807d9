"""Loss heads in device memory: what stable_baselines3 does between the network's output and the scalar loss, with the gradients at the head's
inputs (csrc/tg_loss_head.hip).

    mean, log_std, values = policy(batch.observations)                                   # PPO.train, per minibatch
    loss, stats = tg.ppo_loss(mean, log_std, values, batch.actions, batch.old_log_prob, batch.advantages, batch.returns,
                              old_values=batch.old_values, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5)
    loss.backward()                                                                      # one launch made loss and gradients (B <= 4096)

    actions, log_prob = head.rsample(mean, log_std)                                      # SAC.train: actor.action_log_prob(obs), tg.DeviceSquashedDiagGaussian
    actor_loss = (ent_coef * log_prob - q(obs, actions)).mean()

    critic_loss, cstats = tg.sac_critic_loss(critic(obs, b.actions), q_next, next_log_prob, b.rewards, b.dones, gamma, log_ent_coef=log_ent_coef)
    actor_loss, ent_coef_loss, astats = tg.sac_actor_loss(log_prob, critic(obs, actions), log_ent_coef=log_ent_coef, target_entropy=-A)
                                                                                         # SAC.train's three losses and their gradients, one launch
                                                                                         # each (csrc/tg_sac_loss.hip; tests/sac_loss_ref.py)

`stats` is a float32 device tensor [8]: loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, adv_mean, adv_std; nothing here
reads it.  The gradients are the fused ones of the kernel (torch autograd's rules written out), scaled by the incoming gradient; advantages,
returns, old values and old log-probs are data and get none.  The arithmetic is restated in tests/loss_head_ref.py.  There is no CPU path.
"""
import torch

from . import _capi as capi
from ._device import checked_f32, launch, ptr, ptrs, workspace

__all__ = ["ppo_loss", "squashed_rsample", "sac_critic_loss", "sac_actor_loss", "STATS", "SAC_CRITIC_STATS", "SAC_ACTOR_STATS"]

STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std")
SAC_CRITIC_STATS = ("critic_loss", "ent_coef", "target_q_mean", "min_next_q_mean", "mse_0", "mse_1", "mse_2", "mse_3")
SAC_ACTOR_STATS = ("actor_loss", "ent_coef_loss", "ent_coef", "log_prob_mean", "min_q_pi_mean", "dlog_ent_coef", "unused_6", "unused_7")


class _PpoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, log_std, values, actions, old_log_prob, advantages, returns, old_values, clip_range, clip_range_vf, ent_coef, vf_coef,
                normalize_advantage, path):
        B, A = mean.shape
        need = ctx.needs_input_grad[:3]
        f32 = dict(dtype=torch.float32, device=mean.device)
        stats = torch.empty(8, **f32)
        dmean = torch.empty_like(mean) if need[0] else None
        dls = torch.empty_like(log_std) if need[1] else None
        dvalues = torch.empty_like(values) if need[2] else None
        grid = path == capi.LOSS_PATH_GRID or (path == capi.LOSS_PATH_AUTO and B > capi.LOSS_ONE_MAX_ROWS)
        nbytes = workspace("tg_ppo_loss_workspace", B, A) if grid else 0
        work = torch.empty(nbytes, dtype=torch.uint8, device=mean.device) if grid else None
        launch("tg_ppo_loss", mean.device, ptr(mean), ptr(log_std), 0 if log_std.dim() == 1 else A, ptr(values), ptr(actions),
               ptr(old_log_prob), ptr(advantages), ptr(returns), ptr(old_values), B, A, clip_range, clip_range_vf, ent_coef, vf_coef,
               1 if normalize_advantage else 0, path, ptr(stats), ptr(None), ptr(dmean), ptr(dls), ptr(dvalues), ptr(work), nbytes)
        ctx.grads = (dmean, dls, dvalues)
        ctx.mark_non_differentiable(stats)
        return stats[0], stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        kept = [g for g in ctx.grads if g is not None]
        scaled = iter(torch._foreach_mul(kept, g_loss) if kept else ())      # one launch for the (up to) three products
        return tuple(None if g is None else next(scaled) for g in ctx.grads) + (None,) * 11


def ppo_loss(mean, log_std, values, actions, old_log_prob, advantages, returns, old_values=None, clip_range=0.2, clip_range_vf=None, ent_coef=0.0,
             vf_coef=0.5, normalize_advantage=True, path=capi.LOSS_PATH_AUTO):
    """(loss, stats): stable_baselines3's PPO.train from evaluate_actions to `loss` on a minibatch.  mean, actions: float32 [B, A]; log_std: [A]
    (PPO's parameter) or [B, A]; values, old_log_prob, advantages, returns, old_values: [B] ([B, 1] is refused: flatten, as SB3 does); all
    contiguous device tensors (anything else is refused, not copied).  loss: a 0-dim float32 tensor with gradients for mean, log_std and
    values; stats: float32 [8] (STATS), on the device.  clip_range_vf=None: no value clip (old_values is then not read).  The advantages are
    normalised only when B > 1, as in SB3.  path: capi.LOSS_PATH_* (tests)."""
    if not isinstance(mean, torch.Tensor):
        raise TypeError(f"mean must be a torch tensor, got {type(mean).__name__}")
    B, A = (int(mean.shape[0]), int(mean.shape[1])) if mean.dim() == 2 else (-1, -1)
    mean = checked_f32(mean, "mean", [(B, A)])
    if B < 1 or not 1 <= A <= capi.HEAD_MAX_ACT:
        raise ValueError(f"mean must be [B, A] with B >= 1 and 1 <= A <= {capi.HEAD_MAX_ACT}, got {tuple(mean.shape)}")
    dev = mean.device
    log_std = checked_f32(log_std, "log_std", [(A,), (B, A)], dev)
    values = checked_f32(values, "values", [(B,)], dev)
    actions = checked_f32(actions, "actions", [(B, A)], dev).detach()
    old_log_prob = checked_f32(old_log_prob, "old_log_prob", [(B,)], dev).detach()
    advantages = checked_f32(advantages, "advantages", [(B,)], dev).detach()
    returns = checked_f32(returns, "returns", [(B,)], dev).detach()
    if clip_range_vf is not None:
        if old_values is None:
            raise ValueError("clip_range_vf needs old_values")
        if not clip_range_vf >= 0:
            raise ValueError(f"clip_range_vf must be None or >= 0, got {clip_range_vf}")
        old_values = checked_f32(old_values, "old_values", [(B,)], dev).detach()
    else:
        old_values = None
    if not clip_range >= 0:
        raise ValueError(f"clip_range must be >= 0, got {clip_range}")
    return _PpoLoss.apply(mean, log_std, values, actions, old_log_prob, advantages, returns, old_values, float(clip_range),
                          -1.0 if clip_range_vf is None else float(clip_range_vf), float(ent_coef), float(vf_coef), bool(normalize_advantage),
                          int(path))


class _SquashedRsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, log_std, ls_min, ls_max, seed, counter, noise):
        B, A = mean.shape
        stride = 0 if log_std.dim() == 1 else A
        save = any(ctx.needs_input_grad[:2])          # under torch.no_grad() nothing needs a gradient: nothing is saved
        actions, log_prob = torch.empty_like(mean), torch.empty(B, dtype=torch.float32, device=mean.device)
        eps = torch.empty_like(mean) if save else None
        sigma = torch.empty_like(mean) if save else None
        launch("tg_squashed_rsample", mean.device, ptr(mean), ptr(log_std), stride, B, A, ls_min, ls_max, seed, counter, ptr(noise),
               ptr(actions), ptr(log_prob), ptr(eps), ptr(sigma))
        if save:
            ctx.save_for_backward(actions, eps, sigma, log_std)
            ctx.clamp = (ls_min, ls_max)
        return actions, log_prob

    @staticmethod
    def backward(ctx, g_a, g_lp):
        actions, eps, sigma, log_std = ctx.saved_tensors
        B, A = actions.shape
        g_a = None if g_a is None else g_a.contiguous()
        g_lp = None if g_lp is None else g_lp.contiguous()
        need_mean, need_ls = ctx.needs_input_grad[:2]
        dmean = torch.empty_like(actions) if need_mean else None
        dls = torch.empty_like(actions) if need_ls else None
        launch("tg_squashed_rsample_bwd", actions.device, ptr(g_a), ptr(g_lp), ptr(actions), ptr(eps), ptr(sigma), ptr(log_std),
               0 if log_std.dim() == 1 else A, B, A, ctx.clamp[0], ctx.clamp[1], ptr(dmean), ptr(dls))
        if dls is not None and log_std.dim() == 1:
            dls = dls.sum(dim=0)                      # a state-independent log_std [A] (not SAC's): the rows' sum, on torch
        return dmean, dls, None, None, None, None, None


def squashed_rsample(mean, log_std, log_std_min=-20.0, log_std_max=2.0, seed=0, counter=0, noise=None):
    """(actions, log_prob): SAC's actor.action_log_prob - DeviceSquashedDiagGaussian.sample's arithmetic at (seed, counter) as fresh tensors
    [B, A] and [B] that carry gradients to mean [B, A] and log_std ([B, A] or [A]), for any B >= 1.  noise: float32 [B, A] used in place of the
    draws.  DeviceSquashedDiagGaussian.rsample calls this with the head's clamp, seed and next counter."""
    if not isinstance(mean, torch.Tensor):
        raise TypeError(f"mean must be a torch tensor, got {type(mean).__name__}")
    B, A = (int(mean.shape[0]), int(mean.shape[1])) if mean.dim() == 2 else (-1, -1)
    mean = checked_f32(mean, "mean", [(B, A)])
    if B < 1 or not 1 <= A <= capi.HEAD_MAX_ACT:
        raise ValueError(f"mean must be [B, A] with B >= 1 and 1 <= A <= {capi.HEAD_MAX_ACT}, got {tuple(mean.shape)}")
    log_std = checked_f32(log_std, "log_std", [(A,), (B, A)], mean.device)
    if noise is not None:
        noise = checked_f32(noise, "noise", [(B, A)], mean.device).detach()
    return _SquashedRsample.apply(mean, log_std, float(log_std_min), float(log_std_max), int(seed), int(counter), noise)


# ---------------------------------------------------------------------------------------------------------------- SAC's losses
def _critic_outputs(qs, name, B=None, device=None):
    """A tuple or list of 1 .. SAC_MAX_CRITICS tensors [B] or [B, 1] -> (list, B)."""
    if not isinstance(qs, (tuple, list)):
        raise TypeError(f"{name} must be a tuple or list of tensors (what SB3's critic returns), got {type(qs).__name__}")
    if not 1 <= len(qs) <= capi.SAC_MAX_CRITICS:
        raise ValueError(f"{name} must hold 1 .. {capi.SAC_MAX_CRITICS} tensors, got {len(qs)}")
    if B is None:
        if not isinstance(qs[0], torch.Tensor):
            raise TypeError(f"{name}[0] must be a torch tensor, got {type(qs[0]).__name__}")
        B = int(qs[0].shape[0]) if qs[0].dim() in (1, 2) else -1
        if not 1 <= B <= capi.SAC_MAX_ROWS:
            raise ValueError(f"{name}[0] must have shape [B] or [B, 1] with 1 <= B <= {capi.SAC_MAX_ROWS}, got {tuple(qs[0].shape)}")
        device = checked_f32(qs[0], f"{name}[0]", [(B,), (B, 1)]).device
    return [checked_f32(q, f"{name}[{i}]", [(B,), (B, 1)], device) for i, q in enumerate(qs)], B


def _alpha_source(log_ent_coef, ent_coef, device):
    """Exactly one of log_ent_coef (a float32 device scalar, never read on the host) and ent_coef (a float) -> (tensor or None, float)."""
    if (log_ent_coef is None) == (ent_coef is None):
        raise ValueError("give exactly one of log_ent_coef (a device tensor) and ent_coef (a float)")
    if log_ent_coef is None:
        return None, float(ent_coef)
    return checked_f32(log_ent_coef, "log_ent_coef", [(), (1,)], device), 0.0


class _SacCriticLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, gamma, ent_coef, log_ent_coef, next_log_prob, rewards, dones, *qs):
        q_next, q_cur = qs[:n], qs[n:]
        B, dev = q_cur[0].shape[0], q_cur[0].device
        stats = torch.empty(8, dtype=torch.float32, device=dev)
        grads = [torch.empty_like(q) if need else None for q, need in zip(q_cur, ctx.needs_input_grad[7 + n:])]
        launch("tg_sac_critic_loss", dev, ptrs(q_cur), ptrs(q_next), n, ptr(next_log_prob), ptr(rewards), ptr(dones), B, gamma,
               ptr(log_ent_coef), ent_coef, ptr(stats), ptr(None), ptrs(grads))
        ctx.grads = grads
        ctx.mark_non_differentiable(stats)
        return stats[0], stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        kept = [g for g in ctx.grads if g is not None]
        scaled = iter(torch._foreach_mul(kept, g_loss) if kept else ())      # one launch for the critics' products
        return (None,) * (7 + len(ctx.grads)) + tuple(None if g is None else next(scaled) for g in ctx.grads)


def sac_critic_loss(q_cur, q_next, next_log_prob, rewards, dones, gamma, log_ent_coef=None, ent_coef=None):
    """(critic_loss, stats): stable_baselines3's SAC.train from the target networks' outputs to critic_loss, one launch.  q_cur =
    critic(observations, actions) and q_next = critic_target(next_observations, next_actions): tuples or lists of the same 1 .. 4 contiguous
    float32 device tensors [B] or [B, 1]; next_log_prob, rewards, dones (float32, the buffer's dones * (1 - timeouts)): [B] or [B, 1].
    target = rewards + (1 - dones) * gamma * (min_i q_next_i - alpha * next_log_prob), critic_loss = 0.5 * sum_i mse(q_cur_i, target), alpha =
    exp(log_ent_coef) read on the device (a 0-dim or [1] tensor) or the float ent_coef - exactly one of the two.  critic_loss: a 0-dim float32
    tensor with gradients for every q_cur_i that asks, in its own shape; everything else is data.  stats: float32 [8] (SAC_CRITIC_STATS)."""
    q_cur, B = _critic_outputs(q_cur, "q_cur")
    dev = q_cur[0].device
    q_next, _ = _critic_outputs(q_next, "q_next", B, dev)
    if len(q_next) != len(q_cur):
        raise ValueError(f"q_cur and q_next must hold the same number of tensors, got {len(q_cur)} and {len(q_next)}")
    rows = [(B,), (B, 1)]
    next_log_prob = checked_f32(next_log_prob, "next_log_prob", rows, dev).detach()
    rewards = checked_f32(rewards, "rewards", rows, dev).detach()
    dones = checked_f32(dones, "dones", rows, dev).detach()
    log_ent_coef, ent_coef = _alpha_source(log_ent_coef, ent_coef, dev)
    if log_ent_coef is not None:
        log_ent_coef = log_ent_coef.detach()
    return _SacCriticLoss.apply(len(q_cur), float(gamma), ent_coef, log_ent_coef, next_log_prob, rewards, dones, *[q.detach() for q in q_next],
                                *q_cur)


class _SacActorLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, ent_coef, target_entropy, log_ent_coef, log_prob, *q_pi):
        B, dev = log_prob.shape[0], log_prob.device
        want = target_entropy is not None
        stats = torch.empty(8, dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad
        grads = [torch.empty_like(log_prob) if need[4] else None] + [torch.empty_like(q) if nd else None for q, nd in zip(q_pi, need[5:])]
        launch("tg_sac_actor_loss", dev, ptr(log_prob), ptrs(q_pi), n, B, ptr(log_ent_coef), ent_coef, target_entropy if want else 0.0,
               1 if want else 0, ptr(stats), ptr(grads[0]), ptrs(grads[1:]))
        ctx.grads = grads
        ctx.dlec = stats[5].reshape(log_ent_coef.shape) if want and need[3] else None      # the launch wrote it into the stats
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return stats[0], stats[1], stats

    @staticmethod
    def backward(ctx, g_actor, g_ent, _g_stats):
        kept = [g for g in ctx.grads if g is not None] if g_actor is not None else []
        scaled = iter(torch._foreach_mul(kept, g_actor) if kept else ())     # one launch for log_prob's and the critics' products
        rows = tuple(None if g is None or g_actor is None else next(scaled) for g in ctx.grads)
        dlec = None if ctx.dlec is None or g_ent is None else ctx.dlec * g_ent
        return (None, None, None, dlec) + rows


def sac_actor_loss(log_prob, q_pi, log_ent_coef=None, ent_coef=None, target_entropy=None):
    """(actor_loss, ent_coef_loss, stats): stable_baselines3's actor_loss = mean(alpha * log_prob - min_i q_pi_i) and ent_coef_loss =
    -mean(log_ent_coef * (log_prob + target_entropy)) in one launch.  log_prob: float32 [B] or [B, 1] (head.rsample's); q_pi =
    critic(observations, actions_pi): a tuple or list of 1 .. 4 contiguous float32 device tensors [B] or [B, 1]; alpha = exp(log_ent_coef) read
    on the device, detached as in SB3, or the float ent_coef - exactly one of the two.  ent_coef_loss is None unless log_ent_coef and
    target_entropy are both given.  Gradients, each in its input's own shape: actor_loss gives log_prob alpha / B and, per row, -1 / B to the
    critic that attains the minimum (the lowest index on a tie); ent_coef_loss gives log_ent_coef -mean(log_prob + target_entropy) and
    log_prob nothing.  stats: float32 [8] (SAC_ACTOR_STATS)."""
    if not isinstance(log_prob, torch.Tensor):
        raise TypeError(f"log_prob must be a torch tensor, got {type(log_prob).__name__}")
    B = int(log_prob.shape[0]) if log_prob.dim() in (1, 2) else -1
    log_prob = checked_f32(log_prob, "log_prob", [(B,), (B, 1)])
    if not 1 <= B <= capi.SAC_MAX_ROWS:
        raise ValueError(f"log_prob must have shape [B] or [B, 1] with 1 <= B <= {capi.SAC_MAX_ROWS}, got {tuple(log_prob.shape)}")
    dev = log_prob.device
    q_pi, _ = _critic_outputs(q_pi, "q_pi", B, dev)
    log_ent_coef, ent_coef = _alpha_source(log_ent_coef, ent_coef, dev)
    if target_entropy is not None and log_ent_coef is None:
        raise ValueError("target_entropy (the entropy-coefficient loss) needs log_ent_coef")
    if target_entropy is None and log_ent_coef is not None:
        log_ent_coef = log_ent_coef.detach()
    actor_loss, ent_coef_loss, stats = _SacActorLoss.apply(len(q_pi), ent_coef, None if target_entropy is None else float(target_entropy),
                                                           log_ent_coef, log_prob, *q_pi)
    return actor_loss, (ent_coef_loss if target_entropy is not None else None), stats
