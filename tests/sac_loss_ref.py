"""Restatements of SAC's device losses (tactile_gym_amd.loss_head.sac_critic_loss / sac_actor_loss; csrc/tg_sac_loss.hip).

`sac_critic_exact` and `sac_actor_exact` are stable_baselines3's lines of SAC.train (cat / min, the TD target, F.mse_loss per critic, the actor
loss, the entropy-coefficient loss) in float64 torch, differentiated by torch autograd.  `mistake=` puts one usual mistake into them; dtype=
torch.float32 gives torch's own float32 composition.  `sac_critic_device_order` / `sac_actor_device_order` follow the kernels operation for
operation in numpy float32 (double where the kernels use double, loss_head_ref.tree_sum for the rows).  The scalars gamma, ent_coef and
target_entropy are float32 arguments of the C entries: the float64 composition takes their float32 values.

The bounds.  U = 2^-24, D = 2^-53; one rounding of v errs by at most U |v|; exp evaluated in double and rounded to float32 counts as two
roundings (tests/action_head_ref.py).  First order in U; SLACK = 1 + 1e-5 covers the second-order terms.  A mean over B rows accumulated in
double and rounded once: mean_err(rows' bounds, rows' values) = mean(bounds) + (B + 2) D mean|v| + U |mean v|  (loss_head_ref._mean_err; torch's
own float32 means accumulate in float32, in an order of its own: D is replaced by U, `acc=U`).  Everything is evaluated from the float64 results.

  alpha = fl(exp(log_ent_coef)):  b_alpha = 2 U alpha;  0 for the float ent_coef                                                   stat ent_coef
  critic, per row.  m = min_i q_next_i: one of the inputs, exact.  t1 = fl(alpha^ nlp):  b_t1 = |nlp| b_alpha + U |t1|;
        y = fl(m - t1):  b_y = b_t1 + U |y|;   nd = fl(1 - dones) and g = fl(nd gamma) are exact for dones in {0, 1} (an input condition);
        t2 = fl(g y):  b_t2 = g b_y + U |t2|;   target = fl(rewards + t2):  b_target = b_t2 + U |target|                             target_out
        e_i = fl(q_cur_i - target^):  b_e = b_target + U |e_i|;   sq_i = fl(e_i e_i):  b_sq = 2 |e_i| b_e + U sq_i
  mse_i = mean_err(b_sq, sq_i);   critic_loss = 0.5 (((0 + mse_0) + mse_1) + ...), 0 + mse_0 and the half exact, the n - 1 other additions
        U times a partial sum <= the whole:  b_loss = 0.5 (sum_i b_mse_i + (n - 1) U sum_i mse_i)
  target_q_mean = mean_err(b_target, target);   min_next_q_mean = mean_err(0, m)
  dq_cur_i = fl(e_i^ / B), B exact in float32:  b_e / B + U |dq_cur_i|
        (torch's autograd: 2 (q - t) grad / numel with the 0.5 folded in, up to three roundings: + 2 U |dq_cur_i|, `autograd32`)
  actor, per row.  m = min_i q_pi_i exact, k its lowest index exact (comparisons of the same float32 inputs).  t1 = fl(alpha^ lp): b_t1 as
        above;  a = fl(t1 - m):  b_a = b_t1 + U |a|;   c = fl(lp + target_entropy):  b_c = U |c|;   p = fl(lec c):  b_p = |lec| b_c + U |p|
  actor_loss = mean_err(b_a, a);  ent_coef_loss = mean_err(b_p, p);  dlog_ent_coef = mean_err(b_c, c);  log_prob_mean = mean_err(0, lp);
  min_q_pi_mean = mean_err(0, m)
  dlog_prob = fl(alpha^ / B):  b_alpha / B + U alpha / B;   dq_pi_i = fl(-1 / B) at i == k and 0 elsewhere:  U / B in every element
        (torch's autograd: fl(1 / B) and then the products, the rows' sum for log_ent_coef in float32:  dlog_prob + U alpha / B,
        dlog_ent_coef + 2 U mean|c| with acc=U, `autograd32`)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_head_ref as base  # noqa: E402

U, D, SLACK, tree_sum = base.U, base.D, base.SLACK, base.tree_sum
CRITIC_STATS = ("critic_loss", "ent_coef", "target_q_mean", "min_next_q_mean", "mse_0", "mse_1", "mse_2", "mse_3")
ACTOR_STATS = ("actor_loss", "ent_coef_loss", "ent_coef", "log_prob_mean", "min_q_pi_mean", "dlog_ent_coef", "unused_6", "unused_7")
CRITIC_MISTAKES = ("max for min", "(1 - dones) left out", "entropy sign in the target", "gamma on the reward", "0.5 left out", "mse as a sum")
ACTOR_MISTAKES = ("min passes gradient to every critic", "alpha not detached", "target_entropy sign", "ent_coef_loss not negated")
DEVICE_MISTAKES = ("fmin drops a NaN", "min skips a later NaN")   # the *_device_order selects before the kernels followed torch.min on a NaN
MARGIN = 1e-4          # no two critics' values this close in a row
_f32 = np.float32


def _f(x):
    """A float32 argument of the C entries as the float64 compositions take it."""
    return float(_f32(x))


def _stack(qs):
    return np.stack([np.asarray(q, np.float64).reshape(-1) for q in qs])


# ---------------------------------------------------------------------------------------------------------------- float64 torch, autograd
def sac_critic_exact(q_cur, q_next, next_log_prob, rewards, dones, gamma, log_ent_coef=None, ent_coef=None, mistake=None, dtype=None):
    """SB3's SAC.train from the target networks' outputs to critic_loss -> dict of numpy float64: critic_loss, ent_coef, target_q_mean,
    min_next_q_mean, mse [n], target [B], min_next_q [B], dq_cur [n, B]."""
    import torch
    import torch.nn.functional as F
    dtype = torch.float64 if dtype is None else dtype
    t = lambda x: torch.tensor(np.asarray(x), dtype=dtype).reshape(-1, 1)   # noqa: E731
    q_cur = [t(q).requires_grad_() for q in q_cur]
    q_next, nlp, rewards, dones = [t(q) for q in q_next], t(next_log_prob), t(rewards), t(dones)
    gamma = _f(gamma)
    alpha = torch.exp(torch.tensor(_f(log_ent_coef), dtype=dtype)) if log_ent_coef is not None else torch.tensor(_f(ent_coef), dtype=dtype)
    with torch.no_grad():
        next_q = torch.cat(q_next, dim=1)
        next_q = (torch.max if mistake == "max for min" else torch.min)(next_q, dim=1, keepdim=True)[0]
        min_next_q = next_q
        next_q = next_q + alpha * nlp if mistake == "entropy sign in the target" else next_q - alpha * nlp
        keep = torch.ones_like(dones) if mistake == "(1 - dones) left out" else 1 - dones
        target = (gamma * rewards if mistake == "gamma on the reward" else rewards) + keep * gamma * next_q
    mses = [((q - target) ** 2).sum() if mistake == "mse as a sum" else F.mse_loss(q, target) for q in q_cur]
    loss = (1.0 if mistake == "0.5 left out" else 0.5) * sum(mses)
    loss.backward()
    n = lambda x: x.detach().to(torch.float64).numpy()   # noqa: E731
    return dict(critic_loss=n(loss), ent_coef=n(alpha), target_q_mean=n(target.mean()), min_next_q_mean=n(min_next_q.mean()),
                mse=np.array([n(m) for m in mses]), target=n(target)[:, 0], min_next_q=n(min_next_q)[:, 0],
                dq_cur=np.stack([n(q.grad)[:, 0] for q in q_cur]))


def sac_actor_exact(log_prob, q_pi, log_ent_coef=None, ent_coef=None, target_entropy=None, mistake=None, dtype=None):
    """SB3's actor_loss and ent_coef_loss -> dict of numpy float64: actor_loss, ent_coef_loss, ent_coef, log_prob_mean, min_q_pi_mean,
    dlog_ent_coef (ent_coef_loss and dlog_ent_coef 0 without a target_entropy), dlog_prob [B], dq_pi [n, B], min_q_pi [B]: the gradients of
    actor_loss + ent_coef_loss."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    t = lambda x: torch.tensor(np.asarray(x), dtype=dtype).reshape(-1, 1)   # noqa: E731
    lp = t(log_prob).requires_grad_()
    q_pi = [t(q).requires_grad_() for q in q_pi]
    lec = torch.tensor(_f(log_ent_coef), dtype=dtype, requires_grad=True) if log_ent_coef is not None else None
    if lec is not None:
        alpha = torch.exp(lec if mistake == "alpha not detached" else lec.detach())
    else:
        alpha = torch.tensor(_f(ent_coef), dtype=dtype)
    qs = torch.cat(q_pi, dim=1)
    min_q = torch.min(qs, dim=1, keepdim=True)[0]
    if mistake == "min passes gradient to every critic":                      # the minimum's value, the sum's gradient
        min_q = min_q.detach() + (qs.sum(dim=1, keepdim=True) - qs.sum(dim=1, keepdim=True).detach())
    actor_loss = (alpha * lp - min_q).mean()
    total = actor_loss
    ent_loss = torch.zeros((), dtype=dtype)
    if target_entropy is not None:
        te = _f(target_entropy)
        c = (lp - te if mistake == "target_entropy sign" else lp + te).detach()
        ent_loss = (lec * c).mean() if mistake == "ent_coef_loss not negated" else -(lec * c).mean()
        total = total + ent_loss
    total.backward()
    n = lambda x: x.detach().to(torch.float64).numpy()   # noqa: E731
    dlec = n(lec.grad) if lec is not None and lec.grad is not None else np.zeros(())
    return dict(actor_loss=n(actor_loss), ent_coef_loss=n(ent_loss), ent_coef=n(alpha), log_prob_mean=n(lp.mean()), min_q_pi_mean=n(min_q.mean()),
                dlog_ent_coef=dlec, dlog_prob=n(lp.grad)[:, 0], dq_pi=np.stack([n(q.grad)[:, 0] for q in q_pi]), min_q_pi=n(min_q)[:, 0])


# ---------------------------------------------------------------------------------------------------------------- the kernels' order
def _alpha32(log_ent_coef, ent_coef):
    return _f32(np.exp(np.float64(_f32(log_ent_coef)))) if log_ent_coef is not None else _f32(ent_coef)


def sac_critic_device_order(q_cur, q_next, next_log_prob, rewards, dones, gamma, log_ent_coef=None, ent_coef=None, mistake=None):
    """What one tg_sac_critic_loss call writes: dict(stats [8], target [B], dq_cur [n, B]) of float32 arrays.  The minimum keeps a NaN, as
    torch.min does; mistake="fmin drops a NaN" is the minimum the kernel took before (DEVICE_MISTAKES)."""
    q_cur, q_next = [np.asarray(q, _f32).reshape(-1) for q in q_cur], [np.asarray(q, _f32).reshape(-1) for q in q_next]
    nlp, rewards, dones = (np.asarray(x, _f32).reshape(-1) for x in (next_log_prob, rewards, dones))
    B, n = nlp.shape[0], len(q_cur)
    alpha, fB = _alpha32(log_ent_coef, ent_coef), _f32(B)
    m = q_next[0]
    for q in q_next[1:]:
        m = np.fmin(m, q) if mistake == "fmin drops a NaN" else np.minimum(m, q)
    with np.errstate(all="ignore"):
        return _critic_rest(q_cur, m, nlp, rewards, dones, gamma, alpha, fB, B, n)


def _critic_rest(q_cur, m, nlp, rewards, dones, gamma, alpha, fB, B, n):
    y = m - alpha * nlp
    target = rewards + ((_f32(1.0) - dones) * _f32(gamma)) * y
    e = [q - target for q in q_cur]
    sums = tree_sum(np.stack([x * x for x in e] + [target, m], axis=1), B)
    stats = np.zeros(8, _f32)
    total = _f32(0.0)
    for i in range(n):
        stats[4 + i] = _f32(sums[i] / B)
        total = total + stats[4 + i]
    stats[0], stats[1], stats[2], stats[3] = _f32(0.5) * total, alpha, _f32(sums[n] / B), _f32(sums[n + 1] / B)
    return dict(stats=stats, target=target.astype(_f32), dq_cur=np.stack([(x / fB).astype(_f32) for x in e]))


def sac_actor_device_order(log_prob, q_pi, log_ent_coef=None, ent_coef=None, target_entropy=None, mistake=None):
    """What one tg_sac_actor_loss call writes: dict(stats [8], dlog_prob [B], dq_pi [n, B]) of float32 arrays.  The minimum and its index are
    torch.min(dim)'s: a NaN wins, the lowest index that holds one; mistake="min skips a later NaN" is the select the kernel had before."""
    with np.errstate(all="ignore"):
        return _actor_order(log_prob, q_pi, log_ent_coef, ent_coef, target_entropy, mistake)


def _actor_order(log_prob, q_pi, log_ent_coef, ent_coef, target_entropy, mistake):
    lp = np.asarray(log_prob, _f32).reshape(-1)
    q_pi = [np.asarray(q, _f32).reshape(-1) for q in q_pi]
    B = lp.shape[0]
    alpha, fB = _alpha32(log_ent_coef, ent_coef), _f32(B)
    m, k = q_pi[0], np.zeros(B, int)
    for i, q in enumerate(q_pi[1:], 1):
        take = q < m
        if mistake != "min skips a later NaN":
            take = take | (np.isnan(q) & ~np.isnan(m))
        k = np.where(take, i, k)
        m = np.where(take, q, m)
    cols = [alpha * lp - m, lp, m]
    if target_entropy is not None:
        c = lp + _f32(target_entropy)
        cols += [_f32(log_ent_coef) * c, c]
    sums = tree_sum(np.stack(cols, axis=1), B)
    stats = np.zeros(8, _f32)
    stats[0], stats[2], stats[3], stats[4] = _f32(sums[0] / B), alpha, _f32(sums[1] / B), _f32(sums[2] / B)
    if target_entropy is not None:
        stats[1], stats[5] = -_f32(sums[3] / B), -_f32(sums[4] / B)
    dq = np.stack([np.where(k == i, _f32(-1.0) / fB, _f32(0.0)).astype(_f32) for i in range(len(q_pi))])
    return dict(stats=stats, dlog_prob=np.full(B, alpha / fB, _f32), dq_pi=dq)


# ---------------------------------------------------------------------------------------------------------------- the bounds (module docstring)
def _b_alpha(ex, log_ent_coef):
    return 2 * U * float(ex["ent_coef"]) if log_ent_coef is not None else 0.0


def sac_critic_bounds(ex, q_cur, q_next, next_log_prob, rewards, dones, gamma, log_ent_coef=None, ent_coef=None, acc=D, autograd32=False):
    """name -> bound (float64, the shape of ex[name]) for critic_loss, ent_coef, target_q_mean, min_next_q_mean, mse [n], target [B] and
    dq_cur [n, B]; ex: sac_critic_exact's result.  acc=U and autograd32: the allowances for torch's own float32 composition."""
    q_cur, nlp = _stack(q_cur), np.asarray(next_log_prob, np.float64).reshape(-1)
    dones = np.asarray(dones, np.float64).reshape(-1)
    assert ((dones == 0) | (dones == 1)).all()
    B, n = nlp.shape[0], q_cur.shape[0]
    alpha, b_alpha = float(ex["ent_coef"]), _b_alpha(ex, log_ent_coef)
    m, target = ex["min_next_q"], ex["target"]
    t1 = alpha * nlp
    b_t1 = np.abs(nlp) * b_alpha + U * np.abs(t1)
    y = m - t1
    b_y = b_t1 + U * np.abs(y)
    g = (1 - dones) * _f(gamma)
    b_target = g * b_y + U * np.abs(g * y) + U * np.abs(target)
    e = q_cur - target
    b_e = b_target + U * np.abs(e)
    sq = e * e
    b_sq = 2 * np.abs(e) * b_e + U * sq
    b_mse = np.array([base._mean_err(b_sq[i], sq[i], acc) for i in range(n)])
    dq = e / B
    out = dict(ent_coef=b_alpha, target=b_target, mse=b_mse, critic_loss=0.5 * (b_mse.sum() + (n - 1) * U * ex["mse"].sum()),
               target_q_mean=base._mean_err(b_target, target, acc), min_next_q_mean=base._mean_err(np.zeros(B), m, acc),
               dq_cur=b_e / B + (3 if autograd32 else 1) * U * np.abs(dq))
    return {k: SLACK * np.asarray(v, np.float64) for k, v in out.items()}


def sac_actor_bounds(ex, log_prob, q_pi, log_ent_coef=None, ent_coef=None, target_entropy=None, acc=D, autograd32=False):
    """name -> bound for actor_loss, ent_coef_loss, ent_coef, log_prob_mean, min_q_pi_mean, dlog_ent_coef, dlog_prob [B], dq_pi [n, B]."""
    lp = np.asarray(log_prob, np.float64).reshape(-1)
    B, n = lp.shape[0], len(q_pi)
    alpha, b_alpha = float(ex["ent_coef"]), _b_alpha(ex, log_ent_coef)
    m = ex["min_q_pi"]
    t1 = alpha * lp
    a = t1 - m
    b_a = np.abs(lp) * b_alpha + U * np.abs(t1) + U * np.abs(a)
    out = dict(ent_coef=b_alpha, actor_loss=base._mean_err(b_a, a, acc), log_prob_mean=base._mean_err(np.zeros(B), lp, acc),
               min_q_pi_mean=base._mean_err(np.zeros(B), m, acc), dlog_prob=np.full(B, b_alpha / B + (2 if autograd32 else 1) * U * alpha / B),
               dq_pi=np.full((n, B), U / B), ent_coef_loss=0.0, dlog_ent_coef=0.0)
    if target_entropy is not None:
        lec = _f(log_ent_coef)
        c = lp + _f(target_entropy)
        b_c = U * np.abs(c)
        out["ent_coef_loss"] = base._mean_err(abs(lec) * b_c + U * np.abs(lec * c), lec * c, acc)
        out["dlog_ent_coef"] = base._mean_err(b_c, c, acc) + (2 * U * np.mean(np.abs(c)) if autograd32 else 0.0)
    return {k: SLACK * np.asarray(v, np.float64) for k, v in out.items()}


def critic_named(dev, n):
    """sac_critic_device_order's (or the kernel's) outputs under sac_critic_exact's names."""
    s = np.asarray(dev["stats"], np.float64)
    out = dict(critic_loss=s[0], ent_coef=s[1], target_q_mean=s[2], min_next_q_mean=s[3], mse=s[4:4 + n])
    out.update({k: dev[k] for k in ("target", "dq_cur") if k in dev})
    return out


def actor_named(dev):
    s = np.asarray(dev["stats"], np.float64)
    out = dict(zip(ACTOR_STATS[:6], s[:6]))
    out.update({k: dev[k] for k in ("dlog_prob", "dq_pi") if k in dev})
    return out


# ---------------------------------------------------------------------------------------------------------------- the inputs of the tests
def _apart(qs):
    """Move the draws of a later critic that land within 2 MARGIN of an earlier one's off it (never dropped); assert the condition."""
    for _ in range(100):
        moved = False
        for j in range(1, len(qs)):
            for i in range(j):
                near = np.abs(qs[j].astype(np.float64) - qs[i]) < 2 * MARGIN
                if near.any():
                    qs[j][near] += _f32(1e-3)
                    moved = True
        if not moved:
            break
    assert critics_apart(qs)
    return qs


def critics_apart(qs):
    qs = _stack(qs)
    return all(bool((np.abs(qs[j] - qs[i]) >= MARGIN).all()) for j in range(len(qs)) for i in range(j))


def sac_critic_inputs(B, n, seed):
    """dict(q_cur, q_next: lists of n float32 [B]; next_log_prob, rewards, dones: float32 [B]); dones exactly 0 or 1, both present when
    B >= 2; no two q_next within MARGIN of each other in a row.  No row is excluded."""
    rng = np.random.default_rng(seed)
    q_next = _apart([(2.0 * rng.standard_normal(B) + 1.0).astype(_f32) for _ in range(n)])
    q_cur = [(2.0 * rng.standard_normal(B) + 1.0).astype(_f32) for _ in range(n)]
    dones = (rng.uniform(size=B) < 0.25).astype(_f32)
    if B >= 2:
        dones[0], dones[B - 1] = 1.0, 0.0
    assert ((dones == 0) | (dones == 1)).all() and (B < 2 or ((dones == 0).any() and (dones == 1).any()))
    return dict(q_cur=q_cur, q_next=q_next, next_log_prob=(1.5 * rng.standard_normal(B) - 1.0).astype(_f32),
                rewards=rng.uniform(-1.0, 1.0, B).astype(_f32), dones=dones)


def sac_actor_inputs(B, n, seed):
    """dict(log_prob: float32 [B]; q_pi: list of n float32 [B]), no two q_pi within MARGIN of each other in a row."""
    rng = np.random.default_rng(seed)
    return dict(log_prob=(1.5 * rng.standard_normal(B) - 1.0).astype(_f32),
                q_pi=_apart([(2.0 * rng.standard_normal(B) + 1.0).astype(_f32) for _ in range(n)]))
