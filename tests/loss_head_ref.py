"""Restatements of the device loss heads (tactile_gym_amd.loss_head; csrc/tg_loss_head.hip).

`ppo_exact` and `rsample_exact` are stable_baselines3's lines (PPO.train from evaluate_actions to loss; SAC's actor.action_log_prob) in float64
torch, differentiated by torch autograd.  `mistake=` puts one usual mistake into them.  `ppo_device_order` / `rsample_bwd_device_order`
follow the kernels operation for operation in numpy float32 (double where the kernels use double, the same chunks and lane tree).

The bounds.  U = 2^-24 is the float32 unit roundoff, D = 2^-53 the double one; one rounding of v errs by at most U |v|; a transcendental
function evaluated in double and rounded to float32 counts as two roundings (tests/action_head_ref.py).  First order in U; SLACK = 1 + 1e-5
covers the second-order terms.  A mean over B rows accumulated in double and rounded once: mean_err(rows' bounds, rows' values) =
mean(bounds) + (B + 2) D mean|v| + U |mean v|.  Everything is evaluated from the float64 results `ex` of ppo_exact.

  log_prob   action_head_ref.bound_gaussian_sum with x = actions: U (A + 10) sum_j T_j =: b_lp                      (d = fl(actions - mean): U |d|)
  lr = fl(log_prob - old):  e_lr = b_lp + U |lr|;   ratio = fl(exp(lr)), condition number ratio:  b_ratio = ratio (e_lr + 2 U)
  adv  (normalised)  m^ = fl(m) U |m|;  s^ = fl(s) U s;  c = fl(adv - m^) U |m| + U |c|;  den = fl(s^ + 1e-8f) <= 2 U den;  fl(c / den):
        adv_mean: e_m = (B + 2) D mean|adv| + U |m|;  adv_std: e_s = U s + (B + 2) D s;
        b_adv = (e_m + U |c|) / den + |adv_n| (e_s / den + 2 U)       (0 when not normalised)
  (torch's own float32 composition accumulates its means, std and sums in float32, in an order of its own: for it D is replaced by U, `acc=U`)
  p1 = fl(adv ratio):  b_p1 = |ratio| b_adv + |adv_n| b_ratio + U |p1|;   p2 = fl(adv rc), rc = fl(1 -+ c) (2 U (1 + c)) where clipped:
        b_p2 = |rc| b_adv + |adv_n| 2 U (1 + c) + U |p2|, b_p1 where not;   min is 1-Lipschitz:  b_surr = max(b_p1, b_p2)
  policy_loss = mean_err(b_surr, surrogate)
  value row  no clip: diff = fl(ret - v) U |diff| =: b_diff;  clip: dv = fl(v - ov) U |dv| (U cvf where clipped), vp = fl(ov + dc) U |vp|,
        b_diff = those + U |diff|;   sq = fl(diff diff): 2 |diff| b_diff + U sq;   value_loss = mean_err(.., sq)
  entropy row  h_j = fl(K^ + ls_j), K = 0.5 + log sqrt(2 pi): U K + U |h_j|;  the A - 1 additions U sum_j |h_j| each:
        sum_j (U K + U |h_j|) + (A - 1) U sum_j |h_j|;   entropy_loss = mean_err(.., entropy)
  loss = fl(fl(pl + fl(ec el)) + fl(vc vl)):  b_pl + |ec| b_el + 2 U |ec el| + |vc| b_vl + 2 U |vc vl| + U |pl + ec el| + U |loss|
  approx_kl row  r1 = fl(ratio - 1): b_ratio + U |r1|;  fl(r1 - lr): + e_lr + U |kl|;   mean_err
  clip_fraction  the indicator is exact where no ratio lies within b_ratio of 1 -+ c (an input condition of the tests): mean_err(0, ind)
  coef = dloss / dlog_prob = -fl(p1 / B) where the surrogate passes:  b_coef = b_p1 / B + U |coef|, and + |p1| / B on a row outside the clip
        range whose |adv_n| <= b_adv (the float32 sign of adv, which decides, may differ there)
  dmean_j = fl(coef fl(d / var)):  d U, var = fl(sigma^ sigma^) 5 U, the quotient U: 7 U;   |d / sigma^2| b_coef + 8 U |dmean_j|
  dls_j = fl(fl(coef dl) - ge), dl = fl(fl(q / var) - 1), qs = d^2 / sigma^2 (9 U), ge = fl(ec^ / B) (2 U):
        row: |dl| b_coef + U |coef| (9 qs + 2 |dl|) + 2 U |ge| + U |dls_j|;   [A]: the rows' sum in double, sum(rows) + (B + 2) D sum|.| + U |total|
  dvalues = -fl(fl(fl(2 diff) vc^) / B):  (2 |vc| / B) b_diff + 3 U |dvalues|    (the clip's pass is exact: input condition)

  rsample's backward, against autograd through the float64 composition from (mean, ls, eps), so the forward's errors count too:
        a:  e_a = (1 - a^2) bound_x + 2 U |a|;   om = fl(1 - fl(a a)):  e_om = U (a^2 + |om|) + 2 |a| e_a;   w = fl(om + 1e-6f):  e_w = e_om + U (w + 1e-6)
        s1 = fl(g_a om): |g_a| e_om + U |s1|;   n2 = fl(2 a om): 2 e_a |om| + 2 |a| e_om + U |n2|;   n3 = fl(n2 / w), condition number 1 / w:
        e_n3 = e_n2 / w + |n3| e_w / w + U |n3|;   n4 = fl(g_lp n3): |g_lp| e_n3 + U |n4|;   s = fl(s1 + n4):  b_s = .. + U |s|        dmean
        dls = fl(fl(fl(s sigma^) eps) - g_lp):  |sigma eps| b_s + 4 U |s sigma eps| + U |dls|       (sigma^ 2 U, two products)
  The kernel takes the Gaussian sum's gradient analytically (0 to mean, -1 to log_std).  torch's own float32 autograd walks the two paths that
  cancel, G = g_lp d / sigma^2 = g_lp eps / sigma to x and -G to mean: the sum at x is rounded with G in it, U (|G| + |s|), before -G arrives,
  and at log_std g_lp d^2 / sigma^2 (some 10 roundings) meets -G sigma eps (some 5), with d^ = fl(x - mean) off sigma eps by U (|x| + 2 |sigma eps|).
  For that composition alone (`autograd32`):  dmean + 2 U |G|;   dls + |sigma eps| 2 U |G| + U |g_lp| (15 eps^2 + |eps| / sigma (|x| + 2 |sigma eps|)).
  The fused gradient does not need the allowance: it is the more accurate of the two.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import action_head_ref as head  # noqa: E402

U, SLACK, LOG_SQRT_2PI = head.U, head.SLACK, head.LOG_SQRT_2PI
D = 2.0 ** -53
CHUNK = 256
STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std")
PPO_MISTAKES = ("max for min", "clamp passes when clipped", "variance over B", "1e-8 left out", "value clip when none asked", "entropy sign",
                "entropy missing from dlog_std", "approx_kl as mean(old - new)", "clip_fraction with >=")
DEVICE_MISTAKES = ("gate drops a NaN", "dlog_std factors the two paths")   # ppo_device_order's selects before the kernel followed autograd there
RSAMPLE_DEVICE_MISTAKES = ("cancelled paths taken as 0",)                  # rsample_bwd_device_order's, likewise
RSAMPLE_MISTAKES = ("mask left out", "g_lp term left out", "sigma eps left out", "epsilon inside the square")
_f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- float64 torch, autograd
def ppo_exact(mean, log_std, values, actions, old_log_prob, advantages, returns, old_values=None, clip_range=0.2, clip_range_vf=None, ent_coef=0.0,
              vf_coef=0.5, normalize_advantage=True, mistake=None, dtype=None):
    """SB3's PPO.train on one minibatch -> dict of numpy float64: the eight stats, log_prob, ratio, adv (normalised), surrogate, dmean, dlog_std,
    dvalues.  dtype: torch.float32 gives torch's own float32 composition."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    t = lambda x: None if x is None else torch.tensor(np.asarray(x), dtype=dtype)   # noqa: E731
    mean, log_std, values = (t(x).requires_grad_() for x in (mean, log_std, values))
    actions, old_lp, adv, ret, old_values = t(actions), t(old_log_prob), t(advantages), t(returns), t(old_values)
    B, A = mean.shape
    c = clip_range
    ls = log_std.expand(B, A)
    log_prob = (-(actions - mean) ** 2 / (2 * torch.exp(ls) ** 2) - ls - LOG_SQRT_2PI).sum(dim=1)      # Normal.log_prob, summed
    entropy = (0.5 + LOG_SQRT_2PI + ls).sum(dim=1)                                                   # Normal.entropy, summed
    adv_mean, adv_std = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    if normalize_advantage and B > 1:
        adv_mean, adv_std = adv.mean(), adv.std(unbiased=mistake != "variance over B")
        adv = (adv - adv_mean) / (adv_std + (0.0 if mistake == "1e-8 left out" else 1e-8))
    ratio = torch.exp(log_prob - old_lp)
    p1 = adv * ratio
    clamped = torch.clamp(ratio, 1 - c, 1 + c)
    if mistake == "clamp passes when clipped":
        clamped = ratio + (clamped - ratio).detach()
    p2 = adv * clamped
    surrogate = torch.max(p1, p2) if mistake == "max for min" else torch.min(p1, p2)
    policy_loss = -surrogate.mean()
    if clip_range_vf is None and mistake == "value clip when none asked":
        clip_range_vf = 0.2
    values_pred = values if clip_range_vf is None else old_values + torch.clamp(values - old_values, -clip_range_vf, clip_range_vf)
    value_loss = ((ret - values_pred) ** 2).mean()                                                   # F.mse_loss
    entropy_loss = entropy.mean() if mistake == "entropy sign" else -entropy.mean()
    grad_entropy = entropy_loss.detach() if mistake == "entropy missing from dlog_std" else entropy_loss
    loss = policy_loss + ent_coef * grad_entropy + vf_coef * value_loss
    with torch.no_grad():
        log_ratio = log_prob - old_lp
        approx_kl = (-log_ratio).mean() if mistake == "approx_kl as mean(old - new)" else ((torch.exp(log_ratio) - 1) - log_ratio).mean()
        off = torch.abs(ratio - 1)
        clip_fraction = ((off >= c) if mistake == "clip_fraction with >=" else (off > c)).to(dtype).mean()
    loss.backward()
    n = lambda x: x.detach().to(torch.float64).numpy()   # noqa: E731
    zero = lambda x: n(x.grad) if x.grad is not None else np.zeros(tuple(x.shape))   # noqa: E731
    return dict(loss=n(loss), policy_loss=n(policy_loss), value_loss=n(value_loss), entropy_loss=n(entropy_loss), approx_kl=n(approx_kl),
                clip_fraction=n(clip_fraction), adv_mean=n(adv_mean), adv_std=n(adv_std), log_prob=n(log_prob), ratio=n(ratio), adv=n(adv),
                surrogate=n(surrogate), dmean=zero(mean), dlog_std=zero(log_std), dvalues=zero(values))


def rsample_exact(mean, log_std, eps, g_a=None, g_lp=None, log_std_min=-20.0, log_std_max=2.0, mistake=None, dtype=None):
    """SAC's actor.action_log_prob with the noise given -> dict(actions, log_prob, dmean, dlog_std): the gradients of sum(g_a actions) +
    sum(g_lp log_prob) by autograd through the whole composition."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    t = lambda x: None if x is None else torch.tensor(np.asarray(x), dtype=dtype)   # noqa: E731
    mean, log_std = t(mean).requires_grad_(), t(log_std).requires_grad_()
    eps, g_a, g_lp = t(eps), t(g_a), t(g_lp)
    B, A = mean.shape
    ls = torch.clamp(log_std, log_std_min, log_std_max)
    if mistake == "mask left out":
        ls = log_std + (ls - log_std).detach()
    ls = ls.expand(B, A)
    sigma = torch.exp(ls)
    noise_term = sigma.detach() * eps if mistake == "sigma eps left out" else sigma * eps
    x = mean + noise_term
    gaussian = (-(x - mean) ** 2 / (2 * sigma ** 2) - ls - LOG_SQRT_2PI).sum(dim=1)
    a = torch.tanh(x)
    correction = torch.log(1 - (a + 1e-6) ** 2 if mistake == "epsilon inside the square" else 1 - a ** 2 + 1e-6).sum(dim=1)
    log_prob = gaussian - correction
    if mistake == "g_lp term left out":                   # the Gaussian sum's -1 to log_std never arrives
        log_prob = gaussian.detach() - correction
    out = torch.zeros((), dtype=dtype)
    if g_a is not None:
        out = out + (g_a * a).sum()
    if g_lp is not None:
        out = out + (g_lp * log_prob).sum()
    out.backward()
    n = lambda v: v.detach().to(torch.float64).numpy()   # noqa: E731
    return dict(actions=n(a), log_prob=n(log_prob), dmean=n(mean.grad), dlog_std=n(log_std.grad))


# ---------------------------------------------------------------------------------------------------------------- the kernels' order
def tree_sum(v, B):
    """The sum over rows of v (float64 [B] or [B, K]) the way the kernels take it: chunks of 256 rows, in each wave of 64 lanes
    v[i] += v[i + off] for off = 32 .. 1, the four wave sums in wave order, the chunk sums ascending."""
    v = np.asarray(v, dtype=np.float64).reshape(B, -1)
    chunks = (B + CHUNK - 1) // CHUNK
    pad = np.zeros((chunks * CHUNK, v.shape[1]))
    pad[:B] = v
    lanes = pad.reshape(chunks, 4, 64, -1).copy()
    off = 32
    while off >= 1:
        lanes[:, :, :off] = lanes[:, :, :off] + lanes[:, :, off:2 * off]
        off //= 2
    w = lanes[:, :, 0]
    per_chunk = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    total = np.zeros(v.shape[1])
    for k in range(chunks):
        total = total + per_chunk[k]
    return total


def ppo_device_order(mean, log_std, values, actions, old_log_prob, advantages, returns, old_values=None, clip_range=0.2, clip_range_vf=None,
                     ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, mistake=None):
    """What one tg_ppo_loss call writes: dict(stats [8], log_prob, dmean, dlog_std, dvalues) of float32 arrays.  mistake (DEVICE_MISTAKES): the
    selects the kernel had before it followed torch's autograd on non-finite values."""
    with np.errstate(all="ignore"):
        mean, actions = np.asarray(mean, _f32), np.asarray(actions, _f32)
        B, A = mean.shape
        per_row = np.asarray(log_std).ndim == 2
        ls = np.broadcast_to(np.asarray(log_std, _f32), (B, A))
        values, old_lp, adv, ret = (np.asarray(x, _f32) for x in (values, old_log_prob, advantages, returns))
        c, ec, vc, fB = _f32(clip_range), _f32(ent_coef), _f32(vf_coef), _f32(B)
        sigma = np.exp(ls.astype(np.float64)).astype(_f32)
        d = actions - mean
        var = sigma * sigma
        term = ((-((d * d) / (_f32(2.0) * var)) - ls) - _f32(LOG_SQRT_2PI)).astype(_f32)
        h = (_f32(1.4189385332046727) + ls).astype(_f32)
        lp, ent = np.zeros(B, _f32), np.zeros(B, _f32)
        for j in range(A):
            lp, ent = lp + term[:, j], ent + h[:, j]
        adv_mean, adv_std = _f32(0.0), _f32(1.0)
        if normalize_advantage and B > 1:
            m = tree_sum(adv, B)[0] / float(B)
            ss = tree_sum((adv.astype(np.float64) - m) ** 2, B)[0]
            adv_mean, adv_std = _f32(m), _f32(np.sqrt(ss / float(B - 1)))
            adv = (adv - adv_mean) / (adv_std + _f32(1e-8))
        lr = lp - old_lp
        ratio = np.exp(lr.astype(np.float64)).astype(_f32)
        lo, hi = _f32(1.0) - c, _f32(1.0) + c
        p1 = adv * ratio
        p2 = adv * np.where(ratio < lo, lo, np.where(ratio > hi, hi, ratio)).astype(_f32)
        pm = np.where(p2 < p1, p2, p1)
        inside = (ratio >= lo) & (ratio <= hi)
        g = p1 / fB
        if mistake == "gate drops a NaN":
            coef = np.where(inside | (p1 < p2), -g, _f32(0.0)).astype(_f32)
        else:                                             # chunk_pass: passes (a NaN product too), blocked, equal outside the clip
            blocked = (_f32(0.0) * np.abs(adv)) * ratio
            coef = np.where(inside | ~(p1 >= p2), -g, np.where(p1 > p2, blocked, _f32(0.0) - g)).astype(_f32)
        vp, vpass = values, np.ones(B, bool)
        if clip_range_vf is not None:
            cv, ov = _f32(clip_range_vf), np.asarray(old_values, _f32)
            dv = values - ov
            vp = ov + np.where(dv < -cv, -cv, np.where(dv > cv, cv, dv)).astype(_f32)
            vpass = (dv >= -cv) & (dv <= cv)
        diff = ret - vp
        dvalues = np.where(vpass, -(((_f32(2.0) * diff) * vc) / fB), _f32(0.0)).astype(_f32)
        r1 = ratio - _f32(1.0)
        sums = tree_sum(np.stack([pm, diff * diff, ent, r1 - lr, (np.abs(r1) > c).astype(_f32)], axis=1), B)
        pl, vl, el = _f32(-(sums[0] / B)), _f32(sums[1] / B), _f32(-(sums[2] / B))
        stats = np.array([(pl + ec * el) + vc * vl, pl, vl, el, _f32(sums[3] / B), _f32(sums[4] / B), adv_mean, adv_std], _f32)
        dmean = (coef[:, None] * (d / var)).astype(_f32)
        cl = coef[:, None] * (((d * d) / var) - _f32(1.0))
        if mistake != "dlog_std factors the two paths":   # 0, or NaN for a non-finite coef or sigma (not sigma^2, which overflows first)
            lost = (coef - coef)[:, None] + (sigma - sigma)
            cl = np.where(lost == 0, cl, lost)
        dls = (cl - ec / fB).astype(_f32)
        if not per_row:
            dls = tree_sum(dls, B).astype(_f32)
        return dict(stats=stats, log_prob=lp, dmean=dmean, dlog_std=dls, dvalues=dvalues)


def rsample_saved_eps(mean, eps):
    """What tg_squashed_rsample saves as eps_out: the noise, NaN where mean is not finite (x - mean is NaN there, and autograd's gradients)."""
    with np.errstate(all="ignore"):
        mean, eps = np.asarray(mean, _f32), np.asarray(eps, _f32)
        return np.where(mean - mean == 0, eps, mean - mean).astype(_f32)


def rsample_bwd_device_order(g_a, g_lp, a, eps, sigma, log_std, log_std_min=-20.0, log_std_max=2.0, mistake=None):
    """What one tg_squashed_rsample_bwd call writes: (dmean, dlog_std), float32 [B, A].  mistake="cancelled paths taken as 0": the kernel
    before it gave NaN where the Gaussian sum's two gradients, G to x and -G to mean, are not finite."""
    with np.errstate(all="ignore"):
        return _rsample_bwd(g_a, g_lp, a, eps, sigma, log_std, log_std_min, log_std_max, mistake)


def _rsample_bwd(g_a, g_lp, a, eps, sigma, log_std, log_std_min, log_std_max, mistake):
    a, eps, sigma = (np.asarray(x, _f32) for x in (a, eps, sigma))
    ls = np.broadcast_to(np.asarray(log_std, _f32), a.shape)
    om = _f32(1.0) - a * a
    w = om + _f32(1e-6)
    s = np.zeros_like(a)
    glp = np.zeros((a.shape[0], 1), _f32)
    if g_a is not None:
        s = np.asarray(g_a, _f32) * om
    if g_lp is not None:
        glp = np.asarray(g_lp, _f32)[:, None]
        s = s + glp * (((_f32(2.0) * a) * om) / w)
        if mistake != "cancelled paths taken as 0":
            G = glp * ((sigma * eps) / (sigma * sigma))
            s = np.where(G - G == 0, s, G - G)
    inside = (ls >= _f32(log_std_min)) & (ls <= _f32(log_std_max))
    return s.astype(_f32), np.where(inside, ((s * sigma) * eps) - glp, _f32(0.0)).astype(_f32)


# ---------------------------------------------------------------------------------------------------------------- the bounds (module docstring)
def _mean_err(bounds, v, acc=D):
    v = np.asarray(v, np.float64)
    B = v.shape[0]
    return np.mean(bounds) + (B + 2) * acc * np.mean(np.abs(v)) + U * np.abs(np.mean(v))


def ppo_bounds(ex, mean, log_std, values, actions, old_log_prob, advantages, returns, old_values=None, clip_range=0.2, clip_range_vf=None,
               ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, acc=D):
    """name -> bound (float64, the shape of ex[name]) for the eight stats, log_prob, ratio, dmean, dlog_std, dvalues; ex: ppo_exact's result.
    acc: the unit roundoff of the accumulators of the sums over rows - D for the kernels, U for torch's own float32 mean / std / sum (any order)."""
    f = lambda x: np.asarray(x, np.float64)   # noqa: E731
    mean, values, actions, old_lp, adv0, ret = (f(x) for x in (mean, values, actions, old_log_prob, advantages, returns))
    B, A = mean.shape
    per_row = np.asarray(log_std).ndim == 2
    ls = np.broadcast_to(f(log_std), (B, A))
    c, ec, vc = float(clip_range), float(ent_coef), float(vf_coef)
    b_lp = head.bound_gaussian_sum(actions, mean, ls) / SLACK
    lr = ex["log_prob"] - old_lp
    e_lr = b_lp + U * np.abs(lr)
    ratio, adv = ex["ratio"], ex["adv"]
    b_ratio = ratio * (e_lr + 2 * U)
    out = {"log_prob": b_lp, "ratio": b_ratio}
    if normalize_advantage and B > 1:
        m, s = float(ex["adv_mean"]), float(ex["adv_std"])
        den = s + 1e-8
        out["adv_mean"] = (B + 2) * acc * np.mean(np.abs(adv0)) + U * abs(m)
        out["adv_std"] = U * s + (B + 2) * acc * s
        b_adv = (out["adv_mean"] + U * np.abs(adv * den)) / den + np.abs(adv) * (out["adv_std"] / den + 2 * U)
    else:
        b_adv = np.zeros(B)
        out["adv_mean"] = out["adv_std"] = 0.0
    p1 = adv * ratio
    b_p1 = ratio * b_adv + np.abs(adv) * b_ratio + U * np.abs(p1)
    clipped = (ratio < 1 - c) | (ratio > 1 + c)
    rc = np.clip(ratio, 1 - c, 1 + c)
    b_p2 = np.where(clipped, rc * b_adv + np.abs(adv) * 2 * U * (1 + c) + U * np.abs(adv * rc), b_p1)
    out["policy_loss"] = _mean_err(np.maximum(b_p1, b_p2), ex["surrogate"], acc)
    if clip_range_vf is None:
        vp, b_vp, vpass = values, np.zeros(B), np.ones(B, bool)
    else:
        ov = f(old_values)
        dv = values - ov
        vpass = np.abs(dv) <= clip_range_vf
        vp = ov + np.clip(dv, -clip_range_vf, clip_range_vf)
        b_vp = np.where(vpass, U * np.abs(dv), U * clip_range_vf) + U * np.abs(vp)
    diff = ret - vp
    b_diff = b_vp + U * np.abs(diff)
    out["value_loss"] = _mean_err(2 * np.abs(diff) * b_diff + U * diff * diff, diff * diff, acc)
    K = 0.5 + LOG_SQRT_2PI
    habs = np.abs(K + ls)
    b_ent = (U * K + U * habs).sum(axis=1) + (A - 1) * U * habs.sum(axis=1)
    out["entropy_loss"] = _mean_err(b_ent, (K + ls).sum(axis=1), acc)
    pl, el, vl = float(ex["policy_loss"]), float(ex["entropy_loss"]), float(ex["value_loss"])
    out["loss"] = (out["policy_loss"] + abs(ec) * out["entropy_loss"] + 2 * U * abs(ec * el) + abs(vc) * out["value_loss"] + 2 * U * abs(vc * vl)
                   + U * abs(pl + ec * el) + U * abs(float(ex["loss"])))
    r1 = ratio - 1
    out["approx_kl"] = _mean_err(b_ratio + U * np.abs(r1) + e_lr + U * np.abs(r1 - lr), r1 - lr, acc)
    out["clip_fraction"] = _mean_err(np.zeros(B), (np.abs(r1) > c).astype(np.float64), acc)
    passes = ~clipped | (p1 < adv * rc)
    coef = np.where(passes, -p1 / B, 0.0)
    b_coef = b_p1 / B + U * np.abs(coef) + np.where(clipped & (np.abs(adv) <= b_adv), np.abs(p1) / B, 0.0)
    sig2 = np.exp(2 * ls)
    d = actions - mean
    dm, qs = d / sig2, d * d / sig2
    dl = qs - 1
    out["dmean"] = np.abs(dm) * b_coef[:, None] + 8 * U * np.abs(coef[:, None] * dm)
    ge = ec / B
    gl = coef[:, None] * dl - ge
    rows = np.abs(dl) * b_coef[:, None] + U * np.abs(coef[:, None]) * (9 * qs + 2 * np.abs(dl)) + 2 * U * abs(ge) + U * np.abs(gl)
    out["dlog_std"] = rows if per_row else rows.sum(axis=0) + (B + 2) * acc * np.abs(gl).sum(axis=0) + U * np.abs(gl.sum(axis=0))
    dvalues = np.where(vpass, -2 * diff * vc / B, 0.0)
    out["dvalues"] = np.where(vpass, 2 * abs(vc) / B * b_diff, 0.0) + 3 * U * np.abs(dvalues)
    return {k: SLACK * np.asarray(v, np.float64) for k, v in out.items()}


def rsample_forward_bounds(mean, log_std, eps, log_std_min=-20.0, log_std_max=2.0, log_of_exp=False):
    """dict(actions [B, A], log_prob [B]): a float32 forward pass against rsample_exact, the WHOLE composition from (mean, log_std, eps) - where
    action_head_ref's bounds take each stage at the float32 output of the stage before.  a: (1 - a^2) bound_x + bound_tanh.  log_prob: the
    stages' bound_squashed_sum, plus per column what x^ and a^ carry in: the Gaussian term t = d^2 / (2 sigma^2) has dt/dx = eps / sigma,
    (|eps| / sigma) bound_x, and log w has the condition number 1 / w, 2 |a| b_a / w.  log_of_exp: torch's Normal.log_prob (log of the rounded exp)."""
    f = lambda v: np.asarray(v, np.float64)   # noqa: E731
    mean, eps = f(mean), f(eps)
    ls = np.broadcast_to(np.clip(f(log_std), log_std_min, log_std_max), mean.shape)
    sigma = np.exp(ls)
    x = mean + sigma * eps
    a = np.tanh(x)
    w = 1 - a * a + 1e-6
    b_x = head.bound_x(mean, ls, eps)
    b_a = (1 - a * a) * b_x + head.bound_tanh(x)
    carried = (np.abs(eps) / sigma * b_x + 2 * np.abs(a) * b_a / w).sum(axis=1)
    return dict(actions=b_a, log_prob=head.bound_squashed_sum(x, mean, ls, a, log_of_exp) + SLACK * carried)


def mlp_bounds(x, layers):
    """(q float64 [B], bound [B]) of a float32 Linear - Tanh - Linear evaluated on the float32 rows x [B, n]; layers = (W1, b1, W2, b2), W2 [1, h].
    A float32 dot product of n terms and a bias, summed in any order, with or without FMA: (n + 1) U (|W| |x| + |b|).  tanh: two roundings and
    a slope <= 1.  z = W1 x + b1: e_z;  h = tanh(z): e_h = e_z + 2 U |h|;  q = W2 h + b2:  |W2| e_h + (h + 1) U (|W2| |h| + |b2|)."""
    W1, b1, W2, b2 = (np.asarray(v, np.float64) for v in layers)
    x = np.asarray(x, np.float64)
    z = x @ W1.T + b1
    e_z = (W1.shape[1] + 1) * U * (np.abs(x) @ np.abs(W1).T + np.abs(b1))
    h = np.tanh(z)
    e_h = e_z + 2 * U * np.abs(h)
    q = h @ W2.T + b2
    e_q = e_h @ np.abs(W2).T + (W2.shape[1] + 1) * U * (np.abs(h) @ np.abs(W2).T + np.abs(b2))
    return q[:, 0], SLACK * e_q[:, 0]


def rsample_bounds(mean, log_std, eps, g_a=None, g_lp=None, log_std_min=-20.0, log_std_max=2.0, autograd32=False):
    """dict(dmean, dlog_std) [B, A]: the bounds of tg_squashed_rsample_bwd's outputs against rsample_exact at the same float32 inputs.
    autograd32: the allowance for autograd's two cancelling paths in float32 (module docstring), for torch's own float32 composition."""
    f = lambda x: np.asarray(x, np.float64)   # noqa: E731
    mean, eps = f(mean), f(eps)
    ls = np.broadcast_to(np.clip(f(log_std), log_std_min, log_std_max), mean.shape)
    sigma = np.exp(ls)
    x = mean + sigma * eps
    a = np.tanh(x)
    ga = np.zeros_like(mean) if g_a is None else f(g_a)
    glp = np.zeros((mean.shape[0], 1)) if g_lp is None else f(g_lp)[:, None]
    om = 1 - a * a
    w = om + 1e-6
    e_a = om * head.bound_x(mean, ls, eps) / SLACK + 2 * U * np.abs(a)
    e_om = U * (a * a + np.abs(om)) + 2 * np.abs(a) * e_a
    e_w = e_om + U * (w + 1e-6)
    s1 = ga * om
    n2 = 2 * a * om
    n3 = n2 / w
    n4 = glp * n3
    s = s1 + n4
    e_n2 = 2 * e_a * np.abs(om) + 2 * np.abs(a) * e_om + U * np.abs(n2)
    e_n3 = e_n2 / w + np.abs(n3) * e_w / w + U * np.abs(n3)
    b_s = np.abs(ga) * e_om + U * np.abs(s1) + np.abs(glp) * e_n3 + U * np.abs(n4) + U * np.abs(s)
    sse = s * sigma * eps
    inside = (np.broadcast_to(f(log_std), mean.shape) >= log_std_min) & (np.broadcast_to(f(log_std), mean.shape) <= log_std_max)
    b_dls = np.where(inside, np.abs(sigma * eps) * b_s + 4 * U * np.abs(sse) + U * np.abs(sse - glp), 0.0)
    if autograd32:
        G = np.abs(glp * eps / sigma)
        b_s = b_s + 2 * U * G
        b_dls = b_dls + np.where(inside, np.abs(sigma * eps) * 2 * U * G + U * np.abs(glp) * (15 * eps * eps + np.abs(eps) / sigma * (np.abs(x) + 2 * np.abs(sigma * eps))), 0.0)
    return dict(dmean=SLACK * b_s, dlog_std=SLACK * b_dls)


# ---------------------------------------------------------------------------------------------------------------- the inputs of the tests
MARGIN = 1e-4          # no float64 ratio this close to 1 -+ clip_range, no |values - old_values| this close to clip_range_vf


def ppo_inputs(B, A, per_row, seed, clip_range=0.2, clip_range_vf=0.2, adv_scale=1.0, adv_shift=0.3):
    """dict of float32 arrays: one minibatch whose ratios (about 0.6 .. 1.6) and value moves straddle the clips without touching them - rows
    inside MARGIN of a clip edge are moved off it, never excluded."""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-1.0, 1.0, (B, A)).astype(_f32)
    log_std = rng.uniform(-1.5, -0.5, (B, A) if per_row else (A,)).astype(_f32)
    ls = np.broadcast_to(log_std, (B, A)).astype(np.float64)
    actions = (mean + np.exp(ls) * rng.standard_normal((B, A))).astype(_f32)
    lp = head.exact_log_prob(actions, mean, ls)
    old_log_prob = (lp + 0.15 * rng.standard_normal(B)).astype(_f32)
    values = rng.standard_normal(B).astype(_f32)
    old_values = (values + 0.25 * rng.standard_normal(B)).astype(_f32)
    returns = (values + rng.standard_normal(B)).astype(_f32)
    advantages = (adv_scale * (rng.standard_normal(B) + adv_shift)).astype(_f32)
    for _ in range(100):
        ratio = np.exp(lp - old_log_prob)
        near = (np.abs(ratio - (1 - clip_range)) < 2 * MARGIN) | (np.abs(ratio - (1 + clip_range)) < 2 * MARGIN)
        if not near.any():
            break
        old_log_prob[near] += _f32(1e-3)
    if clip_range_vf is not None:
        for _ in range(100):
            near = np.abs(np.abs(values.astype(np.float64) - old_values) - clip_range_vf) < 2 * MARGIN
            if not near.any():
                break
            old_values[near] += _f32(1e-3)
    return dict(mean=mean, log_std=log_std, values=values, actions=actions, old_log_prob=old_log_prob, advantages=advantages, returns=returns,
                old_values=old_values)


def conditions_hold(ex, inp, clip_range, clip_range_vf):
    """The input conditions of the comparisons, from the float64 results."""
    ok = bool((np.abs(ex["ratio"] - (1 - clip_range)) >= MARGIN).all() and (np.abs(ex["ratio"] - (1 + clip_range)) >= MARGIN).all())
    if clip_range_vf is not None:
        ok = ok and bool((np.abs(np.abs(inp["values"].astype(np.float64) - inp["old_values"]) - clip_range_vf) >= MARGIN).all())
    return ok


def rsample_inputs(B, A, seed, saturated=False):
    """dict(mean, log_std [B, A], eps, g_a, g_lp), float32; log_std exactly at -20 and 2 and beyond both, put in deliberately."""
    rng = np.random.default_rng(seed)
    span = 20.0 if saturated else 1.5
    mean = rng.uniform(-span, span, (B, A)).astype(_f32)
    log_std = rng.uniform(-3.0, -1.0, (B, A)).astype(_f32)
    edge = np.array([-20.0, 2.0, -20.5, 2.5, -25.0, 3.0], _f32)
    n = min(edge.size, log_std.size)
    log_std.reshape(-1)[:: max(1, log_std.size // n)][:n] = edge[:n]
    eps = rng.standard_normal((B, A)).astype(_f32)
    return dict(mean=mean, log_std=log_std, eps=eps, g_a=rng.standard_normal((B, A)).astype(_f32), g_lp=rng.standard_normal(B).astype(_f32))
