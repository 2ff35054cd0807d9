"""The table of non-finite inputs for the device losses, and the comparison that judges one case ("Non-finite values").

One case poisons one element of one device input array of one entry with NaN, +inf or -inf; everything else is the finite data of order 1 that
the entry's *_inputs generator draws.  The reference is stable_baselines3's composition in float64 torch (sac_critic_exact, sac_actor_exact,
ppo_exact, rsample_exact), differentiated by torch autograd.  check() holds whatever stands in the kernel's place to three rules, elementwise, with no element
left out:
  1. the class (finite, +inf, -inf, NaN) of every element is the reference's;
  2. where the reference's float64 element has the same bits in its clean and its poisoned run, the device's float32 element has the same bits
     in its clean and its poisoned run: untouched by the reference is untouched by the device.  No tolerance;
  3. every other finite element lies within the bound that the entry's *_ref.py derives, evaluated at the poisoned inputs and used only where
     the bound itself is finite.  No tolerance of this module's own.
A case is valid only if torch's float32 and float64 compositions agree on the class of every element (classes_agree).

The cases.  Rows 0, 63, 64, 255 and 256 = B - 1 at B = 257 (both sides of the wavefront and of the 256-row chunk, a tail chunk of one row), B = 1,
and row 512 of B = 513 (a third chunk, for the sums over rows); column 0 and A - 1 of the [B][A] and [A] arrays.  The full cross of an entry's
switches is taken at row 64; every other position takes the switches in rotation, so that each is met at every position kind by some input.
LEFT_OUT lists the cells that are not run, each with its reason; no NaN cell may stand there.

The entries: SacCritic(n) and SacActor(n) for n in 1, 2, 4 critics, Ppo, Rsample (tg_squashed_rsample with the noise given and its backward
on what it saved), ActionHead, and Gae and VecNorm, whose positions and scenarios are their own (table()).
"""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_head_ref as ppo_ref  # noqa: E402
import sac_loss_ref as sac_ref  # noqa: E402

FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
VALUES = (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf))
GAMMA, TARGET_ENTROPY = 0.95, -2.0
CLIP, CLIP_VF, ENT, VF = 0.2, 0.2, 0.01, 0.5
ROWS = ((257, 0, "row 0"), (257, 63, "row 63"), (257, 64, "row 64"), (257, 255, "row 255"), (257, 256, "row B - 1, a tail chunk of one row"),
        (1, 0, "B = 1"), (513, 512, "a third chunk"))
CROSS = 2                                  # the index in ROWS of the position that takes the full cross of the switches
COLS = ("column 0", "column A - 1")
# The finite elements that a poison touches and whose *_ref.py bound is itself not finite there (rule 3 judges their class alone), per entry
# over its whole table: counted, so that the number cannot grow unnoticed.  PPO's are the rows' outputs under a log_std [A] or an advantage
# statistic that the poison reaches (b_ratio = ratio e_lr with an infinite e_lr, and the means over them).
UNBOUNDED = {"ppo": 8496, "rsample": 72, "action_head": 125}               # every other entry: 0
LEFT_OUT = {}                              # (entry, input, value name, position kind) -> reason; +-inf cells only
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- the comparison
def value_class(x):
    """FINITE, POS_INF, NEG_INF or NAN for every element of x."""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), NAN, np.where(x == np.inf, POS_INF, np.where(x == -np.inf, NEG_INF, FINITE))).astype(np.int8)


def classes_agree(a, b):
    """The names (of two dicts of arrays) whose elements do not all fall into the same class."""
    return [k for k in a if not np.array_equal(value_class(a[k]), value_class(np.broadcast_to(b[k], np.shape(a[k]))))]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.dtype.itemsize in (4, 8)
    u = np.uint32 if a.dtype.itemsize == 4 else np.uint64
    return a.view(u) == b.view(u)


def _at(where):
    return [int(i) for i in where[0]]


def check(got, want, bound, got_clean, want_clean, what=""):
    """The three rules of the module docstring for one case.  got, got_clean: name -> float32 array (float64 for float64 device state) of the poisoned and the clean device run;
    want, want_clean: name -> float64 array of the poisoned and the clean reference run; bound: name -> float64, broadcast to want[name].
    Every element of every name of `want` is judged by rule 1 and then by rule 2 or rule 3 (a non-finite element by rule 1 alone).
    -> dict(elements, untouched, bounded, unbounded, ratio): the counts of the elements judged, of those under rule 2, under rule 3 with a finite
    bound and without one, and the largest error / bound among the bounded."""
    tally = dict(elements=0, untouched=0, bounded=0, unbounded=0, ratio=0.0)
    for k in want:
        w, wc = np.atleast_1d(np.asarray(want[k], np.float64)), np.atleast_1d(np.asarray(want_clean[k], np.float64))
        g, gc = np.atleast_1d(np.asarray(got[k])), np.atleast_1d(np.asarray(got_clean[k]))
        assert g.dtype == gc.dtype and g.dtype in (np.float32, np.float64) and g.shape == w.shape == gc.shape == wc.shape, (what, k, g.dtype, g.shape)
        cg, cw = value_class(g), value_class(w)
        bad = np.argwhere(cg != cw)
        assert bad.size == 0, f"{what}: {k}{_at(bad)} is of class {cg[tuple(bad[0])]} where the reference's is {cw[tuple(bad[0])]} " \
                              f"({len(bad)} of {w.size} elements; 0 finite, 1 +inf, 2 -inf, 3 NaN)"
        untouched = _same_bits(w, wc)
        moved = np.argwhere(untouched & ~_same_bits(g, gc))
        assert moved.size == 0, f"{what}: {k}{_at(moved)} changed on the device ({gc[tuple(moved[0])]!r} -> {g[tuple(moved[0])]!r}) where " \
                                f"the reference kept its bits ({len(moved)} elements)"
        with np.errstate(all="ignore"):
            b = np.broadcast_to(np.asarray(bound[k], np.float64), w.shape)
            rest = ~untouched & (cw == FINITE)
            judged = rest & np.isfinite(b)
            err = np.abs(g.astype(np.float64) - w)
            over = np.argwhere(judged & (err > b))
            assert over.size == 0, f"{what}: {k}{_at(over)} is off by {err[tuple(over[0])]:.3g}, the bound is {b[tuple(over[0])]:.3g}"
            if judged.any():
                r = err[judged] / np.maximum(b[judged], 1e-300)
                tally["ratio"] = max(tally["ratio"], float(np.where(err[judged] == 0, 0.0, r).max()))
        tally["elements"] += w.size
        tally["untouched"] += int(untouched.sum())
        tally["bounded"] += int(judged.sum())
        tally["unbounded"] += int((rest & ~judged).sum())
    return tally


# ---------------------------------------------------------------------------------------------------------------- the entries
def _poisoned(flat, name, index, value):
    out = {k: v.copy() for k, v in flat.items()}
    out[name][index] = value
    return out


class _Sac:
    """What the two SAC entries share.  A configuration: dict(B, source: "log_ent_coef" | "ent_coef" [, target_entropy: bool]).  The device
    inputs `flat`: name -> float32 array, the critics' outputs as q_cur0 .., log_ent_coef as an array of one element."""

    def __init__(self, n):
        self.n, self.name = n, f"{self.kind}, {n} critic{'s' if n > 1 else ''}"

    def split(self, flat):
        """flat -> (the *_inputs dict with its lists of critics, the source of alpha as keyword arguments)."""
        inp = {k: flat[k] for k in self.rows}
        for k in self.lists:
            inp[k] = [flat[f"{k}{i}"] for i in range(self.n)]
        return inp, (dict(log_ent_coef=float(flat["log_ent_coef"][0])) if "log_ent_coef" in flat else dict(ent_coef=0.2))

    def flat(self, cfg):
        inp = self.draw(cfg["B"], self.n, seed=1000 * self.n + cfg["B"])
        out = {k: inp[k] for k in self.rows}
        for k in self.lists:
            out.update({f"{k}{i}": q for i, q in enumerate(inp[k])})
        if cfg["source"] == "log_ent_coef":
            out["log_ent_coef"] = np.array([-0.75], f32)
        return out

    def inputs(self, cfg):
        """[(name, kind of array)]: "rows" [B] or "scalar"."""
        names = [f"{k}{i}" for k in self.lists for i in range(self.n)] + list(self.rows)
        return [(k, "rows") for k in names] + ([("log_ent_coef", "scalar")] if cfg["source"] == "log_ent_coef" else [])


class SacCritic(_Sac):
    kind, rows, lists = "sac_critic", ("next_log_prob", "rewards", "dones"), ("q_cur", "q_next")
    keys = ("critic_loss", "ent_coef", "target_q_mean", "min_next_q_mean", "mse", "target", "dq_cur")
    draw = staticmethod(sac_ref.sac_critic_inputs)
    configs = [dict(source="log_ent_coef"), dict(source="ent_coef")]

    def exact(self, flat, cfg, dtype=None):
        inp, src = self.split(flat)
        return sac_ref.sac_critic_exact(**inp, gamma=GAMMA, **src, dtype=dtype)

    def bounds(self, ex, flat, cfg):
        """sac_critic_bounds at the poisoned inputs.  Its condition that dones is 0 or 1 holds for every finite element; a non-finite one is
        taken as 0 there: its row's target is not finite (1 - dones is not), so no element that rule 3 judges depends on the choice."""
        inp, src = self.split(flat)
        inp["dones"] = np.where(np.isfinite(inp["dones"]), inp["dones"], f32(0.0))
        with np.errstate(all="ignore"):
            return sac_ref.sac_critic_bounds(ex, **inp, gamma=GAMMA, **src)

    def restate(self, flat, cfg, mistake=None):
        inp, src = self.split(flat)
        return self.named(sac_ref.sac_critic_device_order(**inp, gamma=GAMMA, **src, mistake=mistake))

    def named(self, dev):
        out = sac_ref.critic_named(dev, self.n)
        return {k: np.asarray(out[k], f32) for k in self.keys}


class SacActor(_Sac):
    kind, rows, lists = "sac_actor", ("log_prob",), ("q_pi",)
    keys = ("actor_loss", "ent_coef_loss", "ent_coef", "log_prob_mean", "min_q_pi_mean", "dlog_ent_coef", "dlog_prob", "dq_pi")
    draw = staticmethod(sac_ref.sac_actor_inputs)
    configs = [dict(source="log_ent_coef", target_entropy=True), dict(source="log_ent_coef", target_entropy=False),
               dict(source="ent_coef", target_entropy=False)]

    def te(self, cfg):
        return TARGET_ENTROPY if cfg["target_entropy"] else None

    def exact(self, flat, cfg, dtype=None):
        inp, src = self.split(flat)
        return sac_ref.sac_actor_exact(**inp, **src, target_entropy=self.te(cfg), dtype=dtype)

    def bounds(self, ex, flat, cfg):
        inp, src = self.split(flat)
        with np.errstate(all="ignore"):
            return sac_ref.sac_actor_bounds(ex, **inp, **src, target_entropy=self.te(cfg))

    def restate(self, flat, cfg, mistake=None):
        inp, src = self.split(flat)
        return self.named(sac_ref.sac_actor_device_order(**inp, **src, target_entropy=self.te(cfg), mistake=mistake))

    def named(self, dev):
        out = sac_ref.actor_named(dev)
        return {k: np.asarray(out[k], f32) for k in self.keys}


class Ppo:
    """A configuration: dict(B, per_row, normalize, clip_vf).  The two paths are no switch of the table: whatever runs the kernel runs both at
    every case and holds them to the same bits."""
    name, kind, A = "ppo", "ppo", 3
    keys = ppo_ref.STATS + ("log_prob", "dmean", "dlog_std", "dvalues")
    configs = [dict(per_row=r, normalize=m, clip_vf=v) for r, m, v in itertools.product((False, True), repeat=3)]

    def kw(self, cfg):
        return dict(clip_range=CLIP, clip_range_vf=CLIP_VF if cfg["clip_vf"] else None, ent_coef=ENT, vf_coef=VF, normalize_advantage=cfg["normalize"])

    def flat(self, cfg):
        out = ppo_ref.ppo_inputs(cfg["B"], self.A, cfg["per_row"], seed=7 * cfg["B"] + cfg["per_row"], clip_range=CLIP, clip_range_vf=CLIP_VF)
        if not cfg["clip_vf"]:
            del out["old_values"]                  # not read without the clip: no pointer is passed
        return out

    def inputs(self, cfg):
        out = [("mean", "grid"), ("log_std", "grid" if cfg["per_row"] else "columns"), ("values", "rows"), ("actions", "grid"),
               ("old_log_prob", "rows"), ("advantages", "rows"), ("returns", "rows")]
        return out + ([("old_values", "rows")] if cfg["clip_vf"] else [])

    def exact(self, flat, cfg, dtype=None):
        return ppo_ref.ppo_exact(**flat, **self.kw(cfg), dtype=dtype)

    def bounds(self, ex, flat, cfg):
        with np.errstate(all="ignore"):
            return ppo_ref.ppo_bounds(ex, **flat, **self.kw(cfg))

    def restate(self, flat, cfg, mistake=None):
        return self.named(ppo_ref.ppo_device_order(**flat, **self.kw(cfg), mistake=mistake))

    def named(self, dev):
        out = dict(zip(ppo_ref.STATS, np.asarray(dev["stats"], f32)))
        out.update({k: np.asarray(dev[k], f32) for k in ("log_prob", "dmean", "dlog_std", "dvalues")})
        return out


class Rsample:
    """tg_squashed_rsample with the noise given, and tg_squashed_rsample_bwd on what it saved.  A configuration: dict(B, clamp): log_std
    clamped to [-20, 2], or to (-inf, +inf)."""
    name, kind, A = "rsample", "rsample", 3
    keys = ("actions", "log_prob", "dmean", "dlog_std")
    configs = [dict(clamp=True), dict(clamp=False)]

    def clamp(self, cfg):
        return (-20.0, 2.0) if cfg["clamp"] else (-np.inf, np.inf)

    def flat(self, cfg):
        inp = ppo_ref.rsample_inputs(cfg["B"], self.A, seed=3 * cfg["B"])
        return dict(mean=inp["mean"], log_std=inp["log_std"], noise_in=inp["eps"], g_actions=inp["g_a"], g_log_prob=inp["g_lp"])

    def inputs(self, cfg):
        return [("mean", "grid"), ("log_std", "grid"), ("noise_in", "grid"), ("g_actions", "grid"), ("g_log_prob", "rows")]

    def exact(self, flat, cfg, dtype=None):
        lo, hi = self.clamp(cfg)
        return ppo_ref.rsample_exact(flat["mean"], flat["log_std"], flat["noise_in"], flat["g_actions"], flat["g_log_prob"], lo, hi, dtype=dtype)

    def bounds(self, ex, flat, cfg):
        lo, hi = self.clamp(cfg)
        with np.errstate(all="ignore"):
            out = ppo_ref.rsample_forward_bounds(flat["mean"], flat["log_std"], flat["noise_in"], lo, hi)
            out.update(ppo_ref.rsample_bounds(flat["mean"], flat["log_std"], flat["noise_in"], flat["g_actions"], flat["g_log_prob"], lo, hi))
        return out

    def restate(self, flat, cfg, mistake=None):
        lo, hi = self.clamp(cfg)
        one = np.ones(self.A, f32)
        fwd = ppo_ref.head.device_order(ppo_ref.head.SQUASHED, flat["mean"], flat["log_std"], -one, one, lo, hi, noise=flat["noise_in"])
        with np.errstate(all="ignore"):
            sigma = np.exp(ppo_ref.head.clamp(flat["log_std"], lo, hi).astype(np.float64)).astype(f32)
            eps = fwd["noise"] if mistake else ppo_ref.rsample_saved_eps(flat["mean"], fwd["noise"])
            dmean, dls = ppo_ref.rsample_bwd_device_order(flat["g_actions"], flat["g_log_prob"], fwd["actions"], eps, sigma, flat["log_std"], lo, hi,
                                                          mistake=mistake)
        return dict(actions=fwd["actions"], log_prob=fwd["log_prob"], dmean=dmean, dlog_std=dls)


class ActionHead:
    """tg_action_head.  A configuration: dict(B, mode, deterministic, clamp); the uniform mode has the one input noise_in (its u), the two
    others mean, log_std [B][A] and, unless deterministic, noise_in.  The reference: SB3's DiagGaussianDistribution / its squashed kin /
    action_space.sample's affine map, in float64 numpy (np.clip hands a NaN on, as torch.clamp does); deterministic is the mode, mean itself.
    The env bounds are finite: they are host arguments, not device arrays."""
    name, kind, A = "action_head", "action_head", 3
    keys_of = {0: ("actions", "env", "gaussian", "log_prob", "noise"), 1: ("actions", "env", "gaussian", "log_prob", "noise"),
               2: ("actions", "env", "noise")}
    configs = ([dict(mode=m, deterministic=d, clamp=c) for m in (0, 1) for d in (False, True) for c in (True, False)]
               + [dict(mode=2, deterministic=False, clamp=False)])
    lo, hi = np.array([-0.25, -0.35, -0.45], f32), np.array([0.3, 0.5, 0.7], f32)
    keys = None                                # per configuration: keys_for(cfg)

    def keys_for(self, cfg):
        return self.keys_of[cfg["mode"]]

    def clamp(self, cfg):
        return (-2.5, -2.0) if cfg["clamp"] else (-np.inf, np.inf)

    def flat(self, cfg):
        rng = np.random.default_rng(11 * cfg["B"] + cfg["mode"])
        B, A = cfg["B"], self.A
        if cfg["mode"] == 2:
            return dict(noise_in=rng.uniform(0, 1, (B, A)).astype(f32))
        out = dict(mean=rng.uniform(-1.5, 1.5, (B, A)).astype(f32), log_std=rng.uniform(-3.0, -1.5, (B, A)).astype(f32))
        if not cfg["deterministic"]:
            out["noise_in"] = rng.standard_normal((B, A)).astype(f32)
        return out

    def inputs(self, cfg):
        if cfg["mode"] == 2:
            return [("noise_in", "grid")]
        return [("mean", "grid"), ("log_std", "grid")] + ([] if cfg["deterministic"] else [("noise_in", "grid")])

    def exact(self, flat, cfg, dtype=None):
        t = np.float32 if dtype is not None else np.float64
        lo, hi = self.lo.astype(t), self.hi.astype(t)
        with np.errstate(all="ignore"):
            if cfg["mode"] == 2:
                u = flat["noise_in"].astype(t)
                env = np.minimum(lo + (hi - lo) * u, hi)
                return dict(actions=t(2) * ((env - lo) / (hi - lo)) - t(1), env=env, noise=u)
            mean = flat["mean"].astype(t)
            ls = np.clip(flat["log_std"].astype(t), *[t(c) for c in self.clamp(cfg)])
            sigma = np.exp(ls)
            eps = np.zeros_like(mean) if cfg["deterministic"] else flat["noise_in"].astype(t)
            x = mean if cfg["deterministic"] else mean + sigma * eps
            g = (-(x - mean) ** 2 / (2 * sigma ** 2) - ls - t(ppo_ref.LOG_SQRT_2PI)).sum(axis=1)
            if cfg["mode"] == 0:
                return dict(actions=x, env=np.clip(x, lo, hi), gaussian=x, log_prob=g, noise=eps)
            a = np.tanh(x)
            env = np.clip(lo + (t(0.5) * (a + t(1))) * (hi - lo), lo, hi)
            return dict(actions=a, env=env, gaussian=x, log_prob=g - np.log(t(1) - a * a + t(1e-6)).sum(axis=1), noise=eps)

    def bounds(self, ex, flat, cfg):
        """The whole composition from the inputs: action_head_ref's stage bounds with what each stage carries in, as rsample_forward_bounds
        composes them (x carries (|eps| / sigma) bound_x into the Gaussian term, a carries (1 - a^2) bound_x, the affine maps their slope)."""
        head, U = ppo_ref.head, ppo_ref.U
        lo, hi = self.lo.astype(np.float64), self.hi.astype(np.float64)
        with np.errstate(all="ignore"):
            if cfg["mode"] == 2:
                b_env = 3 * U * (np.abs(ex["env"]) + np.abs((hi - lo) * ex["noise"]) + np.abs(lo))
                return dict(noise=0.0, env=b_env, actions=2 * b_env / (hi - lo) + 5 * U * (np.abs(ex["actions"]) + 1))
            mean, eps = flat["mean"].astype(np.float64), ex["noise"]
            ls = np.clip(flat["log_std"].astype(np.float64), *self.clamp(cfg))
            b_x = np.zeros_like(mean) if cfg["deterministic"] else head.bound_x(mean, ls, eps)
            carried = (np.abs(eps) / np.exp(ls) * b_x).sum(axis=1)
            if cfg["mode"] == 0:
                return dict(noise=0.0, gaussian=b_x, actions=b_x, env=b_x, log_prob=head.bound_gaussian_sum(ex["gaussian"], mean, ls) + carried)
            fwd = ppo_ref.rsample_forward_bounds(mean, flat["log_std"], eps, *self.clamp(cfg))
            return dict(noise=0.0, gaussian=b_x, actions=fwd["actions"], log_prob=fwd["log_prob"],
                        env=0.5 * (hi - lo) * fwd["actions"] + head.bound_unscale(ex["actions"], lo, hi))

    def restate(self, flat, cfg, mistake=None):
        head = ppo_ref.head
        out = head.device_order(cfg["mode"], flat.get("mean"), flat.get("log_std"), self.lo, self.hi, *self.clamp(cfg),
                                deterministic=cfg["deterministic"], noise=flat.get("noise_in"), shape=(cfg["B"], self.A),
                                **({"mistake": mistake} if mistake else {}))
        return {k: out[k] for k in self.keys_for(cfg)}


class Gae:
    """tg_rollout_gae at T = 2 kGaeBlock + 1 = 17 steps and N = 65 envs (two workgroups).  A configuration: dict(t, n, start): the poisoned
    step and env (t = T stands for last_values), and where that env's one episode start lies: "none", or directly "after", "at" or "before"
    the poisoned step (for last_values "at" is dones[n], "before" the last step's episode_starts).  dones are bytes: flags, not numbers."""
    name, kind, T, N = "gae", "gae", 17, 65
    keys = ("advantages", "returns")
    GAMMA, LAMBDA = 0.99, 0.95
    STEPS = ((0, "t = 0"), (1, "t = 1, the low side of the last block"), (8, "t = 8, the high side of a block"), (9, "t = 9, the low side of the first block"),
             (16, "t = T - 1"))
    STARTS = ("none", "after", "at", "before")

    def flat(self, cfg):
        from rollout_ref import gae_edge_inputs
        r, v, es, lv, _ = gae_edge_inputs(self.T, self.N, "none")
        d = (np.arange(self.N) % 3 == 1).astype(np.uint8)
        t, n = cfg["t"], cfg["n"]
        d[n] = 0
        at = {"none": None, "after": t + 1, "at": t, "before": t - 1}[cfg["start"]]
        if at is not None and 0 <= at < self.T:
            es[at, n] = 1.0
        elif at is not None and at == self.T:
            d[n] = 1
        return dict(rewards=r, values=v, episode_starts=es, last_values=lv, dones=d)

    def _run(self, fn, flat, **kw):
        adv, ret = fn(flat["rewards"], flat["values"], flat["episode_starts"], flat["last_values"], flat["dones"], self.GAMMA, self.LAMBDA, **kw)
        return dict(advantages=adv, returns=ret)

    def exact(self, flat, cfg, dtype=None):
        from rollout_ref import gae_f64
        return self._run(gae_f64, flat, dtype=np.float32 if dtype is not None else np.float64)

    def bounds(self, ex, flat, cfg):
        from rollout_ref import gae_bound
        with np.errstate(all="ignore"):
            b = gae_bound(flat["rewards"], flat["values"], flat["last_values"], ex["advantages"], self.GAMMA, self.LAMBDA)
            return dict(advantages=b, returns=b + 2.0 ** -24 * np.abs(ex["returns"]))

    def restate(self, flat, cfg, mistake=None):
        from rollout_ref import gae_f32
        return self._run(gae_f32, flat)

    def table(self):
        out, turn = [], 0
        for name in ("rewards", "values", "episode_starts"):
            for value in VALUES:
                for t, kind in self.STEPS:
                    for start in self.STARTS:
                        turn += 1
                        n = (0, 63, 64)[turn % 3]
                        out.append(Case(self, dict(t=t, n=n, start=start), name, (t, n), value, f"{kind}, start {start}"))
        for value in VALUES:
            for n in (0, 63, 64):
                for start in self.STARTS:
                    out.append(Case(self, dict(t=self.T, n=n, start=start), "last_values", n, value, f"env {n}, start {start}"))
        return out

    def owed(self):
        cells = {(self.name, name, v, f"{kind}, start {s}") for name in ("rewards", "values", "episode_starts") for v, _ in VALUES
                 for _, kind in self.STEPS for s in self.STARTS}
        return cells | {(self.name, "last_values", v, f"env {n}, start {s}") for v, _ in VALUES for n in (0, 63, 64) for s in self.STARTS}


class VecNorm:
    """tg_vecnorm_update and tg_vecnorm_apply on one array of width 3 over N = 600 envs (chunks of 256, 256 and 88 rows), from given finite
    statistics.  A configuration: dict(mode, done): mode "step" is VecNormalize.step_wait (update, then apply with the reset of the done
    envs' returns), "follow" a second, clean step after it whose outputs are judged (what a poisoned step leaves behind), "apply" the apply
    alone with training off; done: the poisoned env is done at the poisoned step.  The inputs: obs [N][3], rewards [N], the statistics mean
    [3], var [3], ret_var [1] and the running returns [N] (float64, device state).  The reference is vecnorm_ref.plain, SB3's formulas in
    float64: there is no float32 composition of float64 statistics, so exact() is the same for either dtype.  The bounds: DESIGN.md 4.12's is
    carried along a clean recurrence and does not exist at non-finite statistics; a finite element that the poison touches is an exact 0 (x /
    inf), a clip value or the float32 rounding of a float64 quotient: vecnorm_ref.output_bound, one float32 rounding, for the outputs,
    nothing judged for the statistics
    (on the device they are held to device_order bit for bit)."""
    name, kind, N, D = "vecnorm", "vecnorm", 600, 3
    keys = ("obs_out", "rew_out", "mean", "var", "count", "ret_mean", "ret_var", "ret_count", "returns")
    ROWS = ((5, "the first chunk"), (300, "a middle chunk"), (599, "the last chunk"))

    def flat(self, cfg):
        rng = np.random.default_rng(42)
        return dict(obs=rng.standard_normal((self.N, self.D)).astype(f32), rewards=rng.standard_normal(self.N).astype(f32),
                    mean=np.array([0.1, -0.2, 0.3]), var=np.array([1.5, 0.5, 2.0]), ret_var=np.array([1.3]),
                    returns=rng.standard_normal(self.N), dones=(np.arange(self.N) == cfg["done"]).astype(np.uint8))

    def second(self):
        rng = np.random.default_rng(43)
        return rng.standard_normal((self.N, self.D)).astype(f32), rng.standard_normal(self.N).astype(f32)

    def _model(self, make, flat, cfg):
        m = make({0: self.D}, self.N, training=cfg["mode"] != "apply")
        m.obs_rms[0].mean, m.obs_rms[0].var, m.obs_rms[0].count = flat["mean"].copy(), flat["var"].copy(), np.float64(100.0)
        m.ret_rms.mean, m.ret_rms.var, m.ret_rms.count = np.float64(0.2), np.float64(flat["ret_var"][0]), np.float64(100.0)
        m.returns = flat["returns"].copy()
        with np.errstate(all="ignore"):
            obs, rew, _ = m.step({0: flat["obs"]}, flat["rewards"], flat["dones"] if cfg["mode"] != "apply" else np.zeros(self.N, np.uint8))
            if cfg["mode"] == "follow":
                o2, r2 = self.second()
                obs, rew, _ = m.step({0: o2}, r2, np.zeros(self.N, np.uint8))
        r = m.obs_rms[0]
        return dict(obs_out=obs[0], rew_out=rew, mean=r.mean, var=r.var, count=r.count, ret_mean=m.ret_rms.mean, ret_var=m.ret_rms.var,
                    ret_count=m.ret_rms.count, returns=m.returns)

    def exact(self, flat, cfg, dtype=None):
        import vecnorm_ref
        return self._model(vecnorm_ref.plain, flat, cfg)

    def restate(self, flat, cfg, mistake=None):
        import vecnorm_ref
        make = vecnorm_ref.device_order
        if mistake:
            make = lambda w, n, **kw: vecnorm_ref.VecNormRef(w, n, moments=vecnorm_ref.device_moments_before, **kw)   # noqa: E731
        out = self._model(make, flat, cfg)
        return {k: np.ascontiguousarray(v, f32 if k in ("obs_out", "rew_out") else np.float64) for k, v in out.items()}

    def bounds(self, ex, flat, cfg):
        with np.errstate(all="ignore"):
            out = {k: np.nan for k in self.keys}
            import vecnorm_ref
            out.update(obs_out=vecnorm_ref.output_bound(ex["obs_out"]), rew_out=vecnorm_ref.output_bound(ex["rew_out"]))
        return out

    def table(self):
        out = []
        for value in VALUES:
            for row, kind in self.ROWS:                # a poisoned observation in the first, a middle and the last chunk, and what it leaves
                for col in (0, self.D - 1):
                    for mode in ("step", "follow", "apply"):
                        out.append(Case(self, dict(mode=mode, done=-1), "obs", (row, col), value, f"{kind}, column {col}, {mode}"))
                for mode, done in (("step", -1), ("step", row), ("follow", -1), ("follow", row), ("apply", -1)):
                    out.append(Case(self, dict(mode=mode, done=done), "rewards", row, value,
                                    f"{kind}, {mode}{', the env done at that step' if done >= 0 else ''}"))
                out.append(Case(self, dict(mode="step", done=-1), "returns", row, value, f"{kind}, step"))
            for name in ("mean", "var"):               # apply (and update) with poisoned statistics
                for col in (0, self.D - 1):
                    for mode in ("apply", "step"):
                        out.append(Case(self, dict(mode=mode, done=-1), name, col, value, f"column {col}, {mode}"))
            for mode in ("apply", "step"):
                out.append(Case(self, dict(mode=mode, done=-1), "ret_var", 0, value, mode))
        for (a, b), kind in (((5, 200), "the same chunk"), ((5, 300), "different chunks"), ((300, 599), "the middle and the last chunk")):
            for first in (np.inf, -np.inf):            # two opposite infinities
                for mode in ("step", "follow"):
                    c = Case(self, dict(mode=mode, done=-1), "obs", (a, 1), ("+inf" if first > 0 else "-inf", first),
                             f"opposite infinities in {kind}, {mode}")
                    c.also = [("obs", (b, 1), -first)]
                    out.append(c)
        return out

    def owed(self):
        """Listed by hand, not from table(): the scenarios that the entry owes."""
        e, chunks, cols = self.name, [k for _, k in self.ROWS], (0, self.D - 1)
        cells = set()
        for v, _ in VALUES:
            cells |= {(e, "obs", v, f"{k}, column {c}, {m}") for k in chunks for c in cols for m in ("step", "follow", "apply")}
            cells |= {(e, "rewards", v, f"{k}, {m}") for k in chunks for m in ("step", "follow", "apply")}
            cells |= {(e, "rewards", v, f"{k}, {m}, the env done at that step") for k in chunks for m in ("step", "follow")}
            cells |= {(e, "returns", v, f"{k}, step") for k in chunks}
            cells |= {(e, name, v, f"column {c}, {m}") for name in ("mean", "var") for c in cols for m in ("apply", "step")}
            cells |= {(e, "ret_var", v, m) for m in ("apply", "step")}
        for v in ("+inf", "-inf"):
            cells |= {(e, "obs", v, f"opposite infinities in {k}, {m}") for k in ("the same chunk", "different chunks", "the middle and the last chunk")
                      for m in ("step", "follow")}
        return cells


def rsample_underflow_case():
    """The one pinned exception: behind the open clamp a finite log_std = -60 makes sigma^2 = 0 in float32 (exp(-120) lies
    below the smallest denormal, so flushing plays no part).  The float64 composition is finite there; torch's own float32 composition is
    NaN in that row's log_prob and in that element's gradients, and the device is pinned to torch float32's classes, not to float64's.
    -> (entry, cfg, flat, (row, column))"""
    entry = Rsample()
    cfg = dict(clamp=False, B=257)
    flat = entry.flat(cfg)
    flat["log_std"][64, 1] = -60.0
    return entry, cfg, flat, (64, 1)


def check_ppo_large_log_std(device):
    """A finite log_std = 45 (and 50), per row and shared: sigma is finite in float32 and its square is not.  torch's float64 and float32
    compositions both give the finite dlog_std = -coef - ent_coef / B there, and so must the device: every output has float64's class."""
    import torch
    entry = Ppo()
    for per_row, ls in ((True, 45.0), (False, 45.0), (True, 50.0)):
        cfg = dict(per_row=per_row, normalize=True, clip_vf=True, B=70)
        flat = entry.flat(cfg)
        flat["log_std"][(5, 1) if per_row else 1] = ls
        wide, narrow, got = entry.exact(flat, cfg), entry.exact(flat, cfg, dtype=torch.float32), device(entry, flat, cfg)
        assert np.isfinite(wide["dlog_std"]).all() and np.isfinite(narrow["dlog_std"]).all()
        for k in entry.keys:
            assert np.array_equal(value_class(got[k]), value_class(wide[k])), (k, per_row, ls)
        err = np.abs(got["dlog_std"].astype(np.float64) - wide["dlog_std"])[(5, 1) if per_row else 1]
        assert err <= entry.bounds(wide, flat, cfg)["dlog_std"][(5, 1) if per_row else 1], (per_row, ls, err)


def check_rsample_underflow(device):
    """Holds device(entry, flat, cfg) to the pinned classes, and every other row to the clean run's bits."""
    import torch
    entry, cfg, flat, (row, col) = rsample_underflow_case()
    wide, narrow = entry.exact(flat, cfg), entry.exact(flat, cfg, dtype=torch.float32)
    assert np.isfinite(wide["dmean"]).all() and np.isfinite(wide["log_prob"]).all()          # a reverse divergence: float64 is finite
    assert np.isnan(narrow["dmean"][row, col]) and np.isnan(narrow["log_prob"][row])
    got, clean = device(entry, flat, cfg), device(entry, entry.flat(cfg), cfg)
    others = np.arange(cfg["B"]) != row
    for k in entry.keys:
        assert np.array_equal(value_class(got[k]), value_class(narrow[k])), k
        assert _same_bits(got[k][others], clean[k][others]).all(), k


ENTRIES = [SacCritic(1), SacCritic(2), SacCritic(4), SacActor(1), SacActor(2), SacActor(4), Ppo(), Rsample(), ActionHead(), Gae(), VecNorm()]


# ---------------------------------------------------------------------------------------------------------------- the table
class Case:
    def __init__(self, entry, cfg, name, index, value, kind):
        self.entry, self.cfg, self.input, self.index, self.value, self.kind = entry, cfg, name, index, value, kind

    @property
    def cell(self):
        return (self.entry.name, self.label(self.input), self.value[0], self.kind)

    def label(self, name):
        """log_std is two inputs: [A] and [B][A]."""
        return f"log_std {'[B][A]' if self.cfg['per_row'] else '[A]'}" if name == "log_std" and "per_row" in self.cfg else name

    def __str__(self):
        switches = ", ".join(f"{k}={v}" for k, v in self.cfg.items())
        return f"{self.entry.name}: {self.value[0]} in {self.label(self.input)}{[int(i) for i in np.atleast_1d(self.index)]} ({self.kind}; {switches})"

    also = ()                                  # further (input, index, value) poisoned in the same case

    def flat(self):
        out = _poisoned(self.entry.flat(self.cfg), self.input, self.index, self.value[1])
        for name, index, value in self.also:
            out[name][index] = value
        return out


def position_kinds(array_kind):
    """The position kinds that the table owes an input of this kind of array."""
    rows = tuple(k for _, _, k in ROWS)
    return {"rows": rows, "grid": tuple(f"{r}, {c}" for r in rows for c in COLS), "columns": COLS + ("B = 1", "a third chunk"),
            "scalar": ("B = 257", "B = 1", "a third chunk")}[array_kind]


def _positions(array_kind, A):
    """[(B, index, position kind)] for one input."""
    cols = ((0, COLS[0]), (A - 1, COLS[1])) if A else ()
    if array_kind == "rows":
        return [(B, r, k) for B, r, k in ROWS]
    if array_kind == "grid":
        return [(B, (r, c), f"{k}, {ck}") for B, r, k in ROWS for c, ck in cols]
    if array_kind == "columns":
        return [(257, c, ck) for c, ck in cols] + [(1, 0, "B = 1"), (513, A - 1, "a third chunk")]
    return [(257, 0, "B = 257"), (1, 0, "B = 1"), (513, 0, "a third chunk")]


def keys_of(entry, cfg):
    """The outputs of one configuration of an entry."""
    return entry.keys_for(cfg) if entry.keys is None else entry.keys


def cases(entry):
    """Every case of one entry: each input, each value, each position; all the entry's switches at ROWS[CROSS] (for an input that is no array
    of rows, at B = 257), one of them in rotation everywhere else.  An entry whose positions are its own (Gae) lists them in table()."""
    if hasattr(entry, "table"):
        return [c for c in entry.table() if c.cell not in LEFT_OUT]
    out, turn = [], 0
    names = {}
    for c in entry.configs:
        for name, kind in entry.inputs(dict(c, B=1)):
            names.setdefault((name, kind), []).append(c)
    for (name, kind), configs in names.items():
        for value in VALUES:
            for B, index, pk in _positions(kind, getattr(entry, "A", 0)):
                cross = B == 257 and (kind in ("columns", "scalar") or np.atleast_1d(index)[0] == ROWS[CROSS][1])
                turn += 1
                for c in (configs if cross else [configs[turn % len(configs)]]):
                    case = Case(entry, dict(c, B=B), name, index, value, pk)
                    if case.cell not in LEFT_OUT:
                        out.append(case)
    return out


def owed_cells(entry):
    """Every (entry, input, value, position kind) cell that cases(entry) or LEFT_OUT must hold."""
    if hasattr(entry, "owed"):
        return entry.owed()
    cells = set()
    for c in entry.configs:
        for name, kind in entry.inputs(dict(c, B=1)):
            label = Case(entry, c, name, 0, VALUES[0], "").label(name) if "per_row" in c else name
            cells |= {(entry.name, label, v, pk) for v, _ in VALUES for pk in position_kinds(kind)}
    return cells


class Runner:
    """Runs cases against `device(entry, flat, cfg) -> name -> float32 array` (the entry's keys), keeping each configuration's clean runs."""

    def __init__(self, device):
        self.device, self.clean = device, {}
        self.tally = dict(cases=0, elements=0, untouched=0, bounded=0, unbounded=0, ratio=0.0)

    def _clean(self, entry, cfg):
        key = (entry.name, tuple(sorted(cfg.items())))
        if key not in self.clean:
            flat = entry.flat(cfg)
            self.clean[key] = (entry.exact(flat, cfg), self.device(entry, flat, cfg))
        return self.clean[key]

    def run(self, case):
        entry, cfg = case.entry, case.cfg
        want_clean, got_clean = self._clean(entry, cfg)
        flat = case.flat()
        want = entry.exact(flat, cfg)
        got = self.device(entry, flat, cfg)
        t = check(got, {k: want[k] for k in keys_of(entry, cfg)}, entry.bounds(want, flat, cfg), got_clean, want_clean, str(case))
        self.tally["cases"] += 1
        for k in ("elements", "untouched", "bounded", "unbounded"):
            self.tally[k] += t[k]
        self.tally["ratio"] = max(self.tally["ratio"], t["ratio"])
        return got

    def failures(self, table):
        """[(case, the first line of its failure)] over a list of cases: for the restatements that are expected to fail."""
        out = []
        for case in table:
            try:
                self.run(case)
            except AssertionError as e:
                out.append((case, str(e)))
        return out
