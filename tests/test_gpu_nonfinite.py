"""The table of non-finite inputs (tests/nonfinite_cases.py) on the device: every case through tg_sac_critic_loss, tg_sac_actor_loss,
tg_ppo_loss (both paths) and tg_squashed_rsample with its backward, on raw pointers between guard bytes, held to check()'s three rules against
the float64 torch composition and, bit for bit with NaN equal to NaN, to the *_device_order restatement - the step that ties what
tests/test_nonfinite_cpu.py shows to the kernels.  Then one poisoned row through each autograd entry: the loss and that row's .grad have the
reference's classes, every other row's .grad the clean run's bits."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_head_ref as ppo_ref  # noqa: E402
import nonfinite_cases as nc  # noqa: E402
import sac_loss_ref as sac_ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from action_head_device import _call as _head_call  # noqa: E402
from device_guard import Guarded  # noqa: E402
from rollout_device import _gae  # noqa: E402
from vecnorm_device import Device  # noqa: E402
from loss_device import GAMMA, GRID, ONE, _actor, _critic, _ppo, _rsample, _rsample_bwd, _upload  # noqa: E402

f32 = np.float32
assert GAMMA == nc.GAMMA


def _same(a, b):
    """Bit for bit, NaN equal to NaN."""
    a, b = np.atleast_1d(np.ascontiguousarray(a)), np.atleast_1d(np.ascontiguousarray(b))
    assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64) and a.shape == b.shape
    return bool((nc._same_bits(a, b) | (np.isnan(a) & np.isnan(b))).all())


def _vecnorm(entry, flat, cfg):
    """The scenario of nonfinite_cases.VecNorm on a guarded device normaliser that starts from the given statistics and returns."""
    N, D = entry.N, entry.D
    dev = Device((D,), N)
    dev.stats = [Guarded((2 * D + 1) * 8, fill=np.concatenate([flat["mean"], flat["var"], [100.0]]))]
    dev.ret_stats = Guarded(24, fill=np.array([0.2, flat["ret_var"][0], 100.0]))
    dev.returns = Guarded(N * 8, fill=flat["returns"])
    train = cfg["mode"] != "apply"
    steps = [(flat["obs"], flat["rewards"], flat["dones"])] + ([entry.second() + (np.zeros(N, np.uint8),)] if cfg["mode"] == "follow" else [])
    for obs, rew, dones in steps:
        if train:
            dev.update([obs], rew)
        outs, rew_out = dev.apply([obs], N, rewards=rew, dones=dones if train else None, reset=train)
    for g in dev.stats + [dev.ret_stats, dev.returns, dev.scratch]:
        assert g.guards_intact()
    st, rs = dev.stats[0].host(np.float64), dev.ret_stats.host(np.float64)
    f = lambda x: np.ascontiguousarray(x, np.float64)   # noqa: E731
    return dict(obs_out=outs[0], rew_out=rew_out, mean=f(st[:D]), var=f(st[D:2 * D]), count=f(st[2 * D]), ret_mean=f(rs[0]), ret_var=f(rs[1]),
                ret_count=f(rs[2]), returns=f(dev.returns.host(np.float64)))


def _device(entry, flat, cfg):
    """One case's call(s) through the C entry -> the entry's named float32 outputs (rsample: and, as saved_*, what the forward saved for its
    backward); the harness functions assert the guards and, where they always did, that the inputs are unchanged."""
    if entry.kind == "gae":
        adv, ret = _gae(flat["rewards"], flat["values"], flat["episode_starts"], flat["last_values"], flat["dones"], entry.GAMMA, entry.LAMBDA,
                        entry.T, entry.N)
        return dict(advantages=adv, returns=ret)
    if entry.kind == "vecnorm":
        return _vecnorm(entry, flat, cfg)
    if entry.kind == "action_head":
        keys = entry.keys_for(cfg)
        return _head_call(cfg["mode"], cfg["B"], entry.A, flat.get("mean"), flat.get("log_std"), entry.lo, entry.hi, entry.clamp(cfg),
                          cfg["deterministic"], noise_in=flat.get("noise_in"), outputs=keys, stride=entry.A)
    if entry.kind == "ppo":
        inp, kw = dict(flat, old_values=flat.get("old_values")), entry.kw(cfg)
        dev = _upload(inp)
        one, grid = _ppo(inp, dev, kw, path=ONE), _ppo(inp, dev, kw, path=GRID)
        assert all(_same(one[k], grid[k]) for k in one), "TG_LOSS_PATH_ONE and TG_LOSS_PATH_GRID differ"
        return entry.named(one)
    if entry.kind == "rsample":
        clamp = entry.clamp(cfg)
        fwd = _rsample(flat["mean"], flat["log_std"], noise_in=flat["noise_in"], clamp=clamp)
        bwd = _rsample_bwd(fwd, flat["log_std"], flat["g_actions"], flat["g_log_prob"], clamp=clamp)
        return dict(actions=fwd["actions"], log_prob=fwd["log_prob"], dmean=bwd["dmean"], dlog_std=bwd["dlog_std"], saved_eps=fwd["eps"],
                    saved_sigma=fwd["sigma"])
    inp, src = entry.split(flat)
    if entry.kind == "sac_critic":
        got = _critic(inp, src)
        return entry.named(dict(stats=got["stats"], target=got["target"], dq_cur=np.stack([got[f"dq_cur{i}"] for i in range(entry.n)])))
    got = _actor(inp, src, entry.te(cfg))
    return entry.named(dict(stats=got["stats"], dlog_prob=got["dlog_prob"], dq_pi=np.stack([got[f"dq_pi{i}"] for i in range(entry.n)])))


@pytest.mark.parametrize("value", [v for v, _ in nc.VALUES])
@pytest.mark.parametrize("entry", nc.ENTRIES, ids=[e.name for e in nc.ENTRIES])
def test_every_case_through_the_c_entry(entry, value):
    run = nc.Runner(_device)
    table = [c for c in nc.cases(entry) if c.value[0] == value]
    assert table
    for case in table:
        got = run.run(case)
        flat = case.flat()
        keys = nc.keys_of(entry, case.cfg)
        if entry.kind == "rsample":
            # tanh, log and exp come from two double libraries that may round one float32 neighbour apart (tests/action_head_ref.py): the
            # forward's bits are not the restatement's to compare.  What it saved is (the noise, NaN at a mean that is not finite), and the
            # backward, which has no such function, is the restatement's bit for bit from the kernel's own saved tensors.
            assert _same(got["saved_eps"], ppo_ref.rsample_saved_eps(flat["mean"], flat["noise_in"])), str(case)
            dmean, dls = ppo_ref.rsample_bwd_device_order(flat["g_actions"], flat["g_log_prob"], got["actions"], got["saved_eps"],
                                                          got["saved_sigma"], flat["log_std"], *entry.clamp(case.cfg))
            want, keys = dict(dmean=dmean, dlog_std=dls), ("dmean", "dlog_std")
        else:
            want = entry.restate(flat, case.cfg)
        if entry.kind == "action_head":            # likewise: bit for bit what no transcendental function lies on the path to
            mode, det = case.cfg["mode"], case.cfg["deterministic"]
            keys = keys if mode == 2 else ("noise", "gaussian", "actions", "env") if (det and mode == 0) else ("noise", "gaussian") if det else ("noise",)
        differ = [k for k in keys if not _same(got[k], want[k])]
        assert not differ, f"{case}: the kernel and its restatement differ in {differ}"
    assert run.tally["cases"] == len(table)
    assert run.tally["unbounded"] <= nc.UNBOUNDED.get(entry.name, 0), run.tally          # this value's share of the entry's limit
    print(f"{entry.name}, {value}: {run.tally}")


def test_ppos_dlog_std_stays_finite_where_only_the_float32_square_of_sigma_overflows():
    nc.check_ppo_large_log_std(_device)


def test_rsamples_float32_underflow_is_pinned_to_torch_float32():
    nc.check_rsample_underflow(_device)


# ---------------------------------------------------------------------------------------------------------------- the autograd entries
B, ROW = 257, 64


def _t(x, grad=False):
    return torch.tensor(np.asarray(x, f32), device="cuda").requires_grad_(grad)


def _rows(grads, want, clean, row, what):
    """grads, clean: name -> float32 [B, ...] of the poisoned and the clean run; want: the reference's poisoned gradients."""
    others = np.arange(B) != row
    for k, g in grads.items():
        assert np.array_equal(nc.value_class(g[row]), nc.value_class(np.asarray(want[k])[row])), (what, k, g[row], np.asarray(want[k])[row])
        assert _same(g[others], clean[k][others]), (what, k)


def _class(x):
    return int(nc.value_class(x.detach().cpu().numpy()))


def test_sac_critic_loss_autograd_with_a_poisoned_row():
    import tactile_gym_amd as tg
    inp = sac_ref.sac_critic_inputs(B, 2, seed=5)

    def run(inp):
        q_cur = [_t(q, True) for q in inp["q_cur"]]
        loss, _ = tg.sac_critic_loss(q_cur, [_t(q) for q in inp["q_next"]], _t(inp["next_log_prob"]), _t(inp["rewards"]), _t(inp["dones"]), GAMMA,
                                     ent_coef=0.2)
        loss.backward()
        return loss, {f"dq_cur{i}": q.grad.cpu().numpy() for i, q in enumerate(q_cur)}

    _, clean = run(inp)
    assert all(np.isfinite(g).all() for g in clean.values())
    bad = dict(inp, q_next=[inp["q_next"][0], inp["q_next"][1].copy()])
    bad["q_next"][1][ROW] = np.nan
    loss, grads = run(bad)
    ex = sac_ref.sac_critic_exact(**bad, gamma=GAMMA, ent_coef=0.2)
    assert _class(loss) == nc.NAN == int(nc.value_class(ex["critic_loss"]))
    _rows(grads, {f"dq_cur{i}": ex["dq_cur"][i] for i in range(2)}, clean, ROW, "sac_critic_loss")
    assert all(np.isnan(g[ROW]) for g in grads.values())


def test_sac_actor_loss_autograd_with_a_poisoned_row():
    import tactile_gym_amd as tg
    inp = sac_ref.sac_actor_inputs(B, 4, seed=6)

    def run(inp):
        lp, q_pi = _t(inp["log_prob"], True), [_t(q, True) for q in inp["q_pi"]]
        lec = _t([-0.75], True)
        actor_loss, ent_loss, _ = tg.sac_actor_loss(lp, q_pi, log_ent_coef=lec, target_entropy=nc.TARGET_ENTROPY)
        (actor_loss + ent_loss).backward()
        grads = {f"dq_pi{i}": q.grad.cpu().numpy() for i, q in enumerate(q_pi)}
        return actor_loss, ent_loss, dict(grads, dlog_prob=lp.grad.cpu().numpy())

    _, _, clean = run(inp)
    bad = dict(inp, q_pi=[q.copy() for q in inp["q_pi"]])
    bad["q_pi"][2][ROW] = bad["q_pi"][3][ROW] = np.nan                        # two NaNs: the lower index takes the gradient
    actor_loss, ent_loss, grads = run(bad)
    ex = sac_ref.sac_actor_exact(**bad, log_ent_coef=-0.75, target_entropy=nc.TARGET_ENTROPY)
    assert _class(actor_loss) == nc.NAN == int(nc.value_class(ex["actor_loss"]))
    assert _class(ent_loss) == nc.FINITE == int(nc.value_class(ex["ent_coef_loss"]))
    _rows(grads, dict({f"dq_pi{i}": ex["dq_pi"][i] for i in range(4)}, dlog_prob=ex["dlog_prob"]), clean, ROW, "sac_actor_loss")
    assert [float(grads[f"dq_pi{i}"][ROW]) for i in range(4)] == [0.0, 0.0, float(f32(-1.0) / f32(B)), 0.0]


def test_ppo_loss_autograd_with_a_poisoned_row():
    import tactile_gym_amd as tg
    inp = ppo_ref.ppo_inputs(B, 3, True, seed=7, clip_range=nc.CLIP, clip_range_vf=nc.CLIP_VF)
    kw = dict(clip_range=nc.CLIP, clip_range_vf=nc.CLIP_VF, ent_coef=nc.ENT, vf_coef=nc.VF, normalize_advantage=False)

    def run(inp):
        mean, log_std, values = _t(inp["mean"], True), _t(inp["log_std"], True), _t(inp["values"], True)
        loss, _ = tg.ppo_loss(mean, log_std, values, *[_t(inp[k]) for k in ("actions", "old_log_prob", "advantages", "returns", "old_values")], **kw)
        loss.backward()
        return loss, dict(dmean=mean.grad.cpu().numpy(), dlog_std=log_std.grad.cpu().numpy(), dvalues=values.grad.cpu().numpy())

    _, clean = run(inp)
    bad = dict(inp, old_log_prob=inp["old_log_prob"].copy())
    bad["old_log_prob"][ROW] = np.nan
    loss, grads = run(bad)
    ex = ppo_ref.ppo_exact(**bad, **kw)
    assert _class(loss) == nc.NAN == int(nc.value_class(ex["loss"]))
    _rows(grads, ex, clean, ROW, "ppo_loss")
    assert np.isnan(grads["dmean"][ROW]).all() and np.isnan(grads["dlog_std"][ROW]).all() and np.isfinite(grads["dvalues"][ROW])


def test_squashed_rsample_autograd_with_a_poisoned_row():
    from tactile_gym_amd.loss_head import squashed_rsample
    inp = ppo_ref.rsample_inputs(B, 3, seed=8)

    def run(inp):
        mean, log_std = _t(inp["mean"], True), _t(inp["log_std"], True)
        actions, log_prob = squashed_rsample(mean, log_std, noise=_t(inp["eps"]))
        ((_t(inp["g_a"]) * actions).sum() + (_t(inp["g_lp"]) * log_prob).sum()).backward()
        return actions, log_prob, dict(dmean=mean.grad.cpu().numpy(), dlog_std=log_std.grad.cpu().numpy())

    _, _, clean = run(inp)
    bad = dict(inp, mean=inp["mean"].copy())
    bad["mean"][ROW, 1] = np.nan
    actions, log_prob, grads = run(bad)
    ex = ppo_ref.rsample_exact(bad["mean"], bad["log_std"], bad["eps"], bad["g_a"], bad["g_lp"])
    assert np.array_equal(nc.value_class(actions.detach().cpu().numpy()), nc.value_class(ex["actions"]))
    assert np.array_equal(nc.value_class(log_prob.detach().cpu().numpy()), nc.value_class(ex["log_prob"]))
    _rows(grads, ex, clean, ROW, "squashed_rsample")
    fwd = _rsample(bad["mean"], bad["log_std"], noise_in=bad["eps"])         # and the C entry on the same row, between guards
    assert _same(fwd["actions"], actions.detach().cpu().numpy()) and _same(fwd["log_prob"], log_prob.detach().cpu().numpy())
