"""tg.mlp_towers, tg.ActorCriticHeads, tg.SacActorHeads and tg.ContinuousCriticHeads on the device.

Autograd: the outputs lie within the propagated bound of the float64 restatement (tests/mlp_ref.py), and every gradient within the backward
bounds of the restatement evaluated at the device's own saved activations - which are read back by running each tower's prefixes, the same bits
by the kernel's row-only rule.  tests/test_mlp_cpu.py holds the other half: the restatement equals torch's float64 autograd on the same weights
to 1e-12.  Then: nothing is kept under no_grad or with everything frozen, the device against the CPU path, PPO's first-epoch ratio behind
collect_rollouts, and one SAC gradient step."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mlp_cases as mc  # noqa: E402
import mlp_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402

MODES = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
             arm_type="ur5", tactile_sensor_name="tactip")
f32 = np.float32


def _host(t):
    return t.detach().cpu().numpy()


def _cuda(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def _within(got, want, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: largest error / bound = {ratio:.3g}")
    assert (err <= bound).all(), (what, ratio)


def _tensors(tower, grad=True):
    """mlp_towers' layer tuples over fresh device leaves of a restatement tower."""
    out = []
    for ly in tower:
        item = [_cuda(ly["w"], grad), _cuda(ly["b"], grad), ly["act"]]
        if ly["w2"] is not None:
            item += [_cuda(ly["w2"], grad), _cuda(ly["b2"], grad)]
        out.append(tuple(item))
    return out


def _joined(y):
    return torch.cat(y, dim=1) if isinstance(y, tuple) else y


def _device_hs(blocks, layers):
    """The device's own h_l of one tower, float32 [B, out + out2] each: the tower's prefixes, run alone under no_grad."""
    import tactile_gym_amd as tg
    hs = []
    with torch.no_grad():
        for l in range(len(layers)):
            prefix = [tuple(t.detach() if isinstance(t, torch.Tensor) else t for t in layer) for layer in layers[:l + 1]]
            hs.append(_host(_joined(tg.mlp_towers(blocks, [prefix])[0])))
    return hs


def _check_gradients(x, towers, hs, dys, layer_grads, dx, what):
    """layer_grads[t][l] = (dweight, dbias) over both row blocks, dx [B, K0] (or None): within the restatement's bounds at the given h."""
    dh0s, e0s = [], []
    for t, tower in enumerate(towers):
        grads, bounds, dh0, e0 = ref.tower_backward(x, tower, hs[t], dys[t])
        dh0s.append(dh0)
        e0s.append(e0)
        for l in range(len(tower)):
            _within(layer_grads[t][l][0], grads[l][0], bounds[l][0], f"{what}: tower {t} layer {l} dweight")
            _within(layer_grads[t][l][1], grads[l][1], bounds[l][1], f"{what}: tower {t} layer {l} dbias")
            assert float(np.abs(grads[l][0]).max()) > 0
    if dx is not None:
        total, bound = ref.sum_dx(dh0s, e0s)
        _within(dx, total, bound, f"{what}: dx")


def _grads_of(layers):
    out = []
    for layer in layers:
        w, b = layer[0].grad, layer[1].grad
        if len(layer) == 5:
            w, b = torch.cat([w, layer[3].grad]), torch.cat([b, layer[4].grad])
        out.append((_host(w), _host(b)))
    return out


CASES = [
    (64, 258, 256, [([256, 256, 1], ["relu", "relu", "none"], 0), ([256, 256, 1], ["relu", "relu", "none"], 0)]),      # SAC's critic
    (65, 33, 33, [([64, 33, 2], ["tanh", "tanh", "none"], 0), ([33, 2], ["relu", "tanh"], 2)]),
    (3, 5, 5, [([7], ["tanh"], 0)]),
    # four towers of mixed depth, all three activations, widths 130 and 255, a 100 + 100 last layer, x cut inside a k tile (tests/mlp_cases.py)
    (65, 40, 33, [(w, mc.random_acts(a, t), two) for t, (w, a, two) in enumerate(mc.TABLE["four-mixed"][3])]),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"b{c[0]}-k{c[1]}-t{len(c[3])}")
def test_mlp_towers_autograd_against_the_float64_restatement(case):
    import tactile_gym_amd as tg
    B, K0, Ka, spec = case
    rng = np.random.default_rng(B + K0)
    x = ref.split_input(ref.random_input(rng, B, K0), Ka)
    towers = [ref.random_tower(rng, K0, w, a, two) for w, a, two in spec]
    blocks = [_cuda(b, True) for b in x if b is not None]
    xin = blocks[0] if len(blocks) == 1 else tuple(blocks)
    layers = [_tensors(tower) for tower in towers]
    outs = tg.mlp_towers(xin, layers)
    assert len(outs) == len(towers)
    dys, loss = [], 0.0
    for t, (y, tower) in enumerate(zip(outs, towers)):
        y = _joined(y)
        want, bound = ref.tower_forward(x, tower)[-1]
        assert y.dtype == torch.float32 and y.requires_grad and tuple(y.shape) == want.shape
        _within(_host(y), want, bound, f"tower {t} output")
        dys.append(rng.standard_normal(want.shape).astype(f32))
        loss = loss + (y * _cuda(dys[-1])).sum()
    loss.backward()
    hs = [_device_hs(xin, ls) for ls in layers]
    dx = np.concatenate([_host(b.grad) for b in blocks], axis=1)
    _check_gradients(x, towers, hs, dys, [_grads_of(ls) for ls in layers], dx, "mlp_towers")
    # only what asks gets a gradient: the first tower's first weight and the last block of x
    blocks2 = [_cuda(b, i == len(blocks) - 1) for i, b in enumerate(b for b in x if b is not None)]
    layers2 = [_tensors(tower, grad=False) for tower in towers]
    layers2[0][0][0].requires_grad_()
    outs2 = tg.mlp_towers(blocks2[0] if len(blocks2) == 1 else tuple(blocks2), layers2)
    sum((_joined(y) * _cuda(d)).sum() for y, d in zip(outs2, dys)).backward()
    assert torch.equal(layers2[0][0][0].grad, layers[0][0][0].grad) and torch.equal(blocks2[-1].grad, blocks[-1].grad)   # and the same bits
    assert layers2[0][0][1].grad is None and (len(blocks2) == 1 or blocks2[0].grad is None)
    assert all(torch.equal(_joined(a), _joined(b)) for a, b in zip(outs, outs2))


def test_nothing_is_kept_under_no_grad_or_with_everything_frozen(monkeypatch):
    """What the launch is asked to write, observed where it is decided: tactile_gym_amd.mlp._run_forward's save_all and the h buffers it
    hands to tg_mlp_forward.  Trainable parameters under no_grad - PPO's collection step - and frozen parameters with gradients enabled both
    write each tower's last layer only and keep nothing; trainable parameters with gradients enabled write every layer."""
    import tactile_gym_amd as tg
    from tactile_gym_amd import mlp
    seen = []
    inner = mlp._run_forward

    def recording(x0, x1, acts, params, save_all):
        hs = inner(x0, x1, acts, params, save_all)
        seen.append((bool(save_all), [[h is not None for h, _ in row] for row in hs]))
        return hs
    monkeypatch.setattr(mlp, "_run_forward", recording)
    rng = np.random.default_rng(1)
    tower = ref.random_tower(rng, 9, [12, 7, 3], ["tanh", "relu", "none"], 2)
    x = _cuda(ref.random_input(rng, 5, 9))
    last_only = (False, [[False, False, True]])
    trainable = _tensors(tower)
    assert all(t.requires_grad for layer in trainable for t in layer if isinstance(t, torch.Tensor))
    with torch.no_grad():
        y, y2 = tg.mlp_towers(x, [trainable])[0]
    assert seen[-1] == last_only                                             # trainable parameters, no_grad: only the last layer is written
    assert y.grad_fn is None and not y.requires_grad and y2.grad_fn is None
    z, z2 = tg.mlp_towers(x, [_tensors(tower, grad=False)])[0]
    assert seen[-1] == last_only                                             # everything frozen, gradients enabled
    assert z.grad_fn is None and not z.requires_grad and torch.equal(z, y) and torch.equal(z2, y2)
    w, w2 = tg.mlp_towers(x, [trainable])[0]
    assert seen[-1] == (True, [[True, True, True]]) and w.grad_fn is not None    # a graph is built: every layer is written and kept
    assert torch.equal(w, y) and torch.equal(w2, y2)                         # the same bits either way
    empty = tg.mlp_towers(torch.zeros(0, 9, device="cuda"), [_tensors(tower)])[0]
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 2)
    with pytest.raises(ValueError, match="x's device"):
        tg.mlp_towers(x, [_tensors(tower)[:1] + [(torch.zeros(7, 12), torch.zeros(7), None)]])
    # the three modules with their trainable parameters under no_grad, as collect_rollouts and collect_transitions call them
    heads = tg.ActorCriticHeads(9, 2, dict(pi=[8, 8], vf=[8])).cuda()
    with torch.no_grad():
        mean, log_std, values = heads(x)
    assert seen[-1] == (False, [[False, False, True], [False, True]])
    assert mean.grad_fn is None and values.grad_fn is None and mean.shape == (5, 2) and values.shape == (5,) and log_std.shape == (2,)
    actor, critic = tg.SacActorHeads(9, 2, [8]).cuda(), tg.ContinuousCriticHeads(9, 2, [8]).cuda()
    with torch.no_grad():
        actor(x)
        assert seen[-1] == (False, [[False, True]])
        critic(x, _cuda(np.zeros((5, 2), f32)))
        assert seen[-1] == (False, [[False, True], [False, True]])
    heads(x)
    assert seen[-1] == (True, [[True, True, True], [True, True]])
    # a double backward is refused, not silently wrong
    xg = _cuda(ref.random_input(rng, 5, 9), True)
    out = tg.mlp_towers(xg, [trainable])[0][0]
    v = torch.ones_like(out).requires_grad_()                                # a gradient that itself asks for one: the second derivative's way in
    (gx,) = torch.autograd.grad(out, xg, grad_outputs=v, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


def _module_towers(module):
    """(restatement towers, the matching nn.Linear groups per tower and layer) of one of the three modules."""
    import tactile_gym_amd as tg

    def lin(seq):
        return [m for m in seq if isinstance(m, nn.Linear)]
    if isinstance(module, tg.ActorCriticHeads):
        groups = [[(m,) for m in lin(module.mlp_extractor.policy_net)] + [(module.action_net,)],
                  [(m,) for m in lin(module.mlp_extractor.value_net)] + [(module.value_net,)]]
    elif isinstance(module, tg.SacActorHeads):
        groups = [[(m,) for m in lin(module.latent_pi)] + [(module.mu, module.log_std)]]
    else:
        groups = [[(m,) for m in lin(getattr(module, f"qf{i}"))] for i in range(module.n_critics)]
    towers = []
    for group in groups:
        tower = []
        for l, ms in enumerate(group):
            ly = ref.layer(_host(ms[0].weight), _host(ms[0].bias), module.act if l < len(group) - 1 else "none")
            if len(ms) == 2:
                ly["w2"], ly["b2"] = _host(ms[1].weight), _host(ms[1].bias)
            tower.append(ly)
        towers.append(tower)
    return towers, groups


@pytest.mark.parametrize("kind", ["actor_critic", "sac_actor", "critic"])
def test_modules_autograd_and_the_cpu_path(kind):
    import tactile_gym_amd as tg
    torch.manual_seed(5)
    rng = np.random.default_rng(6)
    B, fd, A = 64, 40, 2
    feats, actions = rng.standard_normal((B, fd)).astype(f32), rng.uniform(-1, 1, (B, A)).astype(f32)
    if kind == "actor_critic":
        module, x = tg.ActorCriticHeads(fd, A, dict(pi=[64, 33], vf=[64]), activation_fn=nn.Tanh, ortho_init=False), (feats, None)
    elif kind == "sac_actor":
        module, x = tg.SacActorHeads(fd, A, [64, 33]), (feats, None)
    else:
        module, x = tg.ContinuousCriticHeads(fd, A, [64, 33]), (feats, actions)
    module = module.cuda()
    towers, groups = _module_towers(module)
    blocks = [_cuda(b, True) for b in x if b is not None]
    out = module(*blocks)
    if kind == "actor_critic":
        assert out[1] is module.log_std and out[2].shape == (B,)
        ys = [out[0], out[2].reshape(B, 1)]
    elif kind == "sac_actor":
        assert out[0].shape == (B, A) and out[1].shape == (B, A)
        ys = [torch.cat(out, dim=1)]
    else:
        assert isinstance(out, tuple) and all(q.shape == (B, 1) for q in out)
        ys = list(out)
    dys = []
    for t, (y, tower) in enumerate(zip(ys, towers)):
        want, bound = ref.tower_forward(x, tower)[-1]
        _within(_host(y), want, bound, f"{kind}: tower {t} output")
        dys.append(rng.standard_normal(want.shape).astype(f32))
    sum((y * _cuda(d)).sum() for y, d in zip(ys, dys)).backward()
    xin = blocks[0] if len(blocks) == 1 else tuple(blocks)
    hs = [_device_hs(xin, _tensors(tower, grad=False)) for tower in towers]
    grads = [[(_host(torch.cat([m.weight.grad for m in ms])), _host(torch.cat([m.bias.grad for m in ms]))) for ms in group] for group in groups]
    _check_gradients(x, towers, hs, dys, grads, np.concatenate([_host(b.grad) for b in blocks], axis=1), kind)
    # the CPU path of a copy.  ReLU modules: both sides are float32 sums of the same terms in some order and lie within the same propagated
    # bound of the exact value.  Tanh: torch's float32 tanh is not correctly rounded; 2 ulp per Tanh layer (its documented accuracy is
    # within that) pass the later layers like any other error - covered by doubling the bound's Tanh term, that is by one more bound.
    host = copy.deepcopy(module).cpu()
    with torch.no_grad():
        out_host = host(*[torch.from_numpy(b) for b in x if b is not None])
    ys_host = [out_host[0], out_host[2].reshape(B, 1)] if kind == "actor_critic" else [torch.cat(out_host, dim=1)] if kind == "sac_actor" else list(out_host)
    for t, (y, yh, tower) in enumerate(zip(ys, ys_host, towers)):
        bound = ref.tower_forward(x, tower)[-1][1]
        assert (np.abs(_host(y).astype(np.float64) - yh.numpy()) <= (3 if module.act == "tanh" else 2) * bound).all(), (kind, t)


class _Space:
    def __init__(self, shape):
        self.shape, self.dtype = tuple(shape), np.uint8


def test_a_nan_feature_row_is_nan_on_the_device_as_on_the_cpu():
    """ReLU hands a NaN on (torch.relu's rule, which the CPU paths follow): a diverged policy shows on the device as it does on the host."""
    import tactile_gym_amd as tg
    torch.manual_seed(8)
    rng = np.random.default_rng(9)
    B, fd, A, bad = 5, 20, 2, 3
    feats, actions = rng.standard_normal((B, fd)).astype(f32), rng.uniform(-1, 1, (B, A)).astype(f32)
    feats[bad, 7] = np.nan
    image = rng.integers(0, 256, (B, 1, 64, 64)).astype(f32)
    image[bad, 0, 20, 21] = np.nan
    trials = [(tg.ActorCriticHeads(fd, A, dict(pi=[64, 33], vf=[64]), activation_fn=nn.ReLU), (feats,)),
              (tg.SacActorHeads(fd, A, [64, 33]), (feats,)),
              (tg.ContinuousCriticHeads(fd, A, [64, 33]), (feats, actions)),
              (tg.NatureCNN(_Space((1, 64, 64)), features_dim=16, float_scale=1.0 / 255.0), (image,))]
    for module, args in trials:
        host, dev = module, copy.deepcopy(module).cuda()
        with torch.no_grad():
            out_host, out_dev = host(*[torch.from_numpy(a) for a in args]), dev(*[_cuda(a) for a in args])
        out_host, out_dev = ([o.reshape(B, -1) for o in (out if isinstance(out, tuple) else (out,)) if o.shape[0] == B] for out in (out_host, out_dev))
        name = type(module).__name__
        assert len(out_host) == len(out_dev) >= 1
        for h, d in zip(out_host, out_dev):
            assert np.array_equal(np.isnan(_host(d)), np.isnan(h.numpy())), name
            assert np.isnan(_host(d)[bad]).all() and not np.isnan(np.delete(_host(d), bad, axis=0)).any(), name


class CachingPolicy:
    """policy(obs) -> heads(features).  Under no_grad (collection) the features come from the extractor and are kept with their image; with
    gradients (training) each row's features are the kept ones of its image, fed unchanged: what reaches the heads differs from the
    collection pass only in the batch around the row."""

    def __init__(self, extractor, heads):
        self.extractor, self.heads, self.keys, self.feats = extractor, heads, [], []

    def __call__(self, obs):
        x = obs["tactile"]
        flat = x.reshape(x.shape[0], -1).float()
        if not torch.is_grad_enabled():
            f = self.extractor(x)
            self.keys.append(flat.clone())
            self.feats.append(f.clone())
        else:
            eq = (flat[:, None, :] == torch.cat(self.keys)[None]).all(dim=2)
            assert bool(eq.any(dim=1).all())
            f = torch.cat(self.feats)[eq.float().argmax(dim=1)]
        return self.heads(f)


def test_ppo_first_epoch_ratio_is_one_behind_collect_rollouts():
    import tactile_gym_amd as tg
    from tactile_gym_amd.collect import collect_rollouts
    N, T, MB, SIZE = 8, 4, 4, 128
    venv = tg.make_vec("edge_follow-v0", num_envs=N, max_steps=5, image_size=[SIZE, SIZE], env_modes=MODES, seed=3, obs_mode="torch")
    try:
        torch.manual_seed(1)
        extractor = tg.NatureCNN(venv.observation_space.spaces["tactile"], features_dim=48, float_scale=1.0 / 255.0).cuda()
        heads = tg.ActorCriticHeads(48, 2, dict(pi=[64, 33], vf=[64, 33]), log_std_init=-1.0).cuda()
        with torch.no_grad():                                                 # SB3's action_net gain of 0.01 would leave every mean near 0
            heads.action_net.weight.mul_(50.0)
        policy = CachingPolicy(extractor, heads)
        buf = tg.DeviceRolloutBuffer.for_env(venv, T, gamma=0.95, gae_lambda=0.9)
        head = tg.DeviceDiagGaussian.for_env(venv, seed=7)
        collect_rollouts(venv, policy, buf, head, T, venv.reset(), torch.ones(N, dtype=torch.uint8, device="cuda"))
        kw = dict(clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True)
        n = 0
        for b in buf.get(MB):                                                 # every minibatch of the unchanged policy: the ratio is exactly 1
            mean, log_std, values = policy(b.observations)
            _, stats = tg.ppo_loss(mean, log_std, values, b.actions, b.old_log_prob, b.advantages, b.returns, old_values=b.old_values, **kw)
            assert float(stats[4]) == 0.0 and float(stats[5]) == 0.0, (n, stats)      # approx_kl, clip_fraction
            assert torch.equal(values.detach(), b.old_values.reshape(-1))             # the value head's bits, too
            n += 1
        assert n == N * T // MB and float(mean.detach().abs().max()) > 1e-3
        opt = torch.optim.Adam(heads.parameters(), lr=3e-4)
        before = [p.detach().clone() for p in heads.parameters()]
        stats = tg.train.ppo_train(policy, opt, buf, 1, MB, 0.2, None, 0.0, 0.5, 0.5, None)
        assert bool(torch.isfinite(stats).all()) and all(not torch.equal(a, b) for a, b in zip(before, heads.parameters()))
        assert float(stats[4]) != 0.0                                         # the policy has moved, and the ratio with it
        # the whole policy as INTEGRATION.md writes it: the extractor trains, too
        full = lambda obs: heads(extractor(obs["tactile"]))   # noqa: E731
        opt = torch.optim.Adam(list(extractor.parameters()) + list(heads.parameters()), lr=3e-4)
        before = [p.detach().clone() for p in extractor.parameters()]
        stats = tg.train.ppo_train(full, opt, buf, 1, MB, 0.2, None, 0.0, 0.5, 0.5, None)
        assert bool(torch.isfinite(stats).all()) and all(not torch.equal(a, b) for a, b in zip(before, extractor.parameters()))
    finally:
        venv.close()


class Actor(nn.Module):
    def __init__(self, space):
        import tactile_gym_amd as tg
        super().__init__()
        self.features = tg.NatureCNN(space, features_dim=32, float_scale=1.0 / 255.0)
        self.heads = tg.SacActorHeads(32, 2, [64, 33])

    def forward(self, obs):
        return self.heads(self.features(obs["tactile"]))


class Critic(nn.Module):
    def __init__(self, space):
        import tactile_gym_amd as tg
        super().__init__()
        self.features = tg.NatureCNN(space, features_dim=32, float_scale=1.0 / 255.0)
        self.heads = tg.ContinuousCriticHeads(32, 2, [64, 33])

    def forward(self, obs, actions):
        return self.heads(self.features(obs["tactile"]), actions)


def test_one_sac_train_step_with_the_device_heads():
    import tactile_gym_amd as tg
    from tactile_gym_amd.collect import collect_transitions
    N, SIZE, MB, TAU, LR = 8, 128, 16, 0.005, 3e-4
    venv = tg.make_vec("edge_follow-v0", num_envs=N, max_steps=5, image_size=[SIZE, SIZE], env_modes=MODES, seed=3, obs_mode="torch")
    try:
        torch.manual_seed(4)
        space = venv.observation_space.spaces["tactile"]
        actor, critic = Actor(space).cuda(), Critic(space).cuda()
        critic_target = copy.deepcopy(critic)
        lec = torch.zeros(1, device="cuda", requires_grad=True)
        rb = tg.DeviceReplayBuffer.for_env(venv, 8 * N, seed=5)
        head = tg.DeviceSquashedDiagGaussian.for_env(venv, seed=9)
        obs = venv.reset()
        rb.start(obs)
        obs, steps = collect_transitions(venv, actor, rb, head, 4, 0, 2 * N, obs)       # the warm-up, then the actor's own actions
        assert steps == 4 * N
        opts = [torch.optim.Adam(actor.parameters(), lr=LR), torch.optim.Adam(critic.parameters(), lr=LR), torch.optim.Adam([lec], lr=LR)]
        before = [[p.detach().clone() for p in m.parameters()] for m in (actor, critic, critic_target)]
        cstats, astats, n_updates = tg.train.sac_train(actor, critic, critic_target, opts[0], opts[1], rb, head, 1, MB, 0.95, TAU, log_ent_coef=lec,
                                                       ent_coef_optimizer=opts[2], target_entropy=-2.0)
        assert n_updates == 1 and bool(torch.isfinite(cstats).all()) and bool(torch.isfinite(astats).all())
        for name, module, kept in (("actor", actor.heads, before[0]), ("critic", critic.heads, before[1])):
            now = dict(module.named_parameters())
            old = dict(zip([k for k, _ in (actor if name == "actor" else critic).named_parameters()], kept))
            moved = [k for k in now if not torch.equal(now[k].detach(), old["heads." + k])]
            assert len(moved) == len(now), (name, sorted(set(now) - set(moved)))          # every weight and bias of the heads got a gradient
        assert float(lec.detach()) != 0.0
        # the target moves by tau: target' = (1 - tau) target + tau critic', two float32 launches (tests/test_gpu_sac_loss.py derives the
        # rounding: 2 u (|(1 - tau) target| + |tau critic'|), u = 2^-24; twice that is allowed here)
        moved = False
        for t0, t1, c1 in zip(before[2], critic_target.parameters(), critic.parameters()):
            a, c = (1 - TAU) * t0.double(), TAU * c1.detach().double()
            assert bool(((t1.detach().double() - (a + c)).abs() <= 4 * 2.0 ** -24 * (a.abs() + c.abs())).all())
            moved = moved or not torch.equal(t1.detach(), t0)
        assert moved
    finally:
        venv.close()
