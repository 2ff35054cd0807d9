"""tg.sac_critic_loss, tg.sac_actor_loss, tg.train.polyak_update and tg.train.sac_train on the device: autograd through both entries against
the float64 composition of tests/sac_loss_ref.py on the same tensors, the refusals, the polyak update against its float64 formula, and one
SAC.train gradient step on edge_follow-v0 against SB3's own order written out with torch's ops on deep copies of the networks: what each
network is called on, the critic side at bit-equal inputs within the sum of both sides' bounds, the actor side within that sum plus the
derived distance of the two sides' critics after their Adam step."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sac_loss_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

MODES = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
             arm_type="ur5", tactile_sensor_name="tactip")
GAMMA, TE = 0.95, -2.0
U = ref.U
f32 = np.float32


def _host(t):
    return t.detach().cpu().numpy()


def _cuda(x, grad=False, column=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return (t.reshape(-1, 1) if column else t).requires_grad_(grad)


def _within(got, want, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    assert (err <= bound).all(), (what, float(err.max()), float(np.max(bound)))


# ---------------------------------------------------------------------------------------------------------------- autograd wiring
@pytest.mark.parametrize("B,n", [(64, 2), (257, 3)])
def test_critic_loss_autograd_against_the_float64_composition(B, n):
    import tactile_gym_amd as tg
    inp = ref.sac_critic_inputs(B, n, seed=B)
    lec = torch.tensor(-0.7, device="cuda", requires_grad=True)
    ex = ref.sac_critic_exact(**inp, gamma=GAMMA, log_ent_coef=-0.7)
    bounds = ref.sac_critic_bounds(ex, **inp, gamma=GAMMA, log_ent_coef=-0.7)
    outs = {}
    for column in (False, True):                                              # [B] and SB3's [B, 1]: the same memory
        q_cur = [_cuda(q, True, column) for q in inp["q_cur"]]
        data = [_cuda(inp[k], True, column) for k in ("next_log_prob", "rewards", "dones")]
        q_next = [_cuda(q, True, column) for q in inp["q_next"]]
        loss, stats = tg.sac_critic_loss(q_cur, tuple(q_next), *data, GAMMA, log_ent_coef=lec)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad and stats.shape == (8,) and not stats.requires_grad
        assert float(loss.detach()) == float(stats[0])
        (3.0 * loss).backward()                                               # the gradients scale with the incoming one
        named = ref.critic_named(dict(stats=_host(stats)), n)
        for k in ("critic_loss", "ent_coef", "target_q_mean", "min_next_q_mean", "mse"):
            _within(named[k], ex[k], bounds[k], k)
        for i, q in enumerate(q_cur):
            assert q.grad.shape == q.shape                                    # in the input's own shape
            _within(_host(q.grad).reshape(-1), 3.0 * ex["dq_cur"][i], 3.0 * bounds["dq_cur"][i] + 3.0 * U * np.abs(ex["dq_cur"][i]), ("dq_cur", i))
        assert all(t.grad is None for t in data + q_next) and lec.grad is None    # the data and alpha get no gradient
        outs[column] = (_host(stats), [_host(q.grad).reshape(-1) for q in q_cur])
    assert np.array_equal(outs[False][0], outs[True][0]) and all(np.array_equal(a, b) for a, b in zip(outs[False][1], outs[True][1]))
    # only the inputs that ask get a gradient; a float coefficient
    q_cur = [_cuda(q, i == n - 1) for i, q in enumerate(inp["q_cur"])]
    args = [[_cuda(q) for q in inp["q_next"]]] + [_cuda(inp[k]) for k in ("next_log_prob", "rewards", "dones")]
    loss, stats = tg.sac_critic_loss(q_cur, *args, GAMMA, ent_coef=0.2)
    loss.backward()
    ex2 = ref.sac_critic_exact(**inp, gamma=GAMMA, ent_coef=0.2)
    b2 = ref.sac_critic_bounds(ex2, **inp, gamma=GAMMA, ent_coef=0.2)
    assert all(q.grad is None for q in q_cur[:-1]) and float(stats[1]) == float(f32(0.2))
    _within(_host(q_cur[-1].grad), ex2["dq_cur"][n - 1], b2["dq_cur"][n - 1], "one critic alone")
    _within(float(loss.detach()), ex2["critic_loss"], b2["critic_loss"], "critic_loss")
    for grad_mode in (torch.no_grad, torch.enable_grad):                      # nothing asks: no graph
        with grad_mode():
            loss3, stats3 = tg.sac_critic_loss([q.detach() for q in q_cur], *args, GAMMA, ent_coef=0.2)
        assert not loss3.requires_grad and loss3.grad_fn is None and torch.equal(stats3, stats)
    # a second backward through a retained graph: each hands out fresh products of the gradients the launch wrote, so writing into a
    # returned gradient in place does not reach the next one
    q_cur = [_cuda(q, True) for q in inp["q_cur"]]
    loss, _ = tg.sac_critic_loss(q_cur, *args, GAMMA, ent_coef=0.2)
    loss.backward(retain_graph=True)
    first = [q.grad.clone() for q in q_cur]
    for q in q_cur:
        q.grad.zero_()
    loss.backward()
    assert all(torch.equal(q.grad, g) for q, g in zip(q_cur, first)) and float(first[0].abs().max()) > 0


@pytest.mark.parametrize("B,n", [(64, 2), (300, 4)])
def test_actor_loss_autograd_against_the_float64_composition(B, n):
    import tactile_gym_amd as tg
    inp = ref.sac_actor_inputs(B, n, seed=B + 7)
    ex = ref.sac_actor_exact(**inp, log_ent_coef=-0.7, target_entropy=TE)
    bounds = ref.sac_actor_bounds(ex, **inp, log_ent_coef=-0.7, target_entropy=TE)
    outs = {}
    for column in (False, True):
        lec = torch.full((1,) if column else (), -0.7, device="cuda", requires_grad=True)
        lp, q_pi = _cuda(inp["log_prob"], True, column), [_cuda(q, True, column) for q in inp["q_pi"]]
        actor_loss, ent_loss, stats = tg.sac_actor_loss(lp, q_pi, log_ent_coef=lec, target_entropy=TE)
        assert actor_loss.dim() == 0 and ent_loss.dim() == 0 and actor_loss.requires_grad and ent_loss.requires_grad and not stats.requires_grad
        assert float(actor_loss.detach()) == float(stats[0]) and float(ent_loss.detach()) == float(stats[1])
        (2.0 * actor_loss + 3.0 * ent_loss).backward()                        # each loss's leaves scale with its own incoming gradient
        named = ref.actor_named(dict(stats=_host(stats)))
        for k in ref.ACTOR_STATS[:6]:
            _within(named[k], ex[k], bounds[k], k)
        assert lp.grad.shape == lp.shape and lec.grad.shape == lec.shape and all(q.grad.shape == q.shape for q in q_pi)
        _within(_host(lp.grad).reshape(-1), 2.0 * ex["dlog_prob"], 2.0 * bounds["dlog_prob"] + 2.0 * U * np.abs(ex["dlog_prob"]), "dlog_prob")
        _within(_host(lec.grad).reshape(()), 3.0 * ex["dlog_ent_coef"], 3.0 * bounds["dlog_ent_coef"] + 3.0 * U * abs(ex["dlog_ent_coef"]), "dlog_ent_coef")
        for i, q in enumerate(q_pi):
            _within(_host(q.grad).reshape(-1), 2.0 * ex["dq_pi"][i], 2.0 * bounds["dq_pi"][i] + 2.0 * U * np.abs(ex["dq_pi"][i]), ("dq_pi", i))
        outs[column] = (_host(stats), _host(lp.grad).reshape(-1), [_host(q.grad).reshape(-1) for q in q_pi])
    assert np.array_equal(outs[False][0], outs[True][0]) and np.array_equal(outs[False][1], outs[True][1])
    assert all(np.array_equal(a, b) for a, b in zip(outs[False][2], outs[True][2]))
    # each loss alone reaches only its own leaves
    lec = torch.tensor(-0.7, device="cuda", requires_grad=True)
    lp, q_pi = _cuda(inp["log_prob"], True), [_cuda(q, True) for q in inp["q_pi"]]
    actor_loss, ent_loss, _ = tg.sac_actor_loss(lp, q_pi, log_ent_coef=lec, target_entropy=TE)
    ent_loss.backward(retain_graph=True)
    assert lp.grad is None and all(q.grad is None for q in q_pi)
    _within(_host(lec.grad), ex["dlog_ent_coef"], bounds["dlog_ent_coef"], "ent_coef_loss alone")
    first = lec.grad.clone()
    lec.grad.zero_()                                                          # in place, into what the first backward returned
    ent_loss.backward(retain_graph=True)
    assert torch.equal(lec.grad, first)                                       # the view into the stats that the Function keeps is untouched
    lec.grad = None
    actor_loss.backward()
    assert lec.grad is None and lp.grad is not None
    # no target_entropy: no entropy-coefficient loss, and alpha stays data; only the inputs that ask
    lec = torch.tensor(-0.7, device="cuda", requires_grad=True)
    lp, q_pi = _cuda(inp["log_prob"], False), [_cuda(q, i == 0) for i, q in enumerate(inp["q_pi"])]
    actor_loss, ent_loss, stats = tg.sac_actor_loss(lp, q_pi, log_ent_coef=lec)
    assert ent_loss is None and float(stats[1]) == 0 and float(stats[5]) == 0
    actor_loss.backward()
    assert lec.grad is None and lp.grad is None and all(q.grad is None for q in q_pi[1:])
    _within(_host(q_pi[0].grad), ex["dq_pi"][0], bounds["dq_pi"][0], "one critic alone")
    actor_loss2, ent_loss2, stats2 = tg.sac_actor_loss(lp, [q.detach() for q in q_pi], ent_coef=0.2)
    assert ent_loss2 is None and not actor_loss2.requires_grad and actor_loss2.grad_fn is None and float(stats2[2]) == float(f32(0.2))
    ex2 = ref.sac_actor_exact(**inp, ent_coef=0.2)
    _within(float(actor_loss2), ex2["actor_loss"], ref.sac_actor_bounds(ex2, **inp, ent_coef=0.2)["actor_loss"], "the float coefficient")


def test_refusals():
    import tactile_gym_amd as tg
    z = lambda *s: torch.zeros(*s, device="cuda")   # noqa: E731
    good = dict(q_cur=[z(8), z(8)], q_next=[z(8), z(8)], next_log_prob=z(8), rewards=z(8, 1), dones=z(8))
    call = lambda **kw: tg.sac_critic_loss(*(dict(good, **kw)[k] for k in good), 0.95, ent_coef=0.2)   # noqa: E731
    call()
    for k in ("next_log_prob", "rewards", "dones"):
        with pytest.raises(ValueError, match="ROCm device"):
            call(**{k: torch.zeros(8)})
        with pytest.raises(ValueError, match="shape"):
            call(**{k: z(7)})
        with pytest.raises(ValueError, match="contiguous"):
            call(**{k: z(8, 2)[:, 0]})
        with pytest.raises(ValueError, match="float32"):
            call(**{k: z(8).double()})
    for k in ("q_cur", "q_next"):
        with pytest.raises(ValueError, match="ROCm device"):
            call(**{k: [z(8), torch.zeros(8)]})
        with pytest.raises(ValueError, match="shape"):
            call(**{k: [z(8), z(8, 2)]})
        with pytest.raises(ValueError, match="contiguous"):
            call(**{k: [z(8, 2)[:, 1], z(8)]})
        with pytest.raises(ValueError, match="1 .. 4"):
            call(**{k: [z(8)] * 5})
        with pytest.raises(ValueError, match="1 .. 4"):
            call(**{k: []})
        with pytest.raises(TypeError):
            call(**{k: z(8)})
    with pytest.raises(ValueError, match="same number"):
        call(q_next=[z(8)])
    with pytest.raises(ValueError, match="exactly one"):
        tg.sac_critic_loss(good["q_cur"], good["q_next"], z(8), z(8), z(8), 0.95)
    with pytest.raises(ValueError, match="exactly one"):
        tg.sac_critic_loss(good["q_cur"], good["q_next"], z(8), z(8), z(8), 0.95, log_ent_coef=z(1), ent_coef=0.2)
    with pytest.raises(ValueError, match="shape"):
        tg.sac_critic_loss(good["q_cur"], good["q_next"], z(8), z(8), z(8), 0.95, log_ent_coef=z(2))
    with pytest.raises(ValueError, match="ROCm device"):
        tg.sac_critic_loss(good["q_cur"], good["q_next"], z(8), z(8), z(8), 0.95, log_ent_coef=torch.zeros(1))
    with pytest.raises(ValueError, match="shape"):
        tg.sac_critic_loss([z(0)], [z(0)], z(0), z(0), z(0), 0.95, ent_coef=0.2)
    with pytest.raises(ValueError, match="ROCm device"):
        tg.sac_actor_loss(torch.zeros(8), [z(8)], ent_coef=0.2)
    with pytest.raises(ValueError, match="shape"):
        tg.sac_actor_loss(z(8), [z(8), z(9)], ent_coef=0.2)
    with pytest.raises(ValueError, match="contiguous"):
        tg.sac_actor_loss(z(8, 2)[:, 0], [z(8)], ent_coef=0.2)
    with pytest.raises(ValueError, match="1 .. 4"):
        tg.sac_actor_loss(z(8), [z(8)] * 5, ent_coef=0.2)
    with pytest.raises(ValueError, match="exactly one"):
        tg.sac_actor_loss(z(8), [z(8)])
    with pytest.raises(ValueError, match="needs log_ent_coef"):
        tg.sac_actor_loss(z(8), [z(8)], ent_coef=0.2, target_entropy=-2.0)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="device"):
            tg.sac_actor_loss(z(8), [torch.zeros(8, device="cuda:1")], ent_coef=0.2)


# ---------------------------------------------------------------------------------------------------------------- polyak_update
@pytest.mark.parametrize("tau", [0.005, 1.0])
def test_polyak_update_on_the_device_against_the_float64_formula(tau):
    """target' = fl(fl(t s1) + s2 p) with the float32 scalars s1 = fl(1 - tau), s2 = fl(tau) that the two launches receive: the product
    U |s1 t|, the product and the sum of the second launch U |s2 p| + U |target'| (one rounding less where it is fused) - within
    2 U (|s1 t| + |s2 p|) per element of the float64 formula at those scalars."""
    from tactile_gym_amd import train
    gen = torch.Generator(device="cuda").manual_seed(11)
    shapes = [(32, 3, 8, 8), (32,), (0,), (256, 18), (1,), (7, 5)]
    params = [torch.randn(s, generator=gen, device="cuda") for s in shapes]
    targets = [torch.randn(s, generator=gen, device="cuda") for s in shapes]
    kept, before = [_host(x).copy() for x in params], [_host(x).astype(np.float64) for x in targets]
    train.polyak_update(params, targets, tau)
    s1, s2 = float(f32(1 - tau)), float(f32(tau))
    for param, k, t, b in zip(params, kept, targets, before):
        assert np.array_equal(_host(param), k)                                # params are unchanged
        a, c = s1 * b, s2 * k.astype(np.float64)
        _within(_host(t), a + c, ref.SLACK * 2 * U * (np.abs(a) + np.abs(c)), tuple(t.shape))
    if tau == 1.0:
        assert all(torch.equal(t, param) for t, param in zip(targets, params))


# ---------------------------------------------------------------------------------------------------------------- on the env
class Actor(nn.Module):
    """tg.NatureCNN over the tactile image and a linear head -> (mean [B, 2], log_std [B, 2])."""

    def __init__(self, space):
        import tactile_gym_amd as tg
        super().__init__()
        self.features = tg.NatureCNN(space, features_dim=16, float_scale=1.0 / 255.0)
        self.out = nn.Linear(16, 4)

    def forward(self, obs):
        self.seen = getattr(self, "seen", []) + [obs]
        o = self.out(self.features(obs["tactile"]))
        return o[:, :2].contiguous(), (o[:, 2:] - 1.0).contiguous()


class TwoCritics(nn.Module):
    """SB3's ContinuousCritic with n_critics = 2 on small nets: (q_0 [B, 1], q_1 [B, 1]).  Keeps every call's outputs and the gradients
    that reach them."""

    def __init__(self, space):
        import tactile_gym_amd as tg
        super().__init__()
        self.features = tg.NatureCNN(space, features_dim=16, float_scale=1.0 / 255.0)
        self.q_networks = nn.ModuleList([nn.Sequential(nn.Linear(18, 32), nn.Tanh(), nn.Linear(32, 1)) for _ in range(2)])
        self.calls, self.grads, self.inputs = [], [], []

    def forward(self, obs, actions):
        self.inputs.append((obs, actions))
        x = torch.cat([self.features(obs["tactile"]), actions], dim=1)
        qs = tuple(q(x) for q in self.q_networks)
        got = {}
        self.calls.append(qs)
        self.grads.append(got)
        for i, q in enumerate(qs):
            if q.requires_grad:
                q.register_hook(lambda g, i=i, got=got: got.setdefault(i, g.detach().clone()))
        return qs


class NoisyHead:
    """head.rsample with the noise given, in the order of the calls; keeps the outputs and log_prob's gradient."""

    def __init__(self, head, noises):
        self.head, self.noises, self.calls, self.grads = head, list(noises), [], {}

    def rsample(self, mean, log_std):
        k = len(self.calls)
        actions, log_prob = self.head.rsample(mean, log_std, noise=self.noises[k])
        self.calls.append((actions, log_prob))
        if log_prob.requires_grad:
            log_prob.register_hook(lambda g, k=k: self.grads.setdefault(k, g.detach().clone()))
        return actions, log_prob


class KeepingBuffer:
    """rb.sample as asked, keeping what it returned."""

    def __init__(self, rb):
        self.rb, self.asked, self.batches = rb, [], []

    def sample(self, batch_size, **kw):
        self.asked.append((batch_size, kw))
        self.batches.append(self.rb.sample(batch_size, **kw))
        return self.batches[-1]


def _sb3_sac_step(actor, critic, critic_target, actor_opt, critic_opt, lec, ent_opt, batch, head, noise_pi, noise_next, tau):
    """SAC.train's lines in SB3's own order with torch's ops: the entropy step first, cat / min, F.mse_loss, the per-tensor polyak loop."""
    actions_pi, log_prob = head.rsample(*actor(batch.observations), noise=noise_pi)
    log_prob = log_prob.reshape(-1, 1)
    log_prob.retain_grad()
    ent_coef = torch.exp(lec.detach())
    ent_coef_loss = -(lec * (log_prob + TE).detach()).mean()
    ent_opt.zero_grad()
    ent_coef_loss.backward()
    ent_opt.step()
    with torch.no_grad():
        next_actions, next_log_prob = head.rsample(*actor(batch.next_observations), noise=noise_next)
        next_q = torch.cat(critic_target(batch.next_observations, next_actions), dim=1)
        next_q, _ = torch.min(next_q, dim=1, keepdim=True)
        next_q = next_q - ent_coef * next_log_prob.reshape(-1, 1)
        target_q = batch.rewards + (1 - batch.dones) * GAMMA * next_q
    current_q = critic(batch.observations, batch.actions)
    critic_loss = 0.5 * sum(F.mse_loss(q, target_q) for q in current_q)
    critic_opt.zero_grad()
    critic_loss.backward()
    critic_opt.step()
    q_pi = torch.cat(critic(batch.observations, actions_pi), dim=1)
    min_qf_pi, _ = torch.min(q_pi, dim=1, keepdim=True)
    actor_loss = (ent_coef * log_prob - min_qf_pi).mean()
    actor_opt.zero_grad()
    actor_loss.backward()
    actor_opt.step()
    with torch.no_grad():
        for param, target_param in zip(critic.parameters(), critic_target.parameters()):
            target_param.data.mul_(1 - tau)
            torch.add(target_param.data, param.data, alpha=tau, out=target_param.data)
    return dict(critic_loss=float(critic_loss.detach()), actor_loss=float(actor_loss.detach()), ent_coef_loss=float(ent_coef_loss.detach()),
                actions_pi=actions_pi, log_prob=log_prob, next_log_prob=next_log_prob, dlog_prob=_host(log_prob.grad).reshape(-1), dlog_ent_coef=float(lec.grad))


def _q_sensitivity(critic, obs, actions):
    """float64 [2, B]: sum over the critic's parameters theta of |d q_i[b] / d theta| at (obs, actions)."""
    params = list(critic.parameters())
    qs = critic(obs, actions)
    out = np.zeros((2, qs[0].shape[0]))
    for i, q in enumerate(qs):
        for b in range(q.shape[0]):
            grads = torch.autograd.grad(q[b, 0], params, retain_graph=True, allow_unused=True)
            out[i, b] = float(sum(g.abs().sum().double() for g in grads if g is not None))
    return out


def test_one_sac_train_step_on_the_env_against_sb3s_order():
    import tactile_gym_amd as tg
    from tactile_gym_amd.collect import collect_transitions
    N, SIZE, MB, TAU, LR = 4, 128, 16, 0.005, 1e-5       # a small lr: the sides' critics part by at most 2 lr per parameter (below)
    venv = tg.make_vec("edge_follow-v0", num_envs=N, max_steps=5, image_size=[SIZE, SIZE], env_modes=MODES, seed=3, obs_mode="torch")
    try:
        torch.manual_seed(4)
        space = venv.observation_space.spaces["tactile"]
        actor, critic, critic_target = Actor(space).cuda(), TwoCritics(space).cuda(), TwoCritics(space).cuda()
        lec = torch.zeros(1, device="cuda", requires_grad=True)               # ent_coef="auto": log(1.0)
        rb = tg.DeviceReplayBuffer.for_env(venv, 8 * N, seed=5)
        head = tg.DeviceSquashedDiagGaussian.for_env(venv, seed=9)
        obs = venv.reset()
        rb.start(obs)
        obs, steps = collect_transitions(venv, actor, rb, head, 8, 0, 4 * N, obs)
        assert steps == 8 * N
        twins = [copy.deepcopy(m) for m in (actor, critic, critic_target)]
        lec2 = lec.detach().clone().requires_grad_()
        adam = lambda params: torch.optim.Adam(params, lr=LR)   # noqa: E731
        opts = [adam(actor.parameters()), adam(critic.parameters()), adam([lec])]
        opts2 = [adam(twins[0].parameters()), adam(twins[1].parameters()), adam([lec2])]
        noise_pi, noise_next = torch.randn(MB, 2, device="cuda"), torch.randn(MB, 2, device="cuda")
        target_before = [p.detach().clone() for p in critic_target.parameters()]
        critic_before = [p.detach().clone() for p in critic.parameters()]
        # ours
        noisy, keeping = NoisyHead(head, [noise_pi, noise_next]), KeepingBuffer(rb)   # SB3's draw order: actions_pi first
        cstats, astats, n_updates = tg.train.sac_train(actor, critic, critic_target, opts[0], opts[1], keeping, noisy, 1, MB, GAMMA, TAU,
                                                       log_ent_coef=lec, ent_coef_optimizer=opts[2], target_entropy=TE, target_update_interval=1)
        assert n_updates == 1 and cstats.shape == (8,) and astats.shape == (8,) and keeping.asked[0][0] == MB and len(keeping.batches) == 1
        assert len(noisy.calls) == 2 and noisy.calls[0][1].requires_grad and not noisy.calls[1][1].requires_grad
        assert len(critic.calls) == 2 and len(critic_target.calls) == 1
        batch = keeping.batches[0]
        # what every network was called on
        assert actor.seen[-2] is batch.observations and actor.seen[-1] is batch.next_observations
        assert critic.inputs[0][0] is batch.observations and critic.inputs[0][1] is batch.actions
        assert critic.inputs[1][0] is batch.observations and critic.inputs[1][1] is noisy.calls[0][0]          # actions_pi
        assert critic_target.inputs[0][0] is batch.next_observations and critic_target.inputs[0][1] is noisy.calls[1][0]   # next_actions
        # SB3's order on the copies, the same minibatch and the same noise
        theirs = _sb3_sac_step(*twins, opts2[0], opts2[1], lec2, opts2[2], batch, head, noise_pi, noise_next, TAU)
        rewards, dones = _host(batch.rewards), _host(batch.dones)
        assert ((dones == 0) | (dones == 1)).all()
        # Before any step both sides evaluate the same weights on the same minibatch and noise with the same kernels: everything that
        # enters the critic loss, and log_prob, is bit-equal between the sides, so both sides share ONE float64 value
        same = lambda a, b: torch.equal(a.detach().reshape(-1), b.detach().reshape(-1))   # noqa: E731
        assert all(same(a, b) for a, b in zip(critic.calls[0], twins[1].calls[0])), "q_cur"
        assert all(same(a, b) for a, b in zip(critic_target.calls[0], twins[2].calls[0])), "q_next"
        assert same(noisy.calls[1][1], theirs["next_log_prob"]) and same(noisy.calls[0][1], theirs["log_prob"])
        assert same(noisy.calls[0][0], theirs["actions_pi"])
        inp = dict(q_cur=[_host(q) for q in critic.calls[0]], q_next=[_host(q) for q in critic_target.calls[0]],
                   next_log_prob=_host(noisy.calls[1][1]), rewards=rewards, dones=dones)
        ex = ref.sac_critic_exact(**inp, gamma=GAMMA, log_ent_coef=0.0)
        b1 = ref.sac_critic_bounds(ex, **inp, gamma=GAMMA, log_ent_coef=0.0)
        b2 = ref.sac_critic_bounds(ex, **inp, gamma=GAMMA, log_ent_coef=0.0, acc=ref.U, autograd32=True)
        l1, l2 = float(cstats[0]), theirs["critic_loss"]
        dq1, dq2 = (np.stack([_host(c.grads[0][i]).reshape(-1) for i in range(2)]) for c in (critic, twins[1]))
        _within(l1, ex["critic_loss"], b1["critic_loss"], "critic_loss, ours")
        _within(l2, ex["critic_loss"], b2["critic_loss"], "critic_loss, torch's")
        _within(dq1, ex["dq_cur"], b1["dq_cur"], "dq_cur, ours")
        _within(dq2, ex["dq_cur"], b2["dq_cur"], "dq_cur, torch's")
        assert abs(l1 - l2) <= b1["critic_loss"] + b2["critic_loss"]          # within the sum of both sides' bounds, nothing added
        assert (np.abs(dq1 - dq2) <= b1["dq_cur"] + b2["dq_cur"]).all()
        assert float(np.abs(dq1).max()) > 0 and ex["critic_loss"] > 1e-4
        # The actor loss is formed after the critics' Adam step, where the sides differ legitimately.  How far, derived: Adam's first step
        # moves a parameter by lr |g| / (|g| + eps) <= lr whatever its gradient, so the sides' critics differ by at most 2 lr per parameter,
        # and q_pi_i[b] by at most 2 lr sum_theta |d q_i[b] / d theta| to first order in lr; the sum is taken by autograd at both sides'
        # critics (the larger counts), and a factor 2 is allowed for the change of that gradient along a step of 2 lr per coordinate.
        # min is 1-Lipschitz in the largest deviation: actor_loss differs by at most the rows' mean of max_i; the row's minimum may sit at
        # the other critic only where the two critics are closer than their two deviations, and there dq_pi may differ by 1 / B.
        S = np.maximum(_q_sensitivity(critic, batch.observations, noisy.calls[0][0].detach()),
                       _q_sensitivity(twins[1], batch.observations, theirs["actions_pi"].detach()))
        dq = 2 * 2 * LR * S
        lp = _host(noisy.calls[0][1]).reshape(-1)
        q1, q2 = ([_host(q).reshape(-1) for q in c.calls[1]] for c in (critic, twins[1]))
        assert (np.abs(np.stack(q1).astype(np.float64) - np.stack(q2)) <= dq).all()                   # the derived distance holds
        d_actor = float(dq.max(axis=0).mean())
        may_flip = np.abs(q1[0].astype(np.float64) - q1[1]) <= dq[0] + dq[1]
        print(f"q_pi may differ by {dq.max():.3g} (|q_pi| up to {np.abs(np.stack(q1)).max():.3g}); actor_loss by {d_actor:.3g}; "
              f"{int(may_flip.sum())} of {MB} rows may change their minimum")
        sides = []
        for q_pi, got, acc in ((q1, dict(actor_loss=float(astats[0]), ent_coef_loss=float(astats[1]), dlog_prob=_host(noisy.grads[0]).reshape(-1),
                                         dlog_ent_coef=float(lec.grad), dq_pi=np.stack([_host(critic.grads[1][i]).reshape(-1) for i in range(2)])), ref.D),
                               (q2, dict(theirs, dq_pi=np.stack([_host(twins[1].grads[1][i]).reshape(-1) for i in range(2)])), ref.U)):
            inp = dict(log_prob=lp, q_pi=q_pi)
            ex = ref.sac_actor_exact(**inp, log_ent_coef=0.0, target_entropy=TE)
            bd = ref.sac_actor_bounds(ex, **inp, log_ent_coef=0.0, target_entropy=TE, acc=acc, autograd32=acc == ref.U)
            for k in ("actor_loss", "ent_coef_loss", "dlog_prob", "dlog_ent_coef", "dq_pi"):
                _within(got[k], ex[k], bd[k], (k, acc))
            sides.append((got, ex, bd))
        (g1, ex1, b1), (g2, ex2, b2) = sides
        for k in ("ent_coef_loss", "dlog_prob", "dlog_ent_coef"):             # functions of log_prob and log_ent_coef alone: one float64 value
            assert np.array_equal(ex1[k], ex2[k])
            assert (np.abs(np.asarray(g1[k]) - g2[k]) <= b1[k] + b2[k]).all(), k
        assert abs(g1["actor_loss"] - g2["actor_loss"]) <= b1["actor_loss"] + b2["actor_loss"] + d_actor
        assert (np.abs(g1["dq_pi"] - g2["dq_pi"]) <= b1["dq_pi"] + b2["dq_pi"] + np.where(may_flip, 1.0 / MB, 0.0)).all()
        assert float(astats[5]) == g1["dlog_ent_coef"] and abs(g1["dlog_ent_coef"]) > 1e-3
        # log_ent_coef after its step.  Adam's first step from 0 is -lr g / (|g| + eps): each side evaluates it in at most 16 float32
        # roundings of quantities of size lr, and d/dg (g / (|g| + eps)) = eps / (|g| + eps)^2 carries the two gradients' distance
        eps, g = 1e-8, abs(g1["dlog_ent_coef"])
        bound = LR * (2 * 16 * U + eps * abs(g1["dlog_ent_coef"] - g2["dlog_ent_coef"]) / (g + eps) ** 2)
        assert abs(float(lec.detach()) - float(lec2.detach())) <= bound and abs(abs(float(lec.detach())) - LR) <= LR * 1e-5
        # the target critic after the polyak update, target' = (1 - tau) target + tau critic'.  Both sides start from the same target and
        # critic.  Adam's first step moves a parameter by lr |g| / (|g| + eps) <= lr whatever its gradient g (its sign may differ between
        # the sides where g is rounding noise), so the sides' critic' differ by at most 2 lr, which the update scales by tau; each side's
        # own update rounds within 2 U (|(1 - tau) target| + |tau critic'|) (test_polyak_update_on_the_device_...), 3 U with SB3's
        # separately rounded 1 - tau and tau.  Together:  2 tau lr + 5 U (|(1 - tau) target| + tau (|critic| + lr)).
        moved = 0.0
        for t0, c0, t1, t2 in zip(target_before, critic_before, critic_target.parameters(), twins[2].parameters()):
            bound = 2 * TAU * LR + 5 * U * ((1 - TAU) * t0.abs() + TAU * (c0.abs() + LR))
            assert bool(((t1.detach() - t2.detach()).abs() <= ref.SLACK * bound).all())
            moved = max(moved, float(((t1.detach() - t0).abs() / bound).max()))
        assert moved > 100                                                    # and the update happened: it moved some element 100 bounds
        # target_update_interval = 2: the odd update leaves the target network's bits, the even one moves them
        kept = [p.detach().clone() for p in critic_target.parameters()]
        _, _, n_updates = tg.train.sac_train(actor, critic, critic_target, opts[0], opts[1], rb, head, 1, MB, GAMMA, TAU, log_ent_coef=lec,
                                             ent_coef_optimizer=opts[2], target_entropy=TE, target_update_interval=2, n_updates=2)
        assert n_updates == 3 and all(torch.equal(a, b) for a, b in zip(kept, critic_target.parameters()))
        _, _, n_updates = tg.train.sac_train(actor, critic, critic_target, opts[0], opts[1], rb, head, 1, MB, GAMMA, TAU, log_ent_coef=lec,
                                             ent_coef_optimizer=opts[2], target_entropy=TE, target_update_interval=2, n_updates=n_updates)
        assert n_updates == 4 and any(not torch.equal(a, b) for a, b in zip(kept, critic_target.parameters()))
        assert bool(torch.isfinite(lec).all()) and all(bool(torch.isfinite(p).all()) for p in actor.parameters())
    finally:
        venv.close()
