"""tactile_gym_amd.rollout on the device (csrc/tg_rollout.hip, the row-indexed k_random_translate) against tests/rollout_ref.py and
tests/augment_ref.py: stored bytes, GAE bit for bit, minibatches field by field, the fused augmentation bit for bit, and rollouts collected from
device envs."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from augment_ref import warp_f32  # noqa: E402
from rollout_ref import flat_rows, gae_f32, minibatches  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")
PUSH = dict(movement_mode="TyRz", control_mode="TCP_velocity_control", rand_init_orn=True, rand_obj_mass=True, traj_type="straight",
            observation_mode="tactile_and_feature", reward_mode="dense", arm_type="ur5", tactile_sensor_name="digitac")
FIELDS = ("actions", "values", "log_probs", "advantages", "returns")
SAMPLE_FIELDS = dict(actions="actions", values="old_values", log_probs="old_log_prob", advantages="advantages", returns="returns")


def _mods():
    import tactile_gym_amd as tg
    from tactile_gym_amd import spaces
    return tg, spaces


def _box_u8(shape):
    return _mods()[1].Box(low=0, high=255, shape=shape, dtype=np.uint8)


def _box_f32(shape):
    return _mods()[1].Box(low=-np.inf, high=np.inf, shape=shape, dtype=np.float32)


def _obs_space(layout, H=16, W=16):
    """The observation layouts the envs produce, at a small image size."""
    sp = _mods()[1]
    return {"tactile_last": sp.Dict({"tactile": _box_u8((H, W, 2))}),
            "tactile_first": sp.Dict({"tactile": _box_u8((2, H, W))}),
            "tactile_n1": sp.Dict({"tactile": _box_u8((H, W, 1))}),
            "visual": sp.Dict({"visual": _box_u8((6, H, W))}),
            "visuotactile": sp.Dict({"tactile": _box_u8((H, W, 2)), "visual": _box_u8((H, W, 6))}),
            "tactile_and_feature": sp.Dict({"tactile": _box_u8((2, H, W)), "extended_feature": _box_f32((6,))}),
            "oracle": sp.Dict({"oracle": _box_f32((10,))}),
            "odd": sp.Dict({"tactile": _box_u8((10, 6, 1)), "extended_feature": _box_f32((3,))}),
            "box": _box_u8((1, H, W))}[layout]


def _step_inputs(rng, space, N, A, start_dtype):
    sub = space.spaces if hasattr(space, "spaces") else {None: space}
    obs = {k: (rng.integers(0, 256, size=(N,) + tuple(s.shape), dtype=np.uint8) if s.dtype == np.uint8
               else rng.standard_normal((N,) + tuple(s.shape)).astype(np.float32)) for k, s in sub.items()}
    starts = rng.random(N) < 0.3
    return dict(obs=obs if None not in obs else obs[None], action=rng.standard_normal((N, A)).astype(np.float32),
                reward=rng.standard_normal(N).astype(np.float32), episode_start=starts.astype(start_dtype),
                value=rng.standard_normal(N).astype(np.float32), log_prob=rng.standard_normal(N).astype(np.float32))


def _dev(x):
    if isinstance(x, dict):
        return {k: _dev(v) for k, v in x.items()}
    return torch.from_numpy(x).cuda()


def _filled(layout, T, N, A=2, seed=0, numpy_inputs=False, start_dtype=np.uint8, channels_first=None, H=16, W=16, **kw):
    """(buffer, the steps' inputs as numpy) after T adds of random inputs."""
    tg, _ = _mods()
    space = _obs_space(layout, H, W)
    act = _mods()[1].Box(low=-1.0, high=1.0, shape=(A,), dtype=np.float32)
    buf = tg.DeviceRolloutBuffer(T, space, act, "cuda", n_envs=N, channels_first=channels_first, **kw)
    rng = np.random.default_rng(seed)
    steps = []
    for t in range(T):
        assert buf.pos == t and not buf.full and buf.size() == t
        s = _step_inputs(rng, space, N, A, start_dtype)
        steps.append(s)
        if numpy_inputs:
            buf.add(**s)
        else:
            held = {k: _dev(v) for k, v in s.items()}
            buf.add(**held)
            torch.cuda.synchronize()
            for k, v in held.items():                                        # the inputs are only read
                for kk, vv in (v.items() if isinstance(v, dict) else [(None, v)]):
                    ref = s[k][kk] if kk is not None else s[k]
                    assert np.array_equal(vv.cpu().numpy(), ref), (k, kk)
    assert buf.full and buf.pos == T and buf.size() == T
    return buf, steps


def _stacked(steps, name, key=None):
    return np.stack([(s[name][key] if key is not None else s[name]) for s in steps])


def _check_storage(buf, steps):
    torch.cuda.synchronize()
    obs = buf.observations if isinstance(buf.observations, dict) else {None: buf.observations}
    for k, t in obs.items():
        assert np.array_equal(t.cpu().numpy(), _stacked(steps, "obs", k)), k
    for name, src in (("actions", "action"), ("rewards", "reward"), ("values", "value"), ("log_probs", "log_prob")):
        assert np.array_equal(getattr(buf, name).cpu().numpy(), _stacked(steps, src)), name
    es = buf.episode_starts.cpu().numpy()
    assert es.dtype == np.float32 and np.array_equal(es, (_stacked(steps, "episode_start") != 0).astype(np.float32))


@pytest.mark.parametrize("layout", ["tactile_last", "tactile_first", "tactile_n1", "visual", "visuotactile", "tactile_and_feature", "oracle", "box"])
def test_add_stores_every_input(layout):
    buf, steps = _filled(layout, T=5, N=8)
    _check_storage(buf, steps)
    with pytest.raises(RuntimeError, match="full"):
        buf.add(**{k: _dev(v) for k, v in steps[0].items()})
    buf.reset()
    assert buf.pos == 0 and not buf.full


@pytest.mark.parametrize("start_dtype", [np.uint8, np.bool_, np.float32])
def test_add_odd_sizes_take_the_tail_paths(start_dtype):
    """N = 3, 10 x 6 images, 3 actions: slots that are not 16-byte (or 4-byte) multiples."""
    buf, steps = _filled("odd", T=7, N=3, A=3, seed=3, start_dtype=start_dtype)
    _check_storage(buf, steps)


def test_add_full_size_slot():
    buf, steps = _filled("tactile_first", T=2, N=64, H=128, W=128, seed=5)
    _check_storage(buf, steps)


def test_add_numpy_inputs_give_the_same_contents():
    a, steps = _filled("tactile_and_feature", T=4, N=5, seed=7, numpy_inputs=True, start_dtype=np.bool_)
    b, _ = _filled("tactile_and_feature", T=4, N=5, seed=7, numpy_inputs=False, start_dtype=np.bool_)
    _check_storage(a, steps)
    _check_storage(b, steps)
    s = dict(steps[0], reward=steps[0]["reward"].astype(np.float64), value=steps[0]["value"].reshape(5, 1))   # SB3: float64 rewards, [N, 1] values
    a.reset()
    a.add(**s)
    torch.cuda.synchronize()
    assert np.array_equal(a.rewards[0].cpu().numpy(), steps[0]["reward"]) and np.array_equal(a.values[0].cpu().numpy(), steps[0]["value"])


# ---------------------------------------------------------------------------------------------------------------- GAE
def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("gamma,lam", [(0.95, 0.9), (0.99, 0.95), (0.999, 1.0)])
@pytest.mark.parametrize("T,N", [(1, 1), (7, 3), (200, 64), (2048, 1024)])
def test_gae_bit_exact(T, N, gamma, lam):
    tg, sp = _mods()
    rng = np.random.default_rng(T * 7 + N)
    buf = tg.DeviceRolloutBuffer(T, sp.Dict({"oracle": _box_f32((2,))}), sp.Box(low=-1.0, high=1.0, shape=(2,), dtype=np.float32), "cuda",
                                 gae_lambda=lam, gamma=gamma, n_envs=N)
    r = rng.standard_normal((T, N)).astype(np.float32)
    v = (rng.standard_normal((T, N)) * 5).astype(np.float32)
    es = (rng.random((T, N)) < 0.02).astype(np.float32)
    lv = (rng.standard_normal(N) * 5).astype(np.float32)
    d = rng.random(N) < 0.3
    buf.rewards.copy_(torch.from_numpy(r))
    buf.values.copy_(torch.from_numpy(v))
    buf.episode_starts.copy_(torch.from_numpy(es))
    adv, ret = gae_f32(r, v, es, lv, d, gamma, lam)
    for dones in (d.astype(np.uint8), d, d.astype(np.float32)):
        for as_numpy in (False, True):
            buf.advantages.fill_(float("nan"))
            buf.returns.fill_(float("nan"))
            if as_numpy:
                buf.compute_returns_and_advantage(lv.reshape(N, 1), dones)
            else:
                buf.compute_returns_and_advantage(torch.from_numpy(lv).cuda(), torch.from_numpy(dones).cuda())
            torch.cuda.synchronize()
            assert _bits_equal(buf.advantages.cpu().numpy(), adv), (dones.dtype, as_numpy)
            assert _bits_equal(buf.returns.cpu().numpy(), ret), (dones.dtype, as_numpy)
    assert np.array_equal(buf.rewards.cpu().numpy(), r) and np.array_equal(buf.values.cpu().numpy(), v)


# ---------------------------------------------------------------------------------------------------------------- get
def _storage_numpy(buf):
    obs = buf.observations if isinstance(buf.observations, dict) else {None: buf.observations}
    st = {("obs", k): t.cpu().numpy() for k, t in obs.items()}
    st.update({name: getattr(buf, name).cpu().numpy() for name in FIELDS})
    return st


def _check_batches(buf, got, idx, batch_size, out_dtype=np.float32):
    st = _storage_numpy(buf)
    ref = list(minibatches(st, idx, batch_size))
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g._fields == ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns")
        obs = g.observations if isinstance(g.observations, dict) else {None: g.observations}
        for k, t in obs.items():
            want = r[("obs", k)]
            if want.dtype == np.uint8 and want.ndim == 4:
                want = want.astype(out_dtype)
            a = t.cpu().numpy()
            assert a.dtype == want.dtype and np.array_equal(a, want), k
        for name, field in SAMPLE_FIELDS.items():
            a = getattr(g, field).cpu().numpy()
            assert a.dtype == np.float32 and a.shape == r[name].shape and _bits_equal(a, r[name]), name


@pytest.mark.parametrize("layout,T,N,A", [("tactile_and_feature", 6, 5, 2), ("visuotactile", 4, 3, 2), ("oracle", 9, 4, 3), ("odd", 7, 3, 3),
                                           ("box", 3, 4, 1)])
def test_get_explicit_indices(layout, T, N, A):
    buf, _ = _filled(layout, T, N, A, seed=11)
    buf.compute_returns_and_advantage(np.ones(N, np.float32), np.zeros(N, np.uint8))
    rng = np.random.default_rng(1)
    perm = rng.permutation(T * N)
    repeated = rng.integers(0, T * N, size=T * N + 3)
    for idx, bs in ((perm, 4), (perm, None), (repeated, 7), (perm[:5], 2), (np.array([T * N - 1] * 3), 8)):
        for out_dtype in (torch.float32, torch.uint8):
            got = list(buf.get(bs, indices=torch.from_numpy(idx).cuda(), out_dtype=out_dtype))
            torch.cuda.synchronize()
            _check_batches(buf, got, idx, bs or len(idx), np.float32 if out_dtype == torch.float32 else np.uint8)
            assert len(got[-1].actions) == (len(idx) - 1) % (bs or len(idx)) + 1       # the short last batch
    got = list(buf.get(4, indices=perm))                                               # host indices are uploaded
    _check_batches(buf, got, perm, 4)


def test_get_serves_every_index_once():
    """Without indices: a device permutation.  `values` holds each sample's flat index, so the served order can be read back."""
    tg, sp = _mods()
    T, N = 16, 24
    buf = tg.DeviceRolloutBuffer(T, sp.Dict({"tactile": _box_u8((1, 8, 8))}), sp.Box(low=-1.0, high=1.0, shape=(2,), dtype=np.float32), "cuda",
                                 n_envs=N)
    buf.pos, buf.full = T, True
    flat = np.arange(T * N)
    buf.values.copy_(torch.from_numpy((flat % N * T + flat // N).reshape(T, N).astype(np.float32)))     # storage row t N + n holds i = n T + t
    buf.observations["tactile"].copy_(buf.values.to(torch.uint8).view(T, N, 1, 1, 1).expand(T, N, 1, 8, 8))
    orders = []
    for gen in (None, torch.Generator(device="cuda").manual_seed(3), torch.Generator(device="cuda").manual_seed(3)):
        got = list(buf.get(50, generator=gen))
        assert [len(g.old_values) for g in got] == [50] * 7 + [34]
        served = torch.cat([g.old_values for g in got]).cpu().numpy().astype(np.int64)
        assert np.array_equal(np.sort(served), flat)
        assert not np.array_equal(served, flat)
        img = torch.cat([g.observations["tactile"] for g in got]).cpu().numpy()
        assert np.array_equal(img[:, 0, 0, 0], (served % 256).astype(np.float32))
        orders.append(served)
    assert np.array_equal(orders[1], orders[2]) and not np.array_equal(orders[0], orders[1])


@pytest.mark.parametrize("channels_first", [True, False])
@pytest.mark.parametrize("hw", [(128, 128), (48, 80), (10, 6)])
def test_fused_augment_bit_exact(channels_first, hw):
    import tactile_gym_amd.augment as K
    tg, sp = _mods()
    H, W = hw
    T, N, C = 6, 12, 2
    shape = (C, H, W) if channels_first else (H, W, C)
    space = sp.Dict({"tactile": _box_u8(shape), "extended_feature": _box_f32((4,))})
    buf = tg.DeviceRolloutBuffer(T, space, sp.Box(low=-1.0, high=1.0, shape=(2,), dtype=np.float32), "cuda", n_envs=N, channels_first=channels_first)
    rng = np.random.default_rng(H + W)
    store = rng.integers(0, 256, size=(T, N) + shape, dtype=np.uint8)
    buf.observations["tactile"].copy_(torch.from_numpy(store))
    buf.observations["extended_feature"].copy_(torch.from_numpy(rng.standard_normal((T, N, 4)).astype(np.float32)))
    buf.pos, buf.full = T, True
    idx = np.concatenate([rng.permutation(T * N), rng.integers(0, T * N, size=9)])
    rows = flat_rows(idx, T, N)
    aug = torch.nn.Sequential(K.RandomAffine(degrees=0, translate=[0.05, 0.05], scale=[1.0, 1.0], p=0.5, seed=77))
    if not channels_first:
        aug[0].channels_first = False
    aug[0].counter = 5
    flat_dev = buf.observations["tactile"].view((T * N,) + shape)
    applied = 0
    for k, batch in enumerate(buf.get(32, augment=aug, indices=torch.from_numpy(idx).cuda())):
        sel = rows[32 * k:32 * k + 32]
        assert aug[0].counter == 6 + k                                        # one call of the module per image key and minibatch
        prm = torch.cat([aug[0]._params["batch_prob"].float()[:, None], aug[0]._params["translations"]], dim=1).cpu().numpy()
        got = batch.observations["tactile"].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (len(sel),) + shape
        two_step, prm2 = K.random_translate(flat_dev[torch.from_numpy(sel).cuda()], (0.05, 0.05), 0.5, seed=77, counter=5 + k,
                                            channels_first=channels_first, return_params=True)
        assert _bits_equal(prm, prm2.cpu().numpy())
        assert _bits_equal(got, two_step.cpu().numpy())                       # gather, then the augmentation: the same bits
        assert _bits_equal(got, warp_f32(store.reshape((T * N,) + shape)[sel], prm, channels_first))
        assert np.array_equal(batch.observations["extended_feature"].cpu().numpy(),
                              buf.observations["extended_feature"].view(T * N, 4).cpu().numpy()[sel])
        n_app = int(prm[:, 0].sum())
        assert 0 < n_app < len(sel)                                           # applied and unapplied samples in every minibatch
        applied += n_app
    assert np.array_equal(buf.observations["tactile"].cpu().numpy(), store)   # the storage is only read
    assert applied > 0


def test_fused_augment_refuses_other_modules():
    buf, _ = _filled("tactile_first", T=2, N=2)
    with pytest.raises(TypeError, match="Identity"):
        buf.get(2, augment=torch.nn.Identity())


# ---------------------------------------------------------------------------------------------------------------- device envs
def _check_env_rollout(buf, log, T):
    torch.cuda.synchronize()
    for k, t in buf.observations.items():
        assert torch.equal(t, torch.stack([s["obs"][k] for s in log])), k
    for name, key in (("actions", "actions"), ("rewards", "rewards"), ("values", "values"), ("log_probs", "log_probs")):
        assert torch.equal(getattr(buf, name), torch.stack([s[key] for s in log])), name
    es = buf.episode_starts.cpu().numpy()
    dones = torch.stack([s["dones"] for s in log]).cpu().numpy()
    assert np.array_equal(es[0], np.ones(es.shape[1], np.float32))
    assert np.array_equal(es[1:], dones[:-1].astype(np.float32))              # the shifted done flags
    return dones


def test_edge_follow_rollout_end_to_end():
    import tactile_gym_amd.augment as K
    tg, _ = _mods()
    T, N = 16, 64
    venv = tg.make_vec("edge_follow-v0", num_envs=N, max_steps=6, image_size=[128, 128], env_modes=EDGE, seed=4, obs_mode="torch", frame_stack=2,
                       channels_first=True)
    try:
        obs = venv.reset()
        buf = tg.DeviceRolloutBuffer.for_env(venv, T, gamma=0.95, gae_lambda=0.9)
        assert buf.n_envs == N and buf.buffer_size == T and buf._channels_first == {"tactile": True}
        assert tuple(buf.observations["tactile"].shape) == (T, N, 2, 128, 128)
        g = torch.Generator(device="cuda").manual_seed(1)
        starts = torch.ones(N, dtype=torch.uint8, device="cuda")
        log = []
        for t in range(T):
            actions = (torch.rand((N, 2), device="cuda", generator=g) - 0.5) * 0.5
            values, log_probs = torch.randn(N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g)
            clone = {k: v.clone() for k, v in obs.items()}
            buf.add(obs, actions, torch.zeros(N, device="cuda"), starts, values, log_probs)      # the env's zero-copy views, before the step
            obs, _, _, _ = venv.step(actions)
            rewards, dones = venv.reward_done_torch()
            buf.rewards[t].copy_(rewards)                                                        # SB3 adds after the step; the views moved on
            log.append(dict(obs=clone, actions=actions.clone(), rewards=rewards.clone(), dones=dones.clone(), values=values, log_probs=log_probs))
            starts = dones.clone()
        dones = _check_env_rollout(buf, log, T)
        assert dones.any() and not dones.all()                                                   # episodes ended inside the rollout
        last_values = torch.randn(N, device="cuda", generator=g)
        buf.compute_returns_and_advantage(last_values, starts)
        torch.cuda.synchronize()
        adv, ret = gae_f32(buf.rewards.cpu().numpy(), buf.values.cpu().numpy(), buf.episode_starts.cpu().numpy(), last_values.cpu().numpy(),
                           starts.cpu().numpy(), 0.95, 0.9)
        assert _bits_equal(buf.advantages.cpu().numpy(), adv) and _bits_equal(buf.returns.cpu().numpy(), ret)
        aug = torch.nn.Sequential(K.RandomAffine(degrees=0, translate=[0.05, 0.05], scale=[1.0, 1.0], p=0.5, seed=9))
        idx = np.random.default_rng(2).permutation(T * N)
        store = buf.observations["tactile"].cpu().numpy().reshape(T * N, 2, 128, 128)
        rows = flat_rows(idx, T, N)
        n = 0
        for k, batch in enumerate(buf.get(256, augment=aug, indices=torch.from_numpy(idx).cuda())):
            prm = torch.cat([aug[0]._params["batch_prob"].float()[:, None], aug[0]._params["translations"]], dim=1).cpu().numpy()
            sel = rows[256 * k:256 * k + 256]
            assert _bits_equal(batch.observations["tactile"].cpu().numpy(), warp_f32(store[sel], prm, True))
            assert _bits_equal(batch.advantages.cpu().numpy(), adv.reshape(-1)[sel])
            n += len(sel)
        assert n == T * N and aug[0].counter == 4
    finally:
        venv.close()


def test_object_push_rollout_end_to_end():
    tg, _ = _mods()
    T, N = 6, 8
    venv = tg.make_vec("object_push-v0", num_envs=N, max_steps=4, image_size=[64, 64], env_modes=PUSH, seed=2, obs_mode="torch")
    try:
        obs = venv.reset()
        buf = tg.DeviceRolloutBuffer.for_env(venv, T)
        assert set(buf.observations) == {"tactile", "extended_feature"} and buf._channels_first == {"tactile": False}
        g = torch.Generator(device="cuda").manual_seed(1)
        starts = torch.ones(N, dtype=torch.uint8, device="cuda")
        log = []
        for t in range(T):
            actions = (torch.rand((N, venv.act_dim), device="cuda", generator=g) - 0.5) * 0.5
            values, log_probs = torch.randn(N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g)
            clone = {k: v.clone() for k, v in obs.items()}
            buf.add(obs, actions, torch.zeros(N, device="cuda"), starts, values, log_probs)
            obs, _, _, _ = venv.step(actions)
            rewards, dones = venv.reward_done_torch()
            buf.rewards[t].copy_(rewards)
            log.append(dict(obs=clone, actions=actions.clone(), rewards=rewards.clone(), dones=dones.clone(), values=values, log_probs=log_probs))
            starts = dones.clone()
        dones = _check_env_rollout(buf, log, T)
        assert dones.any()
        buf.compute_returns_and_advantage(torch.zeros(N, device="cuda"), starts)
        idx = np.random.default_rng(3).permutation(T * N)
        got = list(buf.get(16, indices=torch.from_numpy(idx).cuda()))
        torch.cuda.synchronize()
        _check_batches(buf, got, idx, 16)
    finally:
        venv.close()
