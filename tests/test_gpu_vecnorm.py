"""tg.DeviceVecNormalize on real envs (64 envs, 64 x 64 images, max_steps=6: every env resets inside a 20-step run): observations, rewards, terminal
observations, statistics and returns against tests/vecnorm_ref.py (device_order) fed by an identically seeded second env, bit for bit; image
keys passed through; reward normalisation alone; the replay buffer's sample(env=); training=False."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vecnorm_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="oracle", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")
ROLL = dict(movement_mode="xy", control_mode="TCP_velocity_control", rand_init_obj_pos=True, rand_obj_size=True, rand_embed_dist=True,
            observation_mode="tactile_and_feature", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
N = 64


def _make(env_id, modes, seed=3, **kw):
    import tactile_gym_amd as tg
    return tg, tg.make_vec(env_id, num_envs=N, max_steps=6, image_size=[64, 64], env_modes=modes, seed=seed, obs_mode="torch", **kw)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _host(obs, keys):
    return {k: obs[k].cpu().numpy() for k in keys}


def _assert_stats(vn, model, what):
    torch.cuda.synchronize()
    for k, rms in model.obs_rms.items():
        got = vn.obs_rms[k]
        assert _bits(got.mean.cpu().numpy(), rms.mean) and _bits(got.var.cpu().numpy(), rms.var) and got.count.item() == rms.count, (what, k)
    got = vn.ret_rms
    assert (got.mean.item(), got.var.item(), got.count.item()) == (model.ret_rms.mean, model.ret_rms.var, model.ret_rms.count), what
    assert _bits(vn.returns.cpu().numpy(), model.returns), what


def _actions(g, act_dim):
    return (torch.rand((N, act_dim), device="cuda", generator=g) - 0.5) * 0.5


def _run(vn, twin, model, keys, steps, g, first=0):
    """`steps` steps of the wrapper next to the restatement fed by the twin env's originals; -> number of terminal observations checked."""
    finished = 0
    for step in range(first, first + steps):
        a = _actions(g, vn.action_space.shape[0])
        obs, rew, dones, infos = vn.step(a)
        t_obs, t_rew, t_dones, t_infos = twin.step(a)
        term = _host(twin._terminal_observation(), keys)
        w_obs, w_rew, w_term = model.step(_host(t_obs, keys), t_rew, t_dones, term)
        assert np.array_equal(dones, t_dones) and _bits(rew, w_rew) and _bits(vn.get_original_reward(), t_rew), step
        assert _bits(vn.reward_done_torch()[0].cpu().numpy(), w_rew)
        for k in keys:
            assert _bits(obs[k].cpu().numpy(), w_obs[k]), (step, k)
            assert _bits(vn.get_original_obs()[k].cpu().numpy(), t_obs[k].cpu().numpy()), (step, k)
        for i in np.nonzero(dones)[0]:
            for k in keys:
                assert _bits(infos[i]["terminal_observation"][k].cpu().numpy(), w_term[k][i]), (step, i, k)
                assert _bits(t_infos[i]["terminal_observation"][k].cpu().numpy(), term[k][i])          # the twin's own: the original
            finished += 1
        _assert_stats(vn, model, step)
    return finished


def test_edge_follow_oracle_equals_the_restatement():
    tg, venv = _make("edge_follow-v0", EDGE)
    _, twin = _make("edge_follow-v0", EDGE)
    try:
        vn = tg.DeviceVecNormalize(venv, gamma=0.95)
        assert vn.norm_obs_keys == ["oracle"] and vn.venv is venv
        d = venv.observation_space.spaces["oracle"].shape[0]
        assert vn.observation_space.spaces["oracle"].shape == (d,) and float(vn.observation_space.spaces["oracle"].high[0]) == 10.0
        model = ref.device_order({"oracle": d}, N, gamma=0.95)
        obs = vn.reset()
        want = model.reset(_host(twin.reset(), ["oracle"]))
        assert _bits(obs["oracle"].cpu().numpy(), want["oracle"]) and obs["oracle"].data_ptr() != venv._observation()["oracle"].data_ptr()
        _assert_stats(vn, model, "reset")
        g = torch.Generator(device="cuda").manual_seed(1)
        assert _run(vn, twin, model, ["oracle"], 20, g) >= N                   # every env finished at least once
        # training=False after the run: everything stays frozen, the outputs still follow
        vn.training = model.training = False
        frozen = vn.state_dict()
        _run(vn, twin, model, ["oracle"], 10, g, first=20)
        for k, v in vn.state_dict().items():
            if k != "returns":
                assert _bits(v, frozen[k]), k
    finally:
        venv.close()
        twin.close()


def test_tactile_and_feature_passes_the_image_through():
    tg, venv = _make("object_roll-v0", ROLL, frame_stack=2, channels_first=True)
    _, twin = _make("object_roll-v0", ROLL, frame_stack=2, channels_first=True)
    try:
        vn = tg.DeviceVecNormalize(venv)
        d = venv.feature_dim
        assert vn.norm_obs_keys == ["extended_feature"] and vn.frame_stack == 2 and tuple(vn.obs_rms["extended_feature"].mean.shape) == (2 * d,)
        with pytest.raises(NotImplementedError, match="tactile"):
            tg.DeviceVecNormalize(venv, norm_obs_keys=["tactile"])
        model = ref.device_order({"extended_feature": 2 * d}, N)
        obs = vn.reset()
        want = model.reset(_host(twin.reset(), ["extended_feature"]))
        inner = venv._observation()
        assert obs["tactile"] is inner["tactile"] and obs["tactile"].data_ptr() == inner["tactile"].data_ptr()
        assert tuple(obs["tactile"].shape) == (N, 2, 64, 64) and _bits(obs["extended_feature"].cpu().numpy(), want["extended_feature"])
        g = torch.Generator(device="cuda").manual_seed(2)
        for step in range(8):
            a = _actions(g, vn.action_space.shape[0])
            obs, rew, dones, infos = vn.step(a)
            t_obs, t_rew, t_dones, _ = twin.step(a)
            w_obs, w_rew, w_term = model.step(_host(t_obs, ["extended_feature"]), t_rew, t_dones, _host(twin._terminal_observation(), ["extended_feature"]))
            assert obs["tactile"].data_ptr() == venv._observation()["tactile"].data_ptr() and torch.equal(obs["tactile"], t_obs["tactile"])
            assert _bits(obs["extended_feature"].cpu().numpy(), w_obs["extended_feature"]) and _bits(rew, w_rew), step
            for i in np.nonzero(dones)[0]:
                assert _bits(infos[i]["terminal_observation"]["extended_feature"].cpu().numpy(), w_term["extended_feature"][i])
                assert infos[i]["terminal_observation"]["tactile"].dtype == torch.uint8
            _assert_stats(vn, model, step)
    finally:
        venv.close()
        twin.close()


def test_tactile_mode_normalises_the_reward_only():
    tg, venv = _make("edge_follow-v0", dict(EDGE, observation_mode="tactile"))
    _, twin = _make("edge_follow-v0", dict(EDGE, observation_mode="tactile"))
    try:
        vn = tg.DeviceVecNormalize(venv)
        assert vn.norm_obs_keys == [] and vn.observation_space.spaces["tactile"] is venv.observation_space.spaces["tactile"]
        model = ref.device_order({}, N)
        assert vn.reset()["tactile"] is venv._observation()["tactile"]
        twin.reset()
        model.reset({})
        g = torch.Generator(device="cuda").manual_seed(3)
        for step in range(8):
            a = _actions(g, 2)
            obs, rew, dones, infos = vn.step(a)
            _, t_rew, t_dones, _ = twin.step(a)
            _, w_rew, _ = model.step({}, t_rew, t_dones)
            assert _bits(rew, w_rew) and obs["tactile"] is venv._observation()["tactile"], step
            _assert_stats(vn, model, step)
    finally:
        venv.close()
        twin.close()


def test_replay_sample_with_the_wrapper_equals_sample_then_normalize():
    import tactile_gym_amd.augment as K
    tg, venv = _make("object_roll-v0", ROLL, frame_stack=2, channels_first=True)
    try:
        vn = tg.DeviceVecNormalize(venv)
        ours, twin = tg.DeviceReplayBuffer.for_env(vn, 8 * N, seed=5), tg.DeviceReplayBuffer.for_env(venv, 8 * N, seed=5)
        assert ours._venv is venv                                                # the originals are stored
        obs = vn.reset()
        ours.start(vn.get_original_obs())
        twin.start(vn.get_original_obs())
        g = torch.Generator(device="cuda").manual_seed(4)
        for _ in range(10):
            a = _actions(g, vn.action_space.shape[0])
            vn.step(a)
            ours.add_from_env(a)
            twin.add_from_env(a)
        for name in ("rewards", "dones", "actions"):
            assert torch.equal(getattr(ours, name), getattr(twin, name))
        assert torch.equal(ours.observations["extended_feature"], twin.observations["extended_feature"])
        a, b = ours.sample(32, env=vn), twin.sample(32)
        for got, plain in ((a.observations, b.observations), (a.next_observations, b.next_observations)):
            want = vn.normalize_obs(plain)
            assert torch.equal(got["extended_feature"], want["extended_feature"]) and not torch.equal(got["extended_feature"], plain["extended_feature"])
            assert torch.equal(got["tactile"], plain["tactile"])
        assert torch.equal(a.rewards, vn.normalize_reward(b.rewards)) and torch.equal(a.actions, b.actions) and torch.equal(a.dones, b.dones)
        host = ref.device_order({"extended_feature": 2 * venv.feature_dim}, N)          # ... and normalize_obs itself is the restatement's
        sd = vn.state_dict()
        rms = host.obs_rms["extended_feature"]
        rms.mean, rms.var, rms.count = sd["obs_rms.extended_feature.mean"], sd["obs_rms.extended_feature.var"], sd["obs_rms.extended_feature.count"]
        host.ret_rms.var = sd["ret_rms.var"]
        assert _bits(a.observations["extended_feature"].cpu().numpy(),
                     host.normalize_obs({"extended_feature": b.observations["extended_feature"].cpu().numpy()})["extended_feature"])
        assert _bits(a.rewards.cpu().numpy(), host.normalize_reward(b.rewards.cpu().numpy()))
        aug1, aug2 = K.RandomTranslate(translate=(0.1, 0.1), p=0.5, seed=7), K.RandomTranslate(translate=(0.1, 0.1), p=0.5, seed=7)
        a, b = ours.sample(32, env=vn, augment=aug1), twin.sample(32, augment=aug2)
        assert torch.equal(a.observations["tactile"], b.observations["tactile"]) and torch.equal(a.next_observations["tactile"], b.next_observations["tactile"])
        assert torch.equal(a.observations["extended_feature"], vn.normalize_obs(b.observations)["extended_feature"])
        with pytest.raises(NotImplementedError, match="VecNormalize"):
            ours.sample(32, env=object())
        rollout = tg.DeviceRolloutBuffer.for_env(vn, 4)                          # stores what the wrapper hands out
        assert rollout.n_envs == N and tuple(rollout.observations["extended_feature"].shape) == (4, N, 2 * venv.feature_dim)
    finally:
        venv.close()
