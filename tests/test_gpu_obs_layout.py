"""channels_first=True (VecTransposeImage on the device; tg_set_obs_layout, csrc/tg_stack.hip: k_obs_stack) and the visual frame stacks against
stable_baselines3's VecTransposeImage(VecFrameStack(venv, n)).

Method (as tests/test_gpu_frame_stack.py): the same env, seed and actions run once with frame_stack=1, channels_first=False and once with the
option under test; the numpy restatement (obs_layout_ref.expected_layout) applied to the first run's observations and terminal observations must
give the second run's observations, reset observations and terminal observations byte for byte, with identical rewards and dones, at every step."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from frame_stack_ref import digest, rollout  # noqa: E402
from obs_layout_ref import expected_layout, is_image_space, is_image_space_channels_first  # noqa: E402

pytestmark = pytest.mark.gpu

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")
BAL = dict(movement_mode="xy", control_mode="TCP_velocity_control", object_mode="pole", rand_gravity=True, rand_embed_dist=True,
           observation_mode="tactile", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
PUSH = dict(movement_mode="TyRz", control_mode="TCP_velocity_control", rand_init_orn=False, rand_obj_mass=False, traj_type="simplex",
            observation_mode="visuotactile_and_feature",
            reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(single, got, n, channels_first, auto_reset=True):
    exp = expected_layout(single, n, channels_first)
    assert len(exp) == len(got)
    partial = 0
    for t, (e, g) in enumerate(zip(exp, got)):
        assert e[0] == g[0]
        assert sorted(e[2]) == sorted(g[2]), t
        for k in e[2]:
            assert _same(e[2][k], g[2][k]), (t, e[0], k, e[2][k].shape, g[2][k].shape)
        if e[0] == "step":
            assert _same(e[3], g[3]) and _same(e[4], g[4]), t          # rewards, dones
            done = e[4].astype(bool)
            partial += int(0 < done.sum() < len(done))
            assert sorted(e[5]) == sorted(g[5]), t
            if auto_reset:
                assert sorted(g[5]) == np.nonzero(done)[0].tolist(), t
            else:
                assert not g[5]
            for i in e[5]:
                assert sorted(e[5][i]) == sorted(g[5][i])
                for k in e[5][i]:
                    assert _same(e[5][i][k], g[5][i][k]), (t, i, k)
    return partial


def _pair(env_id, num_envs, n, channels_first, auto_reset=True, **kw):
    single = rollout(env_id, num_envs, 1, auto_reset=auto_reset, **kw)
    got = rollout(env_id, num_envs, n, auto_reset=auto_reset, channels_first=channels_first, **kw)
    return single, got, _check(single, got, n, channels_first, auto_reset)


@pytest.mark.parametrize("obs_mode", ["torch", "numpy"])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_edge_follow_tactile_1024_channels_first(n, obs_mode):
    _, got, partial = _pair("edge_follow-v0", 1024, n, True, env_modes=EDGE, obs_mode=obs_mode, steps=10, reset_bank="sync")
    assert got[0][2]["tactile"].shape == (1024, n, 128, 128)
    assert partial > 0                                               # steps in which some, not all, envs finished


def test_rewrite_all_switch_changes_no_byte_channels_first():
    """TG_STACK_REWRITE_ALL=1 (read once per process: a child) turns the unchanged-block skip of the planar stack off; the bytes must not change."""
    kw = dict(env_modes=EDGE, steps=10, reset_bank="sync", obs_mode="torch", channels_first=True)
    here = digest(rollout("edge_follow-v0", 1024, 2, **kw))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); from frame_stack_ref import rollout, digest; "
            "print(digest(rollout('edge_follow-v0', 1024, 2, **%r)))" % (HERE, os.path.dirname(HERE), kw))
    env = dict(os.environ, TG_STACK_REWRITE_ALL="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == here


@pytest.mark.parametrize("channels_first", [False, True])
@pytest.mark.parametrize("n", [2, 3])
def test_edge_follow_visuotactile_stack(n, channels_first):
    modes = dict(EDGE, observation_mode="visuotactile")
    _, got, partial = _pair("edge_follow-v0", 64, n, channels_first, env_modes=modes, steps=12, reset_bank="sync")
    assert got[0][2]["visual"].shape == ((64, 3 * n, 128, 128) if channels_first else (64, 128, 128, 3 * n))
    assert got[0][2]["tactile"].shape == ((64, n, 128, 128) if channels_first else (64, 128, 128, n))
    assert partial > 0


@pytest.mark.parametrize("obs_mode", ["torch", "numpy"])
def test_edge_follow_visual_n1_channels_first(obs_mode):
    _, got, partial = _pair("edge_follow-v0", 64, 1, True, env_modes=dict(EDGE, observation_mode="visual"), obs_mode=obs_mode, steps=12,
                            reset_bank="sync")
    assert got[0][2]["visual"].shape == (64, 3, 128, 128)
    assert partial > 0


def test_object_push_all_key_kinds_channels_first():
    """tactile (planar stack), visual and extended_feature in one k_obs_stack launch."""
    _, got, partial = _pair("object_push-v0", 24, 2, True, env_modes=PUSH, steps=12, max_steps=6, obs_mode="torch")
    o = got[0][2]
    assert o["tactile"].shape == (24, 2, 128, 128) and o["visual"].shape == (24, 6, 128, 128) and o["extended_feature"].shape == (24, 24)
    assert partial > 0


def test_object_balance_tactile_channels_first():
    _, _, partial = _pair("object_balance-v0", 24, 2, True, env_modes=BAL, steps=14, max_steps=6)
    assert partial > 0


@pytest.mark.parametrize("modes", [EDGE, dict(EDGE, observation_mode="visuotactile")])
def test_no_auto_reset_channels_first(modes):
    _, _, partial = _pair("edge_follow-v0", 16, 3, True, auto_reset=False, env_modes=modes, steps=12, reset_bank="sync")
    assert partial > 0


def test_copy_obs_false_channels_first():
    _pair("edge_follow-v0", 16, 2, True, env_modes=dict(EDGE, observation_mode="visuotactile"), steps=8, reset_bank="sync", copy_obs=False)


def test_spaces_contiguity_and_render():
    import tactile_gym_amd as tg
    v = tg.make_vec("edge_follow-v0", num_envs=4, max_steps=50, image_size=[128, 128], env_modes=dict(EDGE, observation_mode="visuotactile"), seed=2,
                    obs_mode="torch", frame_stack=2, channels_first=True)
    try:
        for k, shape in (("tactile", (2, 128, 128)), ("visual", (6, 128, 128))):
            sp = v.observation_space[k]
            assert tuple(sp.shape) == shape and is_image_space(sp) and is_image_space_channels_first(sp)
        obs = v.reset()
        obs, _, _, _ = v.step(np.zeros((4, v.act_dim), np.float32))
        for k in ("tactile", "visual"):
            assert obs[k].is_contiguous() and tuple(obs[k].shape) == (4,) + tuple(v.observation_space[k].shape)
        imgs = v.get_images()                                        # render() keeps the unstacked frame
        assert imgs[0].shape == (128, 256, 3)
        assert np.array_equal(imgs[1][:, :128], v.visual_numpy()[1])
    finally:
        v.close()


def test_tactile_n1_channels_first_is_the_observation_buffer():
    import ctypes as C
    import tactile_gym_amd as tg
    v = tg.make_vec("edge_follow-v0", num_envs=8, max_steps=5, image_size=[128, 128], env_modes=EDGE, seed=2, obs_mode="torch", channels_first=True)
    try:
        obs = v.reset()
        assert tuple(obs["tactile"].shape) == (8, 1, 128, 128) and obs["tactile"].is_contiguous()
        assert obs["tactile"].data_ptr() == v.tactile_device_ptr()          # no copy, no stack allocated
        for _ in range(6):
            obs, _, done, infos = v.step(np.zeros((8, v.act_dim), np.float32))
            assert obs["tactile"].data_ptr() == v.tactile_device_ptr()
        n, cf, p = C.c_int32(), C.c_int32(), C.c_void_p()
        assert v._L.tg_get_frame_stack(v._ctx, C.byref(n)) == 0 and n.value == 1
        assert v._L.tg_get_obs_layout(v._ctx, C.byref(cf)) == 0 and cf.value == 1
        assert v._L.tg_get_obs_stack(v._ctx, 0, 0, C.byref(p)) == 0 and p.value == v.tactile_device_ptr()
        assert v._L.tg_get_obs_stack(v._ctx, 3, 0, C.byref(p)) != 0           # no visual key: no visual stack
    finally:
        v.close()


def test_hipvecenv_make_vec_env_route():
    """make_vec_env(..., vec_env_cls=HipVecEnv, vec_env_kwargs=dict(frame_stack=n, channels_first=True)) is the same env as make_vec with the options."""
    import tactile_gym_amd as tg
    from test_host_cpu import sb3_like_make_vec_env
    modes = dict(EDGE, observation_mode="visuotactile")
    a = sb3_like_make_vec_env("edge_follow-v0", n_envs=6, seed=3, env_kwargs=dict(env_modes=modes, image_size=[128, 128], max_steps=5),
                              vec_env_cls=tg.HipVecEnv, vec_env_kwargs=dict(frame_stack=2, channels_first=True))
    b = tg.make_vec("edge_follow-v0", num_envs=6, max_steps=5, image_size=[128, 128], env_modes=modes, seed=3, frame_stack=2, channels_first=True)
    try:
        assert a.frame_stack == 2 and a.channels_first
        assert tuple(a.observation_space["visual"].shape) == (6, 128, 128)
        oa, ob = a.reset(), b.reset()
        rng = np.random.default_rng(0)
        for _ in range(8):
            for k in ob:
                assert _same(oa[k], ob[k]), k
            act = rng.uniform(-1, 1, size=(6, a.act_dim)).astype(np.float32)
            oa, ra, da, ia = a.step(act)
            ob, rb, db, ib = b.step(act)
            assert _same(ra, rb) and _same(da, db)
            for i in np.nonzero(da)[0]:
                for k in ob:
                    assert _same(ia[i]["terminal_observation"][k], ib[i]["terminal_observation"][k])
    finally:
        a.close(); b.close()


def test_sharded_render_targets_refused():
    import tactile_gym_amd as tg
    import torch
    v = tg.make_vec("edge_follow-v0", num_envs=4, max_steps=50, image_size=[128, 128], env_modes=EDGE, seed=2, channels_first=True)
    try:
        buf = torch.zeros((4, 128, 128), dtype=torch.uint8, device="cuda:0")
        with pytest.raises(Exception, match="channels-first"):
            v.set_obs_targets([buf.data_ptr()])
    finally:
        v.close()


def test_obs_guard_covers_the_visual_stack():
    import tactile_gym_amd as tg
    v = tg.make_vec("edge_follow-v0", num_envs=4, max_steps=50, image_size=[128, 128], env_modes=dict(EDGE, observation_mode="visual"), seed=2,
                    obs_mode="torch", channels_first=True)
    try:
        v.set_obs_guard(True)
        obs = v.reset()
        obs["visual"][0, 0, 0, 0] ^= 1
        with pytest.raises(RuntimeError):
            v.step(np.zeros((4, v.act_dim), np.float32))
    finally:
        v.close()
