"""The device frame stack (frame_stack=n; tg_set_frame_stack, csrc/tg_stack.hip) against stable_baselines3's VecFrameStack semantics.

Method: the same env, seed and actions run once with frame_stack=1 and once with frame_stack=n; the numpy restatement (frame_stack_ref.StackRef)
applied to the first run's observations and terminal observations must give the second run's stacked observations and terminal stacks byte for
byte, with identical rewards and dones, at every reset and step."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from frame_stack_ref import digest, expected_from_single, rollout  # noqa: E402

pytestmark = pytest.mark.gpu

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")
BAL = dict(movement_mode="xy", control_mode="TCP_velocity_control", object_mode="pole", rand_gravity=True, rand_embed_dist=True,
           observation_mode="tactile", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
SURF = dict(movement_mode="xyzRxRy", control_mode="TCP_velocity_control", noise_mode="simplex", observation_mode="oracle", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="digit")
ROLL = dict(movement_mode="xy", control_mode="TCP_velocity_control", rand_init_obj_pos=True, rand_obj_size=True, rand_embed_dist=True,
            observation_mode="tactile_and_feature", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(single, stacked, n, auto_reset=True):
    exp = expected_from_single(single, n)
    assert len(exp) == len(stacked)
    partial = 0
    for t, (e, g) in enumerate(zip(exp, stacked)):
        assert e[0] == g[0]
        obs_e, obs_g = e[2], g[2]
        assert sorted(obs_e) == sorted(obs_g), t
        for k in obs_e:
            assert _same(obs_e[k], obs_g[k]), (t, e[0], k, int((obs_e[k] != obs_g[k]).sum()))
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
                for k in e[5][i]:
                    assert _same(e[5][i][k], g[5][i][k]), (t, i, k)
    return partial


@pytest.mark.parametrize("obs_mode", ["numpy", "torch"])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_edge_follow_stack_matches_vecframestack(n, obs_mode):
    kw = dict(env_modes=EDGE, obs_mode=obs_mode, steps=14, reset_bank="sync")
    single = rollout("edge_follow-v0", 24, 1, **kw)
    stacked = rollout("edge_follow-v0", 24, n, **kw)
    assert stacked[0][2]["tactile"].shape == (24, 128, 128, n)
    assert _check(single, stacked, n) > 0                         # steps in which some, not all, envs finished


def test_edge_follow_1024_envs():
    kw = dict(env_modes=EDGE, obs_mode="torch", steps=10, reset_bank="sync")
    single = rollout("edge_follow-v0", 1024, 1, **kw)
    stacked = rollout("edge_follow-v0", 1024, 2, **kw)
    assert _check(single, stacked, 2) > 0


def test_edge_follow_no_auto_reset():
    kw = dict(env_modes=EDGE, steps=12, auto_reset=False, reset_bank="sync")
    single = rollout("edge_follow-v0", 16, 1, **kw)
    stacked = rollout("edge_follow-v0", 16, 3, **kw)
    assert _check(single, stacked, 3, auto_reset=False) > 0


def test_object_balance_pole_stack():
    kw = dict(env_modes=BAL, steps=14, max_steps=6)
    single = rollout("object_balance-v0", 24, 1, **kw)
    stacked = rollout("object_balance-v0", 24, 2, **kw)
    assert _check(single, stacked, 2) > 0


@pytest.mark.parametrize("mode", ["oracle", "tactile_and_feature"])
def test_surface_follow_goal_stack(mode):
    kw = dict(env_modes=dict(SURF, observation_mode=mode), steps=12, max_steps=6, reset_bank="sync")
    single = rollout("surface_follow-v1", 12, 1, **kw)
    stacked = rollout("surface_follow-v1", 12, 2, **kw)
    keys = sorted(stacked[0][2])
    assert keys == (["oracle"] if mode == "oracle" else ["extended_feature", "tactile"])
    if mode == "oracle":
        assert stacked[0][2]["oracle"].shape == (12, 40)
    else:
        assert stacked[0][2]["extended_feature"].shape == (12, 12)
    assert _check(single, stacked, 2) > 0


def test_object_roll_feature_stack():
    kw = dict(env_modes=ROLL, steps=12, max_steps=6, obs_mode="torch")
    single = rollout("object_roll-v0", 12, 1, **kw)
    stacked = rollout("object_roll-v0", 12, 2, **kw)
    assert stacked[0][2]["extended_feature"].shape == (12, 6)
    assert _check(single, stacked, 2) > 0


def test_rewrite_all_switch_changes_no_byte():
    """TG_STACK_REWRITE_ALL=1 (read once per process: a child) turns the unchanged-block skip off; the bytes must not change."""
    kw = dict(env_modes=EDGE, steps=14, reset_bank="sync")
    here = digest(rollout("edge_follow-v0", 24, 3, **kw))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); from frame_stack_ref import rollout, digest; "
            "print(digest(rollout('edge_follow-v0', 24, 3, env_modes=%r, steps=14, reset_bank='sync')))" % (HERE, os.path.dirname(HERE), EDGE))
    env = dict(os.environ, TG_STACK_REWRITE_ALL="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == here


def test_frame_stack_1_is_the_plain_env():
    import tactile_gym_amd as tg
    kw = dict(num_envs=8, max_steps=5, image_size=[128, 128], env_modes=EDGE, seed=2, obs_mode="torch")
    a = tg.make_vec("edge_follow-v0", frame_stack=1, **kw)
    b = tg.make_vec("edge_follow-v0", **kw)
    try:
        for v in (a, b):
            assert v.observation_space["tactile"].shape == (128, 128, 1)
        oa, ob = a.reset(), b.reset()
        assert oa["tactile"].data_ptr() == a.tactile_device_ptr()        # the library's own buffer, as without the option
        rng = np.random.default_rng(0)
        for _ in range(8):
            act = rng.uniform(-1, 1, size=(8, a.act_dim)).astype(np.float32)
            oa, ra, da, _ = a.step(act)
            ob, rb, db, _ = b.step(act)
            assert oa["tactile"].data_ptr() == a.tactile_device_ptr()
            assert _same(oa["tactile"].cpu().numpy(), ob["tactile"].cpu().numpy()) and _same(ra, rb) and _same(da, db)
        import ctypes as C
        n = C.c_int32()
        assert a._L.tg_get_frame_stack(a._ctx, C.byref(n)) == 0 and n.value == 1
        assert a._L.tg_get_obs_stack(a._ctx, 0, 0, C.byref(C.c_void_p())) != 0          # nothing allocated
    finally:
        a.close(); b.close()


def test_obs_guard_covers_the_stack():
    import tactile_gym_amd as tg
    v = tg.make_vec("edge_follow-v0", num_envs=4, max_steps=50, image_size=[128, 128], env_modes=EDGE, seed=2, obs_mode="torch", frame_stack=2)
    try:
        v.set_obs_guard(True)
        obs = v.reset()
        obs["tactile"][0, 0, 0, 0] ^= 1                                 # in-place write into the handed-out stack
        with pytest.raises(RuntimeError):
            v.step(np.zeros((4, v.act_dim), np.float32))
    finally:
        v.close()


def test_sharded_render_targets_refused():
    import tactile_gym_amd as tg
    import torch
    v = tg.make_vec("edge_follow-v0", num_envs=4, max_steps=50, image_size=[128, 128], env_modes=EDGE, seed=2, frame_stack=2)
    try:
        buf = torch.zeros((4, 128, 128), dtype=torch.uint8, device="cuda:0")
        with pytest.raises(Exception, match="frame stack"):
            v.set_obs_targets([buf.data_ptr()])
    finally:
        v.close()
