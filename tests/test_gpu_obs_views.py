"""The zero-copy hand-out of obs_mode="torch" (DESIGN.md 4.19): every key of _observation() and _terminal_observation() is ONE tensor object
for the env's life, at the address the library's matching tg_get_* entry reports, in the observation space's shape; and forgetting the
caller-owned render targets (set_obs_targets([])) drops the views of those targets and no other.  The numpy side: tests/test_vec_env_cpu.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="oracle", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")
PUSH = dict(movement_mode="TyRz", control_mode="TCP_velocity_control", rand_init_orn=False, rand_obj_mass=False, traj_type="simplex",
            observation_mode="visuotactile_and_feature", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
N = 4


def _reported(venv, key, terminal):
    """The device address of `key`'s buffer as the library's own entry reports it."""
    from tactile_gym_amd import _capi
    L, ctx, p, dim, t = venv._L, venv._ctx, C.c_void_p(), C.c_int32(), int(terminal)
    if venv.frame_stack > 1 or (key == "visual" and venv.channels_first):
        rc = L.tg_get_obs_stack(ctx, _capi.OBS_STACK_KEY[key], t, C.byref(p))
    elif key == "tactile":
        rc = (L.tg_get_terminal_obs if terminal else L.tg_get_obs_tactile)(ctx, C.byref(p))
    elif key == "visual":
        rc = L.tg_get_obs_visual(ctx, C.byref(p), t)
    elif key == "extended_feature":
        rc = L.tg_get_obs_feature(ctx, C.byref(p), C.byref(dim), t)
    else:
        rc = L.tg_get_obs_oracle_terminal(ctx, C.byref(p)) if terminal else L.tg_get_obs_oracle(ctx, C.byref(p), C.byref(dim))
    assert rc == 0 and p.value
    return p.value


@pytest.mark.parametrize("frame_stack,channels_first", [(1, False), (2, False), (1, True), (2, True)])
@pytest.mark.parametrize("env_id,modes", [("object_push-v0", PUSH), ("edge_follow-v0", EDGE)], ids=["push_all_keys", "edge_oracle"])
def test_every_view_is_one_object_at_the_librarys_address(env_id, modes, frame_stack, channels_first):
    import torch
    import tactile_gym_amd as tg
    venv = tg.make_vec(env_id, num_envs=N, max_steps=2, image_size=[128, 128], env_modes=modes, seed=3, obs_mode="torch", frame_stack=frame_stack,
                       channels_first=channels_first)
    try:
        keys = list(venv.observation_space.spaces)
        assert keys == (["tactile", "visual", "extended_feature"] if modes is PUSH else ["oracle"])
        first, first_term = venv.reset(), venv._terminal_observation()
        actions = np.zeros((N, venv.act_dim), np.float32)

        def same_objects():
            obs, term = venv._observation(), venv._terminal_observation()
            assert list(obs) == keys and list(term) == keys
            for k in keys:
                assert obs[k] is first[k] and term[k] is first_term[k] and term[k] is not obs[k], k
                assert obs[k].data_ptr() == _reported(venv, k, False) and term[k].data_ptr() == _reported(venv, k, True), k
                assert tuple(obs[k].shape) == tuple(term[k].shape) == (N,) + tuple(venv.observation_space[k].shape), k
                assert obs[k].device == torch.device("cuda", 0) and obs[k].is_contiguous() and term[k].is_contiguous()

        same_objects()
        for _ in range(3):                           # max_steps=2: the envs finish and auto-reset on the way
            obs = venv.step(actions)[0]
            assert all(obs[k] is first[k] for k in keys)
            same_objects()
        others = (venv.reward_done_torch(), venv.packed_torch(), venv.actions_torch())
        venv.set_obs_targets([])                     # nothing to forget: every view stays
        same_objects()
        if "tactile" in keys and frame_stack == 1 and not channels_first:      # (the library takes render targets in this layout only)
            mine = [torch.zeros((N, 128, 128), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
            for buf in mine:                         # the second round: a view of the forgotten first target must not be handed out again
                venv.set_obs_targets([buf.data_ptr()])
                venv.select_obs_target(1)
                t1 = venv.tactile_torch()
                assert t1.data_ptr() == buf.data_ptr() and t1 is venv.tactile_torch() and venv._observation()["tactile"] is t1
                assert venv.tactile_torch(terminal=True) is first_term["tactile"]
                venv.set_obs_targets([])             # selects the context's own buffer again
                same_objects()
        now = (venv.reward_done_torch(), venv.packed_torch(), venv.actions_torch())
        assert now[0][0] is others[0][0] and now[0][1] is others[0][1] and now[1][0] is others[1][0] and now[1][1:] == others[1][1:] and now[2] is others[2]
    finally:
        venv.close()
