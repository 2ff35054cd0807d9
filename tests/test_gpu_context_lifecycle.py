"""A context's device memory has one owner (tg_ctx::dev_allocs, csrc/tg_ctx.hpp): what tg_create refuses leaves nothing behind, what a context
allocated - at creation or later, by any optional feature - goes back with tg_destroy, and a set-up that fails half way leaves a context that works."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")
SURF = dict(movement_mode="xyzRxRy", control_mode="TCP_velocity_control", noise_mode="simplex", observation_mode="tactile", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="digit")
PUSH = dict(movement_mode="TyRz", control_mode="TCP_velocity_control", rand_init_orn=False, rand_obj_mass=False, traj_type="simplex",
            observation_mode="tactile_and_feature", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
ROLL = dict(movement_mode="xy", control_mode="TCP_velocity_control", rand_init_obj_pos=True, rand_obj_size=True, rand_embed_dist=True,
            observation_mode="tactile_and_feature", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
BAL = dict(movement_mode="xy", control_mode="TCP_velocity_control", object_mode="pole", rand_gravity=True, rand_embed_dist=True,
           observation_mode="tactile", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
SPIN = dict(BAL, movement_mode="xyRxRy", object_mode="spinning_plate", rand_embed_dist=False)

# kind -> (env id, env_modes, extra make_vec arguments)
KINDS = {
    "edge_follow": ("edge_follow-v0", EDGE, {}),
    "surface_follow": ("surface_follow-v0", SURF, {}),
    "object_push_gjk": ("object_push-v0", PUSH, dict(narrowphase="gjk_manifold")),
    "object_roll": ("object_roll-v0", ROLL, {}),
    "balance_pole": ("object_balance-v0", BAL, {}),
    "balance_ball_on_plate": ("object_balance-v0", dict(BAL, object_mode="ball_on_plate"), {}),
    "balance_spinning_plate": ("object_balance-v0", SPIN, {}),
}
# env kind -> (build_config's module, env id, modes, the tg_config field build_env_const rejects, its value, a piece of its message)
REJECTED = {
    "edge_follow": ("edge_follow", "edge_follow-v0", EDGE, "movement_mode", 99, "Incorrect movement mode"),
    "surface_follow": ("surface_follow", "surface_follow-v0", SURF, "surf_rows", 1, "heightfield needs at least 2x2"),
    "object_push": ("object_push", "object_push-v0", PUSH, "traj_n_points", 1, "traj_n_points"),
    "object_roll": ("object_roll", "object_roll-v0", ROLL, "tip_link", -1, "tip_link out of range"),
    "object_balance": ("object_balance", "object_balance-v0", BAL, "obj_mass", 0.0, "object mass must be positive"),
}


def _actions(v, rng):
    return rng.uniform(v.action_space.low, v.action_space.high, size=(v.num_envs, v.act_dim)).astype(np.float32)


@pytest.mark.parametrize("kind", sorted(REJECTED))
def test_rejected_after_validation_usable_after(kind):
    """tg_create with a configuration that build_env_const rejects (as a C caller of the ABI may hand one over: the Python build_config functions catch
    these values first): -1, the check's own message, a null context - and the library is as usable as before: a valid context made straight after
    steps three times and closes."""
    import importlib
    import tactile_gym_amd as tg
    from tactile_gym_amd import _capi
    module, env_id, modes, field, value, message = REJECTED[kind]
    built = importlib.import_module(f"tactile_gym_amd.rl_envs.{module}").build_config(8, 10, [128, 128], modes)
    cfg, robot, sensor = built[:3]
    mesh = None if kind == "surface_follow" else built[3]
    setattr(cfg, field, value)
    L = _capi.lib()
    ctx = C.c_void_p(0xdead)
    rc = L.tg_create(C.byref(cfg), C.byref(robot), C.byref(sensor.struct), C.byref(mesh.struct) if mesh is not None else None, C.byref(ctx))
    assert rc == -1 and message in L.tg_last_error().decode() and not ctx.value, (rc, L.tg_last_error(), ctx.value)
    v = tg.make_vec(env_id, num_envs=8, max_steps=10, image_size=[128, 128], env_modes=modes, seed=1)
    rng = np.random.default_rng(0)
    v.reset()
    for _ in range(3):
        obs, rew, done, _ = v.step(_actions(v, rng))
        assert np.isfinite(rew).all()
    v.close()


def _full_cycle(env_id, modes, extra, targets, cycle):
    """One context with everything switched on that allocates, a few steps, close()."""
    import tactile_gym_amd as tg
    from tactile_gym_amd import _capi
    feature = "_and_feature" if "feature" in modes["observation_mode"] else ""
    v = tg.make_vec(env_id, num_envs=1024, max_steps=3, image_size=[128, 128], env_modes=dict(modes, observation_mode="visuotactile" + feature), seed=3 + cycle,
                    frame_stack=4, channels_first=True, **extra)                     # scene, tactile / visual / feature stacks, (reset bank)
    L, ctx = v._L, v._ctx
    rng = np.random.default_rng(cycle)
    v.profile("clock")                                                                # the kernels' clock slots
    v.set_broadphase_guard(True)                                                      # the guard's scene and hulls, installed a second time
    v.reset()
    # render targets of the caller: only without stacks - they are given back (and allocated again below) while the context lives
    _capi.check(L.tg_set_frame_stack(ctx, 1))
    _capi.check(L.tg_set_obs_layout(ctx, 0))
    v.set_obs_targets([t.data_ptr() for t in targets])
    for k in (1, 2, 1):
        v.select_obs_target(k)
        v.step_random_async(seed=11, restart=(k == 1))                                # the draw counter
    v.sync()
    v.select_obs_target(0)
    v.set_obs_targets([])
    _capi.check(L.tg_set_obs_layout(ctx, 1))
    _capi.check(L.tg_set_frame_stack(ctx, 4))
    v.reset()
    finished = []
    for _ in range(4):
        obs, rew, done, infos = v.step(_actions(v, rng))
        finished = np.nonzero(done)[0] if done.any() else finished
    assert len(finished) > 0                                                          # max_steps = 3: every env has finished an episode
    assert v.oracle_obs().shape[0] == 1024                                            # the oracle vectors
    assert v._image_rows(finished[:3], visual=False).shape == (min(3, len(finished)), 128, 128, 1)   # the pinned staging block
    v.close()
    del v
    gc.collect()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_optional_buffer_goes_back(kind):
    """Six contexts in a row, 1024 envs at 128 x 128, each with every optional allocation in use (scene camera, frame_stack = 4 channels first - dropped
    and made again -, oracle observation, a re-installed broadphase guard, tg_step_random's counter, the profiling clock's slots, two render targets
    with their changed-block records, the reset bank or reset template, the pinned row block): after close() the device's free memory
    (torch.cuda.mem_get_info, synchronised) of cycles 2 ... 6 is not below that of cycle 1 by one tactile batch, n * H * W = 16 MiB.  That is the
    smallest buffer class this test can see through the runtime's allocation granularity - a bound from the buffer sizes, not a measured one; the
    per-env vectors of a few KB are below it and are covered by the single owner (every allocation is on the list tg_destroy frees), not by
    this measurement."""
    import torch
    env_id, modes, extra = KINDS[kind]
    targets = [torch.zeros((1024, 128, 128), dtype=torch.uint8, device="cuda") for _ in range(2)]
    free = []
    for cycle in range(6):
        _full_cycle(env_id, modes, extra, targets, cycle)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print(f"{kind}: free device memory after close(), MiB, cycles 1..6: " + " ".join(f"{f / 2**20:.1f}" for f in free))
    batch = 1024 * 128 * 128
    for f in free[1:]:
        assert free[0] - f < batch, [x / 2**20 for x in free]


def test_failed_scene_setup_leaves_a_working_context():
    """tg_set_scene refused (a tri_frame out of range) returns -1 and leaves no scene; the correct scene set on the same context afterwards renders,
    and renders what a context that never saw the failure renders."""
    import tactile_gym_amd as tg
    from tactile_gym_amd.robot_model import SceneDesc

    def make():
        v = tg.make_vec("edge_follow-v0", num_envs=4, max_steps=50, image_size=[128, 128], env_modes=EDGE, seed=2)
        v.reset()
        return v

    v, ref = make(), make()
    sp = v._scene_spec
    bad = SceneDesc(sp["arm_type"], v._sensor.t_s_type, v._sensor.t_s_name, v._robot.ndof, (v.H, v.W), sp["camera"], (v._mesh.verts, v._mesh.tris))
    bad.tri_frame[len(bad.tri_frame) // 2] = 200
    assert v._L.tg_set_scene(v._ctx, C.byref(bad.struct)) == -1
    assert "tri_frame out of range" in v._L.tg_last_error().decode()
    got, want = np.stack(v.get_images()), np.stack(ref.get_images())      # sets the scene, draws it
    assert got.shape == (4, 128, 256, 3) and got[:, :, :128].std() > 0     # the scene camera's half shows the arm on its background
    assert got.tobytes() == want.tobytes()
    v.close()
    ref.close()
