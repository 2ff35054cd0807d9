"""object_balance-v0 with object_mode "spinning_plate" on the HIP path (csrc/tg_spin.hip) against the oracle (oracle/minibullet.c: mb_step_spin,
oracle/ref_env.py; reference: object_balance_env.py:107-108, 198-239, 267-269, 355-358, PARITY A41): the wave-mapped hull - hull GJK / EPA bit
for bit, then whole episodes - reset draws, reset ticks, joint angles, spool and dish poses, contact count and impulse, reward / done, the
tactile image (the spool's underside), the oracle observation (the dish)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "tactile_gym_amd", "assets", "objects")
SPIN_MODES = dict(movement_mode="xyRxRy", control_mode="TCP_velocity_control", object_mode="spinning_plate", rand_gravity=True, rand_embed_dist=False,
                  observation_mode="tactile", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")


def _rot(ax, ang):
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def test_device_hull_hull_gjk_epa_equals_oracle_bit_for_bit():
    from oracle import minibullet as mb
    from tactile_gym_amd import _capi
    dish = np.ascontiguousarray(np.load(os.path.join(OBJ, "spinning_plate.npz"))["hull"], dtype=np.float64)
    spool = np.ascontiguousarray(np.load(os.path.join(OBJ, "plate_buffer.npz"))["hull"], dtype=np.float64)
    n = 600
    rng = np.random.default_rng(11)
    cases = np.zeros((n, dish.shape[0], 3))
    for t in range(n):
        if t % 2:        # the env's neighbourhood: over the spindle, a little apart or a little inside
            R = _rot(rng.normal(size=3), rng.uniform(0, 0.6))
            off = np.array([rng.normal() * 0.004, rng.normal() * 0.004, 0.0125 + 0.009847 + rng.uniform(-0.003, 0.003)])
        else:
            R = _rot(rng.normal(size=3), rng.uniform(0, np.pi))
            p = rng.normal(size=3)
            off = p / np.linalg.norm(p) * rng.uniform(0.0, 0.11)
        cases[t] = dish @ R.T + off
    dp = C.POINTER(C.c_double)
    dev = np.zeros((n, 11))
    assert 0 == _capi.test_lib().tg_selftest_narrowphase_hulls(n, dish.shape[0], cases.ctypes.data_as(dp), spool.shape[0], spool.ctypes.data_as(dp),
                                                               dev.ctypes.data_as(dp))
    L = mb.lib()
    ref = np.zeros((n, 11))
    for t in range(n):
        sd = C.c_double(); nn = (C.c_double * 3)(); pa = (C.c_double * 3)(); pb = (C.c_double * 3)()
        ok = L.mb_gjk_epa_hull_hull(cases[t].ctypes.data_as(dp), dish.shape[0], spool.ctypes.data_as(dp), spool.shape[0], C.byref(sd), nn, pa, pb)
        ref[t] = [ok, sd.value] + list(nn) + list(pa) + list(pb) if ok else [0] + [0.0] * 10
    assert (ref[:, 0] == 1).all() and (dev[:, 0] == 1).all()
    sep, pen = int((ref[:, 1] > 0).sum()), int((ref[:, 1] < 0).sum())
    assert sep > 100 and pen > 100, (sep, pen)
    same = dev.view(np.uint64) == ref.view(np.uint64)
    assert same.all(), (int((~same).any(axis=1).sum()), np.abs(dev - ref).max())


def _compare(venv, oracles, obs, ref, st, tag, q_tol=1e-8, pose_tol=1e-6):
    for i, o in enumerate(oracles):
        d = st["dish_state"][i]
        pos, R = o.body_pose()
        spos, sR = o.stimulus_pose()
        assert np.abs(st["q"][i] - o.arm.q).max() < q_tol, (tag, i, np.abs(st["q"][i] - o.arm.q).max())
        assert np.abs(st["body_pos"][i] - spos).max() < pose_tol and np.abs(st["body_rot"][i] - sR).max() < pose_tol, (tag, i, "spool")
        assert np.abs(d[0:3] - pos).max() < pose_tol and np.abs(d[3:12].reshape(3, 3) - R).max() < pose_tol, (tag, i, "dish", np.abs(d[0:3] - pos).max())
        assert np.abs(d[12:15] - np.array(o.spin.dish.linvel[:])).max() < 1e-5 and np.abs(d[15:18] - np.array(o.spin.dish.angvel[:])).max() < 1e-4, (tag, i, "dish velocity")
        assert int((obs["tactile"][i] != ref[i]["tactile"]).sum()) <= 3, (tag, i, int((obs["tactile"][i] != ref[i]["tactile"]).sum()))


@pytest.mark.parametrize("size,movement", [(128, "xyRxRy"), (64, "RxRy")])
def test_spinning_plate_matches_oracle(size, movement):
    """Two consecutive episodes, 6 envs vs 6 oracle envs, random actions: everything the env reports and the state behind it."""
    import tactile_gym_amd as tg
    from oracle.ref_env import OracleObjectBalanceEnv
    n, steps = 6, 14
    modes = dict(SPIN_MODES, movement_mode=movement)
    act_dim = {"RxRy": 2, "xyRxRy": 4}[movement]
    venv = tg.make_vec("object_balance-v0", num_envs=n, max_steps=steps, image_size=[size, size], env_modes=modes, seed=271, auto_reset=False)
    oracles = [OracleObjectBalanceEnv(seed=271 + i, max_steps=steps, image_size=(size, size), env_modes=modes) for i in range(n)]
    rng = np.random.default_rng(272)
    touched = 0
    for episode in range(2):
        obs = venv.reset()
        ref = [o.reset() for o in oracles]
        st = venv.get_state()
        for i, o in enumerate(oracles):
            assert st["gravity_z"][i] == o.gravity and st["embed_dist"][i] == o.embed_dist
            assert st["reset_ticks"][i] == o.reset_ticks
            assert np.abs(st["body_pos"][i] - o.init_buffer_pos).max() < 1e-15
            assert np.abs(st["dish_state"][i][0:3] - o.init_obj_pos).max() < 1e-15
        _compare(venv, oracles, obs, ref, st, ("reset", episode))
        for step in range(steps):
            a = rng.uniform(-0.25, 0.25, size=(n, act_dim)).astype(np.float32)
            obs, rew, done, _ = venv.step(a)
            st = venv.get_state()
            ref = []
            for i, o in enumerate(oracles):
                ro, rr, rd, _ = o.step(a[i])
                ref.append(ro)
                assert rew[i] == rr and bool(done[i]) == rd, (episode, step, i)
                assert int(st["dish_state"][i][19]) == o.spin.n_contacts, (episode, step, i, st["dish_state"][i][19], o.spin.n_contacts)
                assert abs(st["dish_state"][i][18] - o.spin.normal_impulse) < 1e-7, (episode, step, i, st["dish_state"][i][18], o.spin.normal_impulse)
                touched += int(o.spin.n_contacts > 0)
            _compare(venv, oracles, obs, ref, st, (episode, step))
        assert done.all()
    assert touched > n * steps          # the dish stood on the spindle for most of the run
    venv.close()


def test_spinning_plate_oracle_observation_and_auto_reset():
    """observation_mode "oracle": the object block is the DISH (object_balance_env.py:528-563); auto-reset: a finished env's terminal
    observation is the step's, the returned one the new episode's."""
    import tactile_gym_amd as tg
    from oracle.ref_env import OracleObjectBalanceEnv
    n, steps = 4, 5
    modes = dict(SPIN_MODES, observation_mode="oracle", rand_gravity=False)
    venv = tg.make_vec("object_balance-v0", num_envs=n, max_steps=steps, image_size=[64, 64], env_modes=modes, seed=31, auto_reset=True)
    oracles = [OracleObjectBalanceEnv(seed=31 + i, max_steps=steps, image_size=(64, 64), env_modes=modes) for i in range(n)]
    obs = venv.reset()
    ref = [o.reset() for o in oracles]
    for i in range(n):
        assert np.abs(obs["oracle"][i] - ref[i]["oracle"]).max() < 1e-5
    rng = np.random.default_rng(5)
    for step in range(2 * steps):
        a = rng.uniform(-0.25, 0.25, size=(n, 4)).astype(np.float32)
        obs, rew, done, infos = venv.step(a)
        for i, o in enumerate(oracles):
            ro, rr, rd, _ = o.step(a[i])
            assert rew[i] == rr and bool(done[i]) == rd
            if rd:
                assert np.abs(infos[i]["terminal_observation"]["oracle"] - ro["oracle"]).max() < 1e-4, (step, i)
                ro = o.reset()
            assert np.abs(obs["oracle"][i] - ro["oracle"]).max() < 1e-4, (step, i, np.abs(obs["oracle"][i] - ro["oracle"]).max())
    venv.close()


def test_spinning_plate_random_step_draws_its_actions():
    """step_random_async: k_step_spin does not draw actions itself, so the sampler launch must run - the step's actions are draw k of
    sample_actions(seed, k), new in every step, and the arm moves as in a step() with those actions."""
    import torch
    import tactile_gym_amd as tg
    n = 4
    kw = dict(num_envs=n, max_steps=20, image_size=[64, 64], env_modes=SPIN_MODES, seed=77, auto_reset=False)
    a_env, b_env = tg.make_vec("object_balance-v0", **kw), tg.make_vec("object_balance-v0", **kw)
    a_env.reset(); b_env.reset()
    want = torch.empty(n, a_env.act_dim, device="cuda", dtype=torch.float32)
    prev = None
    for k in range(3):
        a_env.step_random_async(9, k, restart=(k == 0))
        a_env.step_wait()
        used = a_env.actions_torch().cpu().numpy().copy()
        b_env.sample_actions(want, 9, k + 1)
        torch.cuda.synchronize()
        assert np.array_equal(used, want.cpu().numpy()), k
        assert prev is None or not np.array_equal(used, prev), k
        prev = used
        b_env.step(used)
        assert np.array_equal(a_env.get_state()["q"], b_env.get_state()["q"]), k
    a_env.close(); b_env.close()


def test_spinning_plate_refuses_what_is_not_built():
    import tactile_gym_amd as tg
    with pytest.raises(Exception):
        tg.make_vec("object_balance-v0", num_envs=2, max_steps=4, image_size=[64, 64], env_modes=SPIN_MODES, seed=1, solver_residual_threshold=1e-7)
    with pytest.raises(NotImplementedError):
        tg.make_vec("object_balance-v0", num_envs=2, max_steps=4, image_size=[64, 64], env_modes=SPIN_MODES, seed=1, physics_dtype="f32")


def test_spinning_plate_long_horizon_matches_oracle():
    """32 envs, 80 steps (960 ticks) of random actions or until the dish falls: the trajectories stay together (the persistent manifold sees the
    same points on both sides: contact counts equal in every step), rewards and dones equal."""
    import tactile_gym_amd as tg
    from oracle.ref_env import OracleObjectBalanceEnv
    n, steps = 32, 80
    modes = dict(SPIN_MODES, rand_gravity=True)
    venv = tg.make_vec("object_balance-v0", num_envs=n, max_steps=steps, image_size=[64, 64], env_modes=modes, seed=900, auto_reset=False)
    oracles = [OracleObjectBalanceEnv(seed=900 + i, max_steps=steps, image_size=(64, 64), env_modes=modes) for i in range(n)]
    obs = venv.reset()
    for o in oracles:
        o.reset()
    rng = np.random.default_rng(901)
    alive = np.ones(n, bool)
    fell = 0
    worst_q = worst_p = 0.0
    for step in range(steps):
        a = rng.uniform(-0.25, 0.25, size=(n, 4)).astype(np.float32)
        obs, rew, done, _ = venv.step(a)
        st = venv.get_state()
        for i, o in enumerate(oracles):
            if not alive[i]:
                continue
            ro, rr, rd, _ = o.step(a[i])
            d = st["dish_state"][i]
            pos, R = o.body_pose()
            assert rew[i] == rr and bool(done[i]) == rd, (step, i)
            assert int(d[19]) == o.spin.n_contacts, (step, i)
            worst_q = max(worst_q, float(np.abs(st["q"][i] - o.arm.q).max()))
            worst_p = max(worst_p, float(np.abs(d[0:3] - pos).max()), float(np.abs(d[3:12].reshape(3, 3) - R).max()))
            assert int((obs["tactile"][i] != ro["tactile"]).sum()) <= 3, (step, i)
            if rd:
                alive[i] = False
                fell += int(step < steps - 1)
    assert worst_q < 1e-7 and worst_p < 1e-5, (worst_q, worst_p)
    print(f"spinning_plate, {n} envs x {steps} steps: worst |dq| {worst_q:.2e} rad, worst dish pose difference {worst_p:.2e}; {fell} dishes fell before the last step")
    venv.close()
