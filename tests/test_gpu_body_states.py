"""The free-body step kernels from injected object states: k_step_push / k_step_roll / k_step_body (a lane per env) and k_step_contact_wave /
k_step_body_wave / k_step_spin (a wavefront per env) against the CPU oracle, started where an episode from the reset pose never takes them
(tests/body_cases.py: a cube on two vertices, on one, in the air, an impact, friction at the cone limit, the tip on a cube edge, a ball at the
plate's rim, a pole at its fall threshold, a dish tilted on or lifted off its spindle, the last goal).  One batch of 70 envs per test, a case per
env (three envs keep the reset pose), two steps; the states go in through tg_selftest_set_body_state of the test library.  That every case
reaches its regime, is well conditioned and decides nothing on a knife edge is tests/test_body_cases_cpu.py's part, on the oracle alone.

Tolerances are the suite's own per family (test_gpu_parity.py, test_gpu_spinning_plate.py): push / roll joints 1e-9, object pose 1e-8, reward
1e-6, extended_feature 1e-6; pole / ball joints 1e-8, poses and ball position 1e-7, ball velocity 1e-6, ball impulse 1e-9; spinning plate joints
1e-8, poses 1e-6, dish velocity 1e-5 / 1e-4, impulse 1e-7; done, goal index, contact ids and counts exact; tactile images within 3 pixels.  A
velocity the suite has no figure for gets the pose tolerance x 240: an error of that size moves the pose by the tolerance in one tick."""
import numpy as np
import pytest

import body_cases as bc
import body_inject as bi

pytestmark = pytest.mark.gpu
IMAGE_ENVS = (0, 5, 13, 22, 41, 63, 64, 69)        # the tactile image is compared on these envs


def _worst(acc, key, value):
    acc[key] = max(acc.get(key, 0.0), float(value))


def _compare_reset(venv, oracles, obs, ref_obs, family, q_tol, tag, fails):
    st = venv.get_state()
    for i, o in enumerate(oracles):
        r = bi.oracle_report(o, family)
        if np.abs(st["q"][i] - r["q"]).max() >= q_tol:
            fails.append((tag, i, "q", float(np.abs(st["q"][i] - r["q"]).max())))
        if np.abs(st["body_pos"][i] - r["body_pos"]).max() >= 1e-12 or np.abs(st["body_rot"][i] - r["body_rot"]).max() >= 1e-12:
            fails.append((tag, i, "body pose"))
        if family == "ball" and not np.array_equal(st["ball_pos"][i], r["ball_pos"]):
            fails.append((tag, i, "ball_pos"))
        if family == "spin" and np.abs(st["dish_state"][i][:12] - r["dish"][:12]).max() >= 1e-12:
            fails.append((tag, i, "dish pose"))
        if family == "push" and st["goal_id"][i] != r["goal_id"]:
            fails.append((tag, i, "goal_id"))
        if i in IMAGE_ENVS and int((obs["tactile"][i] != ref_obs[i]["tactile"]).sum()) > 3:
            fails.append((tag, i, "tactile"))


def _follow_a29(family, at_reset_pose, st, i, o, goal_before):
    """PARITY_ASSUMPTIONS A29 (the envs left at the reset pose only): goal 0 lies EXACTLY the termination distance from the cube's start, so the
    reference decides by rounding noise; where the device advanced the goal and the oracle did not, follow the device, as test_gpu_parity.py
    does.  True: the oracle's goal was advanced (its observation has to be read again)."""
    if family != "push" or not at_reset_pose:
        return False
    r = bi.oracle_report(o, family)
    if st["goal_id"][i] == r["goal_id"] + 1 and abs(np.linalg.norm(r["body_pos"] - goal_before) - o.termination_pos_dist) < 1e-12:
        assert o._update_goal()
        return True
    return False


def _compare_step(family, i, tag, st, obs, rew, done, o, ro, rr, rd, tol, worst, fails):
    """Env i after a step: the device's state `st`, observation, reward and done against the oracle env `o` and what its step returned (ro, rr,
    rd).  tol: the family's (q, pose) tolerances; the worst difference per key goes to `worst`, every miss to `fails` (prefixed with `tag`)."""
    q_tol, pose_tol = tol
    vel_tol = 240.0 * pose_tol
    r = bi.oracle_report(o, family)

    def check(key, got, want, tol):
        d = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())
        _worst(worst, key, d)
        if not d < tol:
            fails.append(tag + (key, d, tol))

    def exact(key, got, want):
        if got != want:
            fails.append(tag + (key, got, want))

    check("q", st["q"][i], r["q"], q_tol)
    check("body_pos", st["body_pos"][i], r["body_pos"], pose_tol)
    check("body_rot", st["body_rot"][i], r["body_rot"], pose_tol)
    check("body_linvel", st["body_linvel"][i], r["body_linvel"], vel_tol)
    check("body_angvel", st["body_angvel"][i], r["body_angvel"], vel_tol)
    exact("done", bool(done[i]), rd)
    if family in ("push", "roll"):
        check("reward", rew[i], rr, 1e-6)
        check("extended_feature", obs["extended_feature"][i], ro["extended_feature"], 1e-6)
        exact("contact_count", int(st["contact_count"][i]), r["contact_count"])
        exact("contact_ids", list(st["contact_ids"][i]), r["contact_ids"])
    else:
        exact("reward", float(rew[i]), float(rr))
    if family == "push":
        exact("goal_id", int(st["goal_id"][i]), r["goal_id"])
    if family == "ball":
        check("ball_pos", st["ball_pos"][i], r["ball_pos"], 1e-7)
        check("ball_linvel", st["ball_linvel"][i], r["ball_linvel"], 1e-6)
        check("ball_angvel", st["ball_angvel"][i], r["ball_angvel"], vel_tol)
        check("ball_impulse", st["ball_impulse"][i], r["ball_impulse"], 1e-9)
        exact("ball_impulse sign", bool(st["ball_impulse"][i] > 0), bool(r["ball_impulse"] > 0))
    if family == "spin":
        d = st["dish_state"][i]
        check("dish_pos", d[0:3], r["dish"][0:3], pose_tol)
        check("dish_rot", d[3:12], r["dish"][3:12], pose_tol)
        check("dish_linvel", d[12:15], r["dish"][12:15], 1e-5)
        check("dish_angvel", d[15:18], r["dish"][15:18], 1e-4)
        check("dish_impulse", d[18], r["spin_impulse"], 1e-7)
        exact("dish contact count", int(d[19]), r["spin_n"])
    if i in IMAGE_ENVS:
        px = int((obs["tactile"][i] != ro["tactile"]).sum())
        _worst(worst, "tactile_px", px)
        if px > 3:
            fails.append(tag + ("tactile", px))


@pytest.mark.parametrize("family,arm,sensor,nph,mapping", bc.VARIANTS)
def test_injected_states_match_oracle(family, arm, sensor, nph, mapping):
    f = bc.FAMILIES[family]
    q_tol, pose_tol = f["tol"]
    n = bc.N_ENVS
    venv = bi.make_venv(family, arm=arm, sensor=sensor, narrowphase=nph, mapping=mapping)
    oracles = [bi.make_oracle(family, i, arm=arm, sensor=sensor, narrowphase=nph) for i in range(n)]
    fails, worst = [], {}
    obs = venv.reset()
    ref_obs = [o.reset() for o in oracles]
    _compare_reset(venv, oracles, obs, ref_obs, family, q_tol, "reset", fails)
    assert not fails, fails[:10]                    # the cases are placed relative to this state
    cases = bi.case_of_env(family, radii=[o.scaled_obj_radius for o in oracles] if family == "roll" else None)
    acts = bi.case_actions(family, cases)
    states = []
    for i, o in enumerate(oracles):
        st = None if cases[i] is None else f["cases"][cases[i]]["build"](bi.reference(o, family))
        states.append(st)
        if st is not None:
            bi.inject_oracle(o, family, st)
    bi.inject_device(venv, states)
    alive = np.ones(n, bool)
    knife_edges = 0
    for s in range(bc.STEPS):
        obs, rew, done, _ = venv.step(acts[s])
        st = venv.get_state()
        for i, o in enumerate(oracles):
            tag = (s, i, "-" if cases[i] is None else f["cases"][cases[i]]["name"])
            goal_before = np.array(o.goal_pos_world, dtype=np.float64) if family == "push" else None
            ro, rr, rd, _ = o.step(acts[s, i])
            if _follow_a29(family, cases[i] is None, st, i, o, goal_before):
                ro = o._observation()
                knife_edges += 1
            _compare_step(family, i, tag, st, obs, rew, done, o, ro, rr, rd, f["tol"], worst, fails)
            if rd:
                alive[i] = False                    # (counted; both sides step a finished env on alike, and the comparison goes on)
    # the injection left nothing behind: the next reset is the oracle's reset
    obs = venv.reset()
    ref_obs = [o.reset() for o in oracles]
    _compare_reset(venv, oracles, obs, ref_obs, family, q_tol, "reset after", fails)
    venv.close()
    for key in sorted(worst):
        print(f"BODYSTATE {family} {arm} {sensor} {nph} {mapping} {key} {worst[key]:.3e}")
    print(f"BODYSTATE {family} {arm} {sensor} {nph} {mapping} finished_envs {int((~alive).sum())} a29_follows {knife_edges} failures {len(fails)}")
    assert knife_edges <= len(bc.UNINJECTED)
    assert not fails, (len(fails), fails[:12])


def _same_state(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_entry_refuses_and_writes_nothing():
    """-1 and nothing written: a NULL context or struct, a field the env kind does not have, a non-finite value, a rotation that is none, a goal
    index out of range.  And a masked call writes the masked envs only."""
    import ctypes as C
    from tactile_gym_amd import _capi
    n = 6
    import tactile_gym_amd as tg
    modes = dict(bc.PUSH_MODES, arm_type="ur5", tactile_sensor_name="tactip")
    venv = tg.make_vec("object_push-v0", num_envs=n, max_steps=20, image_size=[64, 64], env_modes=modes, seed=7, auto_reset=False, narrowphase="gjk_manifold")
    venv.reset()
    venv.step(np.zeros((n, 2), np.float32))
    before = venv.get_state()
    lic = venv.step_licence()
    T = _capi.test_lib()
    empty = _capi.TgBodyStateTest()
    assert T.tg_selftest_set_body_state(None, C.byref(empty)) == -1 and T.tg_selftest_set_body_state(venv._ctx, None) == -1
    pos, rot = before["body_pos"].copy(), before["body_rot"].reshape(n, 9).copy()
    pos[:, 0] += 0.01
    bad_pos, bad_rot, skew = pos.copy(), rot.copy(), rot.copy()
    bad_pos[4, 1] = np.nan
    bad_rot[2] *= 1.0 + 1e-8                       # off orthonormal by 2e-8 > 1e-9
    skew[1, 0] = np.inf
    goal = np.full(n, 2, np.int32)
    refused = [dict(body_pos=pos, ball_pos=pos), dict(body_pos=pos, dish_state=np.zeros((n, 18))), dict(body_pos=bad_pos), dict(body_pos=pos, body_rot=bad_rot),
               dict(body_pos=pos, body_rot=skew), dict(body_pos=pos, goal_id=np.where(np.arange(n) == 3, -1, goal)),
               dict(body_pos=pos, goal_id=np.where(np.arange(n) == 5, 11, goal)), dict(body_pos=pos, q=np.full((n, venv.ndof), np.inf))]
    for kw in refused:
        assert bi.set_body_state(venv, **kw) == -1, list(kw)
        assert T.tg_selftest_last_error()
        assert _same_state(before, venv.get_state()) and np.array_equal(lic, venv.step_licence()), list(kw)
    # a non-finite value in an env the mask leaves out is not read
    mask = np.array([1, 0, 1, 0, 0, 0], np.uint8)
    assert bi.set_body_state(venv, mask=mask, body_pos=bad_pos, goal_id=goal) == 0
    after = venv.get_state()
    for i in range(n):
        if mask[i]:
            assert np.array_equal(after["body_pos"][i], pos[i]) and after["goal_id"][i] == 2 and after["contact_count"][i] == 0
        else:
            assert all(np.array_equal(after[k][i], before[k][i]) for k in before), i
    assert (venv.step_licence()[mask == 1] == 0).all()
    venv.close()
    roll = tg.make_vec("object_roll-v0", num_envs=2, max_steps=20, image_size=[64, 64], env_modes=bc.ROLL_MODES, seed=7, auto_reset=False)
    roll.reset()
    before = roll.get_state()
    assert bi.set_body_state(roll, body_pos=before["body_pos"], goal_id=np.zeros(2, np.int32)) == -1      # no goal trajectory in object_roll
    assert _same_state(before, roll.get_state())
    roll.close()
