"""Test infrastructure (not collected): writes one case of tests/body_cases.py into an oracle env and into the device
(tg_selftest_set_body_state of the test library), and records what the oracle's ticks do with it."""
import ctypes as C

import numpy as np

from body_cases import FAMILIES, N_ENVS, SIZE, STEPS, actions, assign, not_testable


def make_oracle(family, i, arm="ur5", sensor="tactip", narrowphase=None, max_steps=50):
    from oracle import ref_env
    f = FAMILIES[family]
    modes = dict(f["modes"])
    kw = {}
    if family == "push":
        modes.update(arm_type=arm, tactile_sensor_name=sensor)
        kw["narrowphase"] = narrowphase or "closed_form"
    return getattr(ref_env, f["oracle"])(seed=f["seed"] + i, max_steps=max_steps, image_size=(SIZE, SIZE), env_modes=modes, **kw)


def make_venv(family, arm="ur5", sensor="tactip", narrowphase=None, mapping="wave", max_steps=50, auto_reset=False):
    import tactile_gym_amd as tg
    f = FAMILIES[family]
    modes = dict(f["modes"])
    kw = dict(contact_mapping=mapping)
    if family == "push":
        modes.update(arm_type=arm, tactile_sensor_name=sensor)
        kw["narrowphase"] = narrowphase or "closed_form"
    if family in ("ball", "spin"):
        kw = {}                                   # one mapping each: a lane per env / a wavefront per env
    return tg.make_vec(f["env_id"], num_envs=N_ENVS, max_steps=max_steps, image_size=[SIZE, SIZE], env_modes=modes, seed=f["seed"], auto_reset=auto_reset, **kw)


def tip_gap(o):
    """object_push: distance between the tip core and the cube less the collision margins (the closed-form narrowphase's depth, whatever
    the breaking threshold says), from the env's present state."""
    sc = o.scene
    Rl, pl = o.arm.link_poses()[sc.tip_link]
    pos, R = o.cube_pose()
    w = np.asarray(pl) + o._tip_verts @ np.asarray(Rl).T
    q = np.abs((w - pos) @ R) - np.array(sc.half[:])
    outside = np.linalg.norm(np.maximum(q, 0.0), axis=1)
    sdf = np.where(outside > 0.0, outside, q.max(axis=1))
    return float(sdf.min() - (sc.margin_tip + sc.margin_cube))


def reference(o, family):
    """What the cases are placed relative to: the oracle env's state after reset() (the device's get_state() agrees with it to 1e-12 in the
    object pose and 1e-9 in the TCP position; the GPU test asserts that before it injects)."""
    from oracle import pb_math as pm
    tcp = np.array(o._tcp_world()[0], dtype=np.float64)
    ref = dict(tcp_pos=tcp)
    if family == "push":
        p, R = o.cube_pose()
        ref.update(body_pos=p.copy(), body_rot=R.copy(), goals=np.array(o.traj_pos_world, dtype=np.float64), tip_gap=tip_gap(o))
        # body_cases.NOT_TESTABLE: where the tip on a cube edge is not testable, the yawed cube stands 5 mm off the tip
        nph = {0: "closed_form", 1: "gjk_manifold"}[int(o.scene.narrowphase)]
        ref["edge_standoff"] = "tip_on_cube_edge" in not_testable("push", o.arm_type, nph)
    elif family == "roll":
        p, R = o.ball_pose()
        sc = o.scene
        Rl, pl = o.arm.link_poses()[sc.tip_link]
        cyl_rot = np.array(sc.cyl_rot[:]).reshape(3, 3)
        cap = np.asarray(pl) + np.asarray(Rl) @ np.array(sc.cyl_pos[:])
        axis = np.asarray(Rl) @ cyl_rot[:, 2]
        assert abs(axis[2]) > 0.9999                                           # the cap looks straight down at the reset
        o._update_goal()
        ref.update(body_pos=p.copy(), body_rot=R.copy(), radius=float(o.scaled_obj_radius), cap_pos=cap, cap_bottom=float(cap[2] - sc.cyl_half_len),
                   cap_radius=float(sc.cyl_radius), goal_world=np.array(o.goal_pos_world, dtype=np.float64))

        def ik_lower(dz):
            """Joint angles that put the TCP dz lower than it stands, orientation kept."""
            pos, _, quat, _, _ = o._tcp_world()
            return np.array(o.arm.inverse_kinematics("tcp_link", np.asarray(pos) - np.array([0.0, 0.0, dz]), quat, 100, 1e-8), dtype=np.float64)[:o.arm.n]
        ref["ik_lower"] = ik_lower
    else:
        p, R = np.array(o.body.pos[:]), np.array(o.body.rot[:]).reshape(3, 3)
        pivot_b = np.array(o.p2p.pivot_b[:])
        ref.update(body_pos=p, body_rot=R, pivot_b=pivot_b, pivot=p + R @ pivot_b, init_obj_pos=np.array(o.init_obj_pos))
        if family == "ball":
            ref.update(ball_pos=np.array(o.ball.pos[:]), ball_radius=float(o.ball.radius), plate_radius=float(o.ball.plate_radius),
                       plate_half=float(o.ball.plate_half_len))
        if family == "spin":
            d = o.spin.dish
            ref.update(dish_pos=np.array(d.pos[:]), dish_rot=np.array(d.rot[:]).reshape(3, 3))

        def ik(work_pos):
            """Joint angles that put the TCP at work_pos (work frame, reset orientation), and the pivot's world position there."""
            q0 = o.arm.q
            tpos, trpy = o._work_to_world(work_pos, np.zeros(3))
            q = np.array(o.arm.inverse_kinematics("tcp_link", tpos, pm.quat_from_euler(trpy), 100, 1e-8), dtype=np.float64)[:o.arm.n]
            for k in range(o.arm.n):
                o.arm.state.q[k] = float(q[k])
            link, fpos, _ = o.tg.frames["tcp_link"]
            Rl, pl = o.arm.link_poses()[link]
            pivot = np.asarray(pl) + np.asarray(Rl) @ np.array(o.p2p.pivot_a[:])
            for k in range(o.arm.n):
                o.arm.state.q[k] = float(q0[k])
            return q, pivot
        ref["ik"] = ik
    return ref


def _set_body(b, st, prefix="body"):
    if prefix + "_pos" in st:
        for k in range(3):
            b.pos[k] = float(st[prefix + "_pos"][k])
    if prefix + "_rot" in st:
        for k in range(9):
            b.rot[k] = float(np.asarray(st[prefix + "_rot"]).reshape(9)[k])
    if prefix + "_linvel" in st:
        for k in range(3):
            b.linvel[k] = float(st[prefix + "_linvel"][k])
    if prefix + "_angvel" in st:
        for k in range(3):
            b.angvel[k] = float(st[prefix + "_angvel"][k])


def inject_oracle(o, family, st):
    """The state `st` (a case's build(ref)) into the oracle env, with what a teleport clears."""
    if "q" in st:
        for k in range(o.arm.n):
            o.arm.state.q[k] = float(st["q"][k])
            o.arm.state.qd[k] = float(st["qd"][k])
    if family == "push":
        _set_body(o.cube, st)
        o.scene.mani.n = 0
        if "goal_id" in st:                                  # as _update_goal leaves it
            g = int(st["goal_id"])
            o.targ_traj_list_id = g
            if g < o.traj_n_points:
                o.goal_pos_world, o.goal_orn_world = o.traj_pos_world[g], o.traj_orn_world[g]
                o.goal_pos_work, o.goal_rpy_work = o.traj_pos_work[g], o.traj_rpy_work[g]
    elif family == "roll":
        _set_body(o.ball, st)
    else:
        _set_body(o.body, st)
        o.body.ext_pending = 0
        if o.ball is not None:
            _set_body(o.ball, st, "ball")
            o.ball.ext_pending = 0
            for k in range(3):
                o.ball.ext_torque[k] = 0.0
        if o.spin is not None:
            _set_body(o.spin.dish, st, "dish")
            o.spin.dish.ext_pending = 0
            o.spin.torque_pending = 0
            o.spin.mani.n = 0


def device_arrays(states, ndof, current):
    """[n] case states (None: not injected) -> the arrays of tg_body_state_test, AoS, and the mask.  The entry takes an array for all envs or not
    at all, so where a case leaves a field out that another case of the batch sets, the env's row is what the device holds (current: get_state())."""
    n = len(states)
    out = dict(mask=np.array([s is not None for s in states], dtype=np.uint8))
    keys = set().union(*[set(s) for s in states if s is not None])
    widths = dict(q=ndof, qd=ndof, body_pos=3, body_rot=9, body_linvel=3, body_angvel=3, ball_pos=3, ball_linvel=3, ball_angvel=3)
    for k, w in widths.items():
        if k in keys:
            a = np.array(current[k], dtype=np.float64).reshape(n, w)
            for i, s in enumerate(states):
                if s is not None and k in s:
                    a[i] = np.asarray(s[k], dtype=np.float64).reshape(w)
            out[k] = a
    if "dish_pos" in keys:
        a = np.array(current["dish_state"], dtype=np.float64)[:, :18].copy()
        for i, s in enumerate(states):
            if s is not None and "dish_pos" in s:
                a[i] = np.concatenate([s["dish_pos"], np.asarray(s["dish_rot"]).reshape(9), s["dish_linvel"], s["dish_angvel"]])
        out["dish_state"] = a
    if "goal_id" in keys:
        g = np.array(current["goal_id"], dtype=np.int32)
        for i, s in enumerate(states):
            if s is not None and "goal_id" in s:
                g[i] = int(s["goal_id"])
        out["goal_id"] = g
    return out


def set_body_state(venv, **arrays):
    """tg_selftest_set_body_state on the venv's context; returns the entry's return code."""
    from tactile_gym_amd import _capi
    s = _capi.TgBodyStateTest()
    keep = []
    for k, a in arrays.items():
        if a is None:
            continue
        dt = {"mask": np.uint8, "goal_id": np.int32}.get(k, np.float64)
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        ct = {np.uint8: C.c_uint8, np.int32: C.c_int32, np.float64: C.c_double}[dt]
        setattr(s, k, a.ctypes.data_as(C.POINTER(ct)))
    return _capi.test_lib().tg_selftest_set_body_state(venv._ctx, C.byref(s))


def inject_device(venv, states):
    """The case states into the device; envs whose state is None keep all they hold."""
    rc = set_body_state(venv, **device_arrays(states, venv.ndof, venv.get_state()))
    assert rc == 0, rc


# ---------------------------------------------------------------------------------------------------------------------------------------
def _angle_deg(R, init_rpy):
    from oracle import pb_math as pm
    rpy = np.degrees(pm.euler_from_quat(pm.quat_from_mat(R)))
    return np.abs(((rpy - np.degrees(init_rpy)) + 180) % 360 - 180)


def trace(o, family, acts):
    """Steps the oracle env through acts [steps][act_dim] and returns one row per sim tick: what the tick's contact generation saw (read after the
    tick) and the object's state after it.  Row 0 also carries "ends": per step the done flag, goal index and the distances of every threshold
    decision of the step's end ("margins": (value, threshold) pairs)."""
    rows, ends = [], []
    rest_ids = tuple(int(x) for x in getattr(getattr(o, "scene", None), "contact_ids", [])[:4]) if family == "push" else ()
    gap0 = tip_gap(o) if family == "push" else 0.0                          # before the first tick
    slip0 = 0.0
    if family == "roll":
        v, w = np.array(o.ball.linvel[:]), np.array(o.ball.angvel[:])
        slip0 = float(np.linalg.norm((v + np.cross(w, [0, 0, -o.scene.radius]))[:2]))
    inner = o._step_simulation
    step = [0]

    def tick():
        inner()
        r = dict(step=step[0])
        if family in ("push", "roll"):
            sc = o.scene
            b = o.cube if family == "push" else o.ball
            ids = tuple(int(x) for x in sc.contact_ids[:sc.n_contacts])
            nrm = np.array(sc.tip_normal[:])
            v, w = np.array(b.linvel[:]), np.array(b.angvel[:])
            r.update(n=int(sc.n_contacts), ids=ids, table=sum(1 for x in ids if x < 8), tip_depth=float(sc.tip_depth), tip_nz=float(nrm[2]),
                     speed=float(np.linalg.norm(v)), wz=float(w[2]), rest_ids=rest_ids)
            if family == "push":
                loc = np.abs(np.array(b.rot[:]).reshape(3, 3).T @ nrm)
                r["tip_oblique"] = bool(np.sort(loc)[1] > 0.3)              # the normal has two large components in the cube's frame
                r["gap0"] = gap0
            else:
                r["slip0"] = slip0
                r["slip"] = float(np.linalg.norm((v + np.cross(w, [0, 0, -sc.radius]))[:2]))
        else:
            b = o.body
            R = np.array(b.rot[:]).reshape(3, 3)
            link, _, _ = o.tg.frames["tcp_link"]
            Rl, pl = o.arm.link_poses()[link]
            pa = np.asarray(pl) + np.asarray(Rl) @ np.array(o.p2p.pivot_a[:])
            pb = np.array(b.pos[:]) + R @ np.array(o.p2p.pivot_b[:])
            r.update(pivot_err=float(np.linalg.norm(pa - pb)), spin_axis=float(abs(np.dot(np.array(b.angvel[:]), R[:, 2]))))
            if o.ball is not None:
                bl = o.ball
                p = R.T @ (np.array(bl.pos[:]) - np.array(b.pos[:]))
                r.update(ball_touch=bool(bl.in_contact), ball_rad=float(np.hypot(p[0], p[1])), ball_pz=float(p[2]), plate_radius=float(bl.plate_radius),
                         plate_half=float(bl.plate_half_len), ball_radius=float(bl.radius), ball_speed=float(np.linalg.norm(bl.linvel[:])))
            if o.spin is not None:
                d = o.spin.dish
                Rd = np.array(d.rot[:]).reshape(3, 3)
                off = np.array(d.pos[:]) - np.array(b.pos[:])
                r.update(spin_n=int(o.spin.n_contacts), dish_tilt=float(np.degrees(np.arccos(np.clip(Rd[2, 2], -1, 1)))),
                         dish_off=float(np.hypot(off[0], off[1])), dish_wz=float(d.angvel[2]))
        rows.append(r)

    o._step_simulation = tick
    try:
        for a in acts:
            if family == "push":
                goal_before = np.array(o.goal_pos_world, dtype=np.float64)
            _, rew, done, _ = o.step(np.asarray(a, dtype=np.float32))
            e = dict(done=bool(done), reward=float(rew), margins=[])
            if family == "push":
                e["goal_id"] = int(o.targ_traj_list_id)
                e["margins"].append((float(np.linalg.norm(o.cube_pose()[0] - goal_before)), o.termination_pos_dist))
                if not done:
                    e["margins"].append((float(np.linalg.norm(o.cube_pose()[0] - o.goal_pos_world)), o.termination_pos_dist))
            elif family == "roll":
                e["margins"].append((float(np.linalg.norm(o.ball_pose()[0][:2] - o.goal_pos_world[:2])), o.termination_pos_dist))
            else:
                pos, R = o.body_pose()
                ang = _angle_deg(R, o.init_obj_rpy)
                e["fall_deg"] = float(max(ang[0], ang[1]))
                e["margins"] += [(float(ang[0]), float(o.termination_dist_deg)), (float(ang[1]), float(o.termination_dist_deg)),
                                 (float(np.linalg.norm(pos - o.init_obj_pos)), o.termination_dist_pos)]
            ends.append(e)
            step[0] += 1
            if done:
                break
    finally:
        del o._step_simulation
    if rows:
        rows[0]["ends"] = ends
    return rows


def oracle_report(o, family):
    """What the GPU test compares after a step, from the oracle env."""
    out = dict(q=o.arm.q.copy(), qd=o.arm.qd.copy())
    if family == "push":
        b = o.cube
    elif family == "roll":
        b = o.ball
    else:
        b = o.body
    out.update(body_pos=np.array(b.pos[:]), body_rot=np.array(b.rot[:]).reshape(3, 3), body_linvel=np.array(b.linvel[:]), body_angvel=np.array(b.angvel[:]))
    if family in ("push", "roll"):
        out.update(contact_count=int(o.scene.n_contacts), contact_ids=[int(x) for x in o.scene.contact_ids])
    if family == "push":
        out["goal_id"] = int(o.targ_traj_list_id)
    if family == "ball":
        bl = o.ball
        out.update(ball_pos=np.array(bl.pos[:]), ball_linvel=np.array(bl.linvel[:]), ball_angvel=np.array(bl.angvel[:]), ball_impulse=float(bl.normal_impulse))
    if family == "spin":
        d = o.spin.dish
        out.update(dish=np.concatenate([d.pos[:], d.rot[:], d.linvel[:], d.angvel[:]]), spin_n=int(o.spin.n_contacts), spin_impulse=float(o.spin.normal_impulse))
    return out


def case_actions(family, cases_of_env):
    """[steps][n][act_dim] float32: body_cases.actions, zero for the envs whose case asks for a still arm."""
    f = FAMILIES[family]
    a = np.stack([actions(N_ENVS, f["act_dim"], s) for s in range(STEPS)])
    for i, k in enumerate(cases_of_env):
        if k is not None and f["cases"][k].get("zero_action"):
            a[:, i] = 0.0
    return a


def case_of_env(family, radii=None):
    """Env -> case index.  object_roll: the envs with the smallest and the largest marble of the episode hold the two cap-contact cases."""
    f = FAMILIES[family]
    out = assign(len(f["cases"]))
    if family == "roll" and radii is not None:
        order = [i for i in np.argsort(radii) if out[i] is not None]
        names = [c["name"] for c in f["cases"]]
        out[order[0]], out[order[1]] = names.index("under_centre_pressed"), names.index("under_rim")
        out[order[-1]], out[order[-2]] = names.index("under_rim"), names.index("under_centre_pressed")
    return out
