"""Every reset route from injected end-of-episode states: k_reset_contact_wave's template, optimistic move and literal move (object_push; object_roll
has no template), the always literal k_reset_push / k_reset_roll of the lane mapping, k_reset_body's template (object_balance), and the same code
inside an auto-reset step - against the CPU oracle's reset(), started from where no rollout leaves an object (tests/reset_cases.py: 3.5 mm and
4.5 mm either side of the 4 mm clear test, a vertical edge towards the path, the cube in the tip, on the tip's centre, in the air, on an edge, on
another face, sliding, the marble at either end of its range, a fallen pole, a ball off its plate, a dish off its spindle, the arm anywhere).
One batch of 70 envs per variant at 64 x 64, a case per env; tests/test_reset_cases_cpu.py proves on the oracle alone that the cases reach their
regimes, that the routes predicted here are consistent with the oracle and that nothing is decided on a knife edge.

Which route an env took is read from bank_stats() around masked resets: `swapped` counts template resets, `late` resets that moved.  The
template itself is read back through tg_selftest_get_reset_template of the test library.

Tolerances are those tests/test_gpu_body_states.py states per family: joints 1e-9 (push, roll) / 1e-8 (balance), joint velocities that x 240, the
teleported object 1e-12, extended_feature 1e-6, tactile images within 3 pixels; tick counts, contact ids and counts, goal index, done and the
reset's draws exact."""
import ctypes as C
import time

import numpy as np
import pytest

import body_cases as bc
import body_inject as bi
import reset_cases as rc
from test_gpu_body_states import IMAGE_ENVS, _compare_reset, _compare_step, _follow_a29, _worst

pytestmark = pytest.mark.gpu
PRIME_ENV = bc.UNINJECTED[0]        # object_push: this env's cube is put 10 cm away and the env reset alone, so that the context has its template


def read_template(venv):
    """(return code, words) of tg_selftest_get_reset_template."""
    from tactile_gym_amd import _capi
    buf, n = np.zeros(512), C.c_int32(0)
    code = _capi.test_lib().tg_selftest_get_reset_template(venv._ctx, buf.ctypes.data_as(C.POINTER(C.c_double)), buf.size, C.byref(n))
    return code, buf[:n.value].copy()


def template_fields(words, nd):
    npts = int(words[2 * nd + 2])
    return dict(q=words[:nd], qd=words[nd:2 * nd], ticks=int(words[2 * nd]), valid=words[2 * nd + 1], npts=npts, radius=words[2 * nd + 3],
                path=words[2 * nd + 4:2 * nd + 4 + 3 * npts].reshape(npts, 3))


def _far(ref):
    return next(c for c in rc.PUSH_CASES if c["name"] == "far_10cm")["build"](ref)


def _overlapping(ref):
    return next(c for c in rc.PUSH_CASES if c["name"] == "into_tip_5mm")["build"](ref)


def _prime(venv, ref, oracle=None):
    """A context whose first reset found every cube at the tip has no template yet (a UR5 move of one tick, whose tip was not clear before its
    only tick, included).  One env gets its cube 10 cm away and is reset alone: its optimistic move runs through and is the template."""
    n = venv.num_envs
    states = [None] * n
    states[PRIME_ENV] = _far(ref)
    bi.inject_device(venv, states)
    venv.reset(np.arange(n) == PRIME_ENV)
    if oracle is not None:
        bi.inject_oracle(oracle, "push", states[PRIME_ENV])
        oracle.reset()
    code, words = read_template(venv)
    assert code == 0 and template_fields(words, venv.ndof)["valid"] == 1.0, (code, words[:20])


def _nominal_route(family, case):
    """The route with the device's defaults; an env left at the reset pose has its object at (push) or under (roll) the tip: it moves literally."""
    if family in ("pole", "ball", "spin"):
        return "template"
    return "literal" if case is None else case["route"]


def _draws(family, st, i, o):
    """(key, device, oracle) of what a reset draws or sets per episode; the RNG state after it says that both sides drew alike."""
    out = [("rng_state", int(st["rng_state"][i]), int(o.rng.state))]
    if family == "push":
        return out + [("obj_mass", float(st["obj_mass"][i]), float(o.cube.mass))]
    if family == "roll":
        return out + [("obj_mass", float(st["obj_mass"][i]), float(o.scaled_obj_radius)), ("embed_dist", float(st["embed_dist"][i]), float(o.embed_dist))]
    return out + [("gravity_z", float(st["gravity_z"][i]), float(o.gravity)), ("embed_dist", float(st["embed_dist"][i]), float(o.embed_dist))]


# object_roll's goal in the TCP frame is distance x (cos, sin) of two exact draws: the device's cos / sin and the host's are each within an ulp of the
# true value and the product rounds once more - 4 ulp of the largest goal distance (0.015) bound the difference
GOAL_TOL = 4 * float(np.spacing(0.015))


def _compare_after_reset(family, venv, oracles, obs, ref_obs, names, tol, worst, fails, tag0="reset"):
    q_tol = tol[0]
    st = venv.get_state()
    for i, o in enumerate(oracles):
        tag = (tag0, i, names[i])
        r = bi.oracle_report(o, family)

        def check(key, got, want, t):
            d = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())
            _worst(worst, key, d)
            if not d < t:
                fails.append(tag + (key, d, t))

        def exact(key, got, want):
            if got != want:
                fails.append(tag + (key, got, want))

        exact("reset_ticks", int(st["reset_ticks"][i]), int(o.reset_ticks))
        check("q", st["q"][i], r["q"], q_tol)
        check("qd", st["qd"][i], r["qd"], 240.0 * q_tol)
        check("body_pos", st["body_pos"][i], r["body_pos"], 1e-12)
        check("body_rot", st["body_rot"][i], r["body_rot"], 1e-12)
        exact("body at rest", (float(np.abs(st["body_linvel"][i]).max()), float(np.abs(st["body_angvel"][i]).max())), (0.0, 0.0))
        if family in ("push", "roll"):
            exact("contact_count", int(st["contact_count"][i]), r["contact_count"])
            exact("contact_ids", list(st["contact_ids"][i]), r["contact_ids"])
            check("extended_feature", obs["extended_feature"][i], ref_obs[i]["extended_feature"], 1e-6)
        if family == "push":
            exact("goal_id", int(st["goal_id"][i]), r["goal_id"])
        if family == "ball":
            exact("ball_pos", list(st["ball_pos"][i]), list(r["ball_pos"]))
        if family == "spin":
            check("dish_pose", st["dish_state"][i][:12], r["dish"][:12], 1e-12)
        for key, got, want in _draws(family, st, i, o):
            exact(key, got, want)
        if family == "roll":
            check("goal_pos", st["goal_pos"][i], o.goal_pos_tcp, GOAL_TOL)
        if i in IMAGE_ENVS:
            px = int((obs["tactile"][i] != ref_obs[i]["tactile"]).sum())
            _worst(worst, "tactile_px", px)
            if px > 3:
                fails.append(tag + ("tactile", px))


def _step_and_compare(family, venv, oracles, names, step, tol, worst, fails):
    """One step with body_cases.actions on both sides, compared as tests/test_gpu_body_states.py compares a step."""
    n = len(oracles)
    acts = bc.actions(n, bc.FAMILIES[family]["act_dim"], step)
    obs, rew, done, info = venv.step(acts)
    st = venv.get_state()
    follows = 0
    for i, o in enumerate(oracles):
        goal_before = np.array(o.goal_pos_world, dtype=np.float64) if family == "push" else None
        ro, rr, rd, _ = o.step(acts[i])
        if _follow_a29(family, True, st, i, o, goal_before):            # every env stands at the reset pose
            ro = o._observation()
            follows += 1
        _compare_step(family, i, ("step", i, names[i]), st, obs, rew, done, o, ro, rr, rd, tol, worst, fails)
    return follows


@pytest.mark.parametrize("family,arm,sensor,nph,mapping", rc.VARIANTS)
def test_injected_states_reset_like_the_oracle(family, arm, sensor, nph, mapping):
    t0 = time.time()
    f, tol = rc.FAMILIES[family], bc.FAMILIES[family]["tol"]
    n = bc.N_ENVS
    venv = bi.make_venv(family, arm=arm, sensor=sensor, narrowphase=nph, mapping=mapping)
    oracles, refs, cases = rc.prepare(family, arm, sensor, nph)
    fails, worst = [], {}
    obs = venv.reset()
    _compare_reset(venv, oracles, obs, [r["first_obs"] for r in refs], family, tol[0], "first reset", fails)
    assert not fails, fails[:10]                    # the cases are placed relative to this state
    counted = family == "push" and mapping == "wave"                    # k_reset_contact_wave counts the route of every reset
    template_on = counted and nph == "closed_form"
    if template_on:
        _prime(venv, refs[PRIME_ENV], oracles[PRIME_ENV])
    case_of = [None if k is None else f["cases"][k] for k in cases]
    names = ["-" if c is None else c["name"] for c in case_of]
    states = [None if c is None else c["build"](refs[i]) for i, c in enumerate(case_of)]
    for i, o in enumerate(oracles):
        if states[i] is not None:
            bi.inject_oracle(o, family, states[i])
    bi.inject_device(venv, states)
    nominal = [_nominal_route(family, c) for c in case_of]
    expected = [rc.device_route(dict(route=r), nph, mapping) if family in ("push", "roll") else r for r in nominal]      # on this variant; observed: the counters
    first = np.array([r == "template" for r in nominal])
    # the envs whose route is the template with one masked reset, the rest with a second; the counters around each call
    stats = [venv.bank_stats()]
    for mask in (first, ~first):
        if mask.any():
            obs = venv.reset(mask)
        stats.append(venv.bank_stats())
    d_sw = [stats[k + 1]["swapped"] - stats[k]["swapped"] for k in range(2)]
    d_late = [stats[k + 1]["late"] - stats[k]["late"] for k in range(2)]
    if template_on:
        assert stats[0]["mode"] == "template"
        assert (d_sw[0], d_late[0]) == (int(first.sum()), 0), (d_sw, d_late)                # every template case took the template, none moved
        assert (d_sw[1], d_late[1]) == (0, int((~first).sum())), (d_sw, d_late)             # every other env moved
    elif counted:
        assert d_sw == [0, 0] and d_late == [int(first.sum()), int((~first).sum())], (d_sw, d_late)
    elif family == "push":
        assert stats[-1]["swapped"] == 0, stats
    ref_obs = [o.reset() for o in oracles]
    _compare_after_reset(family, venv, oracles, obs, ref_obs, names, tol, worst, fails)
    follows = _step_and_compare(family, venv, oracles, names, 0, tol, worst, fails)     # nothing of the old object survives: manifold, licence, forces
    venv.close()
    label = f"RESETSTATE {family} {arm} {sensor} {nph} {mapping}"
    for key in sorted(worst):
        print(f"{label} {key} {worst[key]:.3e}")
    routes = {r: (sum(1 for x in nominal if x == r), sum(1 for x in expected if x == r)) for r in ("template", "optimistic", "literal")}
    print(f"{label} routes (with the defaults, on this variant) {routes} counted: swapped {d_sw} late {d_late} a29_follows {follows} failures {len(fails)} wall {time.time() - t0:.1f} s")
    assert follows <= n
    assert not fails, (len(fails), fails[:12])


def _reset_in_context(monkeypatch, env, arm, sensor, states, ref):
    for k in ("TG_LITERAL_RESET", "TG_RESET_BANK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    venv = bi.make_venv("push", arm=arm, sensor=sensor, narrowphase="closed_form", mapping="wave")
    venv.reset()
    if not env:
        _prime(venv, ref)
    else:                                       # the same calls, so that every context draws alike; these contexts keep no template
        st = [None] * venv.num_envs
        st[PRIME_ENV] = _far(ref)
        bi.inject_device(venv, st)
        venv.reset(np.arange(venv.num_envs) == PRIME_ENV)
    before = venv.bank_stats()
    bi.inject_device(venv, states)
    venv.reset()
    out = dict(venv.get_state(), stats=venv.bank_stats(), before=before)
    venv.close()
    return out


@pytest.mark.parametrize("arm,sensor", [("ur5", "tactip"), ("mg400", "digitac")])
def test_routes_agree_bit_for_bit(monkeypatch, arm, sensor):
    """The same injected batch reset with the template, without it (TG_RESET_BANK=0: the optimistic move) and literally (TG_LITERAL_RESET=1)."""
    oracles, refs, cases = rc.prepare("push", arm, sensor, "closed_form")
    case_of = [None if k is None else rc.PUSH_CASES[k] for k in cases]
    states = [None if c is None else c["build"](refs[i]) for i, c in enumerate(case_of)]
    n_tmpl = sum(1 for c in case_of if c is not None and c["route"] == "template")
    tmpl, opt, lit = (_reset_in_context(monkeypatch, env, arm, sensor, states, refs[PRIME_ENV]) for env in ({}, {"TG_RESET_BANK": "0"}, {"TG_LITERAL_RESET": "1"}))
    assert tmpl["stats"]["mode"] == "template" and tmpl["stats"]["swapped"] - tmpl["before"]["swapped"] == n_tmpl, (tmpl["stats"], tmpl["before"], n_tmpl)
    assert tmpl["stats"]["late"] - tmpl["before"]["late"] == bc.N_ENVS - n_tmpl
    assert opt["stats"]["swapped"] == 0 and lit["stats"]["swapped"] == 0
    assert np.array_equal(tmpl["q"], opt["q"]) and np.array_equal(tmpl["qd"], opt["qd"])          # the template IS the optimistic move's result
    for other, name in ((tmpl, "template"), (opt, "optimistic")):
        assert np.array_equal(other["reset_ticks"], lit["reset_ticks"]), name
        assert np.array_equal(other["contact_ids"], lit["contact_ids"]) and np.array_equal(other["contact_count"], lit["contact_count"]), name
        d = float(np.abs(other["q"] - lit["q"]).max())
        print(f"RESETSTATE routes {arm} {name} vs literal: q {d:.3e}")
        assert d < 1e-10, (name, d)


@pytest.mark.parametrize("arm,sensor", [("ur5", "tactip"), ("mg400", "digitac")])
def test_template_is_the_clean_move(arm, sensor):
    """Context A: every cube 10 cm away before the FIRST reset.  Context B: every other env's cube overlapping the tip at the rest pose instead -
    those envs' moves touch in the first tick and are abandoned (MG400) or run their one tick in contact (UR5).  Both templates are the oracle's
    unobstructed move, and equal word for word: an abandoned or touched move leaves nothing in the template."""
    o, twin = (bi.make_oracle("push", 0, arm=arm, sensor=sensor, narrowphase="closed_form") for _ in range(2))
    o.reset(), twin.reset()
    ref = rc.reference(o, twin, "push")
    n = bc.N_ENVS
    words = {}
    for name, states in (("A", [_far(ref)] * n), ("B", [_overlapping(ref) if i % 2 == 0 else _far(ref) for i in range(n)])):
        venv = bi.make_venv("push", arm=arm, sensor=sensor, narrowphase="closed_form", mapping="wave")
        code, w = read_template(venv)
        assert code == 0 and not w.any()                                # nothing before the first reset
        bi.inject_device(venv, states)
        venv.reset()
        code, words[name] = read_template(venv)
        stats = venv.bank_stats()
        assert code == 0 and stats["swapped"] == 0 and stats["late"] == n, (code, stats)
        if len(ref["clean_rows"]) >= 63:                                # the path does not fit: no template, every reset moves
            assert words[name][2 * venv.ndof + 1] == 0.0
            venv.reset()
            assert venv.bank_stats() == dict(stats, late=2 * n)
        nd = venv.ndof
        venv.close()
    if len(ref["clean_rows"]) >= 63:
        return
    assert np.array_equal(words["A"], words["B"]), np.nonzero(words["A"] != words["B"])[0]
    t = template_fields(words["A"], nd)
    assert t["valid"] == 1.0 and t["ticks"] == len(ref["clean_rows"]) and t["npts"] == len(ref["path"]), t
    worst = dict(q=np.abs(t["q"] - ref["clean_q"]).max(), qd=np.abs(t["qd"] - ref["clean_qd"]).max(), radius=abs(t["radius"] - ref["sphere_r"]),
                 path=np.abs(t["path"] - ref["path"]).max())
    print(f"RESETSTATE template {arm}: ticks {t['ticks']} points {t['npts']} " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert all(v < 1e-9 for v in worst.values()), worst
    assert not words["A"][2 * nd + 4 + 3 * t["npts"]:].any()            # nothing behind the path


def test_get_reset_template_refuses(monkeypatch):
    """-1: NULL arguments, a buffer that is too small (the size is still reported), a context without a template (TG_RESET_BANK=0)."""
    from tactile_gym_amd import _capi
    import tactile_gym_amd as tg
    T = _capi.test_lib()
    n = C.c_int32(7)
    buf = np.zeros(512)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert T.tg_selftest_get_reset_template(None, p, 512, C.byref(n)) == -1
    modes = dict(bc.PUSH_MODES, arm_type="ur5", tactile_sensor_name="tactip")
    monkeypatch.delenv("TG_RESET_BANK", raising=False)
    venv = tg.make_vec("object_push-v0", num_envs=2, max_steps=20, image_size=[64, 64], env_modes=modes, seed=7, auto_reset=False)
    assert T.tg_selftest_get_reset_template(venv._ctx, p, 512, None) == -1
    assert T.tg_selftest_get_reset_template(venv._ctx, p, 3, C.byref(n)) == -1 and n.value > 3 and not buf.any()
    assert T.tg_selftest_get_reset_template(venv._ctx, p, 512, C.byref(n)) == 0
    venv.close()
    monkeypatch.setenv("TG_RESET_BANK", "0")
    off = tg.make_vec("object_push-v0", num_envs=2, max_steps=20, image_size=[64, 64], env_modes=modes, seed=7, auto_reset=False)
    assert T.tg_selftest_get_reset_template(off._ctx, p, 512, C.byref(n)) == -1 and n.value == 0 and T.tg_selftest_last_error()
    off.close()


# terminal states per family: (name, build over the reference, nominal route of the reset that follows); None: the env stays at the reset pose and
# ends by max_steps = 1 with its object at (push) or under (roll) the tip
def _terminal_states(family):
    if family == "push":
        return [("short_of_last_goal", lambda ref: bc._on_goal(ref, len(ref["goals"]) - 1), "template"), ("far_10cm", _far, "template"), None,
                ("clear_3.5", next(c for c in rc.PUSH_CASES if c["name"] == "clear_3.5")["build"], "literal"), ("into_tip_5mm", _overlapping, "literal")]
    if family == "roll":
        return [("on_goal", bc._marble_on_goal, "literal"), ("beside_4.5", next(c for c in rc.ROLL_CASES if c["name"] == "beside_4.5")["build"], "optimistic"), None]
    return [("past_fall_angle", bc._tilted(roll_deg=-35.1), "template"), None, ("fallen_52.5_5rad", rc.POLE_CASES[0]["build"], "template")]


@pytest.mark.parametrize("family,arm,sensor,nph,mapping", [("push", "ur5", "tactip", "closed_form", "wave"), ("push", "mg400", "digitac", "closed_form", "wave"),
                                                           ("roll", "ur5", "tactip", None, "wave"), ("pole", "ur5", "tactip", None, "wave"),
                                                           ("pole", "ur5", "tactip", None, "lane")])
def test_auto_reset_from_injected_terminal_states(family, arm, sensor, nph, mapping):
    """auto_reset, max_steps = 1: the step after the injection ends every episode - the cube 1 cm short of the last goal, the marble on its goal,
    the pole past its fall angle, and every other env one step before max_steps, its object clear of the tip or at it.  done, reward, the terminal
    observation and the state after the reset that the step carries against the oracle's step() followed by reset()."""
    t0 = time.time()
    tol = bc.FAMILIES[family]["tol"]
    n = bc.N_ENVS
    venv = bi.make_venv(family, arm=arm, sensor=sensor, narrowphase=nph, mapping=mapping, max_steps=1, auto_reset=True)
    oracles, refs, _ = rc.prepare(family, arm, sensor, nph, max_steps=1)
    fails, worst = [], {}
    obs = venv.reset()
    _compare_reset(venv, oracles, obs, [r["first_obs"] for r in refs], family, tol[0], "first reset", fails)
    assert not fails, fails[:10]
    if family == "push":
        _prime(venv, refs[PRIME_ENV], oracles[PRIME_ENV])
    kinds = _terminal_states(family)
    kind_of = [None if i in bc.UNINJECTED else kinds[i % len(kinds)] for i in range(n)]
    names = ["-" if k is None else k[0] for k in kind_of]
    states = [None if k is None else k[1](refs[i]) for i, k in enumerate(kind_of)]
    for i, o in enumerate(oracles):
        if states[i] is not None:
            bi.inject_oracle(o, family, states[i])
    bi.inject_device(venv, states)
    venv.profile(True)
    before, resets_before = venv.bank_stats(), venv.profile_get()["reset"][1]
    acts = bc.actions(n, bc.FAMILIES[family]["act_dim"], 0)
    obs, rew, done, info = venv.step(acts)
    after, resets_after = venv.bank_stats(), venv.profile_get()["reset"][1]
    venv.profile(False)
    ref_obs = []
    for i, o in enumerate(oracles):
        tag = ("terminal", i, names[i])
        ro, rr, rd, _ = o.step(acts[i])
        if not rd or not bool(done[i]):                   # every episode ends in this step, on both sides
            fails.append(tag + ("done", bool(done[i]), rd))
        d = abs(float(rew[i]) - float(rr))
        _worst(worst, "reward", d)
        if (family == "pole" and float(rew[i]) != float(rr)) or not d < 1e-6:
            fails.append(tag + ("reward", float(rew[i]), float(rr)))
        term = info[i].get("terminal_observation")
        if term is None:
            fails.append(tag + ("no terminal_observation",))
        else:
            if "extended_feature" in ro:
                d = float(np.abs(np.asarray(term["extended_feature"], dtype=np.float64) - ro["extended_feature"]).max())
                _worst(worst, "terminal extended_feature", d)
                if not d < 1e-6:
                    fails.append(tag + ("terminal extended_feature", d))
            if i in IMAGE_ENVS:
                px = int((np.asarray(term["tactile"]) != ro["tactile"]).sum())
                _worst(worst, "terminal tactile_px", px)
                if px > 3:
                    fails.append(tag + ("terminal tactile", px))
        ref_obs.append(o.reset())
    _compare_after_reset(family, venv, oracles, obs, ref_obs, names, tol, worst, fails, tag0="reset in step")
    venv.close()
    d_sw, d_late = after["swapped"] - before["swapped"], after["late"] - before["late"]
    n_tmpl = sum(1 for k in kind_of if k is not None and k[2] == "template")
    label = f"RESETSTATE auto_reset {family} {arm} {mapping}"
    for key in sorted(worst):
        print(f"{label} {key} {worst[key]:.3e}")
    print(f"{label} swapped {d_sw} late {d_late} reset launches {resets_after - resets_before} failures {len(fails)} wall {time.time() - t0:.1f} s")
    if family == "push":                            # both routes were taken, by exactly the envs predicted
        assert n_tmpl > 0 and (d_sw, d_late) == (n_tmpl, n - n_tmpl), (d_sw, d_late, n_tmpl)
    if family == "pole":                            # the wave mapping resets its finished envs inside the step's launch, the lane mapping in a launch of its own
        assert (resets_after - resets_before == 0) == (mapping == "wave"), (mapping, resets_before, resets_after)
    assert not fails, (len(fails), fails[:12])
