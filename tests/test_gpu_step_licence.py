"""The step kernels' solver licence where it is decided (sim_tick in csrc/tg_physics.hpp, step_env in csrc/tg_kernels.hpp,
k_step_body / k_step_body_wave for object_balance): the cases of tests/step_cases.py - a ladder of motor limits from 1000 down to 1 N m, action
patterns from zeros to full-scale sign flips, wavefronts in which one env differs from its neighbours, start states by the wrist singularity and with
|qd| ~ 1 rad/s, episodes out of phase - each run with the default solver and compared, per step, with

  * the device's literal solver (pgs_full_sweeps=True) on the same seeds, actions and start states, for EVERY env: q, qd 1e-11, dones, step
    counts and reset ticks equal, rewards 1e-6, <= 2 differing pixels per image (test_default_solver_equals_literal_solver's figures);
    qd_target 1e-11 and tcp_pos 6e-11 (six joints x a reach below 1 m x 1e-11 rad);
  * the CPU oracle (f64, 150 clamped sweeps in every tick) for the case's fixed subset of envs, at step_cases.TOL_ORACLE / TOL_ORACLE_CLAMP.

Every contact-free UR5 case runs on k_step_quad and on k_step (TG_KSTEP_QUAD, read per context; tg_get_step_mode says which ran).

Coverage is asserted from `venv.step_licence()`, read before the first step and after every step, through step_cases.classify (its module
docstring: a step is "analytic" - no solve in any tick - "solved", or "clamped").  How the conditions read on the licence as the kernels keep it:
  * a licensed rung: from the second step on every step is analytic, except the step after the countdown reached 0, which solves and reads 8.
    (The licence is NOT positive after every step: it reads 0 after the eighth analytic step, and the next step renews it.)
  * a refused rung: no step of any env is analytic and none is "clamped" - every step solves and reads 8 - while test_step_cases_cpu.py shows
    the oracle does not clamp there.  (A refused tick is solved, and the solve renews the verdict: the licence does not read 0 there.)
  * a rung between the two ("flips"): analytic steps and refused ones both occur after the first step, beyond the periodic renewals.
  * a clamping case: test_step_cases_cpu.py shows the oracle clamps; in the first step in which an oracle env's motors reach their limit
    (step_cases.first_clamp_step) that env's step is not analytic.
  * object_balance on the lane mapping: k_step_body keeps its verdict inside the step, the licence reads 0 throughout ("unread").
  * mixed: the vote group of the env that flips solves in every step - all its envs, 63 (15) of which have zero actions - while a group
    without such an env counts down; the group of env 70 counts down for three steps and then reads 8 after every step, from a value that was
    still positive: a licence lost mid-period.
  * held: some step starts from 0 after a countdown (1 -> 0 -> 8) and solves: the licence is renewed through a full solve.
  * after set_joint_state the licence reads 0 for every env; for the MG400 it reads 0 after every step.

Every test prints its figures (one JSON line) before it asserts."""
import contextlib
import json
import os

import numpy as np
import pytest

import step_cases as sc

pytestmark = pytest.mark.gpu

STATE_KEYS = ("q", "qd", "qd_target", "tcp_pos")
BODY_KEYS = ("body_pos", "body_rot")


@contextlib.contextmanager
def _environ(**switches):
    old = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _step_mode(venv):
    import ctypes
    mode, epw = ctypes.c_int32(), ctypes.c_int32()
    assert venv._L.tg_get_step_mode(venv._ctx, ctypes.byref(mode), ctypes.byref(epw)) == 0
    return mode.value, epw.value


def device_run(case, kernel, literal):
    """One rollout of the case: per-step arrays over all envs, the licence before the first step and after every step, the kernel that ran."""
    import tactile_gym_amd as tg
    switches = dict(case.switches)
    if kernel is not None:
        switches["TG_KSTEP_QUAD"] = "1" if kernel == "quad" else "0"
    kw = dict(case.make)
    if case.max_force != 1000.0:
        kw["max_force"] = case.max_force      # 1000: the constructor's default, left alone (None keeps 1000)
    with _environ(**switches):                # the switches are read by tg_create
        venv = tg.make_vec(case.env_id, num_envs=case.n, max_steps=case.max_steps, image_size=[sc.IMAGE, sc.IMAGE], env_modes=case.modes, seed=sc.SEED,
                           auto_reset=case.auto_reset, pgs_full_sweeps=literal, **kw)
    try:
        acts, start = sc.actions(case), sc.start_state(case)
        venv.reset()
        out = {k: [] for k in STATE_KEYS + ("rew", "done", "step_count", "reset_ticks", "img")}
        if start is not None:
            venv.set_joint_state(start[0], start[1])
        lic = [venv.step_licence()]
        for k in range(case.steps):
            m = sc.reset_mask(case, k)
            if m is not None:
                venv.reset(m)
                lic[-1] = venv.step_licence()     # what the step starts from
            obs, rew, done, _ = venv.step(acts[k])
            st = venv.get_state()
            lic.append(venv.step_licence())
            for key in STATE_KEYS + ("step_count", "reset_ticks"):
                out[key].append(st[key].copy())
            for key in BODY_KEYS:
                if key in st:
                    out.setdefault(key, []).append(st[key].copy())
            out["rew"].append(np.asarray(rew, dtype=np.float64).copy()), out["done"].append(np.asarray(done, dtype=bool).copy())
            out["img"].append(np.ascontiguousarray(obs["tactile"]).reshape(case.n, -1).copy())
        res = {key: np.asarray(v) for key, v in out.items()}
        res["lic"] = np.asarray(lic)
        res["mode"], res["epw"] = _step_mode(venv)
        return res
    finally:
        venv.close()


def licence_classes(case, kernel, lic):
    """int8 [steps, n]: step_cases.classify of every step.  With masked resets `lic[k]` is read after the reset, with auto-resets the value a
    finished env's reset left stands in `lic[k + 1]`: both are 8 (the reset's own renewal) on the UR5, which classify reads as "solved"."""
    g = sc.group_size(case, kernel)
    return np.stack([sc.classify(lic[k], lic[k + 1], g) for k in range(case.steps)])


def measure(case, kernel):
    """The runs and every figure the test asserts on."""
    a, b = device_run(case, kernel, literal=False), device_run(case, kernel, literal=True)
    ref = sc.oracle_reference(case)
    sub = list(case.subset)
    fig = dict(case=case.name, kernel=kernel, mode=a["mode"], epw=a["epw"], lit={}, ora={}, lit_ora={})
    for key in STATE_KEYS + tuple(k for k in BODY_KEYS if k in a):
        fig["lit"][key] = float(np.abs(a[key] - b[key]).max())
        fig["ora"][key] = float(np.abs(a[key][:, sub].reshape(ref[key].shape) - ref[key]).max())
        fig["lit_ora"][key] = float(np.abs(b[key][:, sub].reshape(ref[key].shape) - ref[key]).max())
    fig["lit"]["rew"] = float(np.abs(a["rew"] - b["rew"]).max())
    fig["ora"]["rew"] = float(np.abs(a["rew"][:, sub] - ref["rew"]).max())
    fig["lit"]["pixels"] = int((a["img"] != b["img"]).sum(axis=2).max())
    for key in ("done", "step_count", "reset_ticks"):
        fig["lit"][key] = int((a[key] != b[key]).sum())
        fig["ora"][key] = int((a[key][:, sub] != ref[key]).sum())
    fig["dones"] = int(a["done"].sum())
    cls = licence_classes(case, kernel, a["lic"])
    fig["lic0"] = [int(a["lic"][0].min()), int(a["lic"][0].max())]
    fig["lic_env"] = {str(i): a["lic"][:, i].tolist() for i in sorted({0, 5, 6, 16, 64, min(70, case.n - 1), case.n - 1})}
    fig["classes"] = ["%d/%d/%d" % tuple(int((cls[k] == c).sum()) for c in (sc.ANALYTIC, sc.SOLVED, sc.CLAMPED)) for k in range(case.steps)]
    fig["literal_lic_max"] = int(b["lic"][1:].max())
    return fig, a, b, cls


def _group(case, kernel, env):
    g = sc.group_size(case, kernel)
    return slice(env // g * g, min((env // g + 1) * g, case.n))


def check(case, kernel, fig, a, cls):
    lic = a["lic"]
    # ---- which kernel ran
    if case.kind == "balance":
        assert fig["epw"] == (1 if case.make["contact_mapping"] == "wave" else 64), fig
    elif kernel is not None:
        assert fig["mode"] == 0 and fig["epw"] == (16 if kernel == "quad" else 64), fig
    # ---- coverage, from the licence
    if case.start is not None:
        assert fig["lic0"] == [0, 0], "set_joint_state must drop every env's licence"
    if case.expect == "licensed":
        for k in range(1, case.steps):
            renew = lic[k] == 0
            assert (cls[k][~renew] == sc.ANALYTIC).all() and (cls[k][renew] == sc.SOLVED).all(), (k, fig["classes"])
            assert (lic[k + 1][lic[k] != 1] > 0).all(), k
    if case.expect == "flips":
        assert (cls[1:] == sc.ANALYTIC).any() and (cls[1:] == sc.SOLVED).sum() > (lic[1:-1] == 0).sum() and not (cls == sc.CLAMPED).any(), fig["classes"]
    if case.expect == "refused":
        # (an env that finished in the step shows what its reset left: at a weak limit the reset's own renewal may fail and leave 0)
        assert not case.clamps and not (cls == sc.ANALYTIC).any() and ((lic[1:] == 8) | (a["done"] & (lic[1:] == 0))).all(), fig["classes"]
    if case.clamps:
        first = sc.first_clamp_step(case)
        assert (first >= 0).any()
        for col, env in enumerate(case.subset):
            if first[col] >= 0:
                assert cls[first[col], env] != sc.ANALYTIC, ("the fixed point was taken in a step in which the oracle's motors clamp", env, int(first[col]))
    if case.expect == "unread":
        assert (lic == 0).all(), "k_step_body keeps its verdict inside the step"
    if case.expect == "never":
        assert (lic == 0).all(), "the MG400 is never licensed"
    if case.expect == "held":
        renewed = (lic[:-2] == 1) & (lic[1:-1] == 0) & (lic[2:] == 8)
        assert renewed.any(axis=0).all(), fig["lic_env"]
        assert (cls[1:] != sc.CLAMPED).all()
    if case.expect == "mixed":
        g5 = _group(case, kernel, 5)
        assert (cls[:, g5] == sc.SOLVED).all(), ("the flipping env must deny its whole vote group in every step", fig["classes"])
        quiet = [g for g in range(0, case.n, sc.group_size(case, kernel)) if g != g5.start and not (case.n > 70 and g == _group(case, kernel, 70).start)]
        for g in quiet:
            gs = _group(case, kernel, g)
            renew = lic[:-1, gs] == 0
            assert (cls[1:, gs][~renew[1:]] == sc.ANALYTIC).all() and (cls[:, gs][renew] == sc.SOLVED).all(), (g, fig["classes"])
        if case.n > 70:
            g70 = _group(case, kernel, 70)
            if g70.start != g5.start:
                assert (cls[1:3, g70] == sc.ANALYTIC).all() and (cls[3:, g70] == sc.SOLVED).all(), fig["lic_env"]
                assert (lic[3, g70] > 0).all()           # lost mid-period: the step that lost it started from a positive value
    # ---- against the literal run, every env
    tol = dict(sc.TOL_LITERAL, tcp_pos=6e-11)
    for key, v in fig["lit"].items():
        if key in ("done", "step_count", "reset_ticks"):
            assert v == 0, (key, fig["lit"])
        else:
            assert v <= tol[key] if key == "pixels" else v < tol[key], (key, v, fig["lit"])
    assert fig["literal_lic_max"] == 0 or case.phases, "the literal run holds no licence of its own"
    # ---- against the oracle, the subset
    for key, v in fig["ora"].items():
        if key in ("done", "step_count", "reset_ticks"):
            assert v == 0, (key, fig["ora"])
        else:
            assert v < case.tol_oracle[key], (key, v, fig["ora"])
    if case.phases:
        assert fig["dones"] >= case.n          # episodes ended and restarted inside the run, out of phase


PARAMS = [pytest.param(c.name, k, id=f"{c.name}-{k or 'default'}") for c in sc.CASES for k in c.kernels]


@pytest.mark.parametrize("name,kernel", PARAMS)
def test_step_licence_case(name, kernel):
    case = sc.BY_NAME[name]
    fig, a, _, cls = measure(case, kernel)
    print(json.dumps(fig))
    check(case, kernel, fig, a, cls)
