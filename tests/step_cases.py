"""Case tables of the step kernels' solver licence: tests/test_step_cases_cpu.py proves with the CPU oracle alone that
every case is in the regime it claims, tests/test_gpu_step_licence.py runs them on the device.  Not collected by pytest.

What a test can read.  `venv.step_licence()` is State::licence after a step.  A step starts from the value `before` and the vote of its
group (the 64 envs of a k_step wavefront, the 16 of a k_step_quad one, the env itself on object_balance's wave mapping), and leaves `after`:

    group all > 0  and  after == before - 1      "analytic"  no tick of the step ran a solve: every tick took qd = target, q += dt target
    after == 8                                     "solved"    at least one tick ran the full solve (group not all licensed, or the a-priori
                                                               bound refused the tick) and the step's last solve converged inside 80 % of the
                                                               sweep budget on the unclamped path
    after == 0 otherwise                           "clamped"   ... and the step's last solve left through the clamped sweeps (or did not converge)

So the licence does not stay 0 where the bound refuses a tick: the refused tick is solved, the solve renews the verdict, and the step ends on 8.
A refused rung therefore reads 8 after EVERY step (never counting down), a licensed one counts 8, 7, .. 1, 0 and is renewed to 8 by the step
after the 0: the countdown licenses the EIGHT steps that follow a solve, and reads 0 after the last of them.  `classify` below restates this;
the coverage conditions of the GPU test are written on its output (see test_gpu_step_licence.py's docstring for how they map to the issue's).

THE LADDER (edge_follow-v0, UR5 + TacTip, f64; max_force in N m; a row's impulse limit is max_force / 240).  Regimes of the i.i.d. pattern
from the reset pose, as `step_licence()` reported them on the MI355X (both kernels) and, for "clamps", by the CPU oracle (weak limit against
1000 N m, test_step_cases_cpu.py):

    1000   licensed   8 7 6 5 4 3 2 1 0 8 7 ..: every step analytic but the renewal; so are zeros, full-scale sign flips and the held corner,
                      the start states by the wrist singularity (~1 rad/s asked for) and with |qd| ~ 1 rad/s (after their first, solved, step)
     300   flips      the bound holds in some steps and envs and refuses others (8 7 8 7 6 5 4 3 2 8 ..); sign flips are refused throughout
     100   refused    reads 8 after every step; zeros are still licensed there (the mixed cases sit on this rung)
      30   refused    reads 8 after every step; nothing clamps in the oracle for the i.i.d., sign-flip and held patterns from the reset pose
                      (a restart in mid-run can: the out-of-phase cases sit on the 100 N m rung, where the oracle never clamps)
      10   clamps     the oracle's motors saturate in some envs (|dq| up to 1.5e-4 rad against 1000 N m after 8 steps)
       3   clamps     ... in every env; the licence reads 0 throughout (the reset's own renewal fails too)
       1   clamps     ... and zeros clamp as well: the reset's residual velocity is braked over three steps, then the env rests and is licensed

So with ordinary actions the a-priori bound flips between 1000 and 300 N m: the default is within half an order of magnitude of the edge, and the
near-singular pose does NOT cross it at 1000 N m (lambda* there is dominated by the wrist joints' small inertias).  surface_follow (xyzRxRy, 5
actions): 1000 licensed, 100 refused, 10 clamps.  object_balance on the wave mapping (the env's own licence): 1000 licensed; 100 refused for sign flips,
env by env for i.i.d. actions (about a fifth of the envs stay licensed); 10 clamps (the licence still reads 8 there after every step); on the lane mapping k_step_body keeps its verdict inside the step and State::licence reads 0 throughout.
No tolerance had to be measured: every case meets the project's own figures (the largest differences seen: 1e-14 rad against the literal run,
4e-14 rad against the oracle).
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile",
            reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
EDGE_MG400 = dict(EDGE, arm_type="mg400")
SURF = dict(movement_mode="xyzRxRy", control_mode="TCP_velocity_control", noise_mode="simplex", observation_mode="tactile",
            reward_mode="dense", arm_type="ur5", tactile_sensor_name="digit")
BAL = dict(movement_mode="xy", control_mode="TCP_velocity_control", object_mode="pole", rand_gravity=True, rand_embed_dist=True,
           observation_mode="tactile", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")

ENVS = {   # kind -> (env id, oracle class, modes, action dim, ticks per step)
    "edge": ("edge_follow-v0", "OracleEdgeFollowEnv", EDGE, 2, 24),
    "edge_mg400": ("edge_follow-v0", "OracleEdgeFollowEnv", EDGE_MG400, 2, 24),
    "surface": ("surface_follow-v1", "OracleSurfaceFollowGoalEnv", SURF, 5, 24),
    "balance": ("object_balance-v0", "OracleObjectBalanceEnv", BAL, 2, 12),
}
IMAGE = 64
SEED = 40
MAX_ACTION = 0.25
RESET_STEPS = {2: (0, 3), 5: (1, 3), 7: (0, 5)}      # masked resets of the out-of-phase cases: before step k, envs start::stride (test_gpu_kstep_quad.py)

# rung -> regime of the i.i.d. pattern from the reset pose.  "licensed": every step after a solve is analytic; "flips": the bound holds in some
# steps and refuses others; "refused": the bound refuses ticks the oracle does not clamp in (every step solves, the licence reads 8
# throughout); "clamps": the oracle's motors reach their limit.
LADDER = {1000.0: "licensed", 300.0: "flips", 100.0: "refused", 30.0: "refused", 10.0: "clamps", 3.0: "clamps", 1.0: "clamps"}

# Tolerances (the project's own; the issue's figures).  Default run against the literal run (test_default_solver_equals_literal_solver):
TOL_LITERAL = dict(q=1e-11, qd=1e-11, qd_target=1e-11, tcp_pos=1e-11, rew=1e-6, pixels=2, body_pos=1e-11, body_rot=1e-11)
# Against the oracle: test_env_reset_and_steps_match_oracle (q, tcp_pos 1e-8, qd_target 1e-7, reward 1e-5), the saturating-motors test for the
# clamping cases (q 1e-9, qd 1e-7), body_pos 1e-8.  qd is compared in every case at the saturating-motors figure.
TOL_ORACLE = dict(q=1e-8, qd=1e-7, qd_target=1e-7, tcp_pos=1e-8, rew=1e-5, body_pos=1e-8, body_rot=1e-7)
TOL_ORACLE_CLAMP = dict(TOL_ORACLE, q=1e-9)


class Case:
    """One run: env kind, n, motor limit, action pattern, optional start state, optional masked resets."""

    def __init__(self, name, kind="edge", n=128, max_force=1000.0, pattern="iid", steps=12, start=None, phases=False, max_steps=200,
                 switches=None, make=None, kernels=("quad", "lane"), clamps=False, expect=None, tol_oracle=None, oracle_force_ref=None):
        self.name, self.kind, self.n, self.max_force, self.pattern, self.steps = name, kind, n, float(max_force), pattern, steps
        self.start, self.phases, self.max_steps = start, phases, max_steps
        self.switches, self.make, self.kernels = dict(switches or {}), dict(make or {}), tuple(kernels)
        self.clamps, self.expect = clamps, expect
        self.env_id, self.oracle_cls, self.modes, self.act_dim, self.ticks = ENVS[kind]
        self.tol_oracle = dict(tol_oracle or (TOL_ORACLE_CLAMP if clamps else TOL_ORACLE))
        # the limit the CPU check compares this case's oracle against: 1000 N m (the "limit did bite" condition); for a 1000 N m case 1e5
        self.oracle_force_ref = float(oracle_force_ref or (1e5 if self.max_force == 1000.0 else 1000.0))
        assert steps <= 24 and (steps <= 8 or not clamps) and n in (70, 128)

    @property
    def auto_reset(self):
        return self.phases

    @property
    def subset(self):
        """The envs the oracle runs for (<= 16): both ends of both k_step wavefronts and of the first quad groups, the mixed case's envs 5, 6
        and 70 (69 where n = 70: the last env of the ragged wavefront)."""
        s = [0, 5, 6, 15, 16, 63, 64, 70, 127] if self.n == 128 else [0, 5, 6, 15, 16, 63, 64, 69]
        return tuple(s)

    def seed(self):
        return sum(ord(ch) * (k + 1) for k, ch in enumerate(self.name)) % 100003

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------ action patterns
def actions(case):
    """float32 [steps, n, act_dim].  Roles: "zeros" (jump 0), "iid" (+-0.25), "held" (one corner, every step), "flip" (a corner, its sign
    flipped every step: the largest jump), "mixed" (env 5 flips at full scale from the first step, env 70 from step 3 on, all others zeros)."""
    rng = np.random.default_rng(case.seed())
    n, d, steps = case.n, case.act_dim, case.steps
    corner = np.where(rng.random((n, d)) < 0.5, -MAX_ACTION, MAX_ACTION)
    sign = np.where(np.arange(steps) % 2 == 0, 1.0, -1.0)[:, None, None]
    if case.pattern == "zeros":
        a = np.zeros((steps, n, d))
    elif case.pattern == "iid":
        a = rng.uniform(-MAX_ACTION, MAX_ACTION, size=(steps, n, d))
    elif case.pattern == "held":
        a = np.broadcast_to(np.full((n, d), MAX_ACTION), (steps, n, d)).copy()      # work-frame +x +y: towards the corner the start state sits by
    elif case.pattern == "flip":
        a = sign * corner[None]
    elif case.pattern == "mixed":
        a = np.zeros((steps, n, d))
        a[:, 5] = (sign * corner[None])[:, 5]
        if n > 70:
            a[3:, 70] = (sign * corner[None])[3:, 70]
    else:
        raise ValueError(case.pattern)
    return np.ascontiguousarray(a, dtype=np.float32)


PATTERN_ROLES = {"zeros": "jump 0", "iid": "i.i.d. +-0.25", "held": "one corner held", "flip": "sign flipped every step", "mixed": "mixed wavefront"}


def reset_mask(case, k):
    """uint8 [n] or None: the envs that restart before step k of an out-of-phase case."""
    if not case.phases or k not in RESET_STEPS:
        return None
    m = np.zeros(case.n, np.uint8)
    start, stride = RESET_STEPS[k]
    m[start::stride] = 1
    return m


# ------------------------------------------------------------------------------------------------ oracle helpers
def make_oracle(case, env):
    from oracle import ref_env
    return getattr(ref_env, case.oracle_cls)(seed=SEED + env, max_steps=case.max_steps, image_size=(IMAGE, IMAGE), env_modes=case.modes)


@functools.lru_cache(maxsize=None)
def _proto(kind):
    """One oracle env of the kind at its reset pose: the arm model and work frame the start states are built with."""
    from oracle import ref_env
    _, cls, modes, _, _ = ENVS[kind]
    o = getattr(ref_env, cls)(seed=SEED, max_steps=200, image_size=(IMAGE, IMAGE), env_modes=modes)
    o.reset()
    return o, o.arm.q.copy()


def _place_tcp(o, q, work_pos, joints=(0, 1, 2), iters=30):
    """Newton on three joints: the TCP's work-frame position -> work_pos, the other joints as given."""
    q = np.array(q, dtype=np.float64)
    target, _ = o._work_to_world(np.asarray(work_pos, dtype=np.float64), np.zeros(3))
    for _ in range(iters):
        pos = np.asarray(o.arm.link_state("tcp_link", q=q, qd=np.zeros(o.arm.n))[0])
        err = target - pos
        if np.abs(err).max() < 1e-12:
            break
        J = o.arm.jacobian("tcp_link", q)[:3][:, list(joints)]
        q[list(joints)] += np.linalg.solve(J, err)
    return q


SINGULAR_DELTA = 0.01     # rad from sin(q5) = 0: the controller asks for ~1.5 rad/s there (0.03 -> 0.5, 0.003 -> 5; test_step_cases_cpu.py)


@functools.lru_cache(maxsize=None)
def _start_cached(kind, n, start, seed):
    o, q_reset = _proto(kind)
    rng = np.random.default_rng(seed + 17)
    q, qd = np.tile(q_reset, (n, 1)), np.zeros((n, len(q_reset)))
    if start == "spin":                       # the reset pose, |qd| ~ 1 rad/s on every joint
        qd = np.where(rng.random(qd.shape) < 0.5, -1.0, 1.0) * rng.uniform(0.8, 1.2, size=qd.shape)
    elif start == "corner":                   # by the +x +y corner of TCP_lims: the held action (1 mm a step) passes the x limit after 3 - 6 steps
        lim = o.TCP_lims[:2, 1]               # and the y limit after 10 - 14, so the commanded velocity changes twice, before and after the renewal
        for i in range(n):
            xy = lim - 1e-3 * np.array([rng.uniform(2.5, 5.5), rng.uniform(9.5, 13.5)])
            q[i] = _place_tcp(o, q_reset, [xy[0], xy[1], o.embed_dist])
    elif start in ("singular", "singular_matched"):
        for i in range(n):
            qi = q_reset.copy()
            qi[4] = SINGULAR_DELTA * rng.uniform(0.8, 1.25) * (1.0 if i % 2 == 0 else -1.0)
            q[i] = _place_tcp(o, qi, [0.02 * rng.uniform(-1, 1), 0.02 * rng.uniform(-1, 1), 0.0])
    else:
        raise ValueError(start)
    return q, qd


def start_state(case):
    """(q, qd) float64 [n, ndof] for set_joint_state after the reset, or None.  "singular_matched": qd is what the controller will ask for in
    the first step (the jump is ~0 and |qd| ~ 1 rad/s: the damping term of the bound is all that is left)."""
    if case.start is None:
        return None
    q, qd = _start_cached(case.kind, case.n, case.start, case.seed())
    q, qd = q.copy(), qd.copy()
    if case.start == "singular_matched":
        o, _ = _proto(case.kind)
        a = actions(case)[0]
        keep_q, keep_qd = o.arm.q.copy(), o.arm.qd.copy()
        for i in range(case.n):
            o.arm.reset_joint_states(q[i])
            enc = np.clip(o._encode_actions(a[i].astype(np.float64)), o.min_action, o.max_action)
            o._tcp_velocity_control(((enc - o.min_action) * (o.act_hi - o.act_lo)) / (o.max_action - o.min_action) + o.act_lo)
            qd[i] = o.last_req_joint_vels
        o.arm.reset_joint_states(keep_q)
        for k in range(o.arm.n):
            o.arm.state.qd[k] = keep_qd[k]
    return q, qd


def _apply_start(o, q, qd):
    o.arm.reset_joint_states(q)
    for k in range(o.arm.n):
        o.arm.state.qd[k] = qd[k]


def _oracle_frame(o):
    rec = dict(q=o.arm.q.copy(), qd=o.arm.qd.copy(), tcp_pos=np.asarray(o._tcp_world()[0]).copy(), step_count=o.step_counter, reset_ticks=o.reset_ticks)
    if hasattr(o, "body_pose"):
        p, R = o.body_pose()
        rec["body_pos"], rec["body_rot"] = np.asarray(p).copy(), np.asarray(R).copy()
    return rec


def oracle_rollout(case, max_force=None, envs=None, dq0=0.0):
    """The CPU oracle over the case for `envs` (default: case.subset): {key: array [steps, len(envs), ...]} of q, qd, qd_target, tcp_pos, rew,
    done, step_count, reset_ticks (+ body_pos, body_rot), the states AFTER a finished env's reset as the device reports them, and
    "tcp_work" [steps, envs, 3], the TCP's work-frame position at the END of each step before any reset.  max_force: the motor limit from
    the first step on (set after the reset, whose blocking move runs on PyBullet's default as on the device); dq0: added to the start q."""
    envs = list(case.subset if envs is None else envs)
    force = case.max_force if max_force is None else float(max_force)
    acts, start = actions(case), start_state(case)
    keys = None
    out = {}
    for col, i in enumerate(envs):
        o = make_oracle(case, i)
        o.reset()
        o.max_force = force
        if start is not None:
            _apply_start(o, start[0][i] + dq0, start[1][i])
        elif dq0:
            _apply_start(o, o.arm.q + dq0, o.arm.qd.copy())
        for k in range(case.steps):
            m = reset_mask(case, k)
            if m is not None and m[i]:
                o.reset()
            _, rew, done, _ = o.step(acts[k, i])
            frame = dict(qd_target=np.asarray(o.last_req_joint_vels).copy(), rew=float(rew), done=bool(done), tcp_work=np.asarray(o._tcp_work()[0]).copy())
            if done and case.auto_reset:
                o.reset()
                frame["qd_target"] = np.zeros_like(frame["qd_target"])     # the device's reset clears the controller's last targets
            frame.update(_oracle_frame(o))
            if keys is None:
                keys = list(frame)
                out = {key: [[None] * len(envs) for _ in range(case.steps)] for key in keys}
            for key in keys:
                out[key][k][col] = frame[key]
    return {key: np.asarray(v) for key, v in out.items()}


@functools.lru_cache(maxsize=None)
def oracle_reference(case):
    """The oracle at the case's own limit, computed once per process and shared (left unchanged by its readers)."""
    return oracle_rollout(case)


@functools.lru_cache(maxsize=None)
def first_clamp_step(case):
    """int [len(subset)]: the first step in which the oracle at the case's limit leaves the oracle at case.oracle_force_ref (a motor reached its
    limit in that step), -1 where it never does.  The device must not take the fixed point for that env in that step."""
    a, b = oracle_reference(case), oracle_rollout(case, max_force=case.oracle_force_ref)
    differs = (np.abs(a["q"] - b["q"]).max(axis=2) > 0) | (np.abs(a["qd"] - b["qd"]).max(axis=2) > 0)      # [steps, envs]
    return np.where(differs.any(axis=0), differs.argmax(axis=0), -1)


def oracle_sensitivity(case, dq0=1e-13):
    """How far two oracle runs whose start q differs by dq0 drift apart over the case: {key: max abs difference}."""
    a, b = oracle_rollout(case), oracle_rollout(case, dq0=dq0)
    return {key: float(np.abs(a[key].astype(np.float64) - b[key].astype(np.float64)).max()) for key in ("q", "qd", "qd_target", "tcp_pos")}


# ------------------------------------------------------------------------------------------------ reading the licence
def group_size(case, kernel):
    """Envs that share one licence vote."""
    if case.kind == "balance":
        return 1 if case.make.get("contact_mapping") == "wave" else 64
    return 16 if kernel == "quad" else 64


def classify(before, after, group):
    """int8 [n]: 0 "analytic", 1 "solved", 2 "clamped" for one step, from the licence before and after it (module docstring)."""
    before, after = np.asarray(before), np.asarray(after)
    n = len(before)
    out = np.zeros(n, np.int8)
    for g0 in range(0, n, group):
        sl = slice(g0, min(g0 + group, n))
        licensed = bool((before[sl] > 0).all())
        for i in range(sl.start, sl.stop):
            if licensed and after[i] == before[i] - 1:
                out[i] = 0
            elif after[i] == 8:
                out[i] = 1
            elif after[i] == 0:
                out[i] = 2
            else:
                raise AssertionError(f"licence {before[i]} -> {after[i]} of env {i} is no transition the step rule allows (group licensed: {licensed})")
    return out


ANALYTIC, SOLVED, CLAMPED = 0, 1, 2


# ------------------------------------------------------------------------------------------------ the cases
def _edge_cases():
    c = []
    for f, regime in LADDER.items():
        clamps = regime == "clamps"
        c.append(Case(f"edge_iid_{f:g}", max_force=f, pattern="iid", steps=8 if clamps else 12, clamps=clamps, expect=regime))
    c.append(Case("edge_zeros_1000", max_force=1000.0, pattern="zeros", steps=10, expect="licensed"))
    c.append(Case("edge_zeros_1", max_force=1.0, pattern="zeros", steps=8, clamps=True))
    c.append(Case("edge_zeros_100", max_force=100.0, pattern="zeros", steps=10, expect="licensed"))
    for f in (1000.0, 300.0, 100.0, 30.0):
        c.append(Case(f"edge_flip_{f:g}", max_force=f, pattern="flip", steps=8, expect="licensed" if f == 1000.0 else "refused" if f < 300.0 else None))
    c.append(Case("edge_held_1000", max_force=1000.0, pattern="held", steps=20, start="corner", expect="held"))
    c.append(Case("edge_held_30", max_force=30.0, pattern="held", steps=20, start="corner"))
    c.append(Case("edge_mixed_100", max_force=100.0, pattern="mixed", steps=12, expect="mixed"))
    c.append(Case("edge_singular_1000", max_force=1000.0, pattern="held", steps=6, start="singular", expect="licensed"))
    c.append(Case("edge_singular_30", max_force=30.0, pattern="held", steps=6, start="singular", clamps=True))
    c.append(Case("edge_singular_matched_1000", max_force=1000.0, pattern="held", steps=6, start="singular_matched", expect="licensed"))
    c.append(Case("edge_spin_1000", max_force=1000.0, pattern="iid", steps=6, start="spin", expect="licensed"))
    c.append(Case("edge_spin_100", max_force=100.0, pattern="iid", steps=6, start="spin", clamps=True))
    for name, sw in (("bank", {}), ("noinline", {"TG_NO_INLINE_RESET": "1"})):
        c.append(Case(f"edge_phases_{name}_100", max_force=100.0, pattern="iid", steps=24, phases=True, max_steps=7, switches=sw, expect="refused"))
    c.append(Case("edge_ragged_70_100", n=70, max_force=100.0, pattern="mixed", steps=12, expect="mixed"))
    c.append(Case("edge_mg400_1000", kind="edge_mg400", max_force=1000.0, pattern="iid", steps=6, kernels=(None,), expect="never"))
    return c


def _surface_cases():
    c = []
    for f in (1000.0, 100.0, 10.0):
        for pattern in ("iid", "flip"):
            c.append(Case(f"surface_{pattern}_{f:g}", kind="surface", max_force=f, pattern=pattern, steps=8, clamps=f < 100.0,
                          expect={1000.0: "licensed", 100.0: "refused"}.get(f)))
    return c


def _balance_cases():
    c = []
    for mapping in ("lane", "wave"):
        for f in (1000.0, 100.0, 10.0):
            for pattern in ("iid", "flip"):
                c.append(Case(f"balance_{mapping}_{pattern}_{f:g}", kind="balance", max_force=f, pattern=pattern, steps=8, max_steps=250,
                              make=dict(contact_mapping=mapping), kernels=(None,), clamps=f < 100.0,
                              expect="unread" if mapping == "lane" else {1000.0: "licensed", 100.0: "refused" if pattern == "flip" else "flips"}.get(f)))
        c.append(Case(f"balance_{mapping}_mixed_100", kind="balance", max_force=100.0, pattern="mixed", steps=10, max_steps=250,
                      make=dict(contact_mapping=mapping), kernels=(None,), expect="unread" if mapping == "lane" else "mixed"))
    return c


CASES = _edge_cases() + _surface_cases() + _balance_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
