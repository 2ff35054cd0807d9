"""The cases of tests/step_cases.py are what they claim to be - proved with the CPU oracle alone (oracle/ref_env.py), no GPU:

  * a clamping case: the oracle at the weak limit ends more than 1e-5 rad away from the oracle at 1000 N m ("the limit did bite");
  * every other case: the oracle at the case's limit is IDENTICAL to the one at 1000 N m (1e5 N m for the 1000 N m cases): nothing clamps;
  * near-singular starts: the largest joint speed the controller asks for in the first step lies between 0.5 and 5 rad/s for every env of the
    subset, and the TCP stays inside TCP_lims' position box;
  * the held corner: the TCP passes both work-frame limits during the run and stops advancing there, with no change of action;
  * the mixed wavefront, the out-of-phase episodes, the sizes and the oracle subset are as the issue sets them, and every role of the action
    patterns is covered by the chosen subset;
  * step_cases.classify reads the licence as the step kernels write it; the new ABI entry and the max_force keyword are declared and bound."""
import inspect
import os
import re

import numpy as np
import pytest

import step_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in sc.CASES]


def _ref(case):
    return sc.oracle_rollout(case, max_force=case.oracle_force_ref)


@pytest.mark.parametrize("name", NAMES)
def test_case_is_in_the_regime_it_claims(name):
    case = sc.BY_NAME[name]
    own, ref = sc.oracle_reference(case), _ref(case)
    assert not np.array_equal(case.max_force, case.oracle_force_ref)
    if case.clamps:
        assert np.abs(own["q"][-1] - ref["q"][-1]).max() > 1e-5              # the limit did bite
        first = sc.first_clamp_step(case)
        assert (first >= 0).any() and first.max() < case.steps
    else:
        for key in ("q", "qd", "qd_target", "tcp_pos", "rew", "done"):
            assert np.array_equal(own[key], ref[key]), key                   # nothing clamps: the two oracles are identical
    assert np.isfinite(own["q"]).all() and np.isfinite(own["rew"]).all()
    if not case.phases:
        assert not own["done"].any()                                         # no episode ends inside a run without auto-reset


@pytest.mark.parametrize("name", [n for n in NAMES if sc.BY_NAME[n].start in ("singular", "singular_matched")])
def test_near_singular_starts_ask_for_large_joint_speeds_inside_the_tcp_box(name):
    case = sc.BY_NAME[name]
    own = sc.oracle_reference(case)
    q, qd = sc.start_state(case)
    assert np.abs(np.sin(q[:, 4])).max() < 0.02 and np.abs(np.sin(q[:, 4])).min() > 0.005
    top = np.abs(own["qd_target"][0]).max(axis=1)                            # first step, every env of the subset
    assert top.min() > 0.5 and top.max() < 5.0, top
    o, _ = sc._proto(case.kind)
    lims = o.TCP_lims[:3]
    for i in case.subset:
        pos = np.asarray(o.arm.link_state("tcp_link", q=q[i], qd=np.zeros(o.arm.n))[0])
        work, _ = o._world_to_work(pos, np.zeros(3))
        assert (work > lims[:, 0]).all() and (work < lims[:, 1]).all(), (i, work)
    assert (own["tcp_work"] > lims[:, 0]).all() and (own["tcp_work"] < lims[:, 1]).all()      # ... and stays inside over the run
    if case.start == "singular_matched":                                     # the first step's jump is ~0: qd is the controller's own request
        assert np.abs(qd[list(case.subset)] - own["qd_target"][0]).max() < 1e-12 and np.abs(qd).max() > 0.5


def test_spin_start_has_every_joint_near_one_rad_per_second():
    for case in (c for c in sc.CASES if c.start == "spin"):
        q, qd = sc.start_state(case)
        assert np.abs(qd).min() >= 0.8 and np.abs(qd).max() <= 1.2 and np.array_equal(q, np.tile(q[0], (case.n, 1)))


@pytest.mark.parametrize("name", [n for n in NAMES if sc.BY_NAME[n].pattern == "held" and sc.BY_NAME[n].start == "corner"])
def test_held_action_reaches_the_tcp_limits(name):
    case = sc.BY_NAME[name]
    assert case.steps >= 17
    acts = sc.actions(case)
    assert (acts == acts[0]).all() and (np.abs(acts) == sc.MAX_ACTION).all()                   # one corner, held
    own = sc.oracle_reference(case)
    o, _ = sc._proto(case.kind)
    for axis in (0, 1):
        lim = o.TCP_lims[axis, 1]
        x = own["tcp_work"][:, :, axis]                                      # [steps, envs]: the end of every step
        past = x > lim
        assert past.any(axis=0).all() and not past[0].any()
        for col in range(x.shape[1]):
            k = int(past[:, col].argmax())                                   # check_TCP_vel_lims zeroes the component from step k + 1 on
            assert k + 2 < case.steps
            assert np.all(np.diff(x[:k + 1, col]) > 0.9e-3) and np.abs(np.diff(x[k + 1:, col])).max() < 1e-5, (axis, col, x[:, col])
            assert np.abs(own["qd_target"][k + 1, col] - own["qd_target"][k, col]).max() > 1e-3     # the commanded joint velocity changed
    first_x, first_y = (own["tcp_work"][:, :, 0] > o.TCP_lims[0, 1]).argmax(axis=0), (own["tcp_work"][:, :, 1] > o.TCP_lims[1, 1]).argmax(axis=0)
    assert first_x.max() < 8 < first_y.min()                                 # one limit inside the first licence period, the other after its renewal


def test_mixed_cases_and_patterns_are_what_the_issue_sets():
    for case in (c for c in sc.CASES if c.pattern == "mixed"):
        a = sc.actions(case)
        assert (np.abs(a[:, 5]) == sc.MAX_ACTION).all() and (a[1:, 5] == -a[:-1, 5]).all()       # env 5: full scale, sign flipped every step
        quiet = np.ones(case.n, bool)
        quiet[5] = False
        if case.n > 70:
            quiet[70] = False
            assert (a[:3, 70] == 0).all() and (np.abs(a[3:, 70]) == sc.MAX_ACTION).all() and (a[4:, 70] == -a[3:-1, 70]).all()
        assert (a[:, quiet] == 0).all()
        assert {5, 6}.issubset(case.subset) and (case.n <= 70 or 70 in case.subset)
    for case in (c for c in sc.CASES if c.pattern == "flip"):
        a = sc.actions(case)
        assert (np.abs(a) == sc.MAX_ACTION).all() and (a[1:] == -a[:-1]).all()
    for case in (c for c in sc.CASES if c.pattern == "iid"):
        a = sc.actions(case)
        assert np.abs(a).max() <= sc.MAX_ACTION and len(np.unique(a)) > a.size // 2
    assert {c.pattern for c in sc.CASES} == set(sc.PATTERN_ROLES)            # every role is run ...
    for kind in ("edge", "surface", "balance"):
        assert {"iid", "flip"} <= {c.pattern for c in sc.CASES if c.kind == kind}


def test_sizes_and_subsets():
    assert any(c.n == 70 for c in sc.CASES)
    for c in sc.CASES:
        assert c.n in (70, 128) and c.steps <= 24 and (not c.clamps or c.steps <= 8)
        assert len(c.subset) <= 16 and len(set(c.subset)) == len(c.subset) and max(c.subset) < c.n
        groups64, groups16 = {i // 64 for i in c.subset}, {i // 16 for i in c.subset}
        assert groups64 == set(range((c.n + 63) // 64)) and len(groups16) >= 4             # both wavefronts, several quad groups
        ref = sc.oracle_reference(c)
        assert ref["q"].shape[:2] == (c.steps, len(c.subset))
        if c.pattern in ("flip", "held", "mixed", "iid"):                                    # ... and every role is seen by the oracle subset
            assert np.abs(sc.actions(c)[:, list(c.subset)]).max() == pytest.approx(sc.MAX_ACTION, rel=0.2)
    assert sorted(sc.LADDER, reverse=True) == [1000.0, 300.0, 100.0, 30.0, 10.0, 3.0, 1.0]
    assert {sc.LADDER[f] for f in sc.LADDER} == {"licensed", "flips", "refused", "clamps"}


def test_out_of_phase_cases():
    cases = [c for c in sc.CASES if c.phases]
    assert len(cases) == 2 and {bool(c.switches) for c in cases} == {False, True}
    for c in cases:
        assert c.steps % c.max_steps != 0 and sc.LADDER[c.max_force] == "refused" and not c.clamps
        done = sc.oracle_reference(c)["done"]
        per_step = done.sum(axis=1)
        assert done.sum() >= 2 * done.shape[1] and ((per_step > 0) & (per_step < done.shape[1])).sum() >= 4      # some but not all envs finish, in several steps
        masks = [sc.reset_mask(c, k) for k in range(c.steps)]
        assert sum(m is not None for m in masks) == 3 and all(0 < m.sum() < c.n for m in masks if m is not None)


def test_classify_reads_the_licence_as_the_step_writes_it():
    A, S, C = sc.ANALYTIC, sc.SOLVED, sc.CLAMPED
    seq = [8, 7, 6, 5, 4, 3, 2, 1, 0, 8, 7]
    got = [int(sc.classify([a] * 4, [b] * 4, 4)[0]) for a, b in zip(seq[:-1], seq[1:])]
    assert got == [A] * 8 + [S, A]
    assert list(sc.classify([8, 8, 8, 8], [8, 8, 8, 8], 4)) == [S] * 4                         # refused: solved, verdict renewed
    assert list(sc.classify([3, 3, 3, 3], [0, 0, 0, 0], 4)) == [C] * 4                         # the last solve left through the clamped sweeps
    assert list(sc.classify([1, 1, 1, 1], [0, 0, 0, 0], 4)) == [A] * 4                         # the countdown's last step
    assert list(sc.classify([1, 0, 1, 1], [0, 0, 0, 0], 4)) == [C] * 4                         # ... but not where a neighbour held no licence
    assert list(sc.classify([5, 5, 0, 5], [4, 4, 8, 8], 2)) == [A, A, S, S]                    # groups vote on their own
    with pytest.raises(AssertionError):
        sc.classify([5, 0], [4, 8], 2)                                                         # an env cannot count down beside an unlicensed neighbour
    with pytest.raises(AssertionError):
        sc.classify([5, 5], [3, 3], 2)
    case = sc.BY_NAME["edge_iid_1000"]
    assert sc.group_size(case, "quad") == 16 and sc.group_size(case, "lane") == 64
    assert sc.group_size(sc.BY_NAME["balance_wave_iid_1000"], None) == 1 and sc.group_size(sc.BY_NAME["balance_lane_iid_1000"], None) == 64


def test_oracle_sensitivity_is_far_below_the_tolerances():
    """The issue's recipe for a case that misses the project's tolerances (perturb the oracle's start q by 1e-13, allow 10 x the drift) was not
    needed; this keeps the measurement honest for the most sensitive cases: the drift stays below a hundredth of the tolerance."""
    for name in ("edge_singular_1000", "edge_singular_30", "edge_iid_1"):
        case = sc.BY_NAME[name]
        drift = sc.oracle_sensitivity(case)
        for key in ("q", "qd", "qd_target", "tcp_pos"):
            assert drift[key] < 1e-2 * case.tol_oracle[key], (name, key, drift)


def test_plumbing_is_declared_and_bound():
    from tactile_gym_amd import _capi
    from tactile_gym_amd.rl_envs import edge_follow, object_balance, object_push, surface_follow
    from tactile_gym_amd.vec_env import TactileVecEnv
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    assert re.search(r"\bint tg_copy_step_licence\s*\(tg_ctx\* ctx, int32_t\* host_dst\);", header) and "tg_copy_step_licence" in _capi.SYMBOLS
    assert re.search(r"#define TG_ABI_VERSION %d\b" % _capi.ABI_VERSION, header)              # a function added, no struct changed: the version stays
    assert callable(TactileVecEnv.step_licence)
    for cls in (edge_follow.EdgeFollowVecEnv, surface_follow.SurfaceFollowAutoVecEnv, surface_follow.SurfaceFollowGoalVecEnv,
                surface_follow.SurfaceFollowVertVecEnv, object_balance.ObjectBalanceVecEnv, object_push.ObjectPushVecEnv):
        assert inspect.signature(cls.__init__).parameters["max_force"].default is None, cls
