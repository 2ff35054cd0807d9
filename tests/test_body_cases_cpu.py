"""The injected object states of tests/body_cases.py, on the CPU oracle alone: every case reaches the regime it is labelled with (read tick by
tick), is well conditioned against the tolerance the device comparison uses, and decides nothing on a knife edge.  The whole batch of 70 envs is
run as tests/test_gpu_body_states.py runs it - env i seeded seed + i, the cases dealt over the envs, the same actions - so a claim holds for
every env that carries the case, whatever gravity, embed distance, radius or trajectory its seed drew."""
import numpy as np
import pytest

import body_cases as bc
import body_inject as bi

ORACLE_VARIANTS = [("push", arm, sensor, nph) for arm, sensor in (("ur5", "tactip"), ("mg400", "digitac")) for nph in ("closed_form", "gjk_manifold")] \
    + [(f, "ur5", "tactip", None) for f in ("roll", "pole", "ball", "spin")]
SHIFT = 1e-12           # the perturbation of the conditioning check [m]
MARGIN = 1e-6           # decisions at a step's end stay this far (relative to the threshold) off the threshold

_runs = {}


DIAG = (0.6, -0.48, 0.64)
# The GJK / EPA narrowphase is not continuous: where two features of the tip core's hull are equally deep, the witness point (and with it the
# state two steps later, by 1e-7 .. 1e-5) depends on the last bit of the cube's position.  One shift can miss such a place, so its variants are
# probed at more sizes and in more directions; every probe has to meet the same bound.
PROBES = {None: [(SHIFT, DIAG)], "closed_form": [(SHIFT, DIAG)],
          "gjk_manifold": [(SHIFT, DIAG), (1e-15, (1, 0, 0)), (1e-14, (0, 1, 0)), (1e-13, (0, 0, 1)), (1e-13, DIAG), (1e-11, (1, 0, 0)), (1e-11, (0, 1, 0)), (1e-10, DIAG)]}


def run_batch(family, arm, sensor, nph, shift=0.0, direction=DIAG):
    """Per env: (case index or None, trace, report after each step) of the whole batch; cached - the tests below share one run per variant."""
    key = (family, arm, sensor, nph, shift, tuple(direction))
    if key in _runs:
        return _runs[key]
    f = bc.FAMILIES[family]
    oracles = [bi.make_oracle(family, i, arm=arm, sensor=sensor, narrowphase=nph) for i in range(bc.N_ENVS)]
    for o in oracles:
        o.reset()
    cases = bi.case_of_env(family, radii=[o.scaled_obj_radius for o in oracles] if family == "roll" else None)
    acts = bi.case_actions(family, cases)
    out = []
    for i, o in enumerate(oracles):
        if cases[i] is not None:
            st = f["cases"][cases[i]]["build"](bi.reference(o, family))
            if shift:
                key_pos = "dish_pos" if family == "spin" else ("ball_pos" if family == "ball" and "ball_pos" in st else "body_pos")
                st = dict(st)
                st[key_pos] = np.asarray(st[key_pos], dtype=np.float64) + shift * np.array(direction, dtype=np.float64)
            bi.inject_oracle(o, family, st)
        reports = []
        tr = []
        for s in range(bc.STEPS):
            rows = bi.trace(o, family, acts[s:s + 1, i])
            for r in rows:
                r["step"] = s
            tr += rows
            reports.append(bi.oracle_report(o, family))
            if rows[0]["ends"][0]["done"]:
                break
        tr[0]["ends"] = [e for r in tr if "ends" in r for e in r["ends"]]
        out.append((cases[i], tr, reports))
    _runs[key] = out
    return out


@pytest.mark.parametrize("family,arm,sensor,nph", ORACLE_VARIANTS)
def test_every_case_reaches_its_regime_in_every_env_that_carries_it(family, arm, sensor, nph):
    f = bc.FAMILIES[family]
    seen = set()
    batch = run_batch(family, arm, sensor, nph)
    for i, (k, tr, _) in enumerate(batch):
        if k is None:
            continue
        case = f["cases"][k]
        regimes, claims = bc.case_claims(case, family, arm, nph)
        for label, claim in claims:
            assert claim(tr), (family, arm, nph, "env", i, case["name"], label)
        seen.update(regimes)
    # coverage: every regime the family must contain is present.  The one exemption is named, holds for one batch, and is not counted as reached there
    exempt = bc.not_testable(family, arm, nph)
    assert bc.NOT_TESTABLE == {("push", "mg400", "gjk_manifold"): {"tip_on_cube_edge"}}
    assert not exempt & seen, exempt & seen
    assert f["regimes"] - exempt <= seen, f["regimes"] - exempt - seen
    for label, claim in f.get("family_claims", []):
        assert claim([(f["cases"][k]["name"], tr) for k, tr, _ in batch if k is not None]), (family, label)


def _history(tr, family):
    """What a lane's contact loops did over the ticks of both steps: the contact ids (push, roll), the ball's contact flag, the dish's manifold
    count; the pole has no contact, its lanes differ in when they terminate."""
    if family in ("push", "roll"):
        return tuple(r["ids"] for r in tr)
    if family == "ball":
        return tuple(r["ball_touch"] for r in tr)
    if family == "spin":
        return tuple(r["spin_n"] for r in tr)
    return tuple(e["done"] for e in tr[0]["ends"])


@pytest.mark.parametrize("family,arm,sensor,nph", ORACLE_VARIANTS)
def test_lane_layout_mixes_regimes(family, arm, sensor, nph):
    """Lanes 0, 63, 64 and 69 hold cases, a few envs stay un-injected, and the first wavefront of the lane mapping runs at least four different
    contact sets in the same tick and at least four different traced contact histories (_history), not merely four case indices.  The marble has
    two contacts at the most (its first-tick sets are two of the four there are); the pole has none, so its wavefront has to hold all three
    termination histories instead: done in the first step, in the second, in neither."""
    batch = run_batch(family, arm, sensor, nph)
    cases = [k for k, _, _ in batch]
    assert all(cases[i] is not None for i in (0, 63, 64, 69)) and sum(k is None for k in cases) == len(bc.UNINJECTED)
    assert len({k for k in cases if k is not None}) == len(bc.FAMILIES[family]["cases"])
    histories = {_history(tr, family) for _, tr, _ in batch[:64]}
    if family == "pole":
        assert histories == {(True,), (False, True), (False, False)}, histories
    else:
        assert len(histories) >= 4, histories
    if family != "pole":                                                 # within one tick: (tick, different sets) - the ball touches or does not, the
        for t, need in {"push": [(0, 4)], "roll": [(0, 2)], "ball": [(0, 2), (11, 2)], "spin": [(0, 2), (11, 3)]}[family]:      # dish has 0, 1 or 2 points
            sets = {_history(tr, family)[t] for _, tr, _ in batch[:64] if len(tr) > t}
            assert len(sets) >= need, (t, sets)


@pytest.mark.parametrize("family,arm,sensor,nph", ORACLE_VARIANTS)
def test_cases_are_well_conditioned(family, arm, sensor, nph):
    """The injected position moved by 1e-12: after both steps joints and object move by less than a tenth of the device comparison's tolerance,
    and the contact-id history, the dones and the goal indices are the same."""
    q_tol, pose_tol = bc.FAMILIES[family]["tol"]
    a = run_batch(family, arm, sensor, nph)
    worst = 0.0
    for shift, direction in PROBES[nph]:
        b = run_batch(family, arm, sensor, nph, shift=shift, direction=direction)
        grow = max(1.0, shift / SHIFT)               # a larger probe may move the result in proportion: the bound is one on the amplification
        for i, ((k, tr, rep), (_, tr2, rep2)) in enumerate(zip(a, b)):
            if k is None:
                continue
            name = (bc.FAMILIES[family]["cases"][k]["name"], shift, direction)
            assert len(tr) == len(tr2) and len(rep) == len(rep2), (i, name)
            for key in ("ids", "ball_touch", "spin_n"):
                assert [r.get(key) for r in tr] == [r.get(key) for r in tr2], (i, name, key)
            assert [(e["done"], e.get("goal_id")) for e in tr[0]["ends"]] == [(e["done"], e.get("goal_id")) for e in tr2[0]["ends"]], (i, name)
            for r1, r2 in zip(rep, rep2):
                assert np.abs(r1["q"] - r2["q"]).max() < 0.1 * q_tol * grow, (i, name, np.abs(r1["q"] - r2["q"]).max())
                for key in ("body_pos", "body_rot", "ball_pos", "dish"):
                    if key in r1:
                        d = float(np.abs(np.asarray(r1[key])[:12] - np.asarray(r2[key])[:12]).max())
                        worst = max(worst, d)
                        assert d < 0.1 * pose_tol * grow, (i, name, key, d)
        del _runs[(family, arm, sensor, nph, shift, tuple(direction))]
    print(f"{family} {arm} {nph}: the shifts of the injected position move the object by at most {worst:.2e} after two steps")


@pytest.mark.parametrize("family,arm,sensor,nph", ORACLE_VARIANTS)
def test_no_decision_on_a_knife_edge(family, arm, sensor, nph):
    """Fall angle, fall distance, goal distance: every quantity compared with a threshold at a step's end is off it by 1e-6 of the threshold, in
    the injected envs and in the others."""
    for i, (k, tr, _) in enumerate(run_batch(family, arm, sensor, nph)):
        for s, e in enumerate(tr[0]["ends"]):
            for value, thr in e["margins"]:
                if family == "push" and k is None and e["goal_id"] <= 1 and abs(value - thr) < 1e-12:
                    continue     # PARITY_ASSUMPTIONS A29, the envs left at the reset pose only: goal 0 lies EXACTLY the termination distance from the
                                 # cube's start, so until the tip has moved the cube the reference itself decides by rounding noise
                assert abs(value - thr) >= MARGIN * thr, (family, i, k, s, value, thr)
