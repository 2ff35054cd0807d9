"""The end-of-episode states of tests/reset_cases.py, on the CPU oracle alone: every case reaches the regime it is labelled with, the reset route
predicted for the device is consistent with what the oracle's own move does (a template or optimistic case never touches the tip; a literal
case is inside the 3.5 mm), nothing is decided on a knife edge (the move's exit test, the 4 mm test, the contact ids under a 1e-9 shift), and a
moving object stays within the allowance that the device's clear test makes for it.  The whole
batch is run as tests/test_gpu_reset_states.py runs it: env i seeded seed + i, reset once, the cases dealt over the envs, reset again."""
import math

import numpy as np
import pytest

import body_cases as bc
import body_inject as bi
import reset_cases as rc

ORACLE_VARIANTS = [("push", arm, sensor, nph) for arm, sensor in (("ur5", "tactip"), ("mg400", "digitac")) for nph in ("closed_form", "gjk_manifold")] \
    + [(f, "ur5", "tactip", None) for f in ("roll", "pole", "ball", "spin")]
SHIFT = 1e-9
DIAG = np.array([0.6, -0.48, 0.64])
TIP_SHARE, OBJECT_SLACK = 1e-3, 1.8e-3      # of the device's 4 mm (csrc/tg_contact_wave.hip: k_reset_contact_wave): the tip's travel in a tick, the object's beyond its allowance
_runs = {}


def shifted(st, family, shift):
    key = "dish_pos" if "dish_pos" in st else ("ball_pos" if "ball_pos" in st else "body_pos")
    st = dict(st)
    st[key] = np.asarray(st[key], dtype=np.float64) + shift * DIAG
    return st


def run_batch(family, arm, sensor, nph, shift=0.0):
    """Per env a dict: case (None: not injected), state, ref, trace of the second reset, the oracle's report after it, its tick count; cached."""
    key = (family, arm, sensor, nph, shift)
    if key in _runs:
        return _runs[key]
    oracles, refs, cases = rc.prepare(family, arm, sensor, nph)
    out = []
    for i, o in enumerate(oracles):
        case = None if cases[i] is None else rc.FAMILIES[family]["cases"][cases[i]]
        st = None
        if case is not None:
            st = case["build"](refs[i])
            bi.inject_oracle(o, family, shifted(st, family, shift) if shift else st)
        _, tr = rc.trace_reset(o, family)
        out.append(dict(case=case, state=st, ref=refs[i], trace=tr, report=bi.oracle_report(o, family), ticks=int(o.reset_ticks)))
    _runs[key] = out
    return out


@pytest.mark.parametrize("family,arm,sensor,nph", ORACLE_VARIANTS)
def test_every_case_reaches_its_regime_in_every_env_that_carries_it(family, arm, sensor, nph):
    f = rc.FAMILIES[family]
    batch = run_batch(family, arm, sensor, nph)
    seen = set()
    held = [None if e["case"] is None else f["cases"].index(e["case"]) for e in batch]
    for i, e in enumerate(batch):
        case = e["case"]
        if case is None:
            continue
        for label, claim in case["claims"]:
            assert claim(e["trace"]), (family, arm, nph, "env", i, case["name"], label)
        if "geometry" in case:
            assert case["geometry"](e["ref"], e["state"]), (family, arm, nph, "env", i, case["name"], "geometry")
        seen.update(case["regimes"])
        if family == "roll":
            seen |= rc.roll_regimes(case["name"], i, [x["ref"]["radius"] for x in batch], [x["ref"]["new_radius"] for x in batch], held)
        if family in ("push", "roll"):          # a condition on the inputs: nothing within 0.5 mm of the device's 4 mm (1e-9: the bisection's and rounding's)
            d = rc.clear_distance(e["ref"], e["state"], e["ref"]["path"])
            assert abs(d - rc.CLEAR) >= rc.BAND - 1e-9, (i, case["name"], d)
    assert f["regimes"] <= seen, f["regimes"] - seen
    assert {k for k in held if k is not None} == set(range(len(f["cases"])))
    assert all(held[i] is not None for i in (0, 63, 64, 69)) and sum(k is None for k in held) == len(bc.UNINJECTED)
    # no two cases of the family hold the same state (one env's reference)
    ref = batch[0]["ref"]
    states = [c["build"](ref) for c in f["cases"]]
    for a in range(len(states)):
        for b in range(a + 1, len(states)):
            same = set(states[a]) == set(states[b]) and all(np.array_equal(np.asarray(states[a][k]), np.asarray(states[b][k])) for k in states[a])
            assert not same, (f["cases"][a]["name"], f["cases"][b]["name"])


@pytest.mark.parametrize("family,arm,sensor,nph", [v for v in ORACLE_VARIANTS if v[0] in ("push", "roll")])
def test_the_predicted_route_is_consistent_with_the_oracle(family, arm, sensor, nph):
    """A template or optimistic case: the tip never touches the object in the oracle's (literal) move, and the arm ends where the unobstructed move
    ends, bit for bit - freezing the object changes nothing.  A literal case is inside the 3.5 mm.  The smallest clear distance is the device's:
    with the allowance of k dt (|v| + rho |w|) for what the object may have travelled before tick k.  And the allowance holds: before every tick
    the oracle's object has moved by less than it plus the 1.8 mm that the 4 mm keep for an object that picks up speed (a cube tipping from rest);
    the tip travels less than its 1 mm between two tests."""
    worst_travel, worst_excess = 0.0, -1.0
    for i, e in enumerate(run_batch(family, arm, sensor, nph)):
        case, tr = e["case"], e["trace"]
        if case is None:
            continue
        d = rc.clear_distance(e["ref"], e["state"], e["ref"]["path"])
        tag = (family, arm, nph, i, case["name"], d)
        assert np.linalg.norm(np.diff(e["ref"]["path"], axis=0), axis=1).max() < TIP_SHARE
        if case["route"] in ("template", "optimistic"):
            assert d >= rc.FAR - 1e-9, tag
            assert rc.never_touches(tr), tag
            assert e["ticks"] == len(e["ref"]["clean_rows"]) and np.array_equal(e["report"]["q"], e["ref"]["clean_q"]), tag
            per_tick = rc.drift(e["ref"], e["state"])
            for k, r in enumerate(tr):
                excess = float(np.linalg.norm(r["obj_before"] - tr[0]["obj_before"])) - k * per_tick
                worst_excess = max(worst_excess, excess)
                assert excess < OBJECT_SLACK, tag + (k, excess)
        else:
            assert d <= rc.NEAR + 1e-9, tag
        if case.get("moving") == "reachable":
            worst_travel = max(worst_travel, rc.travel(tr))
            assert rc.travel(tr) < 1e-3 and rc.never_touches(tr), tag + (rc.travel(tr),)
    print(f"RESETCASES {family} {arm} {nph}: a reachable moving object travels at most {worst_travel * 1e3:.3f} mm during the move; a frozen object "
          f"exceeds its allowance by at most {worst_excess * 1e3:.3f} mm")


@pytest.mark.parametrize("family,arm,sensor,nph", ORACLE_VARIANTS)
def test_nothing_is_decided_on_a_knife_edge(family, arm, sensor, nph):
    """The three quantities of the blocking move's exit test, at its last tick and the one before, are at least 1 % of the threshold off it; the
    tick count, the contact ids and the goal index after the reset are the same with the injected position moved by 1e-9."""
    a, b = run_batch(family, arm, sensor, nph), run_batch(family, arm, sensor, nph, shift=SHIFT)
    worst = 1.0
    for i, (e, e2) in enumerate(zip(a, b)):
        name = "-" if e["case"] is None else e["case"]["name"]
        for t, what, value, thr, rel in rc.exit_margins(e["trace"]):
            worst = min(worst, rel)
            assert rel >= 0.01, (family, arm, nph, i, name, t, what, value, thr)
        assert e["ticks"] == e2["ticks"], (i, name)
        for key in ("contact_count", "contact_ids", "goal_id"):
            if key in e["report"]:
                assert e["report"][key] == e2["report"][key], (i, name, key, e["report"][key], e2["report"][key])
        # conditioning: both sides are injected with the same f64 numbers, so what reaches the device comparison is the rounding of the two
        # arithmetics (1e-15 of the state) times the amplification measured here; it has to stay below a hundredth of the tolerance q_tol
        amp = np.abs(e["report"]["q"] - e2["report"]["q"]).max() / SHIFT
        assert amp * 1e-15 < 0.01 * bc.FAMILIES[family]["tol"][0], (i, name, amp)
    del _runs[(family, arm, sensor, nph, SHIFT)]
    print(f"RESETCASES {family} {arm} {nph}: the exit quantities are at least {100 * worst:.1f} % off their thresholds")


def _saturated_speed(family):
    """The largest object speed over the ticks of 30 steps with a saturated action, from the reset pose (UR5)."""
    o = bi.make_oracle(family, 0)
    o.reset()
    b = o.cube if family == "push" else o.ball
    inner, top = o._step_simulation, [0.0]

    def tick():
        inner()
        top[0] = max(top[0], float(np.linalg.norm(b.linvel[:])))
    o._step_simulation = tick
    for _ in range(30):
        o.step(np.array([0.25, 0.0] if family == "push" else [0.25, 0.25], dtype=np.float32))
    del o._step_simulation
    return top[0]


@pytest.mark.parametrize("family", ["push", "roll"])
def test_reachable_speed_is_what_the_cases_assume(family):
    v = _saturated_speed(family)
    print(f"RESETCASES {family}: a saturated action moves the object at up to {v:.4f} m/s")
    if family == "push":
        assert 0.5 * rc.REACHABLE[family] < v <= 1.05 * rc.REACHABLE[family], v
    else:       # the tip of this configuration stays 0.25 mm clear of a resting marble: REACHABLE is the kinematic bound, not a measurement
        assert v <= rc.REACHABLE[family], v


