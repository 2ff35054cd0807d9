"""Test infrastructure (not collected): end-of-episode object states that decide which route the NEXT reset takes on the device - the reset
template (no tick), the optimistic move (arm-only ticks beside the frozen old object) or the literal move (every tick a contact tick) - and
what that reset must leave behind.  tests/test_reset_cases_cpu.py proves on the oracle that every case reaches the regime it is labelled with,
that the route predicted for it is consistent with what the oracle's own (literal) move does, and that nothing is decided on a knife edge;
tests/test_gpu_reset_states.py injects the same states into the device and compares its reset with the oracle's.

A case is placed RELATIVE to the env's state after a first reset(), handed to its `build` as `ref`: body_inject.reference plus
    path      [k][3]  the tip sphere's centre before every tick of the coming reset's move with the object out of the way, and at its end
    sphere_r          the sphere's radius
    half      [3]     the cube's half extents (push);   radius: the marble's radius of the episode that ends (roll)
`route` is the route the device must take with its defaults (closed-form narrowphase, wavefront mapping, template on); `claims` are (label,
predicate over the trace of the oracle's reset) pairs, trace_reset says what a row holds.  No case puts its smallest clear_distance within
0.5 mm of the device's 4 mm test: that is a condition on the inputs (test_reset_cases_cpu.py asserts it), not a tolerance."""
import math

import numpy as np

import body_cases as bc
import body_inject as bi
from body_cases import Z, rot

CLEAR = 0.004                        # the device's test: further than this from the old object
BAND = 0.0005                        # no case nearer than this to CLEAR
NEAR, FAR = CLEAR - BAND, CLEAR + BAND
# The largest cube speed a saturated action produced in 30 UR5 push steps on the oracle (test_reset_cases_cpu.py measures it again).  The marble:
# a kinematic bound - pressed under a tip that moves at 0.01 m/s at the most, its centre rolls at half the tip's speed (with the default embed
# distance of these tests the tip stays clear of a resting marble, and the measured speed is 0).
REACHABLE = {"push": 0.0096, "roll": 0.005}
BEYOND = 0.5


# ---------------------------------------------------------------------------------------------------------------------------------------
# the device's clear test, restated in plain f64
def tip_sphere(o, family):
    """(centre in the tip link's frame, radius) of the sphere the device tests: push - the AABB centre of the tip hull's vertices and the largest
    distance from it to a vertex; roll - the tip cylinder's centre and the distance to its rim."""
    sc = o.scene
    if family == "push":
        v = np.asarray(o._tip_verts, dtype=np.float64)
        c = 0.5 * (v.min(axis=0) + v.max(axis=0))
        return c, float(np.sqrt(((v - c) ** 2).sum(axis=1).max()))
    return np.array(sc.cyl_pos[:]), float(math.sqrt(sc.cyl_radius ** 2 + sc.cyl_half_len ** 2))


def sphere_centre(o, family):
    c, _ = tip_sphere(o, family)
    Rl, pl = o.arm.link_poses()[o.scene.tip_link]
    return np.asarray(pl, dtype=np.float64) + np.asarray(Rl, dtype=np.float64) @ c


DT = 1.0 / 240.0


def drift(ref, state):
    """What the device allows the old object to travel in a tick: dt (|v| + rho |w|), rho the farthest point from the object's centre."""
    rho = float(np.linalg.norm(ref["half"])) if "half" in ref else ref["radius"]
    return DT * float(np.linalg.norm(state["body_linvel"]) + rho * np.linalg.norm(state["body_angvel"]))


def clear_distances(ref, state, path):
    """Per path point k: push - the sphere centre's distance to the cube's box, less the sphere's radius; roll - its distance to the old marble's
    centre, less the old marble's radius and the sphere's radius; both less k drift, what the object may have travelled before tick k."""
    pos = np.asarray(state["body_pos"], dtype=np.float64)
    path = np.asarray(path, dtype=np.float64).reshape(-1, 3)
    allow = np.arange(len(path)) * drift(ref, state)
    if "half" in ref:
        R = np.asarray(state["body_rot"], dtype=np.float64).reshape(3, 3)
        loc = (path - pos) @ R                                   # R^T (p - pos), row by row
        out = np.maximum(np.abs(loc) - np.asarray(ref["half"]), 0.0)
        return np.sqrt((out ** 2).sum(axis=1)) - ref["sphere_r"] - allow
    return np.sqrt(((path - pos) ** 2).sum(axis=1)) - ref["radius"] - ref["sphere_r"] - allow


def clear_distance(ref, state, path):
    """The smallest of clear_distances over the path: the device takes its template when this is above CLEAR."""
    return float(clear_distances(ref, state, path).min())


def placed(ref, make, target, lo=0.0, hi=0.3):
    """make(d) for the d in [lo, hi] at which the smallest clear distance is `target` (it grows with d): bisection to 1e-12."""
    f = lambda d: clear_distance(ref, make(d), ref["path"]) - target
    assert f(lo) < 0.0 < f(hi), (f(lo), f(hi))
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) < 0.0 else (lo, mid)
    return make(0.5 * (lo + hi))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle's reset, tick by tick
def trace_reset(o, family):
    """Runs o.reset() and returns (observation, rows): one row per tick of the blocking move.  Before the tick: `centre` (the tip sphere), the
    three quantities of the move's exit test as the move computes them after it (pos_err against 2e-4, orn_err against 1e-3, jvel against
    0.1) and the object's position; after it: the tick's contacts (n, ids, table, tip_depth) and the object's position and speed.  rows[0]
    also carries "end": the sphere's centre after the move."""
    rows, targ = [], {}
    inner_tick, inner_move = o._step_simulation, o._blocking_move
    body = {"push": lambda: o.cube, "roll": lambda: o.ball}.get(family, lambda: o.body)

    def move(tpos, torn, tj, **kw):
        targ.update(pos=np.asarray(tpos, dtype=np.float64), orn=np.asarray(torn, dtype=np.float64))
        return inner_move(tpos, torn, tj, **kw)

    def tick():
        pos, _, orn, _, _ = o._tcp_world()
        r = dict(pos_err=float(np.sum(np.abs(targ["pos"] - pos))), jvel=float(np.sum(np.abs(o.arm.qd))),
                 orn_err=math.acos(float(np.clip(2 * (np.inner(targ["orn"], orn) ** 2) - 1, -1, 1))), obj_before=np.array(body().pos[:]))
        if family in ("push", "roll"):
            r["centre"] = sphere_centre(o, family)
        inner_tick()
        b = body()
        r.update(obj_after=np.array(b.pos[:]), speed=float(np.linalg.norm(b.linvel[:])))
        if family in ("push", "roll"):
            sc = o.scene
            ids = tuple(int(x) for x in sc.contact_ids[:sc.n_contacts])
            r.update(n=int(sc.n_contacts), ids=ids, table=sum(1 for x in ids if x < 8), tip_depth=float(sc.tip_depth))
        rows.append(r)

    o._step_simulation, o._blocking_move = tick, move
    try:
        obs = o.reset()
    finally:
        del o._step_simulation, o._blocking_move
    if family in ("push", "roll"):
        rows[0]["end"] = sphere_centre(o, family)
    return obs, rows


def exit_margins(rows):
    """Relative distance of each exit quantity from its threshold at the move's last tick and the one before: [(tick, name, value, threshold,
    |value - threshold| / threshold)]."""
    out = []
    for t in range(max(0, len(rows) - 2), len(rows)):
        for name, thr in (("pos_err", 2e-4), ("orn_err", 1e-3), ("jvel", 0.1)):
            out.append((t, name, rows[t][name], thr, abs(rows[t][name] - thr) / thr))
    return out


def path_of(rows):
    return np.array([r["centre"] for r in rows] + [rows[0]["end"]])


def move_away(o, family):
    """The oracle env's object out of every reach (1 m up), at rest: the reset that follows is the unobstructed move."""
    b = o.cube if family == "push" else o.ball
    b.pos[2] = 1.0
    for k in range(3):
        b.linvel[k] = 0.0
        b.angvel[k] = 0.0
    if family == "push":
        o.scene.mani.n = 0


def reference(o, twin, family):
    """body_inject.reference of the env after its first reset, with the path of its NEXT reset: `twin` is an env of the same seed and
    configuration in the same state, which is spent here - its object is taken out of the way and its second reset traced (object_roll's start
    pose depends on the marble drawn by that reset, so the path is the env's own; object_push's is the same in every env)."""
    ref = bi.reference(o, family)
    if family in ("push", "roll"):
        move_away(twin, family)
        _, rows = trace_reset(twin, family)
        ref.update(path=path_of(rows), sphere_r=tip_sphere(o, family)[1], clean_rows=rows, clean_q=twin.arm.q.copy(), clean_qd=twin.arm.qd.copy())
        if family == "push":
            ref["half"] = np.array(o.scene.half[:])
        else:
            ref["new_radius"] = float(twin.scaled_obj_radius)
    return ref


# ---------------------------------------------------------------------------------------------------------------------------------------
# predicates over a reset trace
def touches(tr):
    return any(bc.tip_touching(r) for r in tr)


def never_touches(tr):
    return not touches(tr)


def travel(tr):
    """How far the object's centre moved during the move."""
    return float(np.linalg.norm(tr[-1]["obj_after"] - tr[0]["obj_before"]))


NO_TOUCH = ("no tip contact in any tick of the oracle's move", never_touches)


# ---------------------------------------------------------------------------------------------------------------------------------------
# object_push
def _away(ref, target, R=None, **kw):
    """The cube moved along the push direction until its smallest clear distance is `target`."""
    push = bc._push_dir(ref)
    return placed(ref, lambda d: bc._cube(ref, R=R, dpos=d * push, **kw), target)


def _edge_on(ref, yaw_deg, target):
    """Yawed about the vertical, its vertical edge that looks at the tip on the line through the path's start along the push direction, and moved
    along that line: the edge is the cube's nearest feature to the path."""
    push = bc._push_dir(ref)
    R = rot(Z, yaw_deg) @ ref["body_rot"]
    edges = np.array([[sx, sy, 0.0] for sx in (-1, 1) for sy in (-1, 1)]) * 0.04
    world = (R @ edges.T).T
    e = world[np.argmin(world @ push)]

    def make(d):
        pos = ref["path"][0] + d * push - e
        pos[2] = ref["body_pos"][2]
        return dict(body_pos=pos, body_rot=R, body_linvel=np.zeros(3), body_angvel=np.zeros(3), goal_id=1)
    return placed(ref, make, target)


def _edge_is_nearest(ref, st):
    """The nearest path point lies in the Voronoi region of a vertical edge: outside the box in both horizontal axes, inside in the vertical."""
    k = int(np.argmin(clear_distances(ref, st, ref["path"])))
    loc = np.asarray(st["body_rot"]).reshape(3, 3).T @ (ref["path"][k] - st["body_pos"])
    d = np.abs(loc) - ref["half"]
    up = int(np.argmax(np.abs(np.asarray(st["body_rot"]).reshape(3, 3)[2])))          # the cube's axis that is vertical
    return all(d[a] > 0 for a in range(3) if a != up) and d[up] < 0


def _centred(ref):
    """The cube's centre on the tip sphere's centre at the rest pose: every direction is as deep as every other."""
    return dict(body_pos=np.array(ref["path"][0]), body_rot=ref["body_rot"], body_linvel=np.zeros(3), body_angvel=np.zeros(3), goal_id=1)


def _sliding_in(ref, speed, target=FAR):
    """Sliding towards the path, from where the smallest clear distance - the object's allowance of k drift included - is `target`."""
    return _away(ref, target, linvel=-speed * bc._push_dir(ref))


PUSH_CASES = [
    dict(name="where_reset_leaves_it", route="literal", regimes=["at_tip"], build=lambda ref: bc._cube(ref),
         claims=[("four table vertices in every tick", lambda tr: all(r["table"] == 4 for r in tr))]),
    dict(name="clear_3.5", route="literal", regimes=["just_inside"], build=lambda ref: _away(ref, NEAR), claims=[NO_TOUCH]),
    dict(name="clear_4.5", route="template", regimes=["just_outside"], build=lambda ref: _away(ref, FAR), claims=[NO_TOUCH]),
    dict(name="far_10cm", route="template", regimes=["far"], build=lambda ref: bc._cube(ref, dpos=0.10 * bc._push_dir(ref)), claims=[NO_TOUCH]),
    dict(name="edge_30_3.5", route="literal", regimes=["edge_just_inside"], build=lambda ref: _edge_on(ref, 30.0, NEAR), geometry=_edge_is_nearest, claims=[NO_TOUCH]),
    dict(name="edge_30_4.5", route="template", regimes=["edge_just_outside"], build=lambda ref: _edge_on(ref, 30.0, FAR), geometry=_edge_is_nearest, claims=[NO_TOUCH]),
    dict(name="edge_45_3.5", route="literal", regimes=["edge_just_inside"], build=lambda ref: _edge_on(ref, 45.0, NEAR), geometry=_edge_is_nearest, claims=[NO_TOUCH]),
    dict(name="edge_45_4.5", route="template", regimes=["edge_just_outside"], build=lambda ref: _edge_on(ref, 45.0, FAR), geometry=_edge_is_nearest, claims=[NO_TOUCH]),
    dict(name="into_tip_5mm", route="literal", regimes=["deep_overlap_tick0"], build=lambda ref: bc._cube(ref, dpos=-5e-3 * bc._push_dir(ref)),
         claims=[("the tip more than 1 mm deep in the first tick", lambda tr: tr[0]["tip_depth"] < -1e-3)]),
    dict(name="centred_on_tip", route="literal", regimes=["degenerate_normal"], build=_centred,
         claims=[("the tip in contact in the first tick", lambda tr: bc.tip_touching(tr[0]))]),
    dict(name="in_the_air_2cm", route="literal", regimes=["falls_during_move"], build=lambda ref: bc._cube(ref, dpos=(0, 0, 0.02)),
         claims=[("no table contact in the first tick, the cube lower after the move", lambda tr: tr[0]["table"] == 0 and tr[-1]["obj_after"][2] < tr[0]["obj_before"][2])]),
    dict(name="edge_44_far", route="template", regimes=["two_vertex_code"],
         build=lambda ref: bc._cube(ref, R=rot(bc._push_dir(ref), 44), dpos=0.10 * bc._push_dir(ref), on_table=True),
         claims=[NO_TOUCH, ("two table vertices in every tick", lambda tr: all(r["table"] == 2 for r in tr))]),
    dict(name="other_face_far", route="template", regimes=["other_face_code"],
         build=lambda ref: bc._cube(ref, R=rot(bc._push_dir(ref), 90), dpos=0.10 * bc._push_dir(ref), on_table=True),
         claims=[NO_TOUCH, ("four table vertices in every tick", lambda tr: all(r["table"] == 4 for r in tr))]),
    dict(name="sliding_in_reachable", route="template", regimes=["moving_reachable"], moving="reachable", build=lambda ref: _sliding_in(ref, 2 * REACHABLE["push"]),
         claims=[NO_TOUCH]),
    dict(name="sliding_in_reachable_3.5", route="literal", regimes=["moving_reachable_inside"], moving="reachable",
         build=lambda ref: _sliding_in(ref, 2 * REACHABLE["push"], NEAR), claims=[NO_TOUCH]),
    dict(name="sliding_in_0.5", route="template", regimes=["moving_beyond_reach"], moving="beyond_reach", build=lambda ref: _sliding_in(ref, BEYOND),
         claims=[NO_TOUCH, ("the cube slides further than the 4 mm of the clear test unless the move is a single tick", lambda tr: len(tr) == 1 or travel(tr) > CLEAR)]),
    dict(name="sliding_in_0.5_3.5", route="literal", regimes=["moving_beyond_reach_inside"], moving="beyond_reach", build=lambda ref: _sliding_in(ref, BEYOND, NEAR),
         claims=[NO_TOUCH]),
    # 4.5 mm off the path by the geometry alone: frozen, the cube would pass every test of the move; sliding, it is on the MG400's tip within its 13 ticks
    dict(name="sliding_in_0.5_from_4.5", route="literal", regimes=["moving_beyond_reach_arrives"], moving="beyond_reach",
         build=lambda ref: dict(_away(ref, FAR), body_linvel=-BEYOND * bc._push_dir(ref)),
         claims=[("the tip touches the cube in a move of more than one tick", lambda tr: len(tr) == 1 or touches(tr))]),
    dict(name="last_goal_reached", route="template", regimes=["last_goal"], build=lambda ref: dict(bc._cube(ref, dpos=0.10 * bc._push_dir(ref)), goal_id=len(ref["goals"])),
         claims=[NO_TOUCH]),
]


# ---------------------------------------------------------------------------------------------------------------------------------------
# object_roll: no template; the clear test uses the OLD marble's radius, the move's start pose the NEW one's
def _marble_beside(ref, target, direction=(1.0, 0.0), velocity=None):
    """The old marble on the table, moved sideways from under the path's end until its smallest clear distance is `target`.  velocity(position):
    the (linear, angular) velocity it has there."""
    u = np.array([direction[0], direction[1], 0.0]) / math.hypot(*direction)
    base = np.array([ref["path"][-1][0], ref["path"][-1][1], ref["radius"]])

    def make(d):
        v, w = (np.zeros(3), np.zeros(3)) if velocity is None else velocity(base, base + d * u)
        return dict(body_pos=base + d * u, body_rot=np.eye(3), body_linvel=v, body_angvel=w)
    return placed(ref, make, target, lo=1e-6)


def _rolling_in(ref, speed, graze=False, target=FAR):
    """Rolling without slip towards the point under the path's end, from where the smallest clear distance - allowance included - is `target`.
    graze: aimed to pass 2 mm clear of the tip's cylinder instead, through the sphere the device tests but past the cap: a marble that HITS the
    cap at 0.5 m/s changes the oracle's own tick count under a 1e-9 shift (measured), which no comparison can be built on."""
    def velocity(base, pos):
        away = pos - base
        dist = float(np.linalg.norm(away))
        d = -away / dist
        if graze:
            miss = ref["cap_radius"] + ref["radius"] + 2e-3
            d = rot(Z, math.degrees(math.asin(min(1.0, miss / dist)))) @ d
        v = speed * d
        return v, np.cross(Z, v) / ref["radius"]
    return _marble_beside(ref, target, velocity=velocity)


ROLL_CASES = [
    dict(name="beside_3.5", route="literal", regimes=["just_inside"], build=lambda ref: _marble_beside(ref, NEAR), claims=[NO_TOUCH]),
    dict(name="beside_4.5", route="optimistic", regimes=["just_outside"], build=lambda ref: _marble_beside(ref, FAR), claims=[NO_TOUCH]),
    dict(name="under_start_pose", route="literal", regimes=["under_tip"], build=lambda ref: bc._marble(ref),
         geometry=lambda ref, st: float(np.linalg.norm((st["body_pos"] - ref["path"][-1])[:2])) < 0.5 * ref["cap_radius"],     # the tip's cylinder around the centre
         claims=[("the marble stays on the table", lambda tr: all(r["table"] == 1 for r in tr))]),
    dict(name="rolling_in_reachable", route="optimistic", regimes=["moving_reachable"], moving="reachable", build=lambda ref: _rolling_in(ref, 2 * REACHABLE["roll"]),
         claims=[NO_TOUCH]),
    dict(name="rolling_in_reachable_3.5", route="literal", regimes=["moving_reachable_inside"], moving="reachable",
         build=lambda ref: _rolling_in(ref, 2 * REACHABLE["roll"], target=NEAR), claims=[NO_TOUCH]),
    dict(name="rolling_in_0.5", route="optimistic", regimes=["moving_beyond_reach"], moving="beyond_reach", build=lambda ref: _rolling_in(ref, BEYOND, graze=True),
         claims=[NO_TOUCH, ("the marble travels more than the 4 mm of the clear test during the move", lambda tr: travel(tr) > CLEAR)]),
]

# ---------------------------------------------------------------------------------------------------------------------------------------
# object_balance: k_reset_body takes the arm's post-reset state from the template that env 0 computed in the first reset, whatever hangs on the
# constraint; the oracle moves with the object where the episode left it.  The regime of these cases is the injected state itself (`geometry`).
def _arm_far(ref):
    """The TCP 8 cm from the start pose along work-frame x, every joint moving at 0.5 rad/s; the object upright on it."""
    q, pivot = ref["ik"](np.array([0.08, 0.0, 0.0]))
    st = bc._hung(ref, ref["body_rot"], pivot=pivot, q=q)
    st["qd"] = np.full_like(q, 0.5)
    return st


def _tilt_deg(R0, R):
    return math.degrees(math.acos(float(np.clip((np.asarray(R0)[:, 2] @ np.asarray(R)[:, 2]), -1.0, 1.0))))


ONE_TICK = ("the move takes one tick, as from the reset pose", lambda tr: len(tr) == 1)
ARM_FAR = dict(name="arm_far_moving", route="template", regimes=["arm_far"], build=_arm_far, claims=[ONE_TICK],
               geometry=lambda ref, st: float(np.abs(st["qd"]).min()) >= 0.5 and float(np.linalg.norm(st["body_pos"] - ref["body_pos"])) > 0.05)

POLE_CASES = [
    dict(name="fallen_52.5_5rad", route="template", regimes=["fallen_fast"], claims=[ONE_TICK],
         build=lambda ref: bc._hung(ref, bc.rpy_mat(math.radians(1.5 * 35.0), 0.0, -math.pi / 2), angvel=(5.0, 0.0, 0.0)),
         geometry=lambda ref, st: abs(_tilt_deg(ref["body_rot"], st["body_rot"]) - 52.5) < 1e-6 and abs(st["body_angvel"][2]) < 1e-12),
    ARM_FAR,
]
BALL_CASES = [
    dict(name="ball_at_rim", route="template", regimes=["ball_at_rim"], claims=[ONE_TICK], build=lambda ref: bc._ball(ref, local=(ref["plate_radius"] - 0.004, 0, 0)),
         geometry=lambda ref, st: 0.0 < ref["plate_radius"] - float(np.linalg.norm((st["ball_pos"] - ref["ball_pos"])[:2])) < 0.005),
    dict(name="ball_off_plate", route="template", regimes=["ball_off_plate"], claims=[ONE_TICK],
         build=lambda ref: bc._ball(ref, local=(ref["plate_radius"] + 2 * ref["ball_radius"], 0, 0)),
         geometry=lambda ref, st: float(np.linalg.norm((st["ball_pos"] - ref["ball_pos"])[:2])) > ref["plate_radius"] + ref["ball_radius"]),
    ARM_FAR,
]
SPIN_CASES = [
    dict(name="dish_tilted_3", route="template", regimes=["dish_tilted"], claims=[ONE_TICK], build=lambda ref: bc._dish(ref, R=rot(bc.X, 3.0), dpos=(0, 0, 5e-4)),
         geometry=lambda ref, st: abs(_tilt_deg(ref["dish_rot"], st["dish_rot"]) - 3.0) < 1e-6),
    dict(name="dish_lifted_2cm", route="template", regimes=["dish_lifted"], claims=[ONE_TICK], build=lambda ref: bc._dish(ref, dpos=(0, 0, 0.02)),
         geometry=lambda ref, st: abs(st["dish_pos"][2] - ref["dish_pos"][2] - 0.02) < 1e-12),
    dict(name="dish_spin_20", route="template", regimes=["dish_spinning"], claims=[ONE_TICK], build=lambda ref: bc._dish(ref, angvel=(0, 0, 20.0)),
         geometry=lambda ref, st: st["dish_angvel"][2] == 20.0),
    ARM_FAR,
]

FAMILIES = {
    "push": dict(cases=PUSH_CASES, regimes={"at_tip", "just_inside", "just_outside", "far", "edge_just_inside", "edge_just_outside", "deep_overlap_tick0",
                                            "degenerate_normal", "falls_during_move", "two_vertex_code", "other_face_code", "moving_reachable",
                                            "moving_beyond_reach", "moving_reachable_inside", "moving_beyond_reach_inside", "moving_beyond_reach_arrives", "last_goal"}),
    "roll": dict(cases=ROLL_CASES, regimes={"just_inside", "just_outside", "under_tip", "moving_reachable", "moving_reachable_inside", "moving_beyond_reach",
                                            "smallest_just_inside", "smallest_just_outside", "largest_just_inside", "largest_just_outside",
                                            "new_marble_larger", "new_marble_smaller"}),
    "pole": dict(cases=POLE_CASES, regimes={"fallen_fast", "arm_far"}),
    "ball": dict(cases=BALL_CASES, regimes={"ball_at_rim", "ball_off_plate", "arm_far"}),
    "spin": dict(cases=SPIN_CASES, regimes={"dish_tilted", "dish_lifted", "dish_spinning", "arm_far"}),
}
VARIANTS = list(bc.VARIANTS)


def case_of_env(family, radii=None):
    """Env -> case index (None: the env keeps its reset state), the cases dealt in turn as body_cases.assign deals them.  object_roll: the envs
    whose old marble is the smallest and the largest of the batch carry the 3.5 mm and the 4.5 mm case (two envs at either end of the range).
    The marble's radius is drawn by the reset itself and is no field of the injection entry, so 'smallest', 'largest' and 'a new marble larger /
    smaller than the old one' are what the 70 seeds drew - 1.0 .. 2.0 times 2.5 mm, the extremes within 2 % of the range's ends - and the CPU
    test asserts that every one of these regimes is reached."""
    cases = FAMILIES[family]["cases"]
    out = bc.assign(len(cases))
    if family == "roll" and radii is not None:
        order = [i for i in np.argsort(radii) if out[i] is not None]
        names = [c["name"] for c in cases]
        out[order[0]], out[order[1]] = names.index("beside_3.5"), names.index("beside_4.5")
        out[order[-1]], out[order[-2]] = names.index("beside_3.5"), names.index("beside_4.5")
    return out


def roll_regimes(case_name, i, radii, new_radii, cases):
    """The regimes an object_roll env reaches by the marbles its seed drew, beside those of its case."""
    out = set()
    held = [k for k in range(len(radii)) if cases[k] is not None]
    order = sorted(held, key=lambda k: radii[k])
    if case_name in ("beside_3.5", "beside_4.5"):
        side = "inside" if case_name == "beside_3.5" else "outside"
        if i in order[:2]:
            out.add("smallest_just_" + side)
        if i in order[-2:]:
            out.add("largest_just_" + side)
    out.add("new_marble_larger" if new_radii[i] > radii[i] else "new_marble_smaller")
    return out


def device_route(case, nph, mapping, template=True):
    """The route the device takes for a case in a batch: the lane mapping and the GJK / manifold narrowphase always move literally; without the
    template (reset_bank off, object_roll) a template case moves optimistically."""
    if mapping == "lane" or nph == "gjk_manifold":
        return "literal"
    if case["route"] == "template" and not template:
        return "optimistic"
    return case["route"]


def prepare(family, arm, sensor, nph, max_steps=50):
    """The batch's oracle envs after their first reset (env i seeded seed + i), per env the reference its case is placed by (the twins are made and
    spent here), and the case index per env."""
    oracles = [bi.make_oracle(family, i, arm=arm, sensor=sensor, narrowphase=nph, max_steps=max_steps) for i in range(bc.N_ENVS)]
    refs, first_obs = [], []
    for i, o in enumerate(oracles):
        first_obs.append(o.reset())
        twin = None
        if family in ("push", "roll"):
            twin = bi.make_oracle(family, i, arm=arm, sensor=sensor, narrowphase=nph, max_steps=max_steps)
            twin.reset()
        ref = reference(o, twin, family)
        ref["first_obs"] = first_obs[-1]
        refs.append(ref)
    cases = case_of_env(family, radii=[r["radius"] for r in refs] if family == "roll" else None)
    return oracles, refs, cases
