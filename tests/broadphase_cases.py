"""The pose sets of the broadphase guard's exact tests (tests/test_broadphase_exact_cpu.py, tests/test_gpu_broadphase_exact.py): joint states at which
the guard (csrc/tg_broadphase.hip, oracle/broadphase.py) is compared with exact float64 geometry (tests/broadphase_f64.py), not only with itself.

Per arm (ARMS: the UR5 with the standard TacTip in edge_follow, where the edge stimulus is and the tip is filtered out, and in surface_follow, where the
tip's 1089-vertex hull is not; the UR5 with the standard DIGIT in surface_follow; the MG400 with the right-angle DigiTac in object_push - on the CPU
only: tg_set_joint_state refuses an env with a free object - and with the standard DigiTac in edge_follow, on the device as well) a pose set is
  * N_RANDOM seeded random joint states, rest + U(-SPREAD, SPREAD) rad (the MG400's parallel-linkage joints slaved as mg400.py:77-129 slaves them);
  * DIRECTED[arm]: joint states of class a, found by a seeded search over 4000 such states on the CPU.  The classes (re-derived from the exact
    geometry by classes(); the CPU test pins their sizes):
      a  a link THROUGH the table top while every vertex over the table's footprint is above the top (the table's edge is passed lower down):
         one in 256 random states, hence the directed ones; none exists for the MG400 in 4000 states
      d  a link touching the table's interior from above: its lowest vertex is over the footprint, at least 2 cm inside it
      e  the link's BOX within D of the table, its hull further than D away (the UR5's upper arm over the table)
      f  two or more links' boxes within D of the table in one env (two or more stage-3 candidates)
    (d, e and f are plentiful among the random states of every arm)
  * and, for the classes uniform sampling never produced, STICKS: synthetic scenes in which one link's box and hull are replaced by a thin stick
    placed in the WORLD (the arm at rest):
      b  within D of the table with no vertex over the footprint: across a corner just above the top, or along an edge just outside and above it
      c  against a side face from below the top: end on, or alongside
    at gaps either side of D.  stick_scene() puts the stick into a Guard (for tg_set_broadphase); stick_boxes() hands the same box and hull to
    oracle.broadphase.sweep.
Pose p of a set is checked in env p % Arm.envs (64, the MG400's 16) of a 64-env context whose envs are seeded SEED + i: the edge stimulus and
the cube lie where that env's reset put them.  Everything is deterministic in the seeds below; geometry(arm) computes the exact brackets once per process."""
import dataclasses
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import broadphase_f64 as f64                                                     # noqa: E402
from oracle.broadphase import HULL_MARGIN, MARGIN, STIM, TABLE, _load, filtered_links    # noqa: E402  (asset loading and constants only)

D = 2 * MARGIN
N_ENVS, SEED, N_RANDOM, SPREAD, STATE_SEED = 64, 7300, 256, 1.5, 0
IMAGE, MAX_STEPS = 64, 50
UNDECIDED_CAP = 0.01

_EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
             arm_type="ur5", tactile_sensor_name="tactip")
_SURF = dict(movement_mode="xyzRxRy", control_mode="TCP_velocity_control", noise_mode="simplex", observation_mode="tactile", reward_mode="dense",
             arm_type="ur5", tactile_sensor_name="digit")
_PUSH = dict(movement_mode="TyRz", control_mode="TCP_velocity_control", rand_init_orn=False, rand_obj_mass=False, traj_type="simplex",
             observation_mode="tactile_and_feature", reward_mode="dense", arm_type="mg400", tactile_sensor_name="digitac")


@dataclasses.dataclass(frozen=True)
class Arm:
    env_id: str
    oracle_cls: str
    modes: dict
    asset: str                           # assets/collision/<asset>.npz
    t_s_core: str
    stick_link: str                      # the link the synthetic scenes turn into a stick
    device: bool = True                  # False: tg_set_joint_state refuses the env (a free object): the set is held to the geometry on the CPU only
    envs: int = N_ENVS                   # pose p is checked in env p % envs (fewer where a CPU reset is slow: the MG400's takes 0.3 s)


ARMS = {"ur5_tactip": Arm("edge_follow-v0", "OracleEdgeFollowEnv", _EDGE, "ur5_standard_tactip", "no_core", "forearm_link"),
        "ur5_tactip_tip": Arm("surface_follow-v0", "OracleSurfaceFollowAutoEnv", dict(_SURF, tactile_sensor_name="tactip"), "ur5_standard_tactip", "fixed",
                              "forearm_link"),                                   # the same arm with the tip's collisions on: its hull has 1089 vertices
        "ur5_digit": Arm("surface_follow-v0", "OracleSurfaceFollowAutoEnv", _SURF, "ur5_standard_digit", "fixed", "forearm_link"),
        "mg400_digitac": Arm("object_push-v0", "OracleObjectPushEnv", _PUSH, "mg400_right_angle_digitac", "fixed", "link3_1", device=False),
        "mg400_digitac_edge": Arm("edge_follow-v0", "OracleEdgeFollowEnv", dict(_EDGE, arm_type="mg400", tactile_sensor_name="digitac"),
                                  "mg400_standard_digitac", "no_core", "link3_1", envs=16)}   # the MG400 where the device takes joint states: the short edge

# ---- directed joint states (see the module docstring); a pose may belong to several classes
DIRECTED = {
    "ur5_tactip": [[-1.231496, -3.104769, -1.119582, -0.691476, 0.548815, 3.096098],          # class a, six of the 37 found (STATE_SEED + 1)
                   [1.035724, -3.091907, -0.674129, -0.728661, 0.383707, 3.14418],
                   [1.499451, -2.960797, -1.311179, -1.271102, 2.1788, 0.404029],
                   [1.139292, -3.148799, -0.854188, -0.183184, 2.785632, 1.577475],
                   [1.06569, -3.057832, -0.878668, -1.160356, 2.784511, 0.703513],
                   [-0.961196, -3.078876, -0.565364, 0.532078, 0.551422, 1.878445],
                   [1.292, -3.173, -1.076, -1.337, 2.819, 2.495]],                             # the forearm 31 cm under the top, distance 0
    "ur5_digit": [[-1.231503, -3.129049, -1.129502, -0.657276, 0.548815, 3.096098],           # class a, six of the 44 found
                  [1.129294, -2.97866, -0.750231, -0.441711, 2.477784, 1.442995],
                  [0.792895, -3.076349, -0.309263, -0.868026, 1.433313, 0.985515],
                  [1.035717, -3.116187, -0.684049, -0.694461, 0.383707, 3.14418],
                  [1.499444, -2.985077, -1.321099, -1.236902, 2.1788, 0.404029],
                  [1.139285, -3.173079, -0.864108, -0.148984, 2.785632, 1.577475]],
    "mg400_digitac": [],                                                                       # class a: none in 4000 states (its links are short)
}
DIRECTED["ur5_tactip_tip"] = DIRECTED["ur5_tactip"]
DIRECTED["mg400_digitac_edge"] = []
# class sizes over random + directed poses that the CPU test pins as lower bounds (4 where a class is claimed; 0: the search found none for this arm)
CLAIMED = {
    "ur5_tactip": dict(a=4, d=4, e=4, f=4),
    "ur5_tactip_tip": dict(a=4, d=4, e=4, f=4),
    "ur5_digit": dict(a=4, d=4, e=4, f=4),
    "mg400_digitac": dict(a=0, d=4, e=4, f=4),
    "mg400_digitac_edge": dict(a=0, d=4, f=0),                                   # (e: one member, too few to claim; the sensor's links are filtered out)
}
# ... and of the part of class e whose hull stays a centimetre and the margins above the top (the MG400's links are boxy: none)
CLEAR_E = {"ur5_tactip": 4, "ur5_tactip_tip": 4, "ur5_digit": 4, "mg400_digitac": 0, "mg400_digitac_edge": 0}


def oracle_env(arm, i=0):
    """Env i of the arm's context on the CPU, after its reset."""
    from oracle import ref_env
    a = ARMS[arm]
    e = getattr(ref_env, a.oracle_cls)(seed=SEED + i, max_steps=MAX_STEPS, image_size=(IMAGE, IMAGE), env_modes=a.modes)
    e.reset()
    return e


def slave(arm, q):
    """The MG400's parallel-linkage joints follow j2_1, j3_1 (mg400.py:77-129)."""
    q = np.array(q, dtype=np.float64)
    if ARMS[arm].modes["arm_type"] == "mg400":
        q[..., -3], q[..., -2], q[..., -1] = q[..., 1], -q[..., 1], q[..., 1] + q[..., 2]
    return q


def sample_states(arm, n, seed):
    rest = np.asarray(oracle_env(arm).rest_poses, dtype=np.float64)
    return slave(arm, rest + np.random.default_rng(seed).uniform(-SPREAD, SPREAD, size=(n, len(rest))))


@functools.lru_cache(maxsize=None)
def poses(arm):
    """[P][ndof] float64, read-only: the random states, then the directed ones."""
    q = sample_states(arm, N_RANDOM, STATE_SEED)
    if DIRECTED[arm]:
        q = np.concatenate([q, slave(arm, np.asarray(DIRECTED[arm], dtype=np.float64))])
    q.setflags(write=False)
    return q


# ---- geometry of a pose: world hulls and boxes from the assets and the oracle arm's link poses
@functools.lru_cache(maxsize=None)
def links(arm):
    """[(slot, name, link, local hull, (centre, rot, half))] of the arm's unfiltered collision links."""
    a = ARMS[arm]
    rb = _load(a.asset)
    sensor, t_s_type = a.modes["tactile_sensor_name"], a.asset.split("_", 1)[1].rsplit("_", 1)[0]
    off = filtered_links(a.modes["arm_type"], sensor, t_s_type, a.t_s_core)
    return [(i, name, int(rb["link"][i]), np.array(rb["hull_verts"][rb["hull_off"][i]:rb["hull_off"][i + 1]], dtype=np.float64),
             (rb["center"][i].astype(np.float64), rb["rot"][i].astype(np.float64), rb["half"][i].astype(np.float64)))
            for i, name in enumerate(rb["names"].tolist()) if name not in off]


def table_box():
    b = _load("table")
    return (b["center"][0] + b["base_pos"], np.eye(3), b["half"][0].astype(np.float64))


def stim_box(env):
    """The edge stimulus of an edge_follow env (the asset's box as it is); None elsewhere."""
    if type(env).__name__ != "OracleEdgeFollowEnv":
        return None
    b = _load("short_edge" if env.arm_type == "mg400" else "long_edge")
    R = np.asarray(env.edge_rot, dtype=np.float64)
    return (R @ b["center"][0] + np.asarray(env.edge_pos, dtype=np.float64), R @ b["rot"][0], b["half"][0].astype(np.float64))


def world_links(arm, env, q):
    """{slot: (world hull, world box corners)} of the unfiltered links with the env's arm at q (a moving link only: the base never moves)."""
    env.arm.reset_joint_states(np.asarray(q, dtype=np.float64))
    fr = env.arm.link_poses()
    out = {}
    for slot, _, l, hull, (c, rot, half) in links(arm):
        if l < 0:
            continue
        R, p = np.asarray(fr[l][0], dtype=np.float64), np.asarray(fr[l][1], dtype=np.float64)
        out[slot] = (hull @ R.T + p, f64.box_corners(R @ c + p, R @ rot, half))
    return out


@dataclasses.dataclass
class PoseGeometry:
    hull: dict                           # {(slot, TABLE | STIM): Bracket}: the link's hull against the target box
    box: dict                            # {slot: Bracket}: the link's BOX (its 8 corners) against the table
    over: dict                           # {slot: (number of vertices over the table's footprint grown by MARGIN, the lowest z among them or inf,
                                         #         the lowest z of all, whether that lowest vertex is over the footprint and 2 cm inside it)}


def pose_geometry(arm, env, q):
    tb = table_box()
    sb = stim_box(env)
    lo, hi = tb[0] - tb[2] - MARGIN, tb[0] + tb[2] + MARGIN
    g = PoseGeometry({}, {}, {})
    for slot, (hull, corners) in world_links(arm, env, q).items():
        g.hull[(slot, TABLE)] = f64.bracket(hull, tb, decide_at=D)
        if sb is not None:
            g.hull[(slot, STIM)] = f64.bracket(hull, sb, decide_at=D)
        g.box[slot] = f64.bracket(corners, tb, decide_at=D)
        inside = (hull[:, 0] >= lo[0]) & (hull[:, 0] <= hi[0]) & (hull[:, 1] >= lo[1]) & (hull[:, 1] <= hi[1])
        k = int(np.argmin(hull[:, 2]))
        deep = bool((np.abs(hull[k, :2] - tb[0][:2]) <= tb[2][:2] - 0.02).all())
        g.over[slot] = (int(inside.sum()), float(hull[inside, 2].min()) if inside.any() else np.inf, float(hull[k, 2]), deep)
    return g


@functools.lru_cache(maxsize=None)
def geometry(arm):
    """[PoseGeometry] of poses(arm), pose p in env p % ARMS[arm].envs.  Computed once per process and shared."""
    return [pose_geometry(arm, env_of(arm, p), q) for p, q in enumerate(poses(arm))]


def tight(arm, p, pair):
    """The full bracket of one pair of pose p (geometry() stops at the first certificates that decide a pair at D)."""
    e = env_of(arm, p)
    hull = world_links(arm, e, poses(arm)[p])[pair[0]][0]
    return f64.bracket(hull, table_box() if pair[1] == TABLE else stim_box(e))


_ENVS = {}


def env_of(arm, p):
    """The CPU env that pose p is checked in (shared: callers set its joint state and leave everything else alone)."""
    key = (arm, p % ARMS[arm].envs)
    if key not in _ENVS:
        _ENVS[key] = oracle_env(arm, key[1])
    return _ENVS[key]


@functools.lru_cache(maxsize=None)
def verdicts(arm):
    """[oracle.broadphase.check] of poses(arm), pose p in env p % ARMS[arm].envs."""
    from oracle import broadphase as obp
    out = []
    for p, q in enumerate(poses(arm)):
        e = env_of(arm, p)
        e.arm.reset_joint_states(np.asarray(q, dtype=np.float64))
        out.append(obp.check(e))
    return out


def classes(g):
    """The classes a pose belongs to, from its exact geometry alone (module docstring)."""
    top = table_box()[0][2] + table_box()[2][2]
    out = set()
    for slot, b in g.box.items():
        h = g.hull[(slot, TABLE)]
        n_over, z_over, z_min, deep = g.over[slot]
        if f64.classify(h, D) == f64.HIT:
            if n_over > 0 and (z_over - HULL_MARGIN) - MARGIN > top + MARGIN and z_min < top - D:
                out.add("a")
            if n_over == 0:
                out.add("b")
            if deep and z_min <= top + D:
                out.add("d")
        if f64.classify(b, D) == f64.HIT and f64.classify(h, D) == f64.CLEAR:
            out.add("e")
    if sum(f64.classify(b, D) == f64.HIT for b in g.box.values()) >= 2:
        out.add("f")
    return out


def class_sizes(arm):
    n = dict(a=0, b=0, d=0, e=0, f=0)
    for g in geometry(arm):
        for c in classes(g):
            n[c] += 1
    return n


def counts(arm):
    """{"hit", "clear", "undecided"} over every (link, table) and (link, edge stimulus) pair of the arm's pose set."""
    return f64.tally([b for g in geometry(arm) for b in g.hull.values()], D)


# ---- synthetic scenes: one link as a thin stick, placed in the world
STICK_HALF = (0.2, 0.005, 0.005)                                                 # 40 cm long, 1 cm square
GAPS = (0.0, 0.001, 0.0029, 0.0035, 0.008)                                       # metres between stick and table: three within D, two beyond


@dataclasses.dataclass(frozen=True)
class Stick:
    name: str
    cls: str                             # "b" | "c"
    center: np.ndarray                   # world
    axes: np.ndarray                     # world, columns; the first is the long one
    gap: float                           # the distance it was placed at


def _frame(u):
    u = np.asarray(u, float) / np.linalg.norm(u)
    v = np.cross([0.0, 0.0, 1.0], u) if abs(u[2]) < 0.9 else np.cross([1.0, 0.0, 0.0], u)
    v /= np.linalg.norm(v)
    return np.stack([u, v, np.cross(u, v)], axis=1)


@functools.lru_cache(maxsize=None)
def sticks():
    """The synthetic placements, the same for every arm (the table is).  No vertex of any of them is over the table's footprint."""
    c, _, h = table_box()
    top = c[2] + h[2]
    L, t = STICK_HALF[0], STICK_HALF[1]
    rng = np.random.default_rng(41)
    out = []
    for k, gap in enumerate(GAPS):
        sx, sy = (1, 1, -1, -1)[k % 4], (1, -1, 1, -1)[k % 4]
        corner = c[:2] + np.array([sx, sy]) * h[:2]
        # b, corner: a horizontal stick across a corner, `gap` above the top, its ends well outside on both sides
        ang = np.arctan2(sy, -sx) + rng.uniform(-0.3, 0.3)                       # about the corner's own diagonal direction
        u = np.array([np.cos(ang), np.sin(ang), 0.0])
        inward = -np.array([sx, sy]) / np.sqrt(2.0)
        ctr = np.array([*(corner + 0.02 * inward), top + gap + t])
        out.append(Stick(f"corner_{k}_gap{gap}", "b", ctr, _frame(u), gap))
        # b, edge: along the long edge y = +-h, outside and above it: the nearest points are the table's edge and the stick's lower inner edge
        # (outside the footprint grown by MARGIN as well: 1.6 mm out, so no nearer than 2 mm)
        egap = max(gap, 0.002)
        dy = 0.0016
        dz = float(np.sqrt(egap * egap - dy * dy))
        ctr = np.array([c[0] + rng.uniform(-0.3, 0.3), c[1] + sy * (h[1] + dy + t), top + dz + t])
        out.append(Stick(f"edge_{k}_gap{egap}", "b", ctr, _frame([1.0, 0.0, 0.0]), egap))
        # c, end on: pointing at the side face x = +-h from outside, wholly below the top
        ctr = np.array([c[0] + sx * (h[0] + gap + L), c[1] + rng.uniform(-0.3, 0.3), top - 0.02 - rng.uniform(0, 0.02)])
        out.append(Stick(f"endon_{k}_gap{gap}", "c", ctr, _frame([1.0, 0.0, 0.0]), gap))
        # c, alongside: flat against the side face y = +-h, wholly below the top
        ctr = np.array([c[0] + rng.uniform(-0.3, 0.3), c[1] + sy * (h[1] + gap + t), top - 0.01 - t - rng.uniform(0, 0.02)])
        out.append(Stick(f"alongside_{k}_gap{gap}", "c", ctr, _frame([1.0, 0.0, 0.0]), gap))
    return tuple(out)


def stick_world(s):
    """(world hull [8][3], world box) of a stick."""
    return f64.box_corners(s.center, s.axes, STICK_HALF), (s.center, s.axes, np.asarray(STICK_HALF, float))


def stick_local(arm, env, s):
    """(slot, local hull [8][3], local centre, local rot, half): the stick in the frame of the arm's stick link with the env's arm where it is."""
    slot, _, l, _, _ = next(x for x in links(arm) if x[1] == ARMS[arm].stick_link)
    R, p = (np.asarray(v, dtype=np.float64) for v in env.arm.link_poses()[l])
    c, rot = R.T @ (s.center - p), R.T @ s.axes
    return slot, f64.box_corners(c, rot, STICK_HALF), c, rot, np.asarray(STICK_HALF, float)


def stick_scene(guard, arm, env, s):
    """Turns the stick link of a tactile_gym_amd.broadphase.Guard into the stick (its box and its hull range; the hull is appended to the guard's
    vertices).  The caller installs guard.struct with tg_set_broadphase."""
    import ctypes as C
    slot, hull, c, rot, half = stick_local(arm, env, s)
    b = guard.struct.box[slot]
    for i in range(3):
        b.center[i], b.half[i] = float(c[i]), float(half[i])
    for i in range(9):
        b.rot[i] = float(rot.reshape(9)[i])
    n = guard.hull.shape[0]
    guard.hull = np.ascontiguousarray(np.concatenate([guard.hull, hull]), dtype=np.float64)
    b.hull_off, b.hull_n = n, 8
    guard.struct.n_hull_verts = n + 8
    guard.struct.hull_verts = guard.hull.ctypes.data_as(C.POINTER(C.c_double))
    return slot


def stick_boxes(arm, env, s):
    """oracle.broadphase.env_boxes(env) with the stick link's entry replaced by the stick: what stick_scene gives the device, for sweep()."""
    from oracle import broadphase as obp
    slot, hull, c, rot, half = stick_local(arm, env, s)
    boxes, expected = obp.env_boxes(env)
    l = next(x for x in links(arm) if x[0] == slot)[2]
    R, p = env.arm.link_poses()[l]
    boxes = [(i, body, static, *obp._aabb(R, p, c, rot, half), obp.world_hull(hull, R, p)) if i == slot else (i, body, static, lo, hi, obb, h)
             for i, body, static, lo, hi, obb, h in boxes]
    return slot, boxes, expected


# ---- how far a hull vertex travels inside one env step (the guard checks once per step)
_VERT = dict(movement_mode="xRz", control_mode="TCP_velocity_control", noise_mode="vertical_simplex", observation_mode="tactile", reward_mode="dense",
             arm_type="mg400", tactile_sensor_name="tactip")
_ROLL = dict(movement_mode="xy", control_mode="TCP_velocity_control", rand_init_obj_pos=True, rand_obj_size=True, rand_embed_dist=True,
             observation_mode="tactile_and_feature", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
_BAL = dict(movement_mode="xy", control_mode="TCP_velocity_control", object_mode="pole", rand_gravity=True, rand_embed_dist=True,
            observation_mode="tactile", reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
FAMILIES = {   # oracle class, modes, act_dim
    "edge_ur5": ("OracleEdgeFollowEnv", _EDGE, 2),
    "edge_mg400": ("OracleEdgeFollowEnv", dict(_EDGE, arm_type="mg400"), 2),
    "surface_ur5_digit": ("OracleSurfaceFollowAutoEnv", _SURF, 3),
    "surface_v2_mg400": ("OracleSurfaceFollowVertEnv", _VERT, 2),
    "push_mg400_digitac": ("OracleObjectPushEnv", _PUSH, 2),
    "push_ur5_tactip": ("OracleObjectPushEnv", dict(_PUSH, arm_type="ur5", tactile_sensor_name="tactip"), 2),
    "roll": ("OracleObjectRollEnv", _ROLL, 2),
    "balance_pole": ("OracleObjectBalanceEnv", _BAL, 2),
}
TRAVEL_STEPS, TRAVEL_SEED = 3, 7300


def _all_hulls(env):
    from oracle import broadphase as obp
    return [b[6] for b in obp.env_boxes(env)[0] if b[6] is not None]


def step_travel(family):
    """The largest distance any hull vertex of the robot's unfiltered links moves in ONE env step, over TRAVEL_STEPS steps at each corner of the
    family's action box (a fresh env per corner), in metres."""
    import itertools
    from oracle import ref_env
    cls, modes, act_dim = FAMILIES[family]
    worst = 0.0
    for k, corner in enumerate(itertools.product((-0.25, 0.25), repeat=act_dim)):
        e = getattr(ref_env, cls)(seed=TRAVEL_SEED + k, max_steps=MAX_STEPS, image_size=(IMAGE, IMAGE), env_modes=modes)
        e.reset()
        before = _all_hulls(e)
        for _ in range(TRAVEL_STEPS):
            e.step(np.asarray(corner, dtype=np.float64))
            after = _all_hulls(e)
            worst = max(worst, max(float(np.linalg.norm(a - b, axis=1).max()) for a, b in zip(after, before)))
            before = after
    return worst
