"""k_step_quad (tg_kernels.hpp: the UR5's step on a quad of lanes per env, the kinematics by rows) against k_step (one lane per env).

The same rollouts run in child processes with TG_KSTEP_QUAD=1 and =0 (read once per context).  Observations, terminal observations, rewards
and done flags must be identical byte for byte.  Joint angles, joint velocities and the TCP position must agree to 1e-12: the quad kernel's
licence and fast-forward votes cover 16 envs instead of 64, so an env may take a full solve where it took the analytic tick, or the other
way round, which moves the last bits.  Cases: the headline's shape with the in-kernel random draw, a ragged last quad and wavefront,
surface_follow with the reset bank, and episodes out of phase with the in-step reset and with the k_reset launch (TG_NO_INLINE_RESET=1)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes, hashlib, json, sys
import numpy as np
import tactile_gym_amd as tg
env_id, n, steps, max_steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
modes = json.loads(sys.argv[5]); random_step, bank, phases = int(sys.argv[6]), sys.argv[7], int(sys.argv[8])
venv = tg.make_vec(env_id, num_envs=n, max_steps=max_steps, image_size=[128, 128], env_modes=modes, seed=11, auto_reset=True, reset_bank=bank)
h = hashlib.sha256()
traj = []
rng = np.random.default_rng(3)
obs = venv.reset()
h.update(np.ascontiguousarray(obs["tactile"]).tobytes())
dones, terms, partial = 0, 0, 0
for k in range(steps):
    if phases and k in (2, 5, 7):   # three groups of envs restart here: their episodes end in different steps from then on
        m = np.zeros(n, np.uint8)
        m[{2: slice(0, n, 3), 5: slice(1, n, 3), 7: slice(0, n, 5)}[k]] = 1
        venv.reset(m)
    if random_step:
        venv.step_random_async(77, k, restart=(k == 0))
        obs, rew, done, infos = venv.step_wait()
    else:
        obs, rew, done, infos = venv.step(rng.uniform(-0.25, 0.25, size=(n, venv.act_dim)).astype(np.float32))
    h.update(np.ascontiguousarray(obs["tactile"]).tobytes()); h.update(np.asarray(rew, dtype=np.float32).tobytes())
    h.update(np.asarray(done, dtype=np.uint8).tobytes())
    dones += int(np.sum(done)); partial += int(0 < int(np.sum(done)) < n)
    for i in range(n):
        if done[i]:
            h.update(np.ascontiguousarray(infos[i]["terminal_observation"]["tactile"]).tobytes()); terms += 1
    if k % 3 == 2 or k == steps - 1:
        st = venv.get_state()
        traj.append([st[key].tolist() for key in ("q", "qd", "tcp_pos")])
mode, epw = ctypes.c_int32(), ctypes.c_int32()   # which step kernel ran: envs per wavefront of the last arm step launch
assert venv._L.tg_get_step_mode(venv._ctx, ctypes.byref(mode), ctypes.byref(epw)) == 0
print(json.dumps({"sha": h.hexdigest(), "traj": traj, "dones": dones, "terms": terms, "partial": partial, "mode": mode.value, "epw": epw.value}))
"""

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile",
            reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
SURF = dict(movement_mode="xyzRxRy", control_mode="TCP_velocity_control", noise_mode="simplex", observation_mode="tactile",
            reward_mode="dense", arm_type="ur5", tactile_sensor_name="digit")


def _run(env_id, n, steps, max_steps, modes, random_step, bank, phases, **switches):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **switches)
    out = subprocess.run([sys.executable, "-c", CHILD, env_id, str(n), str(steps), str(max_steps), json.dumps(modes), str(random_step), bank, str(phases)],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-4000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.parametrize("env_id,n,steps,max_steps,modes,random_step,bank,phases,switches", [
    ("edge_follow-v0", 1024, 30, 9, EDGE, 1, "auto", 0, {}),                                # the headline's shape, in-kernel random draw
    ("edge_follow-v0", 300, 30, 7, EDGE, 0, "auto", 0, {}),                                 # ragged last quad and wavefront
    ("surface_follow-v0", 200, 24, 8, SURF, 0, "auto", 0, {}),                              # surface_follow, reset bank on
    ("edge_follow-v0", 96, 40, 11, EDGE, 0, "auto", 1, {}),                                 # episodes out of phase, reset inside the step
    ("edge_follow-v0", 96, 40, 11, EDGE, 0, "auto", 1, {"TG_NO_INLINE_RESET": "1"}),        # ... and by the k_reset launch
])
def test_quad_step_equals_the_lane_step(env_id, n, steps, max_steps, modes, random_step, bank, phases, switches):
    import numpy as np
    a = _run(env_id, n, steps, max_steps, modes, random_step, bank, phases, TG_KSTEP_QUAD="1", **switches)
    b = _run(env_id, n, steps, max_steps, modes, random_step, bank, phases, TG_KSTEP_QUAD="0", **switches)
    assert a["mode"] == b["mode"] == 0 and a["epw"] == 16 and b["epw"] == 64   # k_step_quad ran in one child, k_step in the other
    assert a["dones"] >= n and a["terms"] == a["dones"]          # episodes ended and restarted inside the rollout
    if phases:
        assert a["partial"] >= steps // 4                        # some but not all envs finished in many steps
    assert a["sha"] == b["sha"], "observations / rewards / dones / terminal observations differ between k_step_quad and k_step"
    for ta, tb in zip(a["traj"], b["traj"]):
        for xa, xb in zip(ta, tb):
            assert np.max(np.abs(np.asarray(xa) - np.asarray(xb))) <= 1e-12
