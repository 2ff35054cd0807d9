"""tg_step_random's draw counter (tg_kernels.hpp, draw_counter_advance): the step kernels draw the env's actions themselves, and the workgroup
that finishes last moves the device-resident counter on - by one ticket per workgroup, in two levels above 64 workgroups.

Every launch must advance the counter exactly once, and no workgroup may read it late: K = 40 step_random calls, the restart flag set in the
first only, and after every call the actions the step drew equal sample_actions(seed, k) for that k bit for bit; one more pair after the
loop shows the counter at K.  Env counts on both sides of every election edge (one workgroup, a ragged one, 64 workgroups: one level; 65
and more: two levels), on the quad kernel (16 envs per workgroup), on the lane kernel with the MG400 (surface_follow-v2) and with the UR5
(TG_KSTEP_QUAD=0 is read once per process: a child process).  max_steps = 3: finished envs take the in-step reset on the same launches.
(Written for a variant that takes the ticket early in the kernel; that variant did not separate from the barrier-and-atomic at the end in
the headline runs - profiles/blk_tail.txt - and is not in the tree.  The check holds for any way of electing the last workgroup.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SEED = 40, 91

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile",
            reward_mode="dense", arm_type="ur5", tactile_sensor_name="tactip")
VERT = dict(movement_mode="xRz", control_mode="TCP_velocity_control", noise_mode="vertical_simplex", observation_mode="tactile",
            reward_mode="dense", arm_type="mg400", tactile_sensor_name="tactip")


def rollout(env_id, modes, n, want_epw):
    """Returns the number of (env, step) pairs that finished an episode; asserts the draws and the counter."""
    import ctypes
    import torch
    import tactile_gym_amd as tg
    venv = tg.make_vec(env_id, num_envs=n, max_steps=3, image_size=[128, 128], env_modes=modes, seed=3, auto_reset=True, obs_mode="torch")
    try:
        venv.reset()
        want = torch.empty(n, venv.act_dim, device="cuda")
        dones = 0
        for k in range(K + 1):      # the last turn is the pair after the loop: the counter stands at K, so it draws K + 1
            venv.step_random_async(SEED, 0, restart=(k == 0))
            venv.sample_actions(want, SEED, k + 1)
            venv.sync()
            torch.cuda.synchronize()
            got = venv.actions_torch()
            assert torch.equal(got, want), (env_id, n, k, int((got != want).sum().item()))
            dones += int(venv.reward_done_torch()[1].sum().item())
        mode, epw = ctypes.c_int32(), ctypes.c_int32()
        assert venv._L.tg_get_step_mode(venv._ctx, ctypes.byref(mode), ctypes.byref(epw)) == 0
        assert mode.value == 0 and epw.value == want_epw, (mode.value, epw.value)       # the kernel this case is about ran
        assert dones >= n * (K // 3 - 1)                                                # episodes ended inside the step launches
        return dones
    finally:
        venv.close()


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1024, 1025, 2049])
def test_quad_kernel_advances_the_counter_once_per_launch(n):
    rollout("edge_follow-v0", EDGE, n, 16)


@pytest.mark.parametrize("n", [64, 65, 4096, 4097])
def test_lane_kernel_advances_the_counter_once_per_launch(n):
    rollout("surface_follow-v2", VERT, n, 64)


def test_lane_kernel_of_the_ur5_advances_the_counter_once_per_launch():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), TG_KSTEP_QUAD="0")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "64", "65", "4096", "4097"], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert sorted(res) == ["4096", "4097", "64", "65"] and all(v > 0 for v in res.values())


if __name__ == "__main__":
    print(json.dumps({a: rollout("edge_follow-v0", EDGE, int(a), 64) for a in sys.argv[1:]}))
