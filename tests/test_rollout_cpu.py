"""tactile_gym_amd.rollout without a GPU: the two GAE references of tests/rollout_ref.py against each other and against known answers, the flat
index convention, the constructor's and the methods' argument rules, the C ABI entries and the kernels' resources."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from rollout_ref import (GAE_N, GAE_PARAMS, GAE_STARTS, GAE_T, flat_rows, gae_bound, gae_edge_inputs, gae_error, gae_f32, gae_f64,  # noqa: E402
                         minibatches, swap_and_flatten)

from tactile_gym_amd import _capi, spaces  # noqa: E402

ENTRIES = ("tg_rollout_add", "tg_rollout_gae", "tg_rollout_gather", "tg_random_translate_rows")


def _rollout(seed, T, N, p_start, scale):
    rng = np.random.default_rng(seed)
    r = (rng.standard_normal((T, N)) * scale).astype(np.float32)
    v = (rng.standard_normal((T, N)) * scale * 5).astype(np.float32)
    es = (rng.random((T, N)) < p_start).astype(np.float32)
    d = (rng.random(N) < p_start).astype(np.float32)
    lv = (rng.standard_normal(N) * scale * 5).astype(np.float32)
    return r, v, es, lv, d


CASES = [(0.95, 0.9, 2048, 0.005, 1.0), (0.99, 0.95, 512, 0.02, 10.0), (0.999, 1.0, 2048, 0.001, 1.0), (0.95, 0.9, 64, 0.3, 100.0),
         (1.0, 1.0, 256, 0.01, 1.0)]


@pytest.mark.parametrize("gamma,lam,T,p_start,scale", CASES)
def test_f32_restatement_within_the_bound_of_sb3_f64(gamma, lam, T, p_start, scale):
    for seed in range(3):
        r, v, es, lv, d = _rollout(seed, T, 64, p_start, scale)
        a32, r32 = gae_f32(r, v, es, lv, d, gamma, lam)
        a64, r64 = gae_f64(r, v, es, lv, d, gamma, lam)
        bound = gae_bound(r, v, lv, a64, gamma, lam)
        err = max(np.abs(a32 - a64).max(), np.abs(r32 - r64).max() - 2.0 ** -24 * np.abs(r64).max())
        print(f"gamma={gamma} lambda={lam} T={T} seed={seed}: max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.4f}")
        assert a32.dtype == np.float32 and r32.dtype == np.float32
        assert err <= bound, (err, bound)


@pytest.mark.parametrize("T", GAE_T)
def test_f32_restatement_within_the_bound_on_the_edge_shapes(T):
    """The inputs of tests/test_gpu_rollout_abi.py's GAE matrix: the margin that test grants the device against float64 holds for the
    restatement itself."""
    worst = 0.0
    for N in GAE_N:
        for starts in GAE_STARTS:
            r, v, es, lv, d = gae_edge_inputs(T, N, starts)
            for gamma, lam in GAE_PARAMS:
                a32, r32 = gae_f32(r, v, es, lv, d, gamma, lam)
                a64, r64 = gae_f64(r, v, es, lv, d, gamma, lam)
                err, bound = gae_error(a32, r32, a64, r64), gae_bound(r, v, lv, a64, gamma, lam)
                worst = max(worst, err / bound)
                assert err <= bound, (T, N, starts, gamma, lam, err, bound)
    print(f"T={T}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("gamma,lam,T,p_start,scale", CASES[:4])
def test_bound_is_not_vacuous(gamma, lam, T, p_start, scale):
    """episode_starts[t] in place of [t + 1] - the classic off-by-one - breaks the bound by orders of magnitude."""
    r, v, es, lv, d = _rollout(1, T, 64, max(p_start, 0.01), scale)
    a64, _ = gae_f64(r, v, es, lv, d, gamma, lam)
    wrong, _ = gae_f32(r, v, es, lv, d, gamma, lam, starts_offset=0)
    assert np.abs(wrong - a64).max() > 100 * gae_bound(r, v, lv, a64, gamma, lam)


def test_lambda_one_is_discounted_monte_carlo():
    """gae_lambda = 1, no episode boundary: returns[t] = sum_k gamma^k r[t + k] + gamma^(T - t) last_value; advantages = returns - values."""
    T, N, gamma = 12, 3, 0.5                                  # powers of two, small integers: exact in float32
    rng = np.random.default_rng(0)
    r = rng.integers(-4, 5, size=(T, N)).astype(np.float32)
    v = rng.integers(-4, 5, size=(T, N)).astype(np.float32)
    lv = rng.integers(-4, 5, size=N).astype(np.float32)
    es, d = np.zeros((T, N), np.float32), np.zeros(N, np.float32)
    adv, ret = gae_f32(r, v, es, lv, d, gamma, 1.0)
    exp = np.zeros((T, N))
    run = lv.astype(np.float64)
    for t in reversed(range(T)):
        run = r[t] + gamma * run
        exp[t] = run
    assert np.array_equal(ret, exp.astype(np.float32)) and np.array_equal(adv, (exp - v).astype(np.float32))
    a64, r64 = gae_f64(r, v, es, lv, d, gamma, 1.0)
    assert np.array_equal(r64, exp)


def test_episode_start_cuts_the_recurrence():
    """An episode start at t + 1: advantages[t] = rewards[t] - values[t], whatever comes later; dones cut the last step likewise."""
    T, N = 6, 2
    r = np.arange(T * N, dtype=np.float32).reshape(T, N)
    v = np.full((T, N), 2.0, np.float32)
    es = np.zeros((T, N), np.float32)
    es[4, 0] = 1.0
    lv = np.array([100.0, 100.0], np.float32)
    for fn in (gae_f32, gae_f64):
        adv, ret = fn(r, v, es, lv, np.array([0, 1], np.uint8), 0.5, 0.5)
        assert adv[3, 0] == r[3, 0] - 2.0 and ret[3, 0] == r[3, 0]
        assert adv[5, 1] == r[5, 1] - 2.0                                    # done after the last step: no bootstrap
        assert adv[5, 0] == r[5, 0] + 0.5 * 100.0 - 2.0                      # not done: bootstrapped from last_values
        assert adv[4, 1] == (r[4, 1] + 0.5 * 2.0 - 2.0) + 0.25 * adv[5, 1]
        later = r.copy()
        later[4:, 0] += 1000.0
        adv2, _ = fn(later, v, es, lv, np.array([0, 1], np.uint8), 0.5, 0.5)
        assert np.array_equal(adv2[:4, 0], adv[:4, 0])                       # nothing after the cut reaches before it


def test_single_step():
    r, v, lv = np.array([[1.5, -2.0]], np.float32), np.array([[0.25, 4.0]], np.float32), np.array([8.0, 8.0], np.float32)
    for dones in (np.array([False, True]), np.array([0, 1], np.uint8), np.array([0.0, 1.0], np.float32)):
        adv, ret = gae_f32(r, v, np.ones((1, 2), np.float32), lv, dones, 0.5, 0.9)
        assert np.array_equal(adv, np.array([[1.5 + 4.0 - 0.25, -2.0 - 4.0]], np.float32))
        assert np.array_equal(ret, adv + v)


@pytest.mark.parametrize("T,N", [(1, 1), (7, 3), (5, 1), (1, 6), (16, 64)])
def test_flat_index_convention(T, N):
    rng = np.random.default_rng(T * 100 + N)
    arr = rng.integers(0, 1000, size=(T, N, 2, 3))
    idx = np.concatenate([rng.permutation(T * N), rng.integers(0, T * N, size=5)])
    rows = flat_rows(idx, T, N)
    assert np.array_equal(arr.reshape(T * N, 2, 3)[rows], arr.swapaxes(0, 1).reshape(T * N, 2, 3)[idx])
    assert np.array_equal(swap_and_flatten(arr)[idx], arr.reshape(T * N, 2, 3)[rows])
    n, t = idx // T, idx % T
    assert np.array_equal(arr[t, n], arr.reshape(T * N, 2, 3)[rows])
    torch = pytest.importorskip("torch")
    from tactile_gym_amd.rollout import flat_rows as flat_rows_torch
    assert np.array_equal(flat_rows_torch(torch.from_numpy(idx), T, N).numpy(), rows)
    got = list(minibatches({"a": arr}, idx, 4))
    assert sum(len(b["a"]) for b in got) == len(idx) and len(got[-1]["a"]) == (len(idx) - 1) % 4 + 1


# ---------------------------------------------------------------------------------------------------------------- argument rules
def _spaces(H=16, W=16, A=2):
    obs = spaces.Dict({"tactile": spaces.Box(low=0, high=255, shape=(2, H, W), dtype=np.uint8),
                       "extended_feature": spaces.Box(low=-np.inf, high=np.inf, shape=(3,), dtype=np.float32)})
    return obs, spaces.Box(low=-1.0, high=1.0, shape=(A,), dtype=np.float32)


def _unallocated(T=4, N=3, **kw):
    """A buffer whose storage is on torch's meta device: every argument rule runs before anything touches a GPU."""
    import torch
    from tactile_gym_amd.rollout import DeviceRolloutBuffer

    class Unallocated(DeviceRolloutBuffer):
        def _alloc(self, shape, dtype):
            return torch.empty(shape, dtype=dtype, device="meta")
    obs, act = _spaces()
    return Unallocated(T, obs, act, "cuda:0", 0.9, 0.95, N, **kw)


def test_module_is_exported():
    pytest.importorskip("torch")
    import tactile_gym_amd as tg
    from tactile_gym_amd.rollout import DeviceRolloutBuffer
    assert tg.DeviceRolloutBuffer is DeviceRolloutBuffer and tg.rollout.DeviceRolloutBuffer is DeviceRolloutBuffer
    assert DeviceRolloutBuffer.__init__.__code__.co_varnames[1:9] == ("buffer_size", "observation_space", "action_space", "device", "gae_lambda",
                                                                      "gamma", "n_envs", "channels_first")


def test_constructor_errors():
    pytest.importorskip("torch")
    from tactile_gym_amd.rollout import DeviceRolloutBuffer
    obs, act = _spaces()
    with pytest.raises(ValueError, match="device"):
        DeviceRolloutBuffer(4, obs, act, device="cpu")
    with pytest.raises(ValueError, match="buffer_size"):
        DeviceRolloutBuffer(0, obs, act)
    with pytest.raises(ValueError, match="n_envs"):
        DeviceRolloutBuffer(4, obs, act, n_envs=0)
    with pytest.raises(TypeError, match="observation_space"):
        DeviceRolloutBuffer(4, spaces.Box(low=0, high=1, shape=(3,), dtype=np.float64), act)
    with pytest.raises(TypeError, match=r"observation_space\['oracle'\]"):
        DeviceRolloutBuffer(4, spaces.Dict({"oracle": spaces.Box(low=0, high=1, shape=(3,), dtype=np.int32)}), act)
    with pytest.raises(TypeError, match="action_space"):
        DeviceRolloutBuffer(4, obs, spaces.Box(low=0, high=1, shape=(2,), dtype=np.float64))
    with pytest.raises(TypeError, match="action_space"):
        DeviceRolloutBuffer(4, obs, spaces.Box(low=0, high=1, shape=(2, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="channels_first"):
        DeviceRolloutBuffer(4, obs, act, channels_first="yes")


def test_storage_layout_and_state():
    torch = pytest.importorskip("torch")
    b = _unallocated(T=4, N=3)
    assert tuple(b.observations["tactile"].shape) == (4, 3, 2, 16, 16) and b.observations["tactile"].dtype == torch.uint8
    assert tuple(b.observations["extended_feature"].shape) == (4, 3, 3) and b.observations["extended_feature"].dtype == torch.float32
    assert tuple(b.actions.shape) == (4, 3, 2)
    for name in ("rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
        t = getattr(b, name)
        assert tuple(t.shape) == (4, 3) and t.dtype == torch.float32
    assert (b.pos, b.full, b.size(), b.gamma, b.gae_lambda, b.buffer_size, b.n_envs) == (0, False, 0, 0.95, 0.9, 4, 3)
    assert b._channels_first == {"tactile": True}
    assert _unallocated(channels_first=False)._channels_first == {"tactile": False}


def _args(N=3, A=2):
    import torch
    return dict(obs={"tactile": torch.zeros((N, 2, 16, 16), dtype=torch.uint8), "extended_feature": torch.zeros((N, 3))},
                action=torch.zeros((N, A)), reward=torch.zeros(N), episode_start=torch.zeros(N, dtype=torch.uint8), value=torch.zeros(N),
                log_prob=torch.zeros(N))


def test_add_argument_errors():
    torch = pytest.importorskip("torch")
    b = _unallocated()
    with pytest.raises(ValueError, match="device"):                          # well formed, but on the CPU
        b.add(**_args())
    bad = [("action", torch.zeros((3, 3)), ValueError), ("action", torch.zeros((3, 2), dtype=torch.float64), TypeError),
           ("reward", torch.zeros(4), ValueError), ("reward", [0.0, 0.0, 0.0], TypeError),
           ("episode_start", torch.zeros(3, dtype=torch.int64), TypeError), ("episode_start", np.zeros(3, np.int32), TypeError),
           ("value", torch.zeros((3, 2)), ValueError), ("log_prob", torch.zeros((6,))[::2], ValueError),
           ("log_prob", np.zeros(5, np.float32), ValueError)]
    for name, value, exc in bad:
        with pytest.raises(exc, match=name):
            b.add(**dict(_args(), **{name: value}))
    for key, value, exc in (("tactile", torch.zeros((3, 16, 16, 2), dtype=torch.uint8), ValueError),
                            ("tactile", torch.zeros((3, 2, 16, 16)), TypeError),
                            ("extended_feature", torch.zeros((3, 4)), ValueError)):
        a = _args()
        a["obs"][key] = value
        with pytest.raises(exc, match=key):
            b.add(**a)
    a = _args()
    del a["obs"]["extended_feature"]
    with pytest.raises(ValueError, match="obs"):
        b.add(**a)
    with pytest.raises(ValueError, match="obs"):
        b.add(**dict(_args(), obs=torch.zeros((3, 2, 16, 16), dtype=torch.uint8)))
    assert b.pos == 0 and not b.full                                          # a refused add writes nothing and does not advance
    b.pos, b.full = 4, True
    with pytest.raises(RuntimeError, match="full"):
        b.add(**_args())
    b.reset()
    assert (b.pos, b.full) == (0, False)


def test_get_argument_errors():
    torch = pytest.importorskip("torch")
    import tactile_gym_amd.augment as K
    b = _unallocated(T=4, N=3)
    with pytest.raises(RuntimeError, match="full"):
        b.get(2)
    b.pos, b.full = 4, True
    with pytest.raises(ValueError, match="indices"):
        b.get(2, indices=torch.tensor([0, 12]))
    with pytest.raises(ValueError, match="indices"):
        b.get(2, indices=torch.tensor([-1, 3]))
    with pytest.raises(TypeError, match="indices"):
        b.get(2, indices=torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="batch_size"):
        b.get(0)
    with pytest.raises(TypeError, match="out_dtype"):
        b.get(2, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="out_dtype"):
        b.get(2, augment=K.RandomTranslate(seed=1), out_dtype=torch.uint8)
    with pytest.raises(TypeError, match="Identity"):
        b.get(2, augment=torch.nn.Identity())
    with pytest.raises(TypeError, match="function"):
        b.get(2, augment=lambda x: x)
    with pytest.raises(TypeError, match="2 modules"):
        b.get(2, augment=torch.nn.Sequential(K.RandomTranslate(seed=1), K.RandomTranslate(seed=2)))
    with pytest.raises(ValueError, match="last_values"):
        b.compute_returns_and_advantage(torch.zeros(4), torch.zeros(3))
    with pytest.raises(TypeError, match="dones"):
        b.compute_returns_and_advantage(torch.zeros(3), torch.zeros(3, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------- C ABI and resources
def test_c_abi_entries_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in _capi.SYMBOLS, name
    assert re.search(r"#define TG_ABI_VERSION 16\b", header) and _capi.ABI_VERSION == 16
    assert re.search(r"#define TG_ROLLOUT_MAX_ARRAYS 16\b", header) and _capi.ROLLOUT_MAX_ARRAYS == 16
    assert re.search(r"#define TG_ROLLOUT_COPY 0\b", header) and re.search(r"#define TG_ROLLOUT_FLAG_U8 1\b", header)
    assert (_capi.ROLLOUT_COPY, _capi.ROLLOUT_FLAG_U8) == (0, 1)
    assert re.search(r"#define TG_ROLLOUT_DONES_UINT8 0\b", header) and re.search(r"#define TG_ROLLOUT_DONES_FLOAT32 1\b", header)
    assert _capi.ROLLOUT_DONES == {"uint8": 0, "float32": 1}
    assert len(_capi.SYMBOLS["tg_random_translate_rows"][1]) == len(_capi.SYMBOLS["tg_random_translate"][1]) + 1
    assert os.path.exists(_capi.LIB_PATH), "library not built"
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"\b", nm), name


def test_rollout_kernels_use_no_scratch(tmp_path):
    """k_rollout_add, k_rollout_gather, both k_rollout_gae instantiations and the four row-indexed k_random_translate keep their registers."""
    from test_kstep_quad_resources_cpu import LIB, _kernel_scratch
    assert os.path.exists(LIB), "library not built"
    scratch = _kernel_scratch(tmp_path)
    ro = {k: v for k, v in scratch.items() if "k_rollout_" in k}
    assert sum("k_rollout_add" in k for k in ro) == 1 and sum("k_rollout_gather" in k for k in ro) == 1, sorted(ro)
    assert sum("k_rollout_gae" in k for k in ro) == 2, sorted(ro)
    tr = {k: v for k, v in scratch.items() if "k_random_translate" in k}
    assert len(tr) == 4, sorted(tr)
    assert all(v == 0 for v in ro.values()) and all(v == 0 for v in tr.values()), (ro, tr)
