"""tactile_gym_amd.replay without a GPU: the restatement of tests/replay_ref.py against a literal model of SB3's ring, the carried form against
the plain one, the draw formula, range and uniformity, the argument and state rules, the C ABI entries and the kernels' resources."""
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
from augment_ref import GOLDEN, M64, mix64_int  # noqa: E402
from replay_ref import ReplayRef, draw_cells, draw_rows  # noqa: E402

from tactile_gym_amd import _capi, spaces  # noqa: E402

ENTRIES = ("tg_replay_add", "tg_replay_draw")
BOUND = {name: _capi.SYMBOLS[name] for name in ENTRIES}      # at import: the whole file needs the feature
SPEC = {"x": ((2,), np.float32)}


def _transition(rng, g, N, p_done=0.3, p_timeout=0.5):
    """Transition g -> g + 1 of every env: observations encode (global step, env); a finished env's terminal observation is the next one + 0.5."""
    env = np.arange(N, dtype=np.float32)
    o = lambda step: np.stack([np.full(N, step, np.float32), env], axis=1)   # noqa: E731
    done = rng.random(N) < p_done
    timeouts = (done & (rng.random(N) < p_timeout)).astype(np.float32)
    return dict(obs={"x": o(g)}, next_obs={"x": o(g + 1)}, terminal_obs={"x": o(g + 1) + np.float32(0.5)},
                action=rng.standard_normal((N, 3)).astype(np.float32), reward=rng.standard_normal(N).astype(np.float32), done=done.astype(np.uint8),
                timeouts=timeouts)


# ---------------------------------------------------------------------------------------------------------------- the ring
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_restatement_against_a_literal_ring(T, N):
    """SB3's ring as a list of transitions: slot pos is overwritten, pos = (pos + 1) % T, full on the wrap."""
    rng = np.random.default_rng(10 * T + N)
    ref = ReplayRef(T * N + (N - 1), N, SPEC, 3)              # buffer_size // n_envs = T
    assert ref.T == T
    ring, pos, full = [None] * T, 0, False
    for g in range(2 * T + 3):
        tr = _transition(rng, g, N)
        ref.add(tr["obs"], tr["next_obs"], tr["action"], tr["reward"], tr["done"], terminal_obs=tr["terminal_obs"], timeouts=tr["timeouts"])
        ring[pos] = tr
        pos += 1
        if pos == T:
            full, pos = True, 0
        assert (ref.pos, ref.full) == (pos, full) and full == (g + 1 >= T)
        for t, held in enumerate(ring):
            if held is None:
                continue
            d = held["done"] != 0
            assert np.array_equal(ref.observations["x"][t], held["obs"]["x"])
            assert np.array_equal(ref.next_observations["x"][t], np.where(d[:, None], held["terminal_obs"]["x"], held["next_obs"]["x"]))
            assert np.array_equal(ref.actions[t], held["action"]) and np.array_equal(ref.rewards[t], held["reward"])
            assert np.array_equal(ref.dones[t], d.astype(np.float32)) and np.array_equal(ref.timeouts[t], held["timeouts"])
        M, first = ref.slot_range()
        assert (M, first) == ((T, 0) if full else (pos, 0))
        s = ref.sample(50)
        t_idx, n_idx = s["rows"][:50] // N, s["rows"][:50] % N
        assert np.array_equal(s["rows"][50:], s["rows"][:50] + T * N) and (t_idx < M).all()
        for b in range(50):
            held = ring[t_idx[b]]
            assert s["dones"][b, 0] == np.float32(held["done"][n_idx[b]]) * (np.float32(1) - held["timeouts"][n_idx[b]])
            assert s["rewards"][b, 0] == held["reward"][n_idx[b]] and np.array_equal(s["actions"][b], held["action"][n_idx[b]])
            assert np.array_equal(s["observations"]["x"][b], held["obs"]["x"][n_idx[b]])
    assert ReplayRef(3, 5, SPEC, 3).T == 1                    # max(buffer_size // n_envs, 1)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_carried_form_equals_the_plain_one_outside_the_slot_written_ahead(T, N):
    rng = np.random.default_rng(100 * T + N)
    plain, carried = ReplayRef(T * N, N, SPEC, 3), ReplayRef(T * N, N, SPEC, 3)
    seen = set()
    for g in range(2 * T + 3):
        tr = _transition(rng, g, N)
        if g == 0:
            carried.start(tr["obs"])
        plain.add(tr["obs"], tr["next_obs"], tr["action"], tr["reward"], tr["done"], terminal_obs=tr["terminal_obs"], timeouts=tr["timeouts"])
        carried.add_next(tr["next_obs"], tr["action"], tr["reward"], tr["done"], terminal_obs=tr["terminal_obs"], timeouts=tr["timeouts"])
        assert (carried.pos, carried.full, carried.carry) == (plain.pos, plain.full, True)
        ahead = carried.pos                                   # holds the head of transition g + 1 only
        assert np.array_equal(carried.observations["x"][ahead], tr["next_obs"]["x"])     # unselected: the post-reset observation
        for name in ("next_observations", "actions", "rewards", "dones", "timeouts"):
            a, b = getattr(plain, name), getattr(carried, name)
            a, b = (a["x"], b["x"]) if isinstance(a, dict) else (a, b)
            assert np.array_equal(a, b), name                 # add_next writes none of them ahead
        keep = [t for t in range(T) if t != ahead]
        assert np.array_equal(plain.observations["x"][keep], carried.observations["x"][keep])
        if carried.full and T == 1:
            with pytest.raises(RuntimeError):
                carried.slot_range()
            continue
        M, first = carried.slot_range()
        seen.add((M, first))
        slots = [(first + j) % T for j in range(M)]
        assert ahead not in slots and len(set(slots)) == M == (T - 1 if carried.full else carried.pos)
        for t in slots:                                       # every transition sample() can return is a whole one
            o, nx, d = carried.observations["x"][t], carried.next_observations["x"][t], carried.dones[t] != 0
            assert np.array_equal(o[:, 1], np.arange(N)) and np.array_equal(nx[:, 1], np.arange(N) + 0.5 * d)
            assert np.array_equal(nx[:, 0], o[:, 0] + 1 + 0.5 * d)
    if T > 1:
        assert seen == {(m, 0) for m in range(1, T)} | {(T - 1, (p + 1) % T) for p in range(T)}     # every (M, first) the ring produces
    plain.add(tr["obs"], tr["next_obs"], tr["action"], tr["reward"], tr["done"])
    carried.add(tr["obs"], tr["next_obs"], tr["action"], tr["reward"], tr["done"])
    assert not carried.carry                                  # a full add() ends the carried form
    with pytest.raises(RuntimeError):
        carried.add_next(tr["next_obs"], tr["action"], tr["reward"], tr["done"])


# ---------------------------------------------------------------------------------------------------------------- the draw
def test_draw_formula_against_python_integers():
    for seed, counter, M, first, T, N in ((0, 0, 5, 0, 5, 3), (3, 7, 4, 2, 5, 3), (2 ** 64 - 1, 2 ** 64 - 1, 96, 1, 97, 65),
                                          (12345, 1, (1 << 31) - 1, 5, 1 << 31, (1 << 31) - 1), (9, 9, 1 << 20, (1 << 20) - 1, 1 << 20, 1 << 12)):
        t, n = draw_cells(seed, counter, 40, M, first, T, N)
        rows = draw_rows(seed, counter, 40, M, first, T, N)
        head = mix64_int((seed + GOLDEN * (counter + 1)) & M64)
        for b in range(40):
            h = mix64_int((head + GOLDEN * (b + 1)) & M64)
            j = ((h >> 32) * M) >> 32
            tt, nn = (first + j) % T, ((h & 0xFFFFFFFF) * N) >> 32
            assert (int(t[b]), int(n[b]), int(rows[b])) == (tt, nn, tt * N + nn)
            assert 0 <= j < M and 0 <= nn < N


@pytest.mark.parametrize("M,N", [(5, 3), (4, 3), (97, 65), (1, 1), (7, 1024)])
def test_draw_reaches_every_cell_uniformly(M, N):
    """64 expected draws per (slot, env) cell: none is missed, none lies outside, and the chi-square statistic over the cells stays within four
    standard deviations of its mean (the reference formula gives at most 2.44 on these inputs)."""
    T, first = M + 1, M // 2                                  # a range that wraps inside a longer ring
    worst = 0.0
    for seed in range(4):
        for counter in range(4):
            B = 64 * M * N
            t, n = draw_cells(seed, counter, B, M, first, T, N)
            j = (t - first) % T
            assert j.min() >= 0 and j.max() < M and n.min() >= 0 and n.max() < N
            counts = np.bincount(j * N + n, minlength=M * N)
            assert counts.min() > 0, (seed, counter, int((counts == 0).sum()))
            if M * N > 1:
                chi2 = float(((counts - 64.0) ** 2 / 64.0).sum())
                z = (chi2 - (M * N - 1)) / np.sqrt(2.0 * (M * N - 1))
                worst = max(worst, abs(z))
                assert abs(z) < 4, (seed, counter, z)
    print(f"M={M} N={N}: worst |z| {worst:.2f}")


def test_draws_of_different_counters_and_seeds_differ():
    a = draw_rows(1, 0, 256, 50, 0, 50, 8)
    assert not np.array_equal(a, draw_rows(1, 1, 256, 50, 0, 50, 8)) and not np.array_equal(a, draw_rows(2, 0, 256, 50, 0, 50, 8))
    assert np.array_equal(a, draw_rows(1, 0, 256, 50, 0, 50, 8)) and np.array_equal(a[:100], draw_rows(1, 0, 100, 50, 0, 50, 8))


# ---------------------------------------------------------------------------------------------------------------- argument rules
def _spaces(H=16, W=16, A=2):
    obs = spaces.Dict({"tactile": spaces.Box(low=0, high=255, shape=(2, H, W), dtype=np.uint8),
                       "extended_feature": spaces.Box(low=-np.inf, high=np.inf, shape=(3,), dtype=np.float32)})
    return obs, spaces.Box(low=-1.0, high=1.0, shape=(A,), dtype=np.float32)


def _unallocated(T=4, N=3, **kw):
    """A buffer whose storage is on torch's meta device: every argument rule runs before anything touches a GPU."""
    import torch
    from tactile_gym_amd.replay import DeviceReplayBuffer

    class Unallocated(DeviceReplayBuffer):
        def _alloc(self, shape, dtype):
            return torch.empty(shape, dtype=dtype, device="meta")
    obs, act = _spaces()
    return Unallocated(T * N, obs, act, "cuda:0", N, **kw)


def test_module_is_exported_with_sb3s_names():
    pytest.importorskip("torch")
    import tactile_gym_amd as tg
    from tactile_gym_amd.replay import DeviceReplayBuffer, ReplayBufferSamples
    assert tg.DeviceReplayBuffer is DeviceReplayBuffer and tg.replay.DeviceReplayBuffer is DeviceReplayBuffer
    assert DeviceReplayBuffer.__init__.__code__.co_varnames[1:8] == ("buffer_size", "observation_space", "action_space", "device", "n_envs",
                                                                     "optimize_memory_usage", "handle_timeout_termination")
    assert ReplayBufferSamples._fields == ("observations", "actions", "next_observations", "dones", "rewards")
    assert DeviceReplayBuffer.add.__code__.co_varnames[1:7] == ("obs", "next_obs", "action", "reward", "done", "infos")


def test_constructor_errors_and_layout():
    torch = pytest.importorskip("torch")
    from tactile_gym_amd.replay import DeviceReplayBuffer
    obs, act = _spaces()
    with pytest.raises(ValueError, match="device"):
        DeviceReplayBuffer(4, obs, act, device="cpu")
    with pytest.raises(NotImplementedError, match="optimize_memory_usage"):
        DeviceReplayBuffer(4, obs, act, optimize_memory_usage=True)
    with pytest.raises(ValueError, match="buffer_size"):
        DeviceReplayBuffer(0, obs, act)
    with pytest.raises(ValueError, match="n_envs"):
        DeviceReplayBuffer(4, obs, act, n_envs=0)
    with pytest.raises(TypeError, match="observation_space"):
        DeviceReplayBuffer(4, spaces.Box(low=0, high=1, shape=(3,), dtype=np.float64), act)
    with pytest.raises(TypeError, match=r"observation_space\['oracle'\]"):
        DeviceReplayBuffer(4, spaces.Dict({"oracle": spaces.Box(low=0, high=1, shape=(3,), dtype=np.int32)}), act)
    with pytest.raises(TypeError, match="action_space"):
        DeviceReplayBuffer(4, obs, spaces.Box(low=0, high=1, shape=(2, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="channels_first"):
        DeviceReplayBuffer(4, obs, act, channels_first="yes")
    b = _unallocated(T=4, N=3)
    assert (b.buffer_size, b.n_envs, b.pos, b.full, b.size(), b.seed, b.counter) == (4, 3, 0, False, 0, 0, 0)
    assert _unallocated(T=4, N=3).buffer_size == 4 and type(b)(2, *_spaces(), "cuda:0", 3).buffer_size == 1      # max(2 // 3, 1)
    for k, shape, dt in (("tactile", (2, 16, 16), torch.uint8), ("extended_feature", (3,), torch.float32)):
        o, n = b.observations[k], b.next_observations[k]
        assert tuple(o.shape) == tuple(n.shape) == (4, 3) + shape and o.dtype == n.dtype == dt
        assert tuple(b._pair[k].shape) == (2, 4, 3) + shape          # one allocation: the next observation of row r is row r + T N
    assert tuple(b.actions.shape) == (4, 3, 2)
    for name in ("rewards", "dones", "timeouts"):
        assert tuple(getattr(b, name).shape) == (4, 3) and getattr(b, name).dtype == torch.float32
    assert b._channels_first == {"tactile": True} and _unallocated(channels_first=False)._channels_first == {"tactile": False}


def _args(N=3, A=2):
    import torch
    mk = lambda: {"tactile": torch.zeros((N, 2, 16, 16), dtype=torch.uint8), "extended_feature": torch.zeros((N, 3))}   # noqa: E731
    return dict(obs=mk(), next_obs=mk(), action=torch.zeros((N, A)), reward=torch.zeros(N), done=torch.zeros(N, dtype=torch.uint8))


def test_add_argument_errors():
    torch = pytest.importorskip("torch")
    b = _unallocated()
    with pytest.raises(ValueError, match="device"):                          # well formed, but on the CPU
        b.add(**_args())
    bad = [("action", torch.zeros((3, 3)), ValueError), ("action", torch.zeros((3, 2), dtype=torch.float64), TypeError),
           ("reward", torch.zeros(4), ValueError), ("reward", [0.0, 0.0, 0.0], TypeError),
           ("done", torch.zeros(3, dtype=torch.int64), TypeError), ("done", np.zeros(3, np.int32), TypeError),
           ("timeouts", torch.zeros(4), ValueError), ("timeouts", torch.zeros(3, dtype=torch.int32), TypeError),
           ("infos", [{}] * 2, ValueError), ("infos", {}, ValueError)]
    for name, value, exc in bad:
        with pytest.raises(exc, match=name):
            b.add(**dict(_args(), **{name: value}))
    with pytest.raises(ValueError, match="timeouts and infos"):
        b.add(**dict(_args(), timeouts=torch.zeros(3), infos=[{}] * 3))
    for which in ("obs", "next_obs", "terminal_obs"):
        for key, value, exc in (("tactile", torch.zeros((3, 16, 16, 2), dtype=torch.uint8), ValueError),
                                ("tactile", torch.zeros((3, 2, 16, 16)), TypeError), ("extended_feature", torch.zeros((3, 4)), ValueError)):
            a = dict(_args(), terminal_obs=_args()["obs"])
            a[which][key] = value
            with pytest.raises(exc, match=rf"{which}\['{key}'\]"):
                b.add(**a)
        a = dict(_args(), terminal_obs=_args()["obs"])
        del a[which]["extended_feature"]
        with pytest.raises(ValueError, match=which):
            b.add(**a)
    assert b.pos == 0 and not b.full                                          # a refused add writes nothing and does not advance


def test_state_and_sample_errors():
    torch = pytest.importorskip("torch")
    import tactile_gym_amd.augment as K
    b = _unallocated(T=4, N=3)
    a = _args()
    with pytest.raises(RuntimeError, match="start"):
        b.add_next(a["next_obs"], a["action"], a["reward"], a["done"])
    with pytest.raises(RuntimeError, match="for_env"):
        b.add_from_env(a["action"])
    with pytest.raises(ValueError, match="device"):
        b.start(a["obs"])
    with pytest.raises(RuntimeError, match="empty"):
        b.sample(2)
    b.pos = 2
    with pytest.raises(NotImplementedError, match="VecNormalize"):
        b.sample(2, env=object())
    with pytest.raises(ValueError, match="batch_size"):
        b.sample(0)
    with pytest.raises(TypeError, match="out_dtype"):
        b.sample(2, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="out_dtype"):
        b.sample(2, augment=K.RandomTranslate(seed=1), out_dtype=torch.uint8)
    with pytest.raises(TypeError, match="Identity"):
        b.sample(2, augment=torch.nn.Identity())
    assert b._slot_range() == (2, 0)
    b.pos, b.full = 1, True
    assert b._slot_range() == (4, 0)
    b._carry = True
    assert b._slot_range() == (3, 2)                                          # the slot written ahead is left out
    b.pos = 3
    assert b._slot_range() == (3, 0)
    one = _unallocated(T=1, N=3)
    one.full, one._carry = True, True
    with pytest.raises(RuntimeError, match="pending carry"):
        one.sample(2)
    assert b.counter == 0                                                     # a refused sample draws nothing


# ---------------------------------------------------------------------------------------------------------------- C ABI and resources
def test_c_abi_entries_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in _capi.SYMBOLS, name
    assert re.search(r"#define TG_ABI_VERSION 16\b", header) and _capi.ABI_VERSION == 16
    assert len(_capi.SYMBOLS["tg_replay_add"][1]) == 9 and len(_capi.SYMBOLS["tg_replay_draw"][1]) == 18
    assert os.path.exists(_capi.LIB_PATH), "library not built"
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"\b", nm), name


def test_replay_kernels_use_no_scratch(tmp_path):
    from test_kstep_quad_resources_cpu import LIB, _kernel_scratch
    assert os.path.exists(LIB), "library not built"
    scratch = _kernel_scratch(tmp_path)
    rp = {k: v for k, v in scratch.items() if "k_replay_" in k}
    assert sum("k_replay_add" in k for k in rp) == 1 and sum("k_replay_draw" in k for k in rp) == 1 and len(rp) == 2, sorted(rp)
    assert all(v == 0 for v in rp.values()), rp
