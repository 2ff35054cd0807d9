"""tg_sac_critic_loss and tg_sac_actor_loss (csrc/tg_sac_loss.hip) called directly on raw pointers between guard bytes: row counts round the
wavefront and the 256-row chunk, one to four critics, both sources of alpha.  Every stat, the target and every gradient against the float64
composition of tests/sac_loss_ref.py within the bounds its docstring derives (no row left out, the input conditions asserted), a second call
bit for bit, every subset of the nullable outputs, the exact case worked by hand, ties, done rows, extreme coefficients and the error returns."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sac_loss_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from loss_device import GAMMA, _actor, _bits, _critic, f32  # noqa: E402

ROWS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)
CRITICS = (1, 2, 3, 4)
TARGET_ENTROPY = -2.0
CRITIC_KEYS = ("critic_loss", "ent_coef", "target_q_mean", "min_next_q_mean", "mse", "target", "dq_cur")
ACTOR_KEYS = ("actor_loss", "ent_coef_loss", "ent_coef", "log_prob_mean", "min_q_pi_mean", "dlog_ent_coef", "dlog_prob", "dq_pi")


def _critic_named(got, n):
    return ref.critic_named(dict(stats=got["stats"], target=got["target"], dq_cur=np.stack([got[f"dq_cur{i}"] for i in range(n)])), n)


def _actor_named(got, n):
    return ref.actor_named(dict(stats=got["stats"], dlog_prob=got["dlog_prob"], dq_pi=np.stack([got[f"dq_pi{i}"] for i in range(n)])))


def _within(got, ex, bounds, names, what):
    for k in names:
        err = np.abs(np.asarray(got[k], np.float64) - ex[k])
        bad = err > np.broadcast_to(bounds[k], err.shape)
        assert not bad.any(), (what, k, float(err.max()), float(np.max(bounds[k])))


def _sources(B, n):
    return (dict(log_ent_coef=float(f32(-1.5 + 0.25 * n + 0.001 * (B % 7)))), dict(ent_coef=0.2))


@pytest.mark.parametrize("n", CRITICS)
@pytest.mark.parametrize("B", ROWS)
def test_stats_target_and_gradients_within_bounds_and_a_second_call_bit_equal(B, n):
    for src in _sources(B, n):
        inp = ref.sac_critic_inputs(B, n, seed=100 * B + n)
        assert ref.critics_apart(inp["q_next"])
        ex = ref.sac_critic_exact(**inp, gamma=GAMMA, **src)
        got = _critic(inp, src)
        _within(_critic_named(got, n), ex, ref.sac_critic_bounds(ex, **inp, gamma=GAMMA, **src), CRITIC_KEYS, ("critic", B, n, src))
        assert (got["stats"][4 + n:] == 0).all()
        done = inp["dones"] == 1
        assert _bits(got["target"][done], inp["rewards"][done])               # dones == 1: target == rewards bit for bit
        again = _critic(inp, src)
        assert all(_bits(got[k], again[k]) for k in got), ("critic", B, n)
        want = ref.sac_critic_device_order(**inp, gamma=GAMMA, **src)         # and the numpy restatement's bits
        assert _bits(got["stats"], want["stats"]) and _bits(got["target"], want["target"])
        act = ref.sac_actor_inputs(B, n, seed=100 * B + n + 50)
        assert ref.critics_apart(act["q_pi"])
        for te in ((TARGET_ENTROPY, None) if "log_ent_coef" in src else (None,)):
            ex = ref.sac_actor_exact(**act, **src, target_entropy=te)
            got = _actor(act, src, te)
            _within(_actor_named(got, n), ex, ref.sac_actor_bounds(ex, **act, **src, target_entropy=te), ACTOR_KEYS, ("actor", B, n, src, te))
            assert (got["stats"][6:] == 0).all()
            if te is None:
                assert got["stats"][1] == 0 and got["stats"][5] == 0
            again = _actor(act, src, te)
            assert all(_bits(got[k], again[k]) for k in got), ("actor", B, n)
            assert _bits(got["stats"], ref.sac_actor_device_order(**act, **src, target_entropy=te)["stats"])


@pytest.mark.parametrize("B,n", [(257, 2), (65, 4)])
def test_every_subset_of_the_nullable_outputs(B, n):
    src = dict(log_ent_coef=-0.5)
    inp, act = ref.sac_critic_inputs(B, n, seed=B), ref.sac_actor_inputs(B, n, seed=B + 1)
    full_c, full_a = _critic(inp, src), _actor(act, src, TARGET_ENTROPY)
    names_c = ("target",) + tuple(f"dq_cur{i}" for i in range(n))
    names_a = ("dlog_prob",) + tuple(f"dq_pi{i}" for i in range(n))
    for r in range(n + 1):
        for subset in itertools.combinations(names_c, r):
            got = _critic(inp, src, outputs=subset)
            assert set(got) == {"stats", *subset} and all(_bits(got[k], full_c[k]) for k in got), subset
        for subset in itertools.combinations(names_a, r):
            got = _actor(act, src, TARGET_ENTROPY, outputs=subset)
            assert set(got) == {"stats", *subset} and all(_bits(got[k], full_a[k]) for k in got), subset


def test_the_exact_case_worked_by_hand():
    """Small integers, gamma = 0.5, log_ent_coef = 0 (alpha == 1), B = 4: every intermediate is a dyadic rational that float32 holds, so the
    outputs are the hand-worked numbers bit for bit.
      min q_next = [1, -1, 4, -2];  y = min - next_log_prob = [2, -2, 2, -2];  (1 - dones) gamma = [.5, 0, .5, .5];  target = rewards + . y =
      [1 + 1, 2 + 0, -1 + 1, 0 - 1] = [2, 2, 0, -1];  e_0 = [1, 0, 2, 2], e_1 = [-2, 2, -1, -2];  mse = [9 / 4, 13 / 4];  loss = 0.5 * 5.5.
      min q_pi = [0, 0, 2, -2] at k = [1, 0 (a tie), 0, 1];  a = log_prob - min = [-1, 2, -2, 3], mean 0.5;  c = log_prob - 2 = [-3, 0, -2, -1]."""
    v = lambda *x: np.array(x, f32)   # noqa: E731
    src = dict(log_ent_coef=0.0)
    inp = dict(q_cur=[v(3, 2, 2, 1), v(0, 4, -1, -3)], q_next=[v(2, -1, 4, 0), v(1, 3, 4, -2)], next_log_prob=v(-1, 1, 2, 0),
               rewards=v(1, 2, -1, 0), dones=v(0, 1, 0, 0))
    got = _critic(inp, src, gamma=0.5)
    assert _bits(got["target"], v(2, 2, 0, -1))
    assert _bits(got["stats"], v(2.75, 1.0, 0.75, 0.5, 2.25, 3.25, 0, 0))
    assert _bits(got["dq_cur0"], v(0.25, 0, 0.5, 0.5)) and _bits(got["dq_cur1"], v(-0.5, 0.5, -0.25, -0.5))
    act = dict(log_prob=v(-1, 2, 0, 1), q_pi=[v(1, 0, 2, -1), v(0, 0, 3, -2)])
    got = _actor(act, src, -2.0)
    assert np.array_equal(got["stats"], v(0.5, 0, 1.0, 0.5, 0.0, 1.5, 0, 0))  # ent_coef_loss = -(0 * c) is a zero of either sign
    assert _bits(got["stats"][[0, 2, 3, 4, 5]], v(0.5, 1.0, 0.5, 0.0, 1.5))
    assert _bits(got["dlog_prob"], v(0.25, 0.25, 0.25, 0.25))
    assert _bits(got["dq_pi0"], v(0, -0.25, -0.25, 0)) and _bits(got["dq_pi1"], v(-0.25, 0, 0, -0.25))
    got = _actor(act, dict(log_ent_coef=1.0), -2.0)                           # ent_coef_loss = -mean(1 * c) = 1.5, the same as dlog_ent_coef
    assert got["stats"][1] == 1.5 and got["stats"][5] == 1.5


@pytest.mark.parametrize("B", [5, 300])
def test_ties_send_the_whole_gradient_to_the_lowest_index(B):
    rng = np.random.default_rng(B)
    q = rng.standard_normal(B).astype(f32)
    act = dict(log_prob=rng.standard_normal(B).astype(f32), q_pi=[q, q.copy()])
    got = _actor(act, dict(ent_coef=0.2))
    assert _bits(got["dq_pi0"], np.full(B, f32(-1.0) / f32(B), f32)) and _bits(got["dq_pi1"], np.zeros(B, f32))
    act = dict(act, q_pi=[q + f32(1.0), q, q.copy(), q - f32(1.0)] if B == 5 else [q + f32(1.0), q, q.copy()])
    got = _actor(act, dict(ent_coef=0.2))
    k = 3 if B == 5 else 1
    for i in range(len(act["q_pi"])):
        assert _bits(got[f"dq_pi{i}"], np.full(B, f32(-1.0) / f32(B) if i == k else 0.0, f32)), i


def test_extreme_entropy_coefficients_stay_finite():
    inp, act = ref.sac_critic_inputs(70, 2, seed=3), ref.sac_actor_inputs(70, 2, seed=4)
    for lec in (-20.0, 2.0):
        src = dict(log_ent_coef=lec)
        got = _critic(inp, src)
        assert all(np.isfinite(x).all() for x in got.values()) and got["stats"][1] == f32(np.exp(np.float64(lec)))
        ex = ref.sac_critic_exact(**inp, gamma=GAMMA, **src)
        _within(_critic_named(got, 2), ex, ref.sac_critic_bounds(ex, **inp, gamma=GAMMA, **src), CRITIC_KEYS, lec)
        got = _actor(act, src, TARGET_ENTROPY)
        assert all(np.isfinite(x).all() for x in got.values())
        ex = ref.sac_actor_exact(**act, **src, target_entropy=TARGET_ENTROPY)
        _within(_actor_named(got, 2), ex, ref.sac_actor_bounds(ex, **act, **src, target_entropy=TARGET_ENTROPY), ACTOR_KEYS, lec)


def test_error_returns_write_nothing():
    src = dict(log_ent_coef=-0.5)
    inp, act = ref.sac_critic_inputs(70, 2, seed=1), ref.sac_actor_inputs(70, 2, seed=2)
    for name in ("q_cur", "q_next", "q_cur0", "q_cur1", "q_next0", "q_next1", "next_log_prob", "rewards", "dones", "stats"):
        _critic(inp, src, expect_error=True, null=(name,))
    for over in (dict(B=0), dict(B=-1), dict(B=65537), dict(n=0), dict(n=5), dict(n=-1)):
        _critic(inp, src, expect_error=True, **over)
        _actor(act, src, TARGET_ENTROPY, expect_error=True, **over)
    for name in ("log_prob", "q_pi", "q_pi0", "q_pi1", "stats"):
        _actor(act, src, TARGET_ENTROPY, expect_error=True, null=(name,))
    _actor(act, src, TARGET_ENTROPY, expect_error=True, null=("log_ent_coef",))        # the entropy loss asked, no log_ent_coef_dev
    _actor(act, dict(ent_coef=0.2), None, expect_error=True, want=True)
    ok = _actor(act, dict(ent_coef=0.2), None)                                  # not asked: the float coefficient serves
    assert np.isfinite(ok["stats"]).all() and ok["stats"][2] == f32(0.2)
    big = ref.sac_critic_inputs(65536, 1, seed=9)                             # the largest B is served
    got = _critic(big, dict(ent_coef=0.2))
    ex = ref.sac_critic_exact(**big, gamma=GAMMA, ent_coef=0.2)
    _within(_critic_named(got, 1), ex, ref.sac_critic_bounds(ex, **big, gamma=GAMMA, ent_coef=0.2), CRITIC_KEYS, 65536)
