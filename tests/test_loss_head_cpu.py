"""tactile_gym_amd.loss_head without a GPU: at the inputs the GPU tests use, torch's own float32 composition and the numpy restatement of the
kernels (tests/loss_head_ref.py) stay inside every derived bound against the float64 composition; each usual mistake, put into the float64
formula, lands outside by the factor measured here (asserted with a margin of two); the input conditions are asserted; ppo_train's loop on a fake buffer; the C ABI
entries and the kernels' resources."""
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
import build_units  # noqa: E402
import loss_head_ref as ref  # noqa: E402

from tactile_gym_amd import _capi  # noqa: E402

BOUND_ENTRY = _capi.SYMBOLS["tg_ppo_loss"]                   # at import: the whole file needs the feature
torch = pytest.importorskip("torch")

ROWS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097, 5000)             # tests/test_gpu_loss_head_abi.py's shapes
WIDTHS = (1, 2, 6, 16)
CLIP, CLIP_VF, ENT, VF = 0.2, 0.2, 0.01, 0.5
GRADS = ("dmean", "dlog_std", "dvalues")


def ppo_case(B, A, per_row, clip_vf, normalize):
    """The inputs and keyword arguments of one shape of the GPU tests."""
    inp = ref.ppo_inputs(B, A, per_row, seed=1000 * B + 10 * A + per_row, clip_range=CLIP, clip_range_vf=clip_vf)
    return inp, dict(clip_range=CLIP, clip_range_vf=clip_vf, ent_coef=ENT, vf_coef=VF, normalize_advantage=normalize)


def worst(got, ex, bounds, names):
    """name -> worst error / bound over every element (no row is left out); an error of 0 counts as 0 whatever the bound."""
    out = {}
    for k in names:
        err = np.abs(np.asarray(got[k], np.float64) - ex[k])
        b = np.broadcast_to(bounds[k], err.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k] = float(np.max(np.where(err == 0, 0.0, err / b)))
    return out


def as_named(dev):
    got = dict(zip(ref.STATS, dev["stats"].astype(np.float64)))
    got.update({k: dev[k] for k in ("log_prob",) + GRADS})
    return got


@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("B", ROWS)
def test_float32_compositions_stay_within_the_bounds_of_float64(B, A):
    """torch's own float32 ops (its means and std accumulate in float32: acc=U) and the kernels' order in numpy (double accumulators)."""
    per_row, clip_vf, normalize = bool((B + A) % 2), (CLIP_VF if (B // 2 + A) % 2 else None), bool(B % 3)
    for per_row, clip_vf, normalize in ((per_row, clip_vf, normalize), (not per_row, CLIP_VF if clip_vf is None else None, not normalize)):
        inp, kw = ppo_case(B, A, per_row, clip_vf, normalize)
        ex = ref.ppo_exact(**inp, **kw)
        assert ref.conditions_hold(ex, inp, CLIP, clip_vf)                   # asserted, not assumed; no row is excluded
        names = ref.STATS + ("log_prob", "ratio") + GRADS
        w32 = worst(ref.ppo_exact(**inp, **kw, dtype=torch.float32), ex, ref.ppo_bounds(ex, **inp, **kw, acc=ref.U), names)
        wdev = worst(as_named(ref.ppo_device_order(**inp, **kw)), ex, ref.ppo_bounds(ex, **inp, **kw), ref.STATS + ("log_prob",) + GRADS)
        print(f"B={B} A={A} per_row={per_row} clip_vf={clip_vf} normalize={normalize}: torch float32 {max(w32.values()):.3f} ({max(w32, key=w32.get)}), "
              f"device order {max(wdev.values()):.3f} ({max(wdev, key=wdev.get)}) of the bound")
        assert max(w32.values()) <= 1.0, w32
        assert max(wdev.values()) <= 1.0, wdev
        if B > 1 and normalize:
            assert ex["adv_std"] > 0 and abs(float(np.mean(ex["adv"]))) < 1e-12
        else:
            assert ex["adv_mean"] == 0 and ex["adv_std"] == 1


def test_the_lane_tree_is_a_sum_and_chunks_are_added_ascending():
    rng = np.random.default_rng(3)
    for B in (1, 64, 255, 257, 1000):
        v = rng.standard_normal((B, 3))
        assert np.abs(ref.tree_sum(v, B) - v.sum(axis=0)).max() <= 1e-12
    v = np.zeros(600)
    v[[0, 300, 599]] = 1.0, 2.0 ** -53, 2.0 ** -53                            # ascending: each late small chunk sum is lost on its own
    assert ref.tree_sum(v, 600)[0] == 1.0


# ---------------------------------------------------------------------------------------------------------------- the usual mistakes: PPO
# name -> (the quantity that shows it, the worst error / bound measured here); half of it is asserted
PPO_MEASURED = {
    "max for min": ("policy_loss", 1311.0),
    "clamp passes when clipped": ("dmean", 82810.0),
    "variance over B": ("adv_std", 131600.0),
    "1e-8 left out": ("dmean", 699.4),
    "value clip when none asked": ("value_loss", 14110.0),
    "entropy sign": ("entropy_loss", 3403000.0),
    "entropy missing from dlog_std": ("dlog_std", 931.5),
    "approx_kl as mean(old - new)": ("approx_kl", 1989.0),
}


def _mistake_case(name):
    """B = 64, A = 6, log_std [A]; the advantages' spread is 1e-6 (their mean 1e-7) for the 1e-8; no value clip for the clip nobody asked for."""
    tiny = name == "1e-8 left out"
    clip_vf = None if name == "value clip when none asked" else CLIP_VF
    inp = ref.ppo_inputs(64, 6, False, seed=64, clip_range=CLIP, clip_range_vf=CLIP_VF, adv_scale=1e-6 if tiny else 1.0, adv_shift=0.1 if tiny else 0.3)
    return inp, dict(clip_range=CLIP, clip_range_vf=clip_vf, ent_coef=ENT, vf_coef=VF, normalize_advantage=True)


@pytest.mark.parametrize("name", sorted(PPO_MEASURED))
def test_usual_ppo_mistakes_break_the_bound(name):
    key, measured = PPO_MEASURED[name]
    inp, kw = _mistake_case(name)
    ex = ref.ppo_exact(**inp, **kw)
    assert ref.conditions_hold(ex, inp, CLIP, kw["clip_range_vf"] if kw["clip_range_vf"] is not None else CLIP_VF)
    if name == "1e-8 left out":
        assert 1e-7 < ex["adv_std"] < 1e-5
    if name in ("max for min", "clamp passes when clipped"):
        assert ((ex["ratio"] < 1 - CLIP) | (ex["ratio"] > 1 + CLIP)).sum() >= 8                # rows on which the clip acts
    bounds = ref.ppo_bounds(ex, **inp, **kw)
    ratio = worst(ref.ppo_exact(**inp, **kw, mistake=name), ex, bounds, (key,))[key]
    print(f"{name}: {key} lands {ratio:.4g} x its bound outside (measured {measured:.4g}, asserted {measured / 2:.4g})")
    assert ratio > measured / 2 > 1


def test_clip_fraction_with_greater_or_equal_shows_only_on_the_edge():
    """No bound can be broken on the inputs above: the input condition keeps every ratio 1e-4 off 1 -+ c, where > and >= agree.  What can be
    measured is the edge itself, left in on purpose: the old log-prob is the float64 new one (ratio == 1 in every row) and clip_range = 0;
    SB3's > counts no row, >= counts every row, against a bound of 0."""
    inp, kw = _mistake_case("clip_fraction with >=")
    kw = dict(kw, clip_range=0.0)
    inp = dict(inp, old_log_prob=ref.ppo_exact(**inp, **kw)["log_prob"])
    ex = ref.ppo_exact(**inp, **kw)
    assert (ex["ratio"] == 1).all() and ex["clip_fraction"] == 0 and ex["approx_kl"] == 0
    assert ref.ppo_bounds(ex, **inp, **kw)["clip_fraction"] == 0
    assert ref.ppo_exact(**inp, **kw, mistake="clip_fraction with >=")["clip_fraction"] == 1


def test_the_exact_case_in_the_kernels_order():
    """The head's own sample and log-prob fed back: ratio == 1 in every row, approx_kl == 0, clip_fraction == 0 (the device test does this on
    the device; here the restatements of both kernels)."""
    import action_head_ref as head
    rng = np.random.default_rng(9)
    B, A = 257, 6
    mean, ls = rng.uniform(-1, 1, (B, A)).astype(np.float32), rng.uniform(-2, 0, A).astype(np.float32)
    d = head.device_order(head.GAUSSIAN, mean, ls, np.full(A, -1, np.float32), np.full(A, 1, np.float32), seed=4, counter=2)
    zeros = np.zeros(B, np.float32)
    got = ref.ppo_device_order(mean, ls, zeros, d["actions"], d["log_prob"], rng.standard_normal(B).astype(np.float32), zeros)
    assert np.array_equal(got["log_prob"].view(np.uint32), d["log_prob"].view(np.uint32))
    assert got["stats"][4] == 0 and got["stats"][5] == 0


# ---------------------------------------------------------------------------------------------------------------- rsample
RSAMPLE_SHAPES = ((1, 1), (64, 2), (257, 6), (1000, 16))
RSAMPLE_MEASURED = {
    "mask left out": ("dlog_std", 16780000.0),
    "g_lp term left out": ("dlog_std", 16780000.0),
    "sigma eps left out": ("dlog_std", 49810000.0),
    "epsilon inside the square": ("dmean", 44.25),
}


def _rsample_float32(inp, g_a=True, g_lp=True):
    """The backward kernel's order in numpy at the float32 forward's own a and sigma (action_head_ref.device_order)."""
    import action_head_ref as head
    B, A = inp["mean"].shape
    fwd = head.device_order(head.SQUASHED, inp["mean"], inp["log_std"], np.full(A, -1, np.float32), np.full(A, 1, np.float32), -20.0, 2.0,
                            noise=inp["eps"])
    sigma = np.exp(head.clamp(inp["log_std"], -20.0, 2.0).astype(np.float64)).astype(np.float32)
    dmean, dls = ref.rsample_bwd_device_order(inp["g_a"] if g_a else None, inp["g_lp"] if g_lp else None, fwd["actions"], inp["eps"], sigma,
                                              inp["log_std"])
    return dict(dmean=dmean, dlog_std=dls)


@pytest.mark.parametrize("B,A", RSAMPLE_SHAPES)
def test_rsample_gradients_stay_within_the_bounds_of_float64(B, A):
    inp = ref.rsample_inputs(B, A, seed=B + A)
    ls = inp["log_std"].reshape(-1)
    if ls.size >= 6:
        assert all((ls == v).any() for v in (-20.0, 2.0)) and (ls < -20).any() and (ls > 2).any()      # on both edges and beyond both
    for g_a, g_lp in ((True, True), (True, False), (False, True)):
        args = (inp["mean"], inp["log_std"], inp["eps"], inp["g_a"] if g_a else None, inp["g_lp"] if g_lp else None)
        ex, bounds = ref.rsample_exact(*args), ref.rsample_bounds(*args)
        w32 = worst(ref.rsample_exact(*args, dtype=torch.float32), ex, ref.rsample_bounds(*args, autograd32=True), ("dmean", "dlog_std"))
        wdev = worst(_rsample_float32(inp, g_a, g_lp), ex, bounds, ("dmean", "dlog_std"))
        print(f"B={B} A={A} g_a={g_a} g_lp={g_lp}: torch float32 {w32}, device order {wdev} of the bound")
        assert max(w32.values()) <= 1.0 and max(wdev.values()) <= 1.0
        inside = (inp["log_std"] >= -20) & (inp["log_std"] <= 2)
        assert (ex["dlog_std"][~inside] == 0).all()
        if g_lp:
            assert (ex["dlog_std"][inside & ((inp["log_std"] == -20) | (inp["log_std"] == 2))] != 0).all()   # the mask is inclusive


@pytest.mark.parametrize("name", sorted(RSAMPLE_MEASURED))
def test_usual_rsample_mistakes_break_the_bound(name):
    """The epsilon inside the square moves w = 1 - a^2 + 1e-6 by (1 + 2 a) 1e-6 <= 50 U where the bound has to allow U (1 + w) on the same w
    with the same condition number (tests/test_action_head_cpu.py found the same for the log-prob): it cannot be broken by much, and what is
    measured is asserted."""
    key, measured = RSAMPLE_MEASURED[name]
    inp = ref.rsample_inputs(257, 6, seed=263)
    args = (inp["mean"], inp["log_std"], inp["eps"], inp["g_a"], inp["g_lp"])
    ex, bounds = ref.rsample_exact(*args), ref.rsample_bounds(*args)
    if name == "mask left out":                       # where the mask is 0 the bound is 0: measured against the bound without the mask
        bounds = ref.rsample_bounds(inp["mean"], np.clip(inp["log_std"], -20, 2), inp["eps"], inp["g_a"], inp["g_lp"])
    ratio = worst(ref.rsample_exact(*args, mistake=name), ex, bounds, (key,))[key]
    print(f"{name}: {key} lands {ratio:.4g} x its bound outside (measured {measured:.4g}, asserted {measured / 2:.4g})")
    assert ratio > measured / 2 > 1


# ---------------------------------------------------------------------------------------------------------------- C ABI and resources
def test_c_abi_entries_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    assert re.search(r"#define TG_ABI_VERSION 16\b", header) and _capi.ABI_VERSION == 16
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, n_args in (("tg_ppo_loss_workspace", 2), ("tg_ppo_loss", 25), ("tg_squashed_rsample", 15), ("tg_squashed_rsample_bwd", 14)):
        decl = re.search(rf"\b(?:int|int64_t) {name}\s*\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
        assert re.search(rf"\bT {name}\b", nm), name
    for name, value in (("PATH_AUTO", 0), ("PATH_ONE", 1), ("PATH_GRID", 2), ("ONE_MAX_ROWS", 4096)):
        assert re.search(rf"#define TG_LOSS_{name} {value}\b", header) and getattr(_capi, "LOSS_" + name) == value
    build_units.assert_exact_product_unit("tg_loss_head")
    core = open(os.path.join(ROOT, "tactile_gym_amd", "csrc", "tg_head_core.h")).read()
    for unit in ("tg_action_head.hip", "tg_loss_head.hip"):                   # one copy of the chain, in the header both include
        text = open(os.path.join(ROOT, "tactile_gym_amd", "csrc", unit)).read()
        assert '#include "tg_head_core.h"' in text and "0.9189385332046727f" not in text
    assert core.count("0.9189385332046727f") == 1


def test_python_entries_are_exported_and_refuse_cpu_tensors():
    import tactile_gym_amd as tg
    from tactile_gym_amd import loss_head, spaces, train
    assert tg.ppo_loss is loss_head.ppo_loss and tg.loss_head is loss_head and tg.train is train and callable(train.ppo_train)
    assert loss_head.STATS == ref.STATS
    z = torch.zeros
    with pytest.raises(ValueError, match="ROCm device"):
        tg.ppo_loss(z(4, 2), z(2), z(4), z(4, 2), z(4), z(4), z(4))
    with pytest.raises(ValueError, match="float32"):
        tg.ppo_loss(z(4, 2).double(), z(2), z(4), z(4, 2), z(4), z(4), z(4))
    with pytest.raises(TypeError):
        tg.ppo_loss(np.zeros((4, 2), np.float32), z(2), z(4), z(4, 2), z(4), z(4), z(4))
    head = tg.DeviceSquashedDiagGaussian(spaces.Box(low=-0.25, high=0.25, shape=(2,), dtype=np.float32), seed=3)
    with pytest.raises(ValueError, match="ROCm device"):
        head.rsample(z(4, 2), z(4, 2))
    assert head.counter == 0                                                  # a refused call draws nothing


def test_ppo_train_is_sb3s_loop_on_a_fake_buffer(monkeypatch):
    """The loop alone, with tg.ppo_loss replaced by a torch expression: minibatches per epoch, the keyword arguments handed on, the clip of
    the gradient norm, the stop at 1.5 target_kl BEFORE the step, and no host read of the stats without a target_kl."""
    from tactile_gym_amd import train
    from tactile_gym_amd.rollout import RolloutBufferSamples

    class Buf:
        def get(self, batch_size, augment=None, out_dtype=None):
            self.asked = (batch_size, augment, out_dtype)
            for start in range(0, 10, batch_size):
                n = min(batch_size, 10 - start)
                yield RolloutBufferSamples(torch.ones(n, 2), torch.zeros(n, 2), torch.zeros(n), torch.zeros(n), torch.ones(n), torch.zeros(n))

    class Unread(torch.Tensor):
        def __float__(self):
            raise AssertionError("the stats were read on the host")

    w = torch.nn.Parameter(torch.tensor([3.0, -4.0]))
    policy = lambda obs: (obs * w, w, (obs * w).sum(dim=1))   # noqa: E731
    seen, kls = [], []

    def fake_loss(mean, log_std, values, actions, old_log_prob, advantages, returns, **kw):
        seen.append((mean.shape[0], kw))
        stats = torch.zeros(8)
        stats[4] = kls.pop(0) if kls else 0.0
        return 100.0 * (log_std ** 2).sum(), stats.as_subclass(Unread) if kw_target[0] is None else stats

    monkeypatch.setattr(train, "ppo_loss", fake_loss)
    opt, buf = torch.optim.SGD([w], lr=1.0), Buf()
    kw_target = [None]
    stats = train.ppo_train(policy, opt, buf, 2, 4, 0.2, None, 0.01, 0.5, 0.5, None, augment="aug")
    assert [n for n, _ in seen] == [4, 4, 2] * 2 and buf.asked == (4, "aug", torch.float32) and stats.shape == (8,)
    assert seen[0][1] == dict(old_values=seen[0][1]["old_values"], clip_range=0.2, clip_range_vf=None, ent_coef=0.01, vf_coef=0.5,
                              normalize_advantage=True)
    # six SGD steps of a gradient clipped to norm 0.5 along w: |w| went from 5 to 2
    assert abs(float(w.detach().norm()) - 2.0) < 1e-5
    kw_target[0], kls[:] = 0.01, [0.0149, 0.0151, 0.0]
    del seen[:]
    before = w.detach().clone()
    stats = train.ppo_train(policy, opt, buf, 3, 4, 0.2, None, 0.01, 0.5, None, 0.01)
    assert len(seen) == 2 and abs(float(stats[4]) - 0.0151) < 1e-7          # the second minibatch exceeds 1.5 target_kl: no step for it
    assert torch.allclose(w.detach(), before - 200.0 * before)               # one unclipped step (max_grad_norm=None) and no more


def test_loss_head_kernels_use_no_scratch(tmp_path):
    from test_kstep_quad_resources_cpu import LIB, _kernel_scratch
    assert os.path.exists(LIB), "library not built"
    scratch = _kernel_scratch(tmp_path)
    ours = {k: v for k, v in scratch.items() if "k_ppo_" in k or "k_squashed_rsample" in k}
    assert len(ours) == 6, sorted(ours)               # k_ppo_one, k_ppo_stats, k_ppo_chunks, k_ppo_finish, k_squashed_rsample, k_squashed_rsample_bwd
    assert all(v == 0 for v in ours.values()), ours
    head = {k: v for k, v in scratch.items() if "k_action_head" in k}         # the head, now built over the shared header
    assert len(head) == 3 and all(v == 0 for v in head.values()), head
