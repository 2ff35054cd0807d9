"""tg_optim_sumsq and tg_optim_adam (csrc/tg_optim.h in tg_loss_head.hip) called directly on raw pointers between guard bytes: element counts
round the 16-byte vector, the wavefront and the chunk, tensor counts round the table's capacity, a tensor whose base is only 4-byte aligned,
the clip on and off, weight decay zero and not, the coefficient on both sides of 1.  After each of three steps p, m, v and the total norm are
the bits of tests/optim_ref.py, the gradients unchanged and the guards intact; a second run from the same state gives the same bits; a NaN
or an infinity in one gradient goes where the specification sends it; the error returns launch nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import optim_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import PATTERN, Guarded  # noqa: E402
from loss_device import _bits, _lib, _stream  # noqa: E402

f32 = np.float32
CHUNK, CAP = ref.CHUNK, ref.MAX_TENSORS
COUNTS = (1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
LR, B1, B2 = 3e-4, 0.9, 0.999


def _same(a, b):
    """Bit for bit, a NaN for a NaN (its payload is not specified)."""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    nan = np.isnan(a)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and _bits(a[~nan], b[~nan])


def _array(ctype, values):
    return (ctype * max(1, len(values)))(*values)


class Device:
    """The tensors of a call in guarded device buffers (offsets[i]: bytes past a 16-byte address of tensor i's four arrays)."""

    def __init__(self, state, offsets=None):
        self.n = len(state["p"])
        offsets = offsets or [0] * self.n
        self.counts = [int(x.size) for x in state["p"]]
        self.buf = {k: [Guarded(4 * c, offset=o, fill=x) for c, o, x in zip(self.counts, offsets, state[k])] for k in ("p", "m", "v")}
        self.buf["g"] = [Guarded(4 * c, offset=o) for c, o in zip(self.counts, offsets)]
        self.chunks = ref.chunk_prefix(self.counts)[-1]
        self.partials, self.total = Guarded(8 * self.chunks), Guarded(4)

    def ptrs(self, key, null=None):
        return _array(C.c_void_p, [None if i == null else g.ptr for i, g in enumerate(self.buf[key])])

    def step(self, grads, steps, eps, wd, max_norm, lrs=None, expect=None, **over):
        """One optimiser step: tg_optim_sumsq when clipping, then tg_optim_adam.  expect: the entry whose error return is expected; over:
        what the call gets in place of a right argument."""
        capi, L = _lib()
        for g, x in zip(self.buf["g"], grads):
            g.payload().copy_(torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8)))
        before = {k: [g.payload().clone() for g in self.buf[k]] for k in self.buf}
        lrs = lrs or [LR] * self.n
        corr = [ref.corrections(lrs[i], B1, B2, steps[i]) for i in range(self.n)]
        n = over.get("n", self.n)
        counts = _array(C.c_int64, over.get("counts", self.counts))
        clip = max_norm is not None
        rc, entry = 0, None
        if clip:
            entry = "tg_optim_sumsq"
            rc = L.tg_optim_sumsq(n, None if over.get("null") == "grads" else self.ptrs("g", over.get("null_g")), None if over.get("null") == "counts" else counts,
                                  C.c_void_p(None if over.get("null") == "partials" else self.partials.ptr), over.get("workspace", 8 * self.chunks), _stream())
        if rc == 0 and expect != "tg_optim_sumsq":
            entry = "tg_optim_adam"
            null = over.get("null")
            rc = L.tg_optim_adam(n, None if null == "params" else self.ptrs("p", over.get("null_p")), None if null == "grads" else self.ptrs("g", over.get("null_g")),
                                 None if null == "exp_avg" else self.ptrs("m"), None if null == "exp_avg_sq" else self.ptrs("v", over.get("null_v")),
                                 None if null == "counts" else counts, None if null == "step_size" else _array(C.c_float, [c[0] for c in corr]),
                                 None if null == "bias_corr2_sqrt" else _array(C.c_float, [c[1] for c in corr]), B1, B2, eps, wd, 1 if clip else 0,
                                 over.get("bad_max_norm", max_norm if clip else 0.0), C.c_void_p(None if null == "partials" or not clip else self.partials.ptr),
                                 over.get("n_partials", self.chunks if clip else 0), C.c_void_p(None if null == "total" or not clip else self.total.ptr),
                                 _stream())
        torch.cuda.synchronize()
        for k in self.buf:
            for g in self.buf[k]:
                assert g.guards_intact(), k
        assert self.partials.guards_intact() and self.total.guards_intact()
        for g, was in zip(self.buf["g"], before["g"]):
            assert torch.equal(g.payload(), was)                               # the gradients are read, never written
        if expect is not None:
            assert rc != 0 and entry == expect and L.tg_last_error().decode().startswith(expect + ":"), (rc, entry, L.tg_last_error())
            for k in ("p", "m", "v"):
                assert all(torch.equal(g.payload(), was) for g, was in zip(self.buf[k], before[k])), k      # nothing was launched
            if expect == "tg_optim_sumsq":
                assert bool((self.partials.payload() == PATTERN).all())
            return None
        capi.check(rc)
        out = {k: [g.host(f32) for g in self.buf[k]] for k in ("p", "m", "v")}
        out["total"] = self.total.host(f32)[0] if clip else None
        out["partials"] = self.partials.host(np.float64) if clip else None
        return out


def _state(counts, seed):
    rng = np.random.default_rng(seed)
    return dict(p=[rng.standard_normal(c).astype(f32) for c in counts], m=[np.zeros(c, f32) for c in counts], v=[np.zeros(c, f32) for c in counts])


def _grads(counts, rng, scale):
    return [(rng.standard_normal(c) * scale).astype(f32) for c in counts]


def _three_steps(counts, offsets, eps, wd, max_norm, scale, seed):
    """Three steps on the device and in the restatement side by side; returns the coefficients met."""
    state = _state(counts, seed)
    dev = Device(state, offsets)
    rng = np.random.default_rng(seed + 1)
    coefs = []
    for step in (1, 2, 3):
        grads = _grads(counts, rng, scale * (1.0 if step != 2 else 0.5))
        steps = [step] * len(counts)
        got = dev.step(grads, steps, eps, wd, max_norm)
        P, M, V, total = ref.step_device_order(state["p"], grads, state["m"], state["v"], steps, LR, B1, B2, eps, wd, max_norm)
        what = (counts if len(counts) < 4 else len(counts), offsets and max(offsets), eps, wd, max_norm, step)
        if max_norm is not None:
            assert _bits(got["partials"], ref.partial_sums(grads)), what
            assert _bits(np.array([got["total"]]), np.array([total])), what
            coefs.append(float(ref.clip_coef(total, max_norm)))
        for i in range(len(counts)):
            assert _bits(got["m"][i], M[i]) and _bits(got["v"][i], V[i]) and _bits(got["p"][i], P[i]), (what, i)
        state = dict(p=P, m=M, v=V)
    return coefs


@pytest.mark.parametrize("count", COUNTS)
def test_one_tensor_at_every_count_is_the_restatement_bit_for_bit(count):
    """One tensor, aligned and 4 bytes past a 16-byte address (the one-by-one path): the clip with the coefficient on both sides of 1 and
    without, weight decay zero and not."""
    norm = np.sqrt(count)                                                       # of N(0, 1) gradients, roughly
    seen = []
    for offset in (0, 4):
        seen += _three_steps([count], [offset], 1e-5, 0.0, 0.75 * norm, 1.0, seed=count)          # coef ~ 0.75, and ~ 1.5 -> 1 at the half-size step
        _three_steps([count], [offset], 1e-8, 0.01, None, 1.0, seed=count + 1)
        _three_steps([count], [offset], 1e-8, 0.01, 0.5, 30.0, seed=count + 2)
    if count >= 63:
        assert min(seen) < 1.0 and max(seen) == 1.0, seen


@pytest.mark.parametrize("n_tensors", [1, 2, CAP, CAP + 1])
def test_tensor_counts_round_the_table(n_tensors):
    """The counts of COUNTS in turn, tensor 1 (0 where it stands alone) 4 bytes and the last 12 bytes past a 16-byte address; capacity + 1
    tensors take a second launch of each kernel, whose chunks go on from the first's."""
    counts = [COUNTS[(3 * i + 7) % len(COUNTS)] for i in range(n_tensors)]
    offsets = [0] * n_tensors
    offsets[min(1, n_tensors - 1)] = 4
    if n_tensors > 2:
        offsets[-1] = 12
    norm = np.sqrt(sum(counts))
    seen = _three_steps(counts, offsets, 1e-5, 0.0, 0.75 * norm, 1.0, seed=n_tensors)
    assert min(seen) < 1.0 and max(seen) == 1.0, seen
    _three_steps(counts, offsets, 1e-8, 0.01, None, 1.0, seed=n_tensors + 1)
    _three_steps(counts, offsets, 1e-5, 0.01, 0.5, 1.0, seed=n_tensors + 2)
    _three_steps(counts, offsets, 1e-5, 0.0, None, 1.0, seed=n_tensors + 3)


def test_a_second_run_from_the_same_state_is_bit_equal_and_tensors_keep_their_own_factors():
    counts = [5, CHUNK + 1, 2 * CHUNK + 3, 64]
    state = _state(counts, 5)
    rng = np.random.default_rng(6)
    state["m"], state["v"] = _grads(counts, rng, 0.1), [np.abs(x) for x in _grads(counts, rng, 0.01)]
    grads = _grads(counts, rng, 1.0)
    steps, lrs = [3, 1, 7, 2], [LR, 1e-2, LR, 1e-4]                            # per tensor: skipped tensors and param groups
    runs = [Device(state, [0, 4, 0, 8]).step(grads, steps, 1e-5, 0.0, 20.0, lrs) for _ in range(2)]
    for k in ("p", "m", "v", "partials"):
        assert all(_bits(a, b) for a, b in zip(runs[0][k], runs[1][k])), k
    assert runs[0]["total"] == runs[1]["total"]
    P, M, V, total = ref.step_device_order(state["p"], grads, state["m"], state["v"], steps, lrs, B1, B2, 1e-5, 0.0, 20.0)
    assert all(_bits(a, b) for a, b in zip(runs[0]["p"], P)) and all(_bits(a, b) for a, b in zip(runs[0]["v"], V)) and runs[0]["total"] == total
    # the clip may cover more tensors than an Adam call: two calls over the halves read the same partials
    dev = Device(state, [0, 4, 0, 8])
    capi, L = _lib()
    for g, x in zip(dev.buf["g"], grads):
        g.payload().copy_(torch.from_numpy(x.view(np.uint8)))
    capi.check(L.tg_optim_sumsq(4, dev.ptrs("g"), _array(C.c_int64, counts), C.c_void_p(dev.partials.ptr), 8 * dev.chunks, _stream()))
    for half in ((0, 1), (2, 3)):
        corr = [ref.corrections(lrs[i], B1, B2, steps[i]) for i in half]
        pick = lambda k: _array(C.c_void_p, [dev.buf[k][i].ptr for i in half])   # noqa: E731
        capi.check(L.tg_optim_adam(2, pick("p"), pick("g"), pick("m"), pick("v"), _array(C.c_int64, [counts[i] for i in half]),
                                   _array(C.c_float, [c[0] for c in corr]), _array(C.c_float, [c[1] for c in corr]), B1, B2, 1e-5, 0.0, 1, 20.0,
                                   C.c_void_p(dev.partials.ptr), dev.chunks, C.c_void_p(dev.total.ptr), _stream()))
    torch.cuda.synchronize()
    assert all(_bits(g.host(f32), want) for g, want in zip(dev.buf["p"], P)) and dev.total.host(f32)[0] == total
    assert all(g.guards_intact() for k in dev.buf for g in dev.buf[k])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_gradient_that_is_not_finite_goes_where_clip_grad_norm_sends_it(bad):
    counts = [70, CHUNK + 5, 3]
    state = _state(counts, 9)
    rng = np.random.default_rng(10)
    grads = _grads(counts, rng, 1.0)
    grads[1][CHUNK + 2] = bad
    steps = [1, 1, 1]
    got = Device(state).step(grads, steps, 1e-5, 0.0, 0.5)
    P, M, V, total = ref.step_device_order(state["p"], grads, state["m"], state["v"], steps, LR, B1, B2, 1e-5, 0.0, 0.5)
    assert _same(np.array([got["total"]]), np.array([total])) and not np.isfinite(got["total"])
    for i in range(3):
        assert _same(got["p"][i], P[i]) and _same(got["m"][i], M[i]) and _same(got["v"][i], V[i]), i
    if np.isnan(bad):                                                          # a NaN norm: the coefficient is NaN, every element with it
        assert all(np.isnan(x).all() for k in ("p", "m", "v") for x in got[k])
    else:                                                                      # an infinite norm: the coefficient is 0, inf * 0 = NaN where the infinity stood
        assert np.isnan(got["p"][1][CHUNK + 2]) and np.isfinite(np.delete(got["p"][1], CHUNK + 2)).all()
        assert np.isfinite(got["p"][0]).all() and np.isfinite(got["p"][2]).all()
    got = Device(state).step(grads, steps, 1e-5, 0.0, None)                     # without the clip the element alone is lost
    P, M, V, _ = ref.step_device_order(state["p"], grads, state["m"], state["v"], steps, LR, B1, B2, 1e-5)
    assert all(_same(got["p"][i], P[i]) and _same(got["v"][i], V[i]) for i in range(3))
    assert np.isfinite(np.delete(got["p"][1], CHUNK + 2)).all() and not np.isfinite(got["v"][1][CHUNK + 2])


def test_error_returns_launch_nothing():
    counts = [70, CHUNK + 5]
    state = _state(counts, 11)
    grads = _grads(counts, np.random.default_rng(12), 1.0)
    dev = Device(state)
    steps = [1, 1]
    for over in (dict(null="grads"), dict(null="counts"), dict(null="partials"), dict(null_g=1), dict(n=0), dict(n=-1), dict(counts=[70, 0]),
                 dict(counts=[-1, 5]), dict(workspace=8 * dev.chunks - 1), dict(workspace=0)):
        dev.step(grads, steps, 1e-5, 0.0, 0.5, expect="tg_optim_sumsq", **over)
    capi, L = _lib()
    assert L.tg_optim_workspace(dev.chunks) == 8 * dev.chunks and L.tg_optim_workspace(0) < 0 and L.tg_optim_workspace(-3) < 0
    adam_errors = [dict(null=k) for k in ("params", "grads", "exp_avg", "exp_avg_sq", "counts", "step_size", "bias_corr2_sqrt")]
    adam_errors += [dict(null_p=0), dict(null_g=1), dict(null_v=1), dict(n=0), dict(counts=[70, 0])]
    for over in adam_errors:
        dev.step(grads, steps, 1e-5, 0.0, None, expect="tg_optim_adam", **over)
    for over in (dict(bad_max_norm=-0.5), dict(bad_max_norm=float("nan")), dict(n_partials=0), dict(null="total")):      # a clipped call's own, behind a good tg_optim_sumsq
        dev.step(grads, steps, 1e-5, 0.0, 0.5, expect="tg_optim_adam", **over)
    got = dev.step(grads, steps, 1e-5, 0.0, 0.0)                                # max_norm 0 is served: every gradient counts as 0
    assert all(_bits(a, b) for a, b in zip(got["p"], state["p"])) and all((x == 0).all() for x in got["m"] + got["v"])
