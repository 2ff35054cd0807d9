"""tg_mlp_forward, tg_mlp_backward_workspace and tg_mlp_backward (csrc/tg_mlp.hip) called directly on raw pointers, every buffer between guard
bytes inside a larger allocation: the smallest shapes at which the mapping can go wrong (B 1, 3, 33, 65; K0 1, 2, 3, 31, 33 and 256 + 2 as two
column blocks; widths 1, 2, 33, 64, 256; 1 to 4 layers; 1 and 2 towers; all three activations; a last layer of 2 + 2 rows).

On the exact cases float32 arithmetic is exact in every order (tests/mlp_ref.py asserts it per case), so the float64 restatement IS the required
bits; with N(0, 0.05) weights every saved h_l lies within the per-layer bound of the reference computed from the device's own h_{l-1} bits and
the outputs within the propagated bound.  A row's outputs must not depend on the batch or the towers around it; two backward calls must give
the same bits; the error returns take no launch and write nothing."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mlp_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import PATTERN, Guarded  # noqa: E402
from mlp_device import Call, _backward, _bits, _check_backward, _forward, _lib, _stream, _within  # noqa: E402  (shared with test_gpu_mlp_matrix.py)

f32 = np.float32

# (B, K0, Ka, [(widths, acts, two), ...]): Ka < K0 gives two column blocks
CASES = [
    (1, 1, 1, [([1], ["none"], 0)]),
    (3, 2, 2, [([2, 1], ["relu", "none"], 0)]),
    (33, 3, 1, [([33, 64, 2], ["relu", "relu", "none"], 0), ([64, 1], ["none", "relu"], 0)]),
    (65, 31, 31, [([256, 256, 2], ["relu", "relu", "none"], 0), ([256, 256, 1], ["relu", "relu", "none"], 0)]),
    (65, 33, 33, [([64, 33, 2, 1], ["relu", "none", "relu", "none"], 0)]),
    (65, 258, 256, [([256, 256, 1], ["relu", "relu", "none"], 0), ([256, 256, 1], ["relu", "relu", "none"], 0)]),
    (3, 33, 33, [([64, 2], ["relu", "none"], 2)]),
    (33, 258, 256, [([33], ["relu"], 2), ([2, 33], ["none", "relu"], 0)]),
]
# B = 2081: 66 row tiles on 64 workgroups per tower, so workgroups 0 and 1 walk a second tile and continue their own partial sums
BWD_CASES = ([c for c in CASES if c[0] in (1, 3, 65)] + [(65, 3, 2, [([33, 2], ["relu", "none"], 2), ([1], ["none"], 0)]),
                                                         (2081, 3, 2, [([33, 2], ["relu", "none"], 2), ([1], ["none"], 0)])])


def _id(case):
    B, K0, Ka, towers = case
    return f"b{B}-k{K0}" + ("" if Ka == K0 else f"as{Ka}+{K0 - Ka}") + "".join("-" + "x".join(map(str, w)) + (f"+{two}" if two else "") for w, _, two in towers)


def _random_acts(acts, t):
    return [ref.ACTS[(t + l + 1) % 3] for l in range(len(acts))]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_exact_bits_and_random_bounds(case):
    B, K0, Ka, spec = case
    rng = np.random.default_rng(zlib.crc32(_id(case).encode()))
    x = ref.split_input(ref.exact_input(rng, B, K0), Ka)
    towers = [ref.exact_tower(rng, K0, w, a, two) for w, a, two in spec]
    for tower in towers:
        ref.assert_exact_forward(x, tower)
    saved, last = _forward(x, towers, B, True), _forward(x, towers, B, False)
    for t, tower in enumerate(towers):
        want = ref.tower_forward(x, tower)
        for l in range(len(tower)):
            assert _bits(saved.layer_h(t, l), want[l][0].astype(f32)), (t, l)
            assert (last.layer_h(t, l) is None) == (l < len(tower) - 1)
        assert _bits(last.layer_h(t, len(tower) - 1), want[-1][0].astype(f32))
        if any(ly["act"] == "relu" and ly["w"].shape[0] >= 33 for ly in tower):
            h = np.concatenate([want[l][0].reshape(-1) for l, ly in enumerate(tower) if ly["act"] == "relu"])
            assert (h == 0).any() and (h > 0).any()                          # the clamp is exercised
    x = ref.split_input(ref.random_input(rng, B, K0), Ka)
    towers = [ref.random_tower(rng, K0, w, _random_acts(a, t), two) for t, (w, a, two) in enumerate(spec)]
    saved, last = _forward(x, towers, B, True), _forward(x, towers, B, False)
    for t, tower in enumerate(towers):
        want = ref.tower_forward(x, tower)
        hprev = ref.cat_input(x)
        for l, ly in enumerate(tower):
            got = saved.layer_h(t, l)
            h, bound = ref.layer_forward(hprev, ly)                           # from the device's own h_{l-1} bits
            _within(got, h, bound, f"tower {t} h_{l + 1} ({ly['act']})")
            hprev = got
        _within(got, want[-1][0], want[-1][1], f"tower {t} output, propagated")
        assert _bits(last.layer_h(t, len(tower) - 1), got)                    # the same bits whether or not the hidden layers are saved


def test_a_row_alone_equals_the_row_in_a_batch_of_65_and_towers_alone():
    rng = np.random.default_rng(7)
    K0 = 258
    xfull = ref.random_input(rng, 65, K0)
    for at in (0, 31, 64):
        xfull[at] = xfull[5]
    towers = [ref.random_tower(rng, K0, [256, 256, 2], ["tanh", "tanh", "none"]), ref.random_tower(rng, K0, [64, 33, 1], ["relu", "tanh", "none"], 2)]
    batch = _forward(ref.split_input(xfull, 256), towers, 65)
    alone = _forward(ref.split_input(xfull[5:6].copy(), 256), towers, 1)
    one_block = _forward(ref.split_input(xfull, K0), towers, 65)
    singles = [_forward(ref.split_input(xfull, 256), [tower], 65) for tower in towers]
    for t, tower in enumerate(towers):
        for l in range(len(tower)):
            h = batch.layer_h(t, l)
            for at in (0, 5, 31, 64):
                assert _bits(h[at], alone.layer_h(t, l)[0]), (t, l, at)
            assert _bits(h, singles[t].layer_h(0, l)) and _bits(h, one_block.layer_h(t, l))


@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_backward_exact_bits_random_bounds_and_repeat(case):
    B, K0, Ka, spec = case
    rng = np.random.default_rng(zlib.crc32(_id(case).encode()) + 1)
    xs, towers, hs, dys = None, [], [], []
    for w, a, two in spec:
        xfull, tower, h, dy = ref.exact_backward_case(rng, B, K0, w, a, two)
        xs = xfull if xs is None else xs
        ref.assert_exact_backward(ref.split_input(xs, Ka), tower, h, dy)
        towers.append(tower), hs.append(h), dys.append(dy)
    if B >= 33:
        relu = [h for t, (w, a, two) in enumerate(spec) for h, name in zip(hs[t], a) if name == "relu"]
        assert relu and all(0.3 < float((h == 0).mean()) < 0.7 for h in relu)  # about half of the ReLU units are off
    x = ref.split_input(xs, Ka)
    call, dx = _backward(x, towers, hs, dys, B)
    _check_backward(call, dx, x, towers, hs, dys, exact=True)
    xs, towers, hs, dys = None, [], [], []
    for t, (w, a, two) in enumerate(spec):
        xfull, tower, h, dy = ref.random_backward_case(rng, B, K0, w, _random_acts(a, t), two)
        xs = xfull if xs is None else xs
        towers.append(tower), hs.append(h), dys.append(dy)
    x = ref.split_input(xs, Ka)
    call, dx = _backward(x, towers, hs, dys, B, twice=True)
    _check_backward(call, dx, x, towers, hs, dys, exact=False)


def test_backward_options_dx_blocks_frozen_layers_null_dy_and_the_workspace():
    B, K0, Ka = 65, 258, 256
    rng = np.random.default_rng(21)
    spec = [([64, 2], ["relu", "none"], 2), ([33, 1], ["relu", "none"], 0)]
    xs, towers, hs, dys = None, [], [], []
    for w, a, two in spec:
        xfull, tower, h, dy = ref.exact_backward_case(rng, B, K0, w, a, two)
        xs = xfull if xs is None else xs
        towers.append(tower), hs.append(h), dys.append(dy)
    x = ref.split_input(xs, Ka)
    for want in ((False, True), (True, False), (False, False)):
        call, dx = _backward(x, towers, hs, dys, B, want_dx=want)
        _check_backward(call, dx, x, towers, hs, dys, exact=True, want_dx=want)
    # one tower alone (T = 1: dx without the towers' sum), only the actions' block
    call, dx = _backward(x, towers[:1], hs[:1], dys[:1], B, want_dx=(False, True))
    _check_backward(call, dx, x, towers[:1], hs[:1], dys[:1], exact=True, want_dx=(False, True))
    # a NULL dy contributes zeros for its tower
    call, dx = _backward(x, towers, hs, [dys[0], None], B)
    _check_backward(call, dx, x, towers, hs, [dys[0], None], exact=True)
    # a frozen layer's gradients are not written, the others are the same
    call, dx = _backward(x, towers, hs, dys, B, skip={(0, 0), (1, 1)})
    full, _ = _backward(x, towers, hs, dys, B)
    assert all(b is None for b in call.grad[0][0]) and _bits(call.layer_grads(0, 1)[0], full.layer_grads(0, 1)[0])
    assert _bits(call.layer_grads(1, 0)[0], full.layer_grads(1, 0)[0]) and _bits(call.layer_grads(1, 0)[1], full.layer_grads(1, 0)[1])
    # the workspace: exactly the queried size is accepted (every call above), one byte less is refused
    assert _backward(x, towers, hs, dys, B, shrink=1) != 0
    # one row tile holds the batch and one tower runs: no workspace at all
    capi, L = _lib()
    small = Call(ref.split_input(xs[:3], Ka), towers[:1], 3, hs=[[h[:3] for h in hs[0]]], dys=[dys[0][:3]], backward=True)
    assert L.tg_mlp_backward_workspace(3, small.Ka, small.Kb, small.arr, 1) == 0
    assert L.tg_mlp_backward_workspace(65, small.Ka, small.Kb, small.arr, 1) == 3 * 4 * ((64 * 259) + 4 * 65)


def test_forward_output_feeds_the_backward():
    """The kernel's own saved activations as the backward's h: the pair as the autograd function uses it."""
    rng = np.random.default_rng(11)
    B, K0 = 33, 31
    x = ref.split_input(ref.exact_input(rng, B, K0), K0)
    towers = [ref.exact_tower(rng, K0, [64, 33, 2], ["relu", "relu", "none"])]
    ref.assert_exact_forward(x, towers[0])
    fwd = _forward(x, towers, B)
    hs = [[fwd.layer_h(0, l) for l in range(3)]]
    dys = [rng.integers(-2, 3, (B, 2)).astype(f32)]
    ref.assert_exact_backward(x, towers[0], hs[0], dys[0])
    call, dx = _backward(x, towers, hs, dys, B)
    _check_backward(call, dx, x, towers, hs, dys, exact=True)


def test_error_returns_write_nothing_and_name_the_function():
    capi, L = _lib()
    rng = np.random.default_rng(5)
    B, K0 = 3, 4
    x = ref.split_input(ref.exact_input(rng, B, K0), 2)
    towers = [ref.exact_tower(rng, K0, [3, 2], ["relu", "none"], 2), ref.exact_tower(rng, K0, [1], ["none"])]   # two towers: a workspace is needed
    dys = [np.ones((B, 4), f32), np.ones((B, 1), f32)]

    def fresh():
        call = Call(x, towers, B, backward=True, dys=dys)
        gdx, gws = [Guarded(4 * B * 2), Guarded(4 * B * 2)], Guarded(1 << 16)
        return call, gdx, gws

    def run(kind, edit, **kw):
        call, gdx, gws = fresh()
        a = list(call.xargs())
        args = dict(x0=a[0], Ka=a[1], x1=a[2], Kb=a[3], B=a[4], arr=a[5], T=a[6], ws=C.c_void_p(gws.ptr), nbytes=1 << 16)
        if edit:
            edit(call.arr[0])
        args.update(kw)
        head = (args["x0"], args["Ka"], args["x1"], args["Kb"], args["B"], args["arr"], args["T"])
        if kind == "fwd":
            rc, who = L.tg_mlp_forward(*head, 1, _stream()), "tg_mlp_forward:"
        elif kind == "bwd":
            rc, who = L.tg_mlp_backward(*head, C.c_void_p(gdx[0].ptr), C.c_void_p(gdx[1].ptr), args["ws"], args["nbytes"], _stream()), "tg_mlp_backward:"
        else:
            rc, who = L.tg_mlp_backward_workspace(args["B"], args["Ka"], args["Kb"], args["arr"], args["T"]), "tg_mlp_backward_workspace:"
        torch.cuda.synchronize()
        return rc, who, call.outputs + gdx + [gws]

    def setf(t, l, name, v):
        def edit(tw):
            setattr(tw.layer[l], name, v)
        return edit

    def setn(v):
        def edit(tw):
            tw.n_layers = v
        return edit

    null = C.c_void_p(None)
    shape_errors = [dict(T=0), dict(T=5), dict(B=-1), dict(Ka=0), dict(Kb=-1), dict(Ka=1023), dict(arr=None)]
    shape_edits = [setn(0), setn(5), setf(0, 0, "out", 0), setf(0, 0, "out", 257), setf(0, 1, "out2", 255), setf(0, 0, "out2", 1),
                   setf(0, 0, "in_", 5), setf(0, 1, "in_", 4), setf(0, 0, "act", 3), setf(0, 1, "act", -1), setf(0, 1, "out2", -1)]
    pointer_edits = [setf(0, 0, "weight", None), setf(0, 1, "bias", None), setf(0, 1, "weight2", None), setf(0, 1, "bias2", None),
                     setf(0, 1, "h", None), setf(0, 1, "h2", None), setf(0, 0, "h", None)]
    for kind in ("fwd", "bwd", "ws"):
        trials = [(None, kw) for kw in shape_errors] + [(e, {}) for e in shape_edits]
        if kind != "ws":
            trials += [(e, {}) for e in pointer_edits] + [(None, dict(x0=null)), (None, dict(x1=null))]
        if kind == "bwd":
            trials += [(None, dict(ws=null)), (None, dict(nbytes=0)), (None, dict(nbytes=L.tg_mlp_backward_workspace(B, 2, 2, fresh()[0].arr, 2) - 1))]
            assert L.tg_mlp_backward_workspace(B, 2, 2, fresh()[0].arr, 2) == 4 * 2 * B * K0
        for k, (edit, kw) in enumerate(trials):
            rc, who, outs = run(kind, edit, **kw)
            assert rc < 0 and L.tg_last_error().decode().startswith(who), (kind, k, rc, L.tg_last_error())
            for g in outs:
                assert g.guards_intact() and bool((g.payload() == PATTERN).all()), (kind, k)
    rc, who, _ = run("fwd", setf(0, 0, "out", 257))
    assert "wider layers are not built" in L.tg_last_error().decode()
    # B = 0 does nothing
    for kind in ("fwd", "bwd"):
        rc, _, outs = run(kind, None, B=0)
        assert rc == 0
        for g in outs:
            assert g.guards_intact() and bool((g.payload() == PATTERN).all())
    assert run("ws", None, B=0)[0] == 0
