"""tg_conv_relu, tg_conv_relu_bwd_workspace and tg_conv_relu_bwd (csrc/tg_conv.hip) called directly on raw pointers, every buffer between guard
bytes inside a larger allocation: the cases of tests/conv_tail_ref.py (one position, tiles that span images, conv2 / conv3 / linear of the
36 x 36 and 128 x 128 observations, the real 9216-wide linear, a non-square stride-3 layer with three channel tiles, backward walks).

On the grid cases float32 arithmetic is exact in every order, so the float64 restatement IS the required bits; on random inputs the results lie
within the derived bounds (conv_tail_ref's docstring); the order probes pin the ascending chain itself.  A row's output must not depend on
the batch around it; two backward calls must give the same bytes; the error returns take no launch and write nothing."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_tail_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from conv_tail_device import _backward, _bits, _forward, _lib, _p, _stream, _untouched, check_case  # noqa: E402
from conv_tail_device import check_row_alone_equals_the_row_in_batches_of_65_and_33  # noqa: E402
from device_guard import Guarded  # noqa: E402

f32 = np.float32


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_grid_bits_random_bounds_repeat_and_null_dx(case):
    check_case(case)


def test_forward_output_feeds_the_backward():
    """The kernel's own forward output as the backward's y: the pair as the autograd function uses it."""
    case = (32, 31, 31, 64, 4, 4, 2, 3)
    rng = np.random.default_rng(11)
    x, w, b, _, dy = ref.grid_case(rng, case)
    y = _forward(x, w, b, 2)
    r = ref.backward(x, w, y, dy, 2)
    dw, db, dx = _backward(x, w, y, dy, 2)
    assert _bits(dw, r["dw"].astype(f32)) and _bits(db, r["db"].astype(f32)) and _bits(dx, r["dx"].astype(f32))


@pytest.mark.parametrize("which", range(3), ids=["k18", "k512", "k9216"])
def test_forward_order_probes_give_zero(which):
    shape, triples = ref.forward_probe_sets()[which]
    x, w, b, at = ref.forward_probe(shape, triples)
    y = _forward(x, w, b, shape[6])
    got = np.array([y[i, i % shape[3], oy, ox] for i, (oy, ox) in enumerate(at)])
    assert _bits(got, np.zeros(len(at), f32)), [t for t, v in zip(triples, got) if v != 0][:8]       # any other order gives 1


@pytest.mark.parametrize("which", range(3), ids=["stride1", "stride2", "one-by-one"])
def test_dx_order_probes_give_zero(which):
    shape, at = ref.dx_probe_sets()[which]
    x, w, y, dy, B = ref.dx_probe(shape, at)
    _, _, dx = _backward(x, w, y, dy, shape[6])
    got = np.array([dx[i, i % shape[0], at[0], at[1]] for i in range(B)])
    assert _bits(got, np.zeros(B, f32)), [i for i, v in enumerate(got) if v != 0][:8]


@pytest.mark.parametrize("shape", ref.REAL_128, ids=["conv2", "conv3", "linear"])
def test_a_row_alone_equals_the_row_in_batches_of_65_and_33(shape):
    check_row_alone_equals_the_row_in_batches_of_65_and_33(shape)


def test_a_workspace_one_byte_short_is_an_error():
    x, w, b, y, dy = ref.grid_case(np.random.default_rng(3), (32, 8, 8, 64, 4, 4, 2, 3))
    assert _backward(x, w, y, dy, 2, shrink=1) != 0


def test_relu_keeps_a_nan_and_gives_plus_zero_for_everything_not_positive():
    """K = 2, one position an image: z = x0 w0 + x1 w1 + b chosen per image.  A chain that starts at +0 never holds -0 (x - x = +0 in round to
    nearest, and -0 + +0 = +0), so z = -0 needs acc = -0 and cannot arise; a -0 product and a -0 bias still end as +0 bits."""
    z_in = [(1.0, 1.0, 0.5), (1.0, -1.0, 0.5), (1.0, -1.0, -0.0), (0.0, -1.0, -0.0), (np.nan, 1.0, 0.0), (np.inf, 1.0, 0.0), (np.inf, -1.0, 0.0),
            (np.inf, 0.0, 0.0), (1e-30, -1e-30, 0.0)]
    B = len(z_in)
    x = np.zeros((B, 2, 1, 1), f32)
    w = np.zeros((32, 2, 1, 1), f32)
    b = np.zeros((32,), f32)
    w[:, 0, 0, 0] = 1.0
    y_all = []
    for i, (x0, w0, bias) in enumerate(z_in):                                  # one launch per bias value: the bias is per channel
        x[:] = 0
        x[i, 0, 0, 0] = x0
        w[:, 0, 0, 0] = w0
        b[:] = bias
        y_all.append(_forward(x, w, b, 1)[i, :, 0, 0])
    y = np.stack(y_all)
    pz = np.zeros(32, f32)
    assert _bits(y[0], np.full(32, 1.5, f32)) and _bits(y[1], pz) and _bits(y[2], pz) and _bits(y[3], pz)
    assert np.isnan(y[4]).all() and _bits(y[5], np.full(32, np.inf, f32)) and _bits(y[6], pz) and np.isnan(y[7]).all() and _bits(y[8], pz)
    # the backward's mask: only y > 0 passes dy on; a NaN or a -0 in y does not
    yv = np.array([1.0, 0.0, -0.0, np.nan, -1.0, np.inf, 1e-40, 2.0, 0.5], f32)
    yb = np.repeat(yv[:, None], 32, 1).reshape(B, 32, 1, 1).copy()
    x = np.ones((B, 2, 1, 1), f32)
    w = np.ones((32, 2, 1, 1), f32)
    dy = np.full((B, 32, 1, 1), 3.0, f32)
    dw, db, dx = _backward(x, w, yb, dy, 1)
    passed = 5                                                              # 1, inf, the subnormal, 2, 0.5
    assert _bits(db, np.full(32, 3.0 * passed, f32)) and _bits(dw, np.full((32, 2, 1, 1), 3.0 * passed, f32))
    assert _bits(dx[:, 0, 0, 0], np.where(yv > 0, 96.0, 0.0).astype(f32))


def test_error_returns_write_nothing_and_name_the_function():
    capi, L = _lib()
    x = np.zeros((1, 32, 8, 8), f32)
    gx, gw, gb, gy = Guarded(x.nbytes, fill=x), Guarded(4 * 64 * 512), Guarded(4 * 64), Guarded(4 * 64 * 9)
    gdw, gdb, gdx, gws = Guarded(4 * 64 * 512), Guarded(4 * 64), Guarded(x.nbytes), Guarded(1 << 18)
    outs = (gy, gdw, gdb, gdx, gws)
    ok = dict(B=1, Cin=32, H=8, W=8, Cout=64, KH=4, KW=4, stride=2)

    def fwd(xp=gx, wp=gw, bp=gb, yp=gy, **kw):
        a = dict(ok, **kw)
        return (L.tg_conv_relu(_p(xp), a["B"], a["Cin"], a["H"], a["W"], _p(wp), _p(bp), a["Cout"], a["KH"], a["KW"], a["stride"], _p(yp), _stream()),
                "tg_conv_relu:")

    def bwd(xp=gx, wp=gw, yp=gy, dyp=gy, dwp=gdw, dbp=gdb, dxp=gdx, wsp=gws, nbytes=1 << 18, **kw):
        a = dict(ok, **kw)
        return (L.tg_conv_relu_bwd(_p(xp), a["B"], a["Cin"], a["H"], a["W"], _p(wp), _p(yp), _p(dyp), a["Cout"], a["KH"], a["KW"], a["stride"],
                                   _p(dwp), _p(dbp), _p(dxp), _p(wsp), nbytes, _stream()), "tg_conv_relu_bwd:")

    limits = [(dict(Cin=0), "Cin"), (dict(Cin=65), "Cin"), (dict(Cout=48), "Cout"), (dict(Cout=0), "Cout"), (dict(Cout=544), "Cout"),
              (dict(KH=0), "KH"), (dict(KW=0), "KW"), (dict(KH=9), "KH <= H"), (dict(KW=9), "KW <= W"), (dict(KH=17, H=20), "KH"),
              (dict(stride=0), "stride"), (dict(stride=5), "stride"), (dict(Cin=1, KH=3, KW=3), "even"), (dict(B=-1), "B >= 0"),
              (dict(B=2 ** 29 // 64), "positions")]
    calls = [(lambda: fwd(xp=None), "NULL"), (lambda: fwd(wp=None), "NULL"), (lambda: fwd(bp=None), "NULL"), (lambda: fwd(yp=None), "NULL"),
             (lambda: bwd(xp=None), "NULL"), (lambda: bwd(wp=None), "NULL"), (lambda: bwd(yp=None), "NULL"), (lambda: bwd(dyp=None), "NULL"),
             (lambda: bwd(dwp=None), "NULL"), (lambda: bwd(dbp=None), "NULL"), (lambda: bwd(wsp=None), "NULL"), (lambda: bwd(nbytes=0), "workspace")]
    for change, word in limits:
        calls.append((lambda change=change: fwd(**change), word))
        calls.append((lambda change=change: bwd(**change), word))
    for k, (call, word) in enumerate(calls):
        rc, who = call()
        torch.cuda.synchronize()
        text = L.tg_last_error().decode()
        assert rc != 0 and text.startswith(who) and word in text, (k, rc, text)
        for g in outs:
            assert _untouched(g), k
    for change, word in limits:
        a = dict(ok, **change)
        assert L.tg_conv_relu_bwd_workspace(*a.values()) < 0
        text = L.tg_last_error().decode()
        assert text.startswith("tg_conv_relu_bwd_workspace:") and word in text
    # B = 0 does nothing
    capi.check(fwd(B=0)[0])
    capi.check(bwd(B=0)[0])
    assert L.tg_conv_relu_bwd_workspace(*dict(ok, B=0).values()) >= 0
    torch.cuda.synchronize()
    for g in outs:
        assert _untouched(g)
