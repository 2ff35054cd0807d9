"""What tests/test_gpu_conv_tail_abi.py and tests/test_gpu_conv_tail_paths.py share: tg_conv_relu and tg_conv_relu_bwd (csrc/tg_conv.hip) called
on raw pointers with every buffer between guard bytes, and the per-case body that holds them to the grid bits and the derived bounds of
tests/conv_tail_ref.py.  Import it from a test that needs a GPU only."""
import ctypes as C

import numpy as np
import torch

import conv_tail_ref as ref
from device_guard import PATTERN, Guarded

f32 = np.float32


def _lib():
    from tactile_gym_amd import _capi
    _capi.SYMBOLS["tg_conv_relu"]
    return _capi, _capi.lib()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _p(g):
    return C.c_void_p(g.ptr if g is not None else None)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _untouched(g):
    return g.guards_intact() and bool((g.payload() == PATTERN).all())


def _forward(x, w, b, stride, x_offset=0, w_offset=0):
    """One tg_conv_relu call between guards -> host float32 [B, Cout, OH, OW]; the inputs must come back unchanged.  x and w stand x_offset and
    w_offset bytes past a 16-byte aligned address."""
    capi, L = _lib()
    B, Cin, H, W = x.shape
    Cout, _, KH, KW = w.shape
    OH, OW = ref.out_hw(H, W, KH, KW, stride)
    gx, gw, gb = Guarded(x.nbytes, offset=x_offset, fill=x), Guarded(w.nbytes, offset=w_offset, fill=w), Guarded(b.nbytes, fill=b)
    assert gx.ptr % 16 == x_offset % 16 and gw.ptr % 16 == w_offset % 16
    gy = Guarded(4 * B * Cout * OH * OW)
    capi.check(L.tg_conv_relu(_p(gx), B, Cin, H, W, _p(gw), _p(gb), Cout, KH, KW, stride, _p(gy), _stream()))
    torch.cuda.synchronize()
    for g in (gx, gw, gb, gy):
        assert g.guards_intact()
    assert _bits(gx.host(f32).reshape(x.shape), x) and _bits(gw.host(f32).reshape(w.shape), w) and _bits(gb.host(f32), b)
    return gy.host(f32).reshape(B, Cout, OH, OW)


def _backward(x, w, y, dy, stride, with_dx=True, shrink=0, twice=False):
    """One tg_conv_relu_bwd call (two with twice=True, into fresh outputs) with a workspace of exactly the queried size less `shrink` bytes
    -> (dweight, dbias, dx or None) host float32, or the return code when shrink > 0.  Without dx a canary stands where dx would be."""
    capi, L = _lib()
    B, Cin, H, W = x.shape
    Cout, _, KH, KW = w.shape
    nbytes = L.tg_conv_relu_bwd_workspace(B, Cin, H, W, Cout, KH, KW, stride)
    assert nbytes > 0
    gx, gw, gy, gdy = Guarded(x.nbytes, fill=x), Guarded(w.nbytes, fill=w), Guarded(y.nbytes, fill=y), Guarded(dy.nbytes, fill=dy)
    gws = Guarded(nbytes - shrink)
    results = []
    for _ in range(2 if twice else 1):
        gdw, gdb, gdx = Guarded(w.nbytes), Guarded(4 * Cout), Guarded(x.nbytes)
        rc = L.tg_conv_relu_bwd(_p(gx), B, Cin, H, W, _p(gw), _p(gy), _p(gdy), Cout, KH, KW, stride, _p(gdw), _p(gdb), _p(gdx if with_dx else None),
                                _p(gws), nbytes - shrink, _stream())
        torch.cuda.synchronize()
        for g in (gx, gw, gy, gdy, gws, gdw, gdb, gdx):
            assert g.guards_intact()
        if shrink:
            assert rc != 0 and L.tg_last_error().decode().startswith("tg_conv_relu_bwd:")
            assert _untouched(gdw) and _untouched(gdb) and _untouched(gws) and _untouched(gdx)
            return rc
        capi.check(rc)
        for g, a in ((gx, x), (gw, w), (gy, y), (gdy, dy)):
            assert _bits(g.host(f32).reshape(a.shape), a)
        if not with_dx:
            assert _untouched(gdx)                                            # dx_dev = NULL: nothing is written where dx would have gone
        results.append((gdw.host(f32).reshape(w.shape).copy(), gdb.host(f32).copy(), gdx.host(f32).reshape(x.shape).copy() if with_dx else None))
    if twice:
        assert all(_bits(a, b) for a, b in zip(results[0][:2 + with_dx], results[1]))
    return results[0]


def _within(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: largest error / bound = {ratio:.3g}")
    assert (err <= bound).all(), (what, ratio)


def check_case(case):
    """Grid bits for y, dweight, dbias and dx; dx = 0 where no output reads; dx_dev = NULL gives the same dweight and dbias; random inputs within
    the derived bounds, the second backward call byte-equal; guards intact and inputs unchanged (in _forward and _backward)."""
    stride = case[6]
    rng = np.random.default_rng(hash(case) % 2**32)
    x, w, b, y, dy = ref.grid_case(rng, case)
    want, _ = ref.forward(x, w, b, stride)
    if want.size >= 64:
        assert (want > 0).any() and (want == 0).any()                      # the clamp is exercised
    assert _bits(_forward(x, w, b, stride), want.astype(f32))
    assert (y == 0).any() and (dy[y == 0] != 0).any()                      # the mask matters
    r = ref.backward(x, w, y, dy, stride)
    dw, db, dx = _backward(x, w, y, dy, stride)
    assert _bits(db, r["db"].astype(f32))
    assert _bits(dw, r["dw"].astype(f32))
    assert _bits(dx, r["dx"].astype(f32))
    assert (dx[:, :, ref.unread(case)] == 0).all()                         # input rows and columns that no output reads
    dw0, db0, _ = _backward(x, w, y, dy, stride, with_dx=False)
    assert _bits(dw0, dw) and _bits(db0, db)
    x, w, b, y, dy = ref.random_case(rng, case)
    want, bound = ref.forward(x, w, b, stride)
    _within(_forward(x, w, b, stride), want, bound, "y")
    r = ref.backward(x, w, y, dy, stride)
    dw, db, dx = _backward(x, w, y, dy, stride, twice=True)
    _within(db, r["db"], r["db_bound"], "dbias")
    _within(dw, r["dw"], r["dw_bound"], "dweight")
    _within(dx, r["dx"], r["dx_bound"], "dx")


def check_row_alone_equals_the_row_in_batches_of_65_and_33(shape):
    """A row's output must not depend on the batch around it, on its index or on where its tile falls."""
    stride = shape[6]
    rng = np.random.default_rng(7)
    x, w, b, _, _ = ref.random_case(rng, shape + (65,))
    row = x[5].copy()
    for at in (0, 31, 64):
        x[at] = row
    batch = _forward(x, w, b, stride)
    alone = _forward(row[None].copy(), w, b, stride)
    for at in (0, 5, 31, 64):
        assert _bits(batch[at], alone[0]), at
    x33 = np.ascontiguousarray(x[:33])
    x33[17] = row
    assert _bits(_forward(x33, w, b, stride)[17], alone[0])
