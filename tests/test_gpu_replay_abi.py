"""tg_replay_add and tg_replay_draw (csrc/tg_replay.hip) called directly on raw pointers: the address-driven choices of the copy unit that the
Python buffer never makes (its tensors are all torch-aligned), the tails of the four-units-per-lane loop, every select pattern, full and sparse
array tables, the draw on both sides of its workgroup boundary and past 2^31 rows, and the error returns that take no launch.  Every
destination sits between guard bytes inside a larger buffer; misaligned means an offset INSIDE that buffer.

The copies are compared with numpy selections of the same bytes, the draw with tests/replay_ref.py bit for bit."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from replay_ref import draw_rows  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import PATTERN, Guarded  # noqa: E402

OFFSETS = (0, 4, 1)                     # address classes mod 16: vector aligned, float aligned, byte aligned
ROW_BYTES = (16, 48, 4, 12, 1, 3)       # one and three units of every class (at aligned addresses)
N_ROWS = (1, 255, 256, 257, 1023, 1024, 1025, 4097)     # x 1 or 3 units per row: around the 1024-unit workgroup and its 256-lane passes
SELECTS = ("none", "all", "alternating", "first", "last")


def _capi():
    from tactile_gym_amd import _capi
    return _capi


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptrs(items):
    return (C.c_void_p * max(len(items), 1))(*[(x.ptr if x is not None else None) for x in items])


def _bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


def _select(pattern, n):
    s = np.zeros(n, np.uint8)
    if pattern == "all":
        s[:] = 1
    elif pattern == "alternating":
        s[::2] = 7                      # any non-zero byte selects
    elif pattern == "first":
        s[0] = 1
    elif pattern == "last":
        s[-1] = 255
    return s


def _add(srcs, alts, dsts, row_bytes, kinds, n_rows, select):
    n = len(srcs)
    rc = _capi().lib().tg_replay_add(n, _ptrs(srcs), _ptrs(alts), _ptrs(dsts), (C.c_int64 * max(n, 1))(*row_bytes), (C.c_int32 * max(n, 1))(*kinds),
                                     n_rows, select.ptr if select is not None else None, _stream())
    torch.cuda.synchronize()
    return rc


def _untouched(g):
    return g.guards_intact() and bool((g.payload() == PATTERN).all())


def _expected(src, alt, sel, flag):
    out = np.where(sel[:, None] != 0, alt, src) if alt is not None else src
    return (out != 0).astype(np.float32).view(np.uint8).reshape(len(out), -1) if flag else out


def _unit(rb, *addrs):
    m = rb
    for a in addrs:
        m |= a
    return 16 if m % 16 == 0 else 4 if m % 4 == 0 else 1


def test_add_matrix_reaches_every_unit_and_tail():
    seen = {(_unit(rb, s, a, d), (n * (rb // _unit(rb, s, a, d))) % 1024) for s in OFFSETS for a in OFFSETS for d in OFFSETS for rb in ROW_BYTES
            for n in N_ROWS}
    for u in (16, 4, 1):
        assert {(u, r) for r in (1, 255, 256, 257, 1023, 0, 1)} <= seen
    assert {_unit(rb, 0, 0, 0) for rb in ROW_BYTES} == {16, 4, 1} and {rb // _unit(rb, 0, 0, 0) for rb in ROW_BYTES} == {1, 3}


@pytest.mark.parametrize("src_off,alt_off,dst_off", list(itertools.product(OFFSETS, OFFSETS, OFFSETS)))
def test_add_alignment_classes(src_off, alt_off, dst_off):
    """Per call: a copy array of every row size with an alternative source, one without (NULL alt beside the select), and a flag array."""
    seed = 100 * src_off + 10 * alt_off + dst_off
    for n_rows in N_ROWS:
        data = [(_bytes(seed + i, n_rows * rb).reshape(n_rows, rb), _bytes(seed + 50 + i, n_rows * rb).reshape(n_rows, rb)) for i, rb in enumerate(ROW_BYTES)]
        plain = _bytes(seed + 90, n_rows * 20).reshape(n_rows, 20)
        fsrc, falt = (np.random.default_rng(seed + k).choice(np.array([0, 1, 2, 255], np.uint8), size=(n_rows, 1)) for k in (91, 92))
        srcs = [Guarded(s.size, src_off, fill=s) for s, _ in data] + [Guarded(plain.size, src_off, fill=plain), Guarded(n_rows, src_off, fill=fsrc)]
        alts = [Guarded(a.size, alt_off, fill=a) for _, a in data] + [None, Guarded(n_rows, alt_off, fill=falt)]
        row_bytes, kinds = list(ROW_BYTES) + [20, 1], [0] * (len(ROW_BYTES) + 1) + [1]
        for pattern in SELECTS:
            sel = _select(pattern, n_rows)
            dsts = [Guarded(s.size, dst_off) for s, _ in data] + [Guarded(plain.size, dst_off), Guarded(4 * n_rows, 0 if dst_off == 1 else dst_off)]
            assert _add(srcs, alts, dsts, row_bytes, kinds, n_rows, Guarded(n_rows, 1, fill=sel)) == 0
            want = [_expected(s, a, sel, False) for s, a in data] + [plain, _expected(fsrc, falt, sel, True)]
            for i, (d, w) in enumerate(zip(dsts, want)):
                assert np.array_equal(d.host(np.uint8).reshape(n_rows, -1), w), (n_rows, pattern, i)
                assert d.guards_intact(), (n_rows, pattern, i)
        for g, (s, a) in zip(srcs, data):                                     # the sources are only read
            assert g.guards_intact() and np.array_equal(g.host(np.uint8).reshape(n_rows, -1), s)
        for g, (s, a) in zip(alts, data):
            assert g.guards_intact() and np.array_equal(g.host(np.uint8).reshape(n_rows, -1), a)


def test_add_without_alternatives_needs_no_select():
    n_rows = 1500
    data = [_bytes(i, n_rows * rb).reshape(n_rows, rb) for i, rb in enumerate(ROW_BYTES)]
    flags = np.random.default_rng(9).choice(np.array([0, 1, 2, 255], np.uint8), size=n_rows)
    srcs = [Guarded(d.size, 0, fill=d) for d in data] + [Guarded(n_rows, 1, fill=flags)]
    dsts = [Guarded(d.size, 0) for d in data] + [Guarded(4 * n_rows, 4)]
    assert _add(srcs, [None] * 7, dsts, list(ROW_BYTES) + [1], [0] * 6 + [1], n_rows, None) == 0
    for d, w in zip(dsts, data):
        assert np.array_equal(d.host(np.uint8).reshape(n_rows, -1), w) and d.guards_intact()
    assert np.array_equal(dsts[-1].host(np.float32), (flags != 0).astype(np.float32)) and dsts[-1].guards_intact()


def test_add_sixteen_arrays_with_empty_ones_between():
    capi = _capi()
    assert capi.ROLLOUT_MAX_ARRAYS == 16
    n_rows = 700
    sel = _select("alternating", n_rows)
    #        src off, alt off (None: NULL), dst off, row bytes, kind
    spec = [(0, 0, 0, 0, 0), (0, 0, 0, 64, 0), (4, None, 0, 8, 0), (0, 0, 0, 0, 1), (1, 1, 0, 5, 0), (0, 4, 4, 16, 0), (1, 1, 0, 1, 1), (0, 0, 0, 1, 0),
            (4, 4, 4, 24, 0), (0, None, 0, 0, 0), (0, 0, 1, 32, 0), (0, 0, 0, 2048, 0), (1, None, 4, 1, 1), (0, 0, 0, 40, 0), (4, 0, 0, 4, 0),
            (0, 0, 0, 0, 0)]
    assert len(spec) == 16
    srcs, alts, dsts, want = [], [], [], []
    for i, (so, ao, do, rb, kind) in enumerate(spec):
        if rb == 0:
            srcs.append(None); alts.append(None); dsts.append(None); want.append(None)
            continue
        s, a = _bytes(i, n_rows * rb).reshape(n_rows, rb), (_bytes(50 + i, n_rows * rb).reshape(n_rows, rb) if ao is not None else None)
        if kind:                                              # flags: zeros in a third of the rows
            s, a = s % np.uint8(3), (a % np.uint8(3) if a is not None else None)
        srcs.append(Guarded(s.size, so, fill=s))
        alts.append(Guarded(a.size, ao, fill=a) if a is not None else None)
        dsts.append(Guarded(s.size * (4 if kind else 1), do))
        want.append(_expected(s, a, sel, bool(kind)))
    assert _add(srcs, alts, dsts, [s[3] for s in spec], [s[4] for s in spec], n_rows, Guarded(n_rows, 0, fill=sel)) == 0
    for i, w in enumerate(want):
        if w is not None:
            assert np.array_equal(dsts[i].host(np.uint8).reshape(n_rows, -1), w) and dsts[i].guards_intact(), i


def test_add_error_returns_write_nothing():
    L = _capi().lib()
    n_rows, rb = 256, 16
    d = _bytes(0, n_rows * rb)
    src, alt, dst = Guarded(d.size, 0, fill=d), Guarded(d.size, 0, fill=d[::-1].copy()), Guarded(d.size, 0)
    flag_dst = Guarded(4 * n_rows, 1)
    both = Guarded(2 * d.size, 0, fill=np.concatenate([d, d]))
    sel = Guarded(n_rows, 0, fill=_select("all", n_rows))

    class At:                                                     # an address inside a guarded buffer
        def __init__(self, ptr):
            self.ptr = ptr
    assert _add([], [], [], [], [], n_rows, None) == 0                                            # no arrays: nothing to do
    assert L.tg_replay_add(0, None, None, None, None, None, n_rows, None, _stream()) == 0
    assert _add([src], [alt], [dst], [rb], [0], 0, sel) == 0                                      # no rows, no bytes: success, nothing written
    assert _add([src], [alt], [dst], [0], [0], n_rows, sel) == 0
    assert _add([src], [None], [dst], [rb], [2], n_rows, None) == -1                              # unknown kind
    assert _add([src], [None], [dst], [-1], [0], n_rows, None) == -1                              # negative counts
    assert _add([src], [None], [dst], [rb], [0], -1, None) == -1
    assert _add([None], [None], [dst], [rb], [0], n_rows, None) == -1 and _add([src], [None], [None], [rb], [0], n_rows, None) == -1
    assert _add([src], [alt], [dst], [rb], [0], n_rows, None) == -1                               # an alternative source without a select
    assert _add([src], [None], [flag_dst], [1], [1], n_rows, None) == -1                          # a flag destination that is no float32 address
    assert _add([src], [None], [dst], [4], [1], n_rows, None) == -1                               # flags are one byte per row
    assert _add([both], [None], [At(both.ptr + d.size)], [rb], [0], n_rows + 1, None) == -1       # the destination starts inside the source
    assert _add([src], [both], [At(both.ptr + d.size - 16)], [rb], [0], n_rows, sel) == -1        # ... inside the alternative source
    assert _add([At(both.ptr + 512)], [None], [both], [1], [1], n_rows, None) == -1               # flags: 4 bytes out per byte in reach the source
    assert _add([src, src], [None, None], [dst, dst], [rb, rb], [0, 7], n_rows, None) == -1       # a bad second array: the first is not copied
    assert L.tg_replay_add(17, None, None, None, None, None, n_rows, None, _stream()) == -1
    assert L.tg_replay_add(-1, None, None, None, None, None, n_rows, None, _stream()) == -1
    assert L.tg_replay_add(1, None, None, None, None, None, n_rows, None, _stream()) == -1        # NULL tables
    assert b"tg_replay_add" in L.tg_last_error()
    torch.cuda.synchronize()
    assert _untouched(dst) and _untouched(flag_dst)
    assert both.guards_intact() and np.array_equal(both.host(np.uint8), np.concatenate([d, d]))
    assert _add([src], [alt], [dst], [rb], [0], n_rows, sel) == 0                                 # and the call itself works
    assert np.array_equal(dst.host(np.uint8), d[::-1]) and dst.guards_intact()


# ---------------------------------------------------------------------------------------------------------------- draw
def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


T_DRAW = 5


@pytest.mark.parametrize("A", [1, 6])
@pytest.mark.parametrize("N", [1, 3, 1024])
def test_draw_bit_exact(N, A):
    L = _capi().lib()
    T = T_DRAW
    rng = np.random.default_rng(10 * N + A)
    actions = rng.standard_normal((T * N, A)).astype(np.float32)
    rewards = rng.standard_normal(T * N).astype(np.float32)
    dones = rng.choice(np.array([0.0, 1.0, 0.75], np.float32), size=T * N)          # flags, and a value whose product rounds
    timeouts = rng.choice(np.array([0.0, 1.0, 0.3], np.float32), size=T * N)
    dev = [Guarded(a.nbytes, 0, fill=a) for a in (actions, rewards, dones, timeouts)]
    next_offset = T * N
    for k, (B, M, first) in enumerate(itertools.product((1, 63, 64, 65, 1000), (1, 2, T - 1, T), (0, T - 1))):
        seed, counter = 7 + k, k % 3
        rows_out, a_out, r_out, d_out = Guarded(16 * B, 0), Guarded(4 * B * A, 0), Guarded(4 * B, 0), Guarded(4 * B, 0)
        rc = L.tg_replay_draw(B, M, first, T, N, seed, counter, dev[0].ptr, A, dev[1].ptr, dev[2].ptr, dev[3].ptr, next_offset, rows_out.ptr,
                              a_out.ptr, r_out.ptr, d_out.ptr, _stream())
        torch.cuda.synchronize()
        assert rc == 0, L.tg_last_error().decode()
        rows = draw_rows(seed, counter, B, M, first, T, N)
        got = rows_out.host(np.int64)
        assert np.array_equal(got[:B], rows) and np.array_equal(got[B:], rows + next_offset), (B, M, first)
        assert np.isin((rows // N - first) % T, np.arange(M)).all()
        assert _bits_equal(a_out.host(np.float32).reshape(B, A), actions[rows]) and _bits_equal(r_out.host(np.float32), rewards[rows])
        assert _bits_equal(d_out.host(np.float32), dones[rows] * (np.float32(1) - timeouts[rows])), (B, M, first)
        for g in (rows_out, a_out, r_out, d_out):
            assert g.guards_intact()
    for g, a in zip(dev, (actions, rewards, dones, timeouts)):
        assert g.guards_intact() and np.array_equal(g.host(np.float32), a.reshape(-1))


def test_draw_rows_only_past_two_to_the_31_rows():
    """T N = 2^32 cells without their memory: the four inputs NULL together, only the rows are written."""
    L = _capi().lib()
    T, N, B = 1 << 20, 1 << 12, 1000
    for M, first, seed in ((T, 0, 1), (T - 1, T - 1, 2), (T, T - 1, 3)):
        rows_out = Guarded(16 * B, 0)
        rc = L.tg_replay_draw(B, M, first, T, N, seed, 5, None, 0, None, None, None, T * N, rows_out.ptr, None, None, None, _stream())
        torch.cuda.synchronize()
        assert rc == 0, L.tg_last_error().decode()
        rows = draw_rows(seed, 5, B, M, first, T, N)
        got = rows_out.host(np.int64)
        assert np.array_equal(got[:B], rows) and np.array_equal(got[B:], rows + T * N) and rows_out.guards_intact()
        assert rows.max() >= 1 << 31 and got[B:].min() >= 1 << 32


def test_draw_error_returns_write_nothing():
    L = _capi().lib()
    T, N, A, B = 5, 3, 2, 64
    z = np.zeros(T * N * A, np.float32)
    src = Guarded(z.nbytes, 0, fill=z)
    rows_out, a_out, r_out, d_out = Guarded(16 * B, 0), Guarded(4 * B * A, 0), Guarded(4 * B, 0), Guarded(4 * B, 0)

    def call(B=B, M=T, first=0, T=T, N=N, inputs=(src.ptr,) * 4, A=A, off=T * N, rows=rows_out.ptr, outs=(a_out.ptr, r_out.ptr, d_out.ptr)):
        return L.tg_replay_draw(B, M, first, T, N, 1, 0, inputs[0], A, inputs[1], inputs[2], inputs[3], off, rows, outs[0], outs[1], outs[2], _stream())
    assert call(B=-1) == -1 and call(T=0) == -1 and call(N=0) == -1 and call(N=1 << 31) == -1 and call(T=1 << 30, N=1 << 30, M=1) == -1
    assert call(M=0) == -1 and call(M=T + 1) == -1 and call(first=-1) == -1 and call(first=T) == -1 and call(off=-1) == -1
    for i in range(4):
        assert call(inputs=tuple(None if j == i else src.ptr for j in range(4))) == -1          # NULL together or not at all
    assert call(A=0) == -1 and call(rows=None) == -1
    for i in range(3):
        assert call(outs=tuple(None if j == i else (a_out.ptr, r_out.ptr, d_out.ptr)[j] for j in range(3))) == -1
    assert b"tg_replay_draw" in L.tg_last_error()
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert all(_untouched(g) for g in (rows_out, a_out, r_out, d_out))
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(rows_out.host(np.int64)[:B], draw_rows(1, 0, B, T, 0, T, N))
