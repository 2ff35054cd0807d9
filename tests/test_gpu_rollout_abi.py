"""tg_rollout_add, tg_rollout_gather and tg_rollout_gae (csrc/tg_rollout.hip) called directly on raw pointers: the address-driven choices of the
copy unit that the Python buffer never makes (its tensors are all torch-aligned), the tails of the four-units-per-lane loop, full and sparse
array tables, the GAE kernel on both sides of its block and workgroup boundaries, and the error returns that take no launch.  Every destination
sits between guard bytes inside a larger buffer; misaligned means an offset INSIDE that buffer.

The copy kernels are compared with numpy slices of the same bytes.  The unit a call must pick is restated from the rule in the kernel file's
header - the widest of 16, 4 or 1 bytes that divides the byte count (per row for the gather) and both addresses - only to show that the matrix
reaches every unit with every tail; the kernels' outputs alone are compared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from rollout_ref import GAE_N, GAE_PARAMS, GAE_STARTS, GAE_T, gae_bound, gae_edge_inputs, gae_error, gae_f32, gae_f64  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import PATTERN, Guarded  # noqa: E402
from rollout_device import _bits_equal, _gae  # noqa: E402

OFFSETS = (0, 4, 1)                     # address classes mod 16: vector aligned, float aligned, byte aligned
PER_BLOCK = 1024                        # units per workgroup


def _capi():
    from tactile_gym_amd import _capi
    return _capi


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _unit(src, dst, nbytes):
    m = src | dst | nbytes
    return 16 if m % 16 == 0 else 4 if m % 4 == 0 else 1


def _tail(units):
    return "below" if units < PER_BLOCK else "exact" if units == PER_BLOCK else {1: "plus1", PER_BLOCK - 1: "plus1023"}.get(units % PER_BLOCK)


def _bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _add(srcs, dsts, nbytes, kinds):
    L = _capi().lib()
    n = len(srcs)
    rc = L.tg_rollout_add(n, _ptr_array([s.ptr if s else None for s in srcs]), _ptr_array([d.ptr if d else None for d in dsts]),
                          (C.c_int64 * n)(*nbytes), (C.c_int32 * n)(*kinds), _stream())
    torch.cuda.synchronize()
    return rc


def _gather(srcs, dsts, row_bytes, rows_dev, B):
    L = _capi().lib()
    n = len(srcs)
    rc = L.tg_rollout_gather(n, _ptr_array([s.ptr if s else None for s in srcs]), _ptr_array([d.ptr if d else None for d in dsts]),
                             (C.c_int64 * n)(*row_bytes), rows_dev.data_ptr() if rows_dev is not None else None, B, _stream())
    torch.cuda.synchronize()
    return rc


def _untouched(g):
    return g.guards_intact() and bool((g.payload() == PATTERN).all())


# ---------------------------------------------------------------------------------------------------------------- add
ADD_BYTES = tuple(n * u for u in (16, 4, 1) for n in (700, 1024, 2 * 1024 + 1, 2 * 1024 + 1023))


def test_add_matrix_reaches_every_unit_with_every_tail():
    seen = {(_unit(so, do, nb), _tail(nb // _unit(so, do, nb))) for so in OFFSETS for do in OFFSETS for nb in ADD_BYTES}
    assert {(u, t) for u in (16, 4, 1) for t in ("below", "exact", "plus1", "plus1023")} <= seen
    assert {(so, do, nb % 16 == 0, nb % 4 == 0) for so in OFFSETS for do in OFFSETS for nb in ADD_BYTES} >= \
        {(so, do, a16, a4) for so in OFFSETS for do in OFFSETS for a16, a4 in ((True, True), (False, True), (False, False))}


@pytest.mark.parametrize("dst_off", OFFSETS)
@pytest.mark.parametrize("src_off", OFFSETS)
def test_add_alignment_classes(src_off, dst_off):
    """Twelve arrays in one call, every one at the same pair of address classes: byte counts of every class and tail."""
    data = [_bytes(100 * src_off + 10 * dst_off + i, nb) for i, nb in enumerate(ADD_BYTES)]
    srcs = [Guarded(len(d), src_off, fill=d) for d in data]
    dsts = [Guarded(len(d), dst_off) for d in data]
    for s, d in zip(srcs, dsts):
        assert s.ptr % 16 == src_off and d.ptr % 16 == dst_off
    assert _add(srcs, dsts, [len(d) for d in data], [0] * len(data)) == 0
    for i, (s, d) in enumerate(zip(srcs, dsts)):
        assert np.array_equal(d.host(np.uint8), data[i]), (i, len(data[i]))
        assert d.guards_intact() and s.guards_intact() and np.array_equal(s.host(np.uint8), data[i]), i


def _flag_bytes(n, seed):
    return np.random.default_rng(seed).choice(np.array([0, 1, 2, 255], np.uint8), size=n)


def test_add_sixteen_arrays_of_mixed_units_lengths_and_kinds():
    capi = _capi()
    assert capi.ROLLOUT_MAX_ARRAYS == 16
    spec = [(0, 0, 16 * 3000, 0), (4, 0, 4 * 1500, 0), ("flag", 0, 2500, 1), (1, 0, 777, 0), (0, 4, 4096, 0), (0, 0, 16, 0), ("flag", 4, 1025, 1),
            (0, 1, 5000, 0), (4, 4, 4 * 1024, 0), (0, 0, 20, 0), (1, 1, 1, 0), ("flag", 0, 1, 1), (0, 0, 16 * 1024, 0), (4, 4, 8196, 0),
            (0, 0, 3, 0), ("flag", 0, 4 * 1024 + 7, 1)]
    assert len(spec) == 16
    srcs, dsts, data = [], [], []
    for i, (so, do, nb, kind) in enumerate(spec):
        d = _flag_bytes(nb, i) if kind else _bytes(i, nb)
        data.append(d)
        srcs.append(Guarded(nb, 1 if so == "flag" else so, fill=d))          # a flag source is bytes: any address
        dsts.append(Guarded(nb * 4 if kind else nb, do))
    assert _add(srcs, dsts, [s[2] for s in spec], [s[3] for s in spec]) == 0
    for i, (so, do, nb, kind) in enumerate(spec):
        if kind:
            assert np.array_equal(dsts[i].host(np.float32), (data[i] != 0).astype(np.float32)), i
            assert set(np.unique(data[i])) == {0, 1, 2, 255} or nb < 16
        else:
            assert np.array_equal(dsts[i].host(np.uint8), data[i]), i
        assert dsts[i].guards_intact() and np.array_equal(srcs[i].host(np.uint8), data[i]), i


@pytest.mark.parametrize("empty", [(0,), (2,), (4,), (0, 2, 4), (0, 1), (3, 4)])
def test_add_zero_byte_arrays_in_the_table(empty):
    """Arrays of no bytes (null pointers) at the head, in the middle and at the end of a table of five: the others are copied as before."""
    sizes = [16 * 1500, 2500, 4 * 1025, 3000, 16 * 64]
    kinds = [0, 1, 0, 0, 0]
    data, srcs, dsts, nbytes = [], [], [], []
    for i, (nb, kind) in enumerate(zip(sizes, kinds)):
        if i in empty:
            data.append(None); srcs.append(None); dsts.append(None); nbytes.append(0)
            continue
        d = _flag_bytes(nb, i) if kind else _bytes(i, nb)
        data.append(d); nbytes.append(nb)
        srcs.append(Guarded(nb, 0, fill=d))
        dsts.append(Guarded(nb * 4 if kind else nb, 0))
    assert _add(srcs, dsts, nbytes, kinds) == 0
    for i, d in enumerate(data):
        if d is not None:
            want = (d != 0).astype(np.float32).view(np.uint8) if kinds[i] else d
            assert np.array_equal(dsts[i].host(np.uint8), want) and dsts[i].guards_intact(), i


def test_add_error_returns_write_nothing():
    capi = _capi()
    L = capi.lib()
    d = _bytes(0, 4096)
    src, dst = Guarded(4096, 0, fill=d), Guarded(4096, 0)
    flag_dst = Guarded(4096 * 4, 1)
    both = Guarded(8192, 0, fill=np.concatenate([d, d]))

    class At:                                                     # an address inside a guarded buffer
        def __init__(self, ptr):
            self.ptr = ptr
    assert _add([], [], [], []) == 0                                                      # no arrays: nothing to do
    assert L.tg_rollout_add(0, None, None, None, None, _stream()) == 0
    assert _add([src], [dst], [4096], [2]) == -1                                          # unknown kind
    assert _add([src], [dst], [-1], [0]) == -1                                            # negative count
    assert _add([None], [dst], [4096], [0]) == -1 and _add([src], [None], [4096], [0]) == -1    # NULL with bytes to move
    assert _add([src], [flag_dst], [4096], [1]) == -1                                     # a flag destination that is no float32 address
    assert _add([both], [At(both.ptr + 4096)], [4097], [0]) == -1                         # the destination starts inside the source
    assert _add([At(both.ptr + 2048)], [both], [1024], [1]) == -1                         # flags: 4 bytes out per byte in reach the source
    assert _add([src, src], [dst, dst], [4096, 4096], [0, 7]) == -1                       # a bad second array: the first is not copied either
    assert L.tg_rollout_add(17, None, None, None, None, _stream()) == -1 and L.tg_rollout_add(-1, None, None, None, None, _stream()) == -1
    assert L.tg_rollout_add(1, None, None, None, None, _stream()) == -1
    assert b"tg_rollout_add" in L.tg_last_error()
    torch.cuda.synchronize()
    assert _untouched(dst) and _untouched(flag_dst)
    assert both.guards_intact() and np.array_equal(both.host(np.uint8), np.concatenate([d, d]))
    assert _add([src], [dst], [0], [0]) == 0 and _untouched(dst)                          # zero bytes: success, nothing written


# ---------------------------------------------------------------------------------------------------------------- gather
ROW_BYTES = (16, 48, 4, 12, 20, 1, 3, 7)
N_SRC = 64


def _rows(B, seed):
    """Descending runs over the source rows with repeats; the last source row first."""
    rng = np.random.default_rng(seed)
    rows = (N_SRC - 1 - np.arange(B) // 2) % N_SRC                 # every row twice, descending, wrapping
    rows[rng.random(B) < 0.1] = N_SRC - 1
    return rows.astype(np.int64)


def test_gather_matrix_reaches_every_unit_with_and_without_rows_of_one_unit():
    seen = {(_unit(so, do, rb), rb // _unit(so, do, rb) == 1) for so in OFFSETS for do in OFFSETS for rb in ROW_BYTES}
    assert seen == {(u, one) for u in (16, 4, 1) for one in (True, False)}
    totals = {_tail(B * (rb // _unit(so, do, rb))) for so in OFFSETS for do in OFFSETS for rb in ROW_BYTES for B in (700, 1024, 1025, 2047)}
    assert {"below", "exact", "plus1", "plus1023"} <= totals


@pytest.mark.parametrize("B", [700, 1024, 1025, 2047])
@pytest.mark.parametrize("dst_off", OFFSETS)
@pytest.mark.parametrize("src_off", OFFSETS)
def test_gather_alignment_classes(src_off, dst_off, B):
    rows = _rows(B, B)
    assert len(set(rows.tolist())) < B and (np.diff(rows) < 0).any() and rows.max() == N_SRC - 1
    rows_dev = torch.from_numpy(rows).cuda()
    data = [_bytes(1000 * src_off + 100 * dst_off + i, N_SRC * rb).reshape(N_SRC, rb) for i, rb in enumerate(ROW_BYTES)]
    srcs = [Guarded(d.size, src_off, fill=d) for d in data]
    dsts = [Guarded(B * rb, dst_off) for rb in ROW_BYTES]
    assert _gather(srcs, dsts, list(ROW_BYTES), rows_dev, B) == 0
    for i, rb in enumerate(ROW_BYTES):
        assert np.array_equal(dsts[i].host(np.uint8).reshape(B, rb), data[i][rows]), (i, rb)
        assert dsts[i].guards_intact() and srcs[i].guards_intact() and np.array_equal(srcs[i].host(np.uint8).reshape(N_SRC, rb), data[i]), i
    assert np.array_equal(rows_dev.cpu().numpy(), rows)


def test_gather_sixteen_arrays_with_empty_ones_between():
    B = 1500
    rows = _rows(B, 5)
    rows_dev = torch.from_numpy(rows).cuda()
    spec = [(0, 0, 0), (0, 0, 64), (4, 0, 8), (0, 0, 0), (1, 0, 5), (0, 4, 16), (0, 0, 4), (0, 0, 1), (4, 4, 24), (0, 0, 0), (0, 1, 32),
            (0, 0, 2048), (1, 1, 1), (0, 0, 40), (4, 0, 4), (0, 0, 0)]
    assert len(spec) == 16
    data, srcs, dsts = [], [], []
    for i, (so, do, rb) in enumerate(spec):
        if rb == 0:
            data.append(None); srcs.append(None); dsts.append(None)
            continue
        d = _bytes(i, N_SRC * rb).reshape(N_SRC, rb)
        data.append(d)
        srcs.append(Guarded(d.size, so, fill=d))
        dsts.append(Guarded(B * rb, do))
    assert _gather(srcs, dsts, [s[2] for s in spec], rows_dev, B) == 0
    for i, d in enumerate(data):
        if d is not None:
            assert np.array_equal(dsts[i].host(np.uint8).reshape(B, -1), d[rows]) and dsts[i].guards_intact(), i


def test_gather_error_returns_write_nothing():
    L = _capi().lib()
    d = _bytes(0, N_SRC * 16)
    src, dst = Guarded(d.size, 0, fill=d), Guarded(8 * 16, 0)
    rows_dev = torch.arange(8, dtype=torch.int64, device="cuda")
    assert _gather([], [], [], rows_dev, 8) == 0 and _gather([src], [dst], [16], rows_dev, 0) == 0      # nothing to do
    assert _gather([src], [dst], [16], rows_dev, -1) == -1
    assert _gather([src], [dst], [-16], rows_dev, 8) == -1
    assert _gather([None], [dst], [16], rows_dev, 8) == -1 and _gather([src], [None], [16], rows_dev, 8) == -1
    assert _gather([src], [dst], [16], None, 8) == -1
    assert L.tg_rollout_gather(17, None, None, None, None, 8, _stream()) == -1
    assert b"tg_rollout_gather" in L.tg_last_error()
    assert _gather([src], [dst], [0], rows_dev, 8) == 0
    torch.cuda.synchronize()
    assert _untouched(dst)


# ---------------------------------------------------------------------------------------------------------------- GAE
def _odd_float_flags(d, seed):
    """float32 dones with the same truth as d but other values: 0.5, -3 or 1 where set, +0.0 or -0.0 where not."""
    rng = np.random.default_rng(seed)
    on = rng.choice(np.array([0.5, -3.0, 1.0], np.float32), size=d.shape)
    off = rng.choice(np.array([0.0, -0.0], np.float32), size=d.shape)
    return np.where(d != 0, on, off).astype(np.float32)


@pytest.mark.parametrize("starts", GAE_STARTS)
@pytest.mark.parametrize("T", GAE_T)
def test_gae_on_both_sides_of_every_boundary(T, starts):
    """Bit for bit the restatement, and inside tests/rollout_ref.py's bound of the float64 recurrence (tests/test_rollout_cpu.py holds the
    restatement to the same bound on the same inputs)."""
    for N in GAE_N:
        r, v, es, lv, d = gae_edge_inputs(T, N, starts)
        for k, (gamma, lam) in enumerate(GAE_PARAMS):
            a32, r32 = gae_f32(r, v, es, lv, d, gamma, lam)
            a64, r64 = gae_f64(r, v, es, lv, d, gamma, lam)
            bound = gae_bound(r, v, lv, a64, gamma, lam)
            for dones in (d.astype(np.uint8), d, _odd_float_flags(d, T + N + k)):
                adv, ret = _gae(r, v, es, lv, dones, gamma, lam, T, N)
                assert _bits_equal(adv, a32) and _bits_equal(ret, r32), (T, N, starts, gamma, lam, dones.dtype)
                assert gae_error(adv, ret, a64, r64) <= bound


def test_gae_error_returns_write_nothing():
    capi = _capi()
    L = capi.lib()
    T, N = 9, 65
    r, v, es, lv, d = gae_edge_inputs(T, N, "alternating")
    dev = [Guarded(a.nbytes, 0, fill=a) for a in (r, v, es, lv, d)]
    adv, ret = Guarded(T * N * 4, 0), Guarded(T * N * 4, 0)
    p = [g.ptr for g in dev]

    def call(ptrs=p, dtype=1, a=adv.ptr, b=ret.ptr, T=T, N=N):
        return L.tg_rollout_gae(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], dtype, a, b, T, N, 0.99, 0.95, _stream())
    assert call(dtype=2) == -1 and call(T=0) == -1 and call(N=0) == -1 and call(T=-3) == -1
    assert call(T=1 << 30, N=1 << 30) == -1
    for i in range(5):
        assert call(ptrs=p[:i] + [None] + p[i + 1:]) == -1
    assert call(a=None) == -1 and call(b=None) == -1
    assert b"tg_rollout_gae" in L.tg_last_error()
    torch.cuda.synchronize()
    assert _untouched(adv) and _untouched(ret)
    assert call() == 0
    torch.cuda.synchronize()
    a32, r32 = gae_f32(r, v, es, lv, d, 0.99, 0.95)
    assert _bits_equal(adv.host(np.float32).reshape(T, N), a32) and _bits_equal(ret.host(np.float32).reshape(T, N), r32)
