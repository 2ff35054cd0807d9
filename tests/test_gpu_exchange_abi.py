"""The context-free entries of csrc/tg_exchange.hip called directly on raw pointers: tg_tiles_capacity, tg_pack_tiles, tg_unpack_tiles,
tg_unpack_tiles_multi (both forms), tg_copy_bytes, tg_copy_bytes2(_flag), tg_flag_set / tg_flag_wait, over the tables of
tests/exchange_cases.py: every tile count round the 64-lane wavefront, non-square images, no / one / every tile live, tiles that differ in one
byte, every tail size, message sequences with moving live sets and broken headers, ids outside the batch, one case beyond every block cap, copy
sizes round the 16-byte piece and the block cap, and the error returns that take no launch.

Every device buffer is a device_guard.Guarded payload between guard bytes; every comparison is byte equality with tests/exchange_ref.py."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exchange_cases as XC  # noqa: E402
import exchange_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import Guarded  # noqa: E402

P = C.c_void_p
FLAG_VALUE = 0xC0FFEE01


def _lib():
    from tactile_gym_amd import _capi
    return _capi, _capi.lib()


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _ptr(g):
    return P(g.ptr if g is not None else None)


def _holds(g, data):
    """The payload equals `data` byte for byte and the guards are intact."""
    return np.array_equal(g.host(np.uint8), np.ascontiguousarray(data).reshape(-1).view(np.uint8)) and g.guards_intact()


def _untouched(g):
    return g.guards_intact() and bool((g.payload() == XC.FILL).all())


def _sorted_message(host, want):
    """The device's message buffer with its records put in id order (the kernel's record order is not defined); the ids must be unique."""
    count = int(host[:4].view(np.uint32)[0])
    assert count == int(want[:4].view(np.uint32)[0]), (count, want[:16].view(np.uint32))
    ids, rec = ref.sort_records(host, count)
    assert len(np.unique(ids)) == count
    out = host.copy()
    out[16:16 + ref.REC * count] = rec.reshape(-1)
    return out


def _pack(L, capi, obs, tm, case, msg, counters, tail_g, tail_bytes, off):
    capi.check(L.tg_pack_tiles(_stream(), _ptr(obs), _ptr(tm), case.n_images, case.h, case.w, _ptr(msg), _ptr(counters), _ptr(tail_g), tail_bytes, off))


@pytest.mark.parametrize("T", sorted(XC.SHAPES))
def test_tiles_capacity(T):
    _, L = _lib()
    for h, w in (XC.SHAPES[T],) + (XC.TALL_SHAPES if T == 1 else ()):
        for n in (1, 2, 7, 33001):
            out = C.c_int64(-1)
            assert L.tg_tiles_capacity(n, h, w, C.byref(out)) == 0
            assert out.value == 16 + 272 * n * (h // 16) * (w // 16) == ref.capacity(n, h, w)


@pytest.mark.parametrize("case", XC.CASES, ids=lambda c: c.name)
def test_pack_and_unpack_equal_the_reference(case):
    capi, L = _lib()
    tmpl, img, tail, off, nbytes = XC.build(case)
    want = XC.expected_message(case)
    obs = Guarded(img.nbytes, fill=img)
    tm = Guarded(tmpl.nbytes, offset=16 * (case.seed % 4), fill=tmpl)
    counters = Guarded(8, fill=np.zeros(2, np.uint32))                         # exactly the two uint32 the header documents
    tail_g = None if tail is None else Guarded(len(tail), offset=16 * (case.seed % 2), fill=tail if len(tail) else None)
    tail_bytes = 17 if tail is None else len(tail)                             # a NULL tail comes with a size, a tail of no bytes with a pointer
    for rep in range(2):                                                       # the counters are left zero: a second launch gives the same message
        msg = Guarded(nbytes, offset=16 * ((case.seed + rep) % 3))
        _pack(L, capi, obs, tm, case, msg, counters, tail_g, tail_bytes, off)
        torch.cuda.synchronize()
        host = msg.host(np.uint8)
        assert host[:16].view(np.uint32).tolist() == [int(want[:4].view(np.uint32)[0]), case.n_images, case.T, ref.MAGIC]
        assert np.array_equal(_sorted_message(host, want), want), rep          # records, pad bytes, the fill behind them, the tail, the byte after it
        assert msg.guards_intact() and _holds(counters, np.zeros(2, np.uint32)), rep
    assert _holds(obs, img) and _holds(tm, tmpl) and (tail_g is None or (_holds(tail_g, tail) if len(tail) else tail_g.guards_intact()))
    for src in (msg, Guarded(len(want), fill=want)):                           # the device's own message, then the reference's (sorted: one more order)
        dst = Guarded(img.nbytes, offset=16 * (case.seed % 5))                 # holds the pattern: the entry promises the template everywhere first
        capi.check(L.tg_unpack_tiles(_stream(), _ptr(src), _ptr(tm), case.n_images, case.h, case.w, _ptr(dst)))
        torch.cuda.synchronize()
        assert _holds(dst, img) and src.guards_intact()
    assert _holds(src, want) and _holds(tm, tmpl)


@pytest.mark.parametrize("mal", XC.MALFORMED, ids=lambda m: m.name)
def test_malformed_messages_are_tolerated(mal):
    """A wrong magic or tile count leaves the template; a count above the capacity is clamped; a record whose id is outside the batch is
    ignored by every scatter and by the restore (its id still enters the list), and nothing lands outside the destination."""
    capi, L = _lib()
    tmpl, want, msg = XC.build_malformed(mal)
    n, h, w = mal.n_images, mal.h, mal.w
    tm, src = Guarded(tmpl.nbytes, fill=tmpl), Guarded(2 * len(msg), fill=np.concatenate([msg, msg]))
    dst = Guarded(want.nbytes)
    capi.check(L.tg_unpack_tiles(_stream(), _ptr(src), _ptr(tm), n, h, w, _ptr(dst)))
    torch.cuda.synchronize()
    assert np.array_equal(want, ref.unpack(msg, tmpl, n, h, w))
    assert _holds(dst, want)
    both = np.stack([want, want])
    fill = Guarded(both.nbytes)
    keep = Guarded(both.nbytes, fill=np.broadcast_to(tmpl, both.shape))
    prev = Guarded(4 * 2 * (1 + n * mal.T), fill=np.zeros(2 * (1 + n * mal.T), np.uint32))
    model = ref.UnpackMulti(tmpl, 2, n, h, w, -1, True)
    for rep in range(2):                                                       # the second call restores from a list that holds the bad ids
        capi.check(L.tg_unpack_tiles_multi(_stream(), _ptr(src), len(msg), 2, -1, _ptr(tm), n, h, w, _ptr(fill), None))
        capi.check(L.tg_unpack_tiles_multi(_stream(), _ptr(src), len(msg), 2, -1, _ptr(tm), n, h, w, _ptr(keep), _ptr(prev)))
        torch.cuda.synchronize()
        model.step([msg, msg])
        assert np.array_equal(model.dst, both)
        assert _holds(fill, both) and _holds(keep, both), rep
        lists = prev.host(np.uint32).reshape(2, -1)
        for r, (count, ids) in enumerate(model.list_sets()):
            assert lists[r, 0] == count and np.array_equal(np.sort(lists[r, 1:1 + count]), ids), (rep, r)
        assert prev.guards_intact()
    assert _holds(src, np.concatenate([msg, msg])) and _holds(tm, tmpl)


@pytest.mark.parametrize("seq", XC.SEQUENCES, ids=lambda s: s.name)
def test_unpack_multi_follows_the_model_through_a_sequence(seq):
    capi, L = _lib()
    tmpl, images, messages = XC.build_sequence(seq)
    R, n, h, w, T = seq.n_ranks, seq.n_images, seq.h, seq.w, seq.T
    shape = (R, n, h, w)

    def start(value):
        d = np.broadcast_to(tmpl, shape).copy() if value is None else np.full(shape, value, np.uint8)
        if seq.skip_rank >= 0:
            d[seq.skip_rank] = XC.SKIP_FILL
        return d

    lists0 = np.zeros((R, 1 + n * T), np.uint32)
    if seq.skip_rank >= 0:
        lists0[seq.skip_rank] = 0xA5A5A5A5
    tm, src = Guarded(tmpl.nbytes, fill=tmpl), Guarded(R * seq.stride, offset=32)
    # the fill form over a patterned destination; the list form over the template; the list form over bytes that are not the template (it may
    # touch the previous and the new tiles only)
    runs = [(Guarded(int(np.prod(shape)), fill=start(v)), Guarded(lists0.nbytes, fill=lists0) if with_list else None,
             ref.UnpackMulti(tmpl, R, n, h, w, seq.skip_rank, with_list, start(v), lists0 if with_list else None))
            for v, with_list in ((XC.FILL, False), (None, True), (0x3C, True))]
    for m in range(XC.N_MESSAGES):
        batch = np.concatenate(messages[m])
        src.payload().copy_(torch.from_numpy(batch))
        for dst, prev, model in runs:
            capi.check(L.tg_unpack_tiles_multi(_stream(), _ptr(src), seq.stride, R, seq.skip_rank, _ptr(tm), n, h, w, _ptr(dst), _ptr(prev)))
        torch.cuda.synchronize()
        for k, (dst, prev, model) in enumerate(runs):
            model.step(messages[m])
            assert _holds(dst, model.dst), (m, k)
            if prev is None:
                continue
            lists = prev.host(np.uint32).reshape(R, -1)
            for r, (count, ids) in enumerate(model.list_sets()):
                if r == seq.skip_rank:
                    assert (lists[r] == 0xA5A5A5A5).all(), (m, k)
                else:
                    assert lists[r, 0] == count and np.array_equal(np.sort(lists[r, 1:1 + count]), ids), (m, k, r)
            assert prev.guards_intact()
        for r in range(R):                                                     # the model is the images themselves
            if r != seq.skip_rank:
                assert np.array_equal(runs[0][2].dst[r], images[m][r]) and np.array_equal(runs[1][2].dst[r], images[m][r])
        assert _holds(src, batch) and _holds(tm, tmpl), m


def test_the_large_case_crosses_every_block_cap():
    """32 MiB of images, more than 65 536 records in one message: every fill, scatter and restore kernel takes grid-stride steps."""
    capi, L = _lib()
    case = XC.LARGE
    tmpl, img = XC.build_large()
    n, h, w, T = case.n_images, case.h, case.w, case.T
    hdr, rec = ref.pack(img, tmpl)
    cap = ref.capacity(n, h, w)
    stride = (cap + 15) // 16 * 16 + 48
    want = ref.message(hdr, rec, stride, XC.FILL)
    obs, tm, counters = Guarded(img.nbytes, fill=img), Guarded(tmpl.nbytes, fill=tmpl), Guarded(8, fill=np.zeros(2, np.uint32))
    src = Guarded(2 * stride)
    _pack(L, capi, obs, tm, case, src, counters, None, 0, 0)
    torch.cuda.synchronize()
    host = src.host(np.uint8)[:stride]
    assert np.array_equal(_sorted_message(host, want), want)
    assert _holds(counters, np.zeros(2, np.uint32)) and bool((src.payload()[stride:] == XC.FILL).all()) and src.guards_intact()
    dst = Guarded(img.nbytes)
    capi.check(L.tg_unpack_tiles(_stream(), _ptr(src), _ptr(tm), n, h, w, _ptr(dst)))
    torch.cuda.synchronize()
    assert _holds(dst, img)
    del dst, obs
    # two ranks: the device's own message and the reference's; then the batch reversed, so that the restore walks the whole previous list
    src.payload()[stride:].copy_(torch.from_numpy(want))
    both = np.stack([img, img])
    fill, keep = Guarded(both.nbytes), Guarded(both.nbytes, fill=np.broadcast_to(tmpl, both.shape))
    prev = Guarded(4 * 2 * (1 + n * T), fill=np.zeros(2 * (1 + n * T), np.uint32))
    ids = rec[:, :4].copy().view(np.uint32).reshape(-1)
    for step in range(2):
        capi.check(L.tg_unpack_tiles_multi(_stream(), _ptr(src), stride, 2, -1, _ptr(tm), n, h, w, _ptr(fill), None))
        capi.check(L.tg_unpack_tiles_multi(_stream(), _ptr(src), stride, 2, -1, _ptr(tm), n, h, w, _ptr(keep), _ptr(prev)))
        torch.cuda.synchronize()
        assert _holds(fill, both) and _holds(keep, both), step
        lists = prev.host(np.uint32).reshape(2, -1)
        for r in range(2):
            assert lists[r, 0] == len(ids) and np.array_equal(np.sort(lists[r, 1:1 + len(ids)]), ids), (step, r)
        assert prev.guards_intact() and _holds(tm, tmpl)
        if step == 0:
            img = np.ascontiguousarray(img[::-1])
            hdr, rec = ref.pack(img, tmpl)
            ids = rec[:, :4].copy().view(np.uint32).reshape(-1)
            m = torch.from_numpy(ref.message(hdr, rec[np.random.default_rng(1).permutation(len(rec))], stride, XC.FILL))
            src.payload()[:stride].copy_(m)
            src.payload()[stride:].copy_(m)
            both = np.stack([img, img])


def _bytes(size, seed):
    return np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)


@pytest.mark.parametrize("size", XC.COPY_SIZES)
def test_copy_bytes(size):
    capi, L = _lib()
    data = _bytes(size, size)
    src, dst = Guarded(size, fill=data if size else None), Guarded(size, offset=16)
    assert L.tg_copy_bytes(_stream(), _ptr(dst), _ptr(src), size) == 0
    torch.cuda.synchronize()
    assert _holds(dst, data) and _holds(src, data)                             # the byte behind the destination is a guard byte


@pytest.mark.parametrize("pair", XC.COPY_PAIRS, ids=lambda p: f"{p[0]}+{p[1]}")
def test_copy_bytes2(pair):
    capi, L = _lib()
    b1, b2 = pair
    d1, d2 = _bytes(b1, b1 + 1), _bytes(b2, b2 + 2)
    s1, s2 = Guarded(b1, offset=16, fill=d1 if b1 else None), Guarded(b2, fill=d2 if b2 else None)
    o1, o2 = Guarded(b1), Guarded(b2, offset=48)
    capi.check(L.tg_copy_bytes2(_stream(), _ptr(o1), _ptr(s1), b1, _ptr(o2), _ptr(s2), b2))
    torch.cuda.synchronize()
    assert _holds(o1, d1) and _holds(o2, d2) and _holds(s1, d1) and _holds(s2, d2)


@pytest.mark.parametrize("n_flags,stride", [(n, s) for n in (1, 3, 64) for s in (1, 16)])
def test_copy_bytes2_flag(n_flags, stride):
    """Exactly the words i * stride, i < n_flags, hold the value afterwards; every word between and behind them is untouched."""
    capi, L = _lib()
    words = (n_flags - 1) * stride + 1 + 40
    for k, (b1, b2) in enumerate(XC.COPY_PAIRS[(n_flags + stride) % 2::2]):
        d1, d2 = _bytes(b1, k), _bytes(b2, k + 50)
        s1, s2 = Guarded(b1, fill=d1 if b1 else None), Guarded(b2, offset=16, fill=d2 if b2 else None)
        o1, o2, flags = Guarded(b1, offset=32), Guarded(b2), Guarded(4 * words)
        capi.check(L.tg_copy_bytes2_flag(_stream(), _ptr(o1), _ptr(s1), b1, _ptr(o2), _ptr(s2), b2, _ptr(flags), n_flags, stride, FLAG_VALUE))
        torch.cuda.synchronize()
        want = np.full(words, 0xA5A5A5A5, np.uint32)
        want[:(n_flags - 1) * stride + 1:stride] = FLAG_VALUE
        assert (want == FLAG_VALUE).sum() == n_flags
        assert _holds(flags, want) and _holds(o1, d1) and _holds(o2, d2) and _holds(s1, d1) and _holds(s2, d2), (b1, b2)
    capi.check(L.tg_copy_bytes2_flag(_stream(), _ptr(o1), _ptr(s1), b1, _ptr(o2), _ptr(s2), b2, None, n_flags, stride, FLAG_VALUE + 1))   # NULL: none
    torch.cuda.synchronize()
    assert _holds(flags, want) and _holds(o1, d1) and _holds(o2, d2)


def test_flags_compare_modulo_two_to_the_32():
    """n = 64 with stride 1.  A flag of 2 has passed 0xFFFFFFFE (the counter wrapped): no wait.  A flag of 0xFFFFFFFE has not reached 3: that
    wait, with an error word of its own, runs into its timeout (the one wait of this file on a flag nobody raises)."""
    capi, L = _lib()
    flags = Guarded(64 * 4, fill=np.zeros(64, np.uint32))
    err, err2 = Guarded(4, fill=np.zeros(1, np.uint32)), Guarded(4, fill=np.zeros(1, np.uint32))
    s = _stream()
    capi.check(L.tg_flag_set(s, _ptr(flags), 64, 1, 2))
    torch.cuda.synchronize()
    assert _holds(flags, np.full(64, 2, np.uint32))
    t0 = time.perf_counter()
    capi.check(L.tg_flag_wait(s, _ptr(flags), 64, 1, 0xFFFFFFFE, _ptr(err), 2000))
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 0.25 and _holds(err, np.zeros(1, np.uint32))
    capi.check(L.tg_flag_set(s, _ptr(flags), 64, 1, 0xFFFFFFFE))
    torch.cuda.synchronize()
    assert _holds(flags, np.full(64, 0xFFFFFFFE, np.uint32))
    t0 = time.perf_counter()
    capi.check(L.tg_flag_wait(s, _ptr(flags), 64, 1, 3, _ptr(err2), 300))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert 0.25 < dt < 3.0, dt
    assert _holds(err2, np.full(1, 0xFFFFFFFF, np.uint32)) and _holds(err, np.zeros(1, np.uint32))     # bit i & 31 of all 64 lanes
    assert _holds(flags, np.full(64, 0xFFFFFFFE, np.uint32))


def test_error_returns_take_no_launch():
    _, L = _lib()
    obs, tm, msg, cnt, tail, dst, prev, flags = (Guarded(4096) for _ in range(8))     # n = 2 images of 32 x 32: 2048 bytes, a message of 2192
    s = _stream()
    bad = []

    def expect(name, rc):
        bad.append((name, rc, L.tg_last_error().decode()))

    def pack(obs=obs.ptr, tm=tm.ptr, n=2, h=32, w=32, msg=msg.ptr, cnt=cnt.ptr, tail=tail.ptr, tail_bytes=64, off=2208):
        expect("tg_pack_tiles", L.tg_pack_tiles(s, P(obs), P(tm), n, h, w, P(msg), P(cnt), P(tail), tail_bytes, off))

    def unpack(src=msg.ptr, tm=tm.ptr, n=2, h=32, w=32, dst=dst.ptr):
        expect("tg_unpack_tiles", L.tg_unpack_tiles(s, P(src), P(tm), n, h, w, P(dst)))

    def multi(src=msg.ptr, stride=2208, ranks=1, skip=-1, tm=tm.ptr, n=2, h=32, w=32, dst=dst.ptr, prev=prev.ptr):
        expect("tg_unpack_tiles_multi", L.tg_unpack_tiles_multi(s, P(src), stride, ranks, skip, P(tm), n, h, w, P(dst), P(prev)))

    def copy(dst=dst.ptr, src=obs.ptr, size=64):
        expect("tg_copy_bytes", L.tg_copy_bytes(s, P(dst), P(src), size))

    def copy2(d1=dst.ptr, s1=obs.ptr, b1=64, d2=msg.ptr, s2=tm.ptr, b2=64, flag=False, fl=flags.ptr, n=1, stride=1):
        if flag:
            expect("tg_copy_bytes2", L.tg_copy_bytes2_flag(s, P(d1), P(s1), b1, P(d2), P(s2), b2, P(fl), n, stride, 7))
        else:
            expect("tg_copy_bytes2", L.tg_copy_bytes2(s, P(d1), P(s1), b1, P(d2), P(s2), b2))

    def flag_set(fl=flags.ptr, n=1, stride=1):
        expect("tg_flag_set", L.tg_flag_set(s, P(fl), n, stride, 7))

    def flag_wait(fl=flags.ptr, n=1, stride=1, err=cnt.ptr, timeout=300):
        expect("tg_flag_wait", L.tg_flag_wait(s, P(fl), n, stride, 0, P(err), timeout))

    sides = [dict(h=0), dict(h=-16), dict(h=24), dict(w=0), dict(w=-32), dict(w=8), dict(n=0), dict(n=-1)]
    for kw in [dict(obs=None), dict(tm=None), dict(msg=None), dict(cnt=None)] + sides:
        pack(**kw)
    for kw in (dict(tail_bytes=(1 << 20) + 1), dict(tail_bytes=-1), dict(off=2200), dict(off=-16), dict(tail=tail.ptr + 8),
               dict(obs=obs.ptr + 8), dict(tm=tm.ptr + 4), dict(msg=msg.ptr + 1)):
        pack(**kw)
    for kw in [dict(src=None), dict(tm=None), dict(dst=None), dict(src=msg.ptr + 8), dict(tm=tm.ptr + 1), dict(dst=dst.ptr + 4)] + sides:
        unpack(**kw)
    for kw in [dict(src=None), dict(tm=None), dict(dst=None), dict(src=msg.ptr + 8), dict(tm=tm.ptr + 1), dict(dst=dst.ptr + 4), dict(stride=0),
               dict(stride=8), dict(stride=-16), dict(stride=2200), dict(ranks=0), dict(ranks=65536), dict(ranks=-1)] + sides:
        multi(**kw)
        multi(prev=None, **kw)
    for kw in (dict(dst=None), dict(src=None), dict(size=-1), dict(dst=dst.ptr + 8), dict(src=obs.ptr + 1)):
        copy(**kw)
    for flag in (False, True):
        for kw in (dict(d1=None), dict(s1=None), dict(d2=None), dict(s2=None), dict(b1=-1), dict(b2=-1), dict(d1=dst.ptr + 8), dict(s1=obs.ptr + 4),
                   dict(d2=msg.ptr + 2), dict(s2=tm.ptr + 1)):
            copy2(flag=flag, **kw)
    for kw in (dict(n=0), dict(n=65), dict(n=-1), dict(stride=0), dict(stride=-1)):
        copy2(flag=True, **kw)
        flag_set(**kw)
        flag_wait(**kw)
    flag_set(fl=None)
    flag_wait(fl=None)
    flag_wait(timeout=0)
    flag_wait(timeout=-5)
    out = C.c_int64(-7)
    for n, h, w, ref_out in ((0, 32, 32, out), (2, 0, 32, out), (2, 32, 24, out), (2, -16, 32, out), (2, 32, 32, None)):
        expect("tg_tiles_capacity", L.tg_tiles_capacity(n, h, w, C.byref(ref_out) if ref_out is not None else None))
    assert out.value == -7
    wrong = [b for b in bad if b[1] != -1 or b[0] not in b[2]]
    assert not wrong and len(bad) > 120, wrong
    assert L.tg_copy_bytes(s, P(dst.ptr), P(obs.ptr), 0) == 0                  # nothing to copy: no launch, no error
    torch.cuda.synchronize()
    for g in (obs, tm, msg, cnt, tail, dst, prev, flags):
        assert _untouched(g)                                                   # nothing was written
