"""The wave-mapped GJK / EPA of csrc/tg_narrowphase.hpp against oracle/narrowphase.c over the case matrix of tests/narrow_cases.py, BIT FOR
BIT, in every class: face-parallel and touching placements, symmetric overlaps, deep overlaps and containment (EPA's LDS lists at their
caps), hulls of 1 to 1152 and 1 to 256 vertices, duplicate vertices, three boxes, two scales.  What the oracle itself is worth on the
matrix: tests/test_narrow_cases_cpu.py; the manifold: tests/test_gpu_manifold_scripts.py.
Reference call site: pb.stepSimulation(), robots/arms/robot.py:141.

The selftest entries refuse n_hull 0 and 1153, n_b 0 and 257, n_cases 0 and NULL pointers with -1 before any allocation or launch (the first
statement of each entry in csrc/tg_narrow_test.hip)."""
import ctypes as C

import numpy as np
import pytest

import narrow_cases as nc

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)


def _device(indexed):
    from tactile_gym_amd import _capi
    T = _capi.test_lib()
    dev = {}
    for idx, hulls, half, hull_b in nc.batches(indexed):
        out = np.zeros((len(idx), 11))
        if hull_b is None:
            e = np.array(half, dtype=np.float64)
            rc = T.tg_selftest_narrowphase(len(idx), hulls.shape[1], hulls.ctypes.data_as(dp), e.ctypes.data_as(dp), out.ctypes.data_as(dp))
        else:
            b = np.ascontiguousarray(hull_b)
            rc = T.tg_selftest_narrowphase_hulls(len(idx), hulls.shape[1], hulls.ctypes.data_as(dp), b.shape[0], b.ctypes.data_as(dp), out.ctypes.data_as(dp))
        assert rc == 0
        for k, i in enumerate(idx):
            dev[i] = out[k]
    return dev


@pytest.mark.parametrize("cls", nc.CLASSES)
def test_device_equals_oracle_bit_for_bit(cls):
    indexed = nc.of_class(cls)
    ref = nc.oracle_results()
    dev = _device(indexed)
    bad = []
    for i, c in indexed:
        d, r = dev[i], ref[i]
        words = 11 if r[0] == 1.0 else 1                   # `found` as it comes; the other ten words where a normal was found
        if d[0] != r[0] or not np.array_equal(d[:words].view(np.uint64), r[:words].view(np.uint64)):
            bad.append((c.name, d[:5].tolist(), r[:5].tolist()))
    assert not bad, (len(bad), len(indexed), bad[:5])
    print(f"{cls}: {len(indexed)} cases in {len(nc.batches(indexed))} launches, {int(sum(ref[i, 0] for i, _ in indexed))} with a normal: all words bit-identical to the oracle")


def test_selftest_entries_refuse_bad_arguments():
    from tactile_gym_amd import _capi
    T = _capi.test_lib()
    h, e, b, out = np.zeros((1153, 3)), np.full(3, 0.04), np.zeros((257, 3)), np.zeros(11)
    P = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    for n_cases, n_hull, hp, ep, op in ((1, 0, P(h), P(e), P(out)), (1, 1153, P(h), P(e), P(out)), (0, 8, P(h), P(e), P(out)), (1, 8, None, P(e), P(out)),
                                         (1, 8, P(h), None, P(out)), (1, 8, P(h), P(e), None)):
        assert T.tg_selftest_narrowphase(n_cases, n_hull, hp, ep, op) == -1
    for n_cases, n_hull, n_b, hp, bp, op in ((1, 0, 8, P(h), P(b), P(out)), (1, 1153, 8, P(h), P(b), P(out)), (1, 8, 0, P(h), P(b), P(out)), (1, 8, 257, P(h), P(b), P(out)),
                                              (0, 8, 8, P(h), P(b), P(out)), (1, 8, 8, None, P(b), P(out)), (1, 8, 8, P(h), None, P(out)), (1, 8, 8, P(h), P(b), None)):
        assert T.tg_selftest_narrowphase_hulls(n_cases, n_hull, hp, n_b, bp, op) == -1
    ops = np.zeros((1, 1, nc.OP_WORDS))
    for n_cases, n_ops, pp, op in ((0, 1, P(ops), P(out)), (1, 0, P(ops), P(out)), (1, 1, None, P(out)), (1, 1, P(ops), None)):
        assert T.tg_selftest_manifold(n_cases, n_ops, pp, op) == -1
    assert (out == 0).all()
