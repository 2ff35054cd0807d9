"""The persistent manifold of csrc/tg_narrowphase.hpp (manifold_add / manifold_refresh, btPersistentManifold's cache rules: PARITY A36-A38) on
the device, directly: tg_selftest_manifold applies a script of operations to a manifold in LDS, one wavefront per script, and returns the
manifold after every operation; the same script goes through mb_manifold_add / mb_manifold_refresh (oracle/narrowphase.c), and count, la, lb,
normal, pa, pb and depth of the live slots are compared BIT FOR BIT after every operation.  The scripts (tests/narrow_cases.py): known answers
- the replace rule, the threshold itself and one ulp past it, the fifth point with every slot and the new point as the deepest, exact ties,
refresh dropping a middle, the last and every point, drift exactly at the threshold - whose outcomes tests/test_narrow_cases_cpu.py asserts
on the oracle; and 300 random scripts of 24 operations.  Reference call site: pb.stepSimulation(), robots/arms/robot.py:141."""
import ctypes as C

import numpy as np
import pytest

import narrow_cases as nc

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)


def _device_manifold(scripts):
    """scripts [n][n_ops][36] -> the manifold after every operation [n][n_ops][65]"""
    from tactile_gym_amd import _capi
    scripts = np.ascontiguousarray(scripts, dtype=np.float64)
    out = np.full(scripts.shape[:2] + (nc.MANI_WORDS,), np.nan)
    assert 0 == _capi.test_lib().tg_selftest_manifold(scripts.shape[0], scripts.shape[1], scripts.ctypes.data_as(dp), out.ctypes.data_as(dp))
    return out


def _same_live_words(dev, ref, tag):
    assert np.array_equal(dev[..., 64], ref[..., 64]), (tag, "counts", np.argwhere(dev[..., 64] != ref[..., 64])[:5].tolist())
    m = nc.live(ref)
    same = dev.view(np.uint64)[m] == ref.view(np.uint64)[m]
    assert same.all(), (tag, int((~same).sum()), np.argwhere(m & (dev.view(np.uint64) != ref.view(np.uint64)))[:5].tolist())


def test_device_manifold_known_scripts_equal_oracle_bit_for_bit():
    known = nc.known_scripts()
    n_ops = max(len(v) for v in known.values())
    pad = np.zeros((len(known), n_ops, nc.OP_WORDS))
    pad[:, :, 0] = nc.NOP                                  # a shorter script ends in operations that do nothing
    for k, v in enumerate(known.values()):
        pad[k, :len(v)] = v
    dev = _device_manifold(pad)
    for k, (name, v) in enumerate(known.items()):
        ref = nc.replay(v)
        _same_live_words(dev[k, :len(v)], ref, name)
        assert (dev[k, len(v):] == dev[k, len(v) - 1]).all(), name          # ... and they do nothing


def test_device_manifold_random_scripts_equal_oracle_bit_for_bit():
    rs = nc.random_scripts()
    ref = np.stack([nc.replay(s) for s in rs])
    shares = nc.rule_shares(rs, ref)
    assert min(shares.values()) >= 0.1, shares             # the replace rule, the fifth-point rule and the drop with a swap each fire
    _same_live_words(_device_manifold(rs), ref, "random")
    print(f"{rs.shape[0]} scripts x {rs.shape[1]} operations, rules fired in {shares} of the scripts: live slots and counts bit-identical after every operation")
