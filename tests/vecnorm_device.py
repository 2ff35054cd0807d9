"""The device side of VecNormalize's raw-pointer tests (tests/test_gpu_vecnorm_abi.py, tests/test_gpu_nonfinite.py): the state of one normaliser
in guarded device blocks, with tg_vecnorm_update and tg_vecnorm_apply on it, and the numpy model next to it."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vecnorm_ref as ref  # noqa: E402
from device_guard import Guarded  # noqa: E402


def _lib():
    from tactile_gym_amd import _capi
    return _capi, _capi.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptrs(items, n=4):
    return (C.c_void_p * max(len(items), n))(*[(x.ptr if x is not None else None) for x in items])


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _done_pattern(pattern, n):
    s = np.zeros(n, np.uint8)
    if pattern == "all":
        s[:] = 1
    elif pattern == "alternating":
        s[::2] = 7                      # any non-zero byte counts
    elif pattern == "first":
        s[0] = 1
    elif pattern == "last":
        s[-1] = 255
    return s


class Device:
    """The device state of one normaliser: guarded statistics blocks, returns and scratch, and the numpy model next to it."""

    def __init__(self, widths, N, gamma=0.99, clip_obs=10.0, clip_reward=10.0, epsilon=1e-8):
        self.widths, self.N, self.gamma, self.clip_obs, self.clip_reward, self.epsilon = widths, N, gamma, clip_obs, clip_reward, epsilon
        init = lambda d: np.concatenate([np.zeros(d), np.ones(d), [1e-4]])   # noqa: E731
        self.stats = [Guarded((2 * d + 1) * 8, fill=init(d)) for d in widths]
        self.ret_stats = Guarded(24, fill=init(1))
        self.returns = Guarded(N * 8, fill=np.zeros(N))
        self.scratch = Guarded(2 * ((N + 255) // 256) * (sum(widths) + 1) * 8)
        self.model = ref.device_order(dict(enumerate(widths)), N, gamma=gamma, clip_obs=clip_obs, clip_reward=clip_reward, epsilon=epsilon)
        self.w_tab = (C.c_int32 * 4)(*widths)

    def update(self, xs, rewards=None):
        capi, L = _lib()
        rw = Guarded(self.N * 4, fill=rewards) if rewards is not None else None
        self.keep = [Guarded(x.nbytes, fill=x) for x in xs]
        p = C.c_void_p
        capi.check(L.tg_vecnorm_update(len(xs), _ptrs(self.keep), self.w_tab, _ptrs(self.stats), self.N, p(self.returns.ptr if rw else None),
                                       p(rw.ptr if rw else None), self.gamma, p(self.ret_stats.ptr if rw else None), p(self.scratch.ptr), _stream()))
        return rw

    def apply(self, xs, rows, rewards=None, dones=None, reset=False):
        """-> (outputs per array, rewards_out or None)"""
        capi, L = _lib()
        ins = [Guarded(x.nbytes, fill=x) for x in xs]
        outs = [Guarded(x.nbytes) for x in xs]
        rw = Guarded(rewards.nbytes, fill=rewards) if rewards is not None else None
        ro = Guarded(rewards.nbytes) if rewards is not None else None
        dn = Guarded(self.N, fill=dones) if dones is not None else None
        p = C.c_void_p
        capi.check(L.tg_vecnorm_apply(len(xs), _ptrs(ins), _ptrs(outs), self.w_tab, _ptrs(self.stats), rows, self.clip_obs, self.epsilon,
                                      p(rw.ptr if rw else None), p(ro.ptr if ro else None), rewards.size if rewards is not None else 0,
                                      p(self.ret_stats.ptr), self.clip_reward, p(self.returns.ptr if reset else None), p(dn.ptr if dn else None),
                                      self.N if reset else 0, _stream()))
        torch.cuda.synchronize()
        for g in ins + outs + [x for x in (rw, ro, dn) if x is not None]:
            assert g.guards_intact()
        return [o.host(np.float32).reshape(x.shape) for o, x in zip(outs, xs)], (ro.host(np.float32) if ro else None)

    def check(self, what):
        torch.cuda.synchronize()
        for i, (g, d) in enumerate(zip(self.stats, self.widths)):
            rms, got = self.model.obs_rms[i], g.host(np.float64)
            assert _bits(got[:d], rms.mean) and _bits(got[d:2 * d], rms.var) and got[2 * d] == rms.count, (what, i)
            assert g.guards_intact(), (what, i)
        got = self.ret_stats.host(np.float64)
        assert got[0] == self.model.ret_rms.mean and got[1] == self.model.ret_rms.var and got[2] == self.model.ret_rms.count, what
        assert _bits(self.returns.host(np.float64), self.model.returns), what
        assert self.ret_stats.guards_intact() and self.returns.guards_intact() and self.scratch.guards_intact(), what
