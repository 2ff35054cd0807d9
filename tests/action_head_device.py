"""The device side of the action head's raw-pointer tests (tests/test_gpu_action_head_abi.py, tests/test_gpu_nonfinite.py): one tg_action_head
call on buffers between guard bytes, behind its memory checks."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from device_guard import PATTERN, Guarded  # noqa: E402

OUTPUTS = ("actions", "env", "gaussian", "log_prob", "noise")
f32 = np.float32


def _lib():
    from tactile_gym_amd import _capi
    return _capi, _capi.lib()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _bounds(A):
    j = np.arange(A)
    return (-0.25 - 0.1 * j).astype(f32), (0.3 + 0.2 * j).astype(f32)


def _call(mode, N, A, mean=None, log_std=None, lo=None, hi=None, clamp=(-np.inf, np.inf), deterministic=False, seed=0, counter=0, noise_in=None,
          outputs=OUTPUTS, stride=None, expect_error=False):
    """One tg_action_head call between guards -> {output name: host float32 array} (the outputs asked for)."""
    capi, L = _lib()
    if lo is None:
        lo, hi = _bounds(A)
    keep = {k: Guarded(v.nbytes, fill=v) for k, v in (("mean", mean), ("log_std", log_std), ("noise_in", noise_in)) if v is not None}
    outs = {k: Guarded(4 * N * (1 if k == "log_prob" else A)) for k in outputs}
    if stride is None:
        stride = A if (log_std is not None and log_std.ndim == 2) else 0
    p = lambda g: C.c_void_p(g.ptr if g is not None else None)   # noqa: E731
    rc = L.tg_action_head(p(keep.get("mean")), p(keep.get("log_std")), stride, N, A, (C.c_float * len(lo))(*lo.tolist()),
                          (C.c_float * len(hi))(*hi.tolist()), clamp[0], clamp[1], mode, 1 if deterministic else 0, seed, counter,
                          p(keep.get("noise_in")), p(outs.get("actions")), p(outs.get("env")), p(outs.get("gaussian")), p(outs.get("log_prob")),
                          p(outs.get("noise")), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for g in list(keep.values()) + list(outs.values()):
        assert g.guards_intact()
    if expect_error:
        assert rc != 0 and L.tg_last_error().decode().startswith("tg_action_head:")
        for k, g in outs.items():
            assert bool((g.payload() == PATTERN).all()), k                    # nothing was written
        return None
    capi.check(rc)
    return {k: g.host(f32).reshape((N,) if k == "log_prob" else (N, A)) for k, g in outs.items()}
