"""Guarded device buffers for the tests that call the C entry points on raw pointers (tests/test_gpu_augment_paths.py,
tests/test_gpu_rollout_abi.py, tests/test_gpu_vecnorm_abi.py, tests/test_gpu_stack_matrix.py): a payload at a chosen offset inside a larger allocation, with bytes of a known pattern in front of and behind it."""
import numpy as np
import torch

GUARD = 4096
PATTERN = 0xA5


class Guarded:
    """nbytes at `offset` past a 16-byte aligned address inside a flat uint8 device buffer, GUARD + offset bytes of PATTERN in front and
    GUARD behind."""

    def __init__(self, nbytes, offset=0, fill=None):
        self.front, self.nbytes = GUARD + offset, nbytes
        self.buf = torch.full((self.front + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.front
        if fill is not None:
            self.payload().copy_(torch.from_numpy(np.ascontiguousarray(fill).reshape(-1).view(np.uint8)))

    def payload(self):
        return self.buf[self.front:self.front + self.nbytes]

    def host(self, dtype):
        return self.payload().cpu().numpy().view(dtype)

    def guards_intact(self):
        return bool((self.buf[:self.front] == PATTERN).all()) and bool((self.buf[self.front + self.nbytes:] == PATTERN).all())
