"""k_render_blocks' register budget, read from the built library's gfx950 code object (no GPU needed): no scratch memory.  The kernel runs
four wavefronts per SIMD; step 4 (one whole block per wavefront, the next block's inputs fetched ahead) must fit its registers without a
spill to scratch.  The code object is read as tests/test_kstep_quad_resources_cpu.py reads it."""
import os

import pytest

from test_kstep_quad_resources_cpu import LIB, _kernel_scratch


def test_block_raster_uses_no_scratch(tmp_path):
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    scratch = _kernel_scratch(tmp_path)
    blocks = {k: v for k, v in scratch.items() if "k_render_blocks" in k}
    assert len(blocks) == 1, sorted(scratch)[:20]          # k_render_blocks<16>
    assert all(v == 0 for v in blocks.values()), blocks
