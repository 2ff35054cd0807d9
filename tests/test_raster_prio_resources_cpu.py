"""Register budgets of the two kernels of the headline step, read from the built library's gfx950 code objects (no GPU needed), as
tests/test_kstep_quad_resources_cpu.py reads them; here the vector register counts too (.vgpr_count of the kernel metadata).

k_render_blocks<16> runs four wavefronts per SIMD (its front end at raised issue priority, TG_BLK_PRIO): no scratch and at most 96 VGPRs.
k_step_quad<double, true / false> fills the register file of its SIMD lane nearly to the brim: no scratch and no more than the 504 / 490
VGPRs it has (taking tg_step_random's election ticket right behind the draws was measured at 505 / 492 and is not in the tree)."""
import os
import re
import subprocess

import pytest

from test_kstep_quad_resources_cpu import LIB, MAGIC, _tool


def _kernel_resources(tmp_path):
    """{kernel symbol: (private segment bytes, VGPRs)} over every gfx950 code object in the library."""
    objcopy, bundler, readelf = _tool("llvm-objcopy"), _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not (objcopy and bundler and readelf):
        pytest.skip("LLVM tools of the ROCm install not found")
    fatbin = tmp_path / "fatbin"
    subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fatbin}", LIB, str(tmp_path / "stripped")], check=True)
    data = fatbin.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = {}
    for k, s in enumerate(starts):
        chunk = tmp_path / f"b{k}"
        chunk.write_bytes(data[s:starts[k + 1] if k + 1 < len(starts) else len(data)])
        co = tmp_path / f"b{k}.co"
        r = subprocess.run([bundler, "--unbundle", "--type=o", f"--input={chunk}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"],
                           capture_output=True)
        if r.returncode != 0 or not co.exists() or co.stat().st_size == 0:
            continue
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n\s*- \.", notes):
            name = re.search(r"\.name:\s+(\S+)", block)
            scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            vgprs = re.search(r"\.vgpr_count:\s+(\d+)", block)
            if name and scratch and vgprs:
                out[name.group(1)] = (int(scratch.group(1)), int(vgprs.group(1)))
    return out


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    return _kernel_resources(tmp_path_factory.mktemp("co"))


def test_block_raster_has_no_scratch_and_at_most_96_vgprs(resources):
    blocks = {k: v for k, v in resources.items() if "k_render_blocks" in k}
    assert len(blocks) == 1, sorted(resources)[:20]          # k_render_blocks<16>
    (scratch, vgprs), = blocks.values()
    assert scratch == 0 and vgprs <= 96, blocks


def test_quad_step_kernels_have_no_scratch_and_at_most_504_and_490_vgprs(resources):
    quad = {k: v for k, v in resources.items() if "k_step_quad" in k}
    assert len(quad) == 2, sorted(resources)[:20]
    limits = {"Lb1E": 504, "Lb0E": 490}                      # <double, true> (the in-step reset), <double, false>
    for name, (scratch, vgprs) in quad.items():
        limit, = [v for k, v in limits.items() if f"IdLb{k[2]}E" in name]
        assert scratch == 0 and vgprs <= limit, (name, scratch, vgprs, limit)
