"""k_step_quad's register budget, read from the built library's gfx950 code objects (no GPU needed): no scratch memory.

The library's .hip_fatbin section holds one clang offload bundle per translation unit.  Each is unbundled with clang-offload-bundler, and the
kernel metadata (llvm-readelf --notes) gives every kernel's .private_segment_fixed_size: the bytes of scratch per lane."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tactile_gym_amd", "lib", "libtactile_gym_hip.so")
LLVM = "/opt/rocm/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else shutil.which(name)


def _kernel_scratch(tmp_path):
    """{kernel symbol: private segment bytes} over every gfx950 code object in the library."""
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
        # one metadata map per kernel: .name, ..., .private_segment_fixed_size, ... (key order as the compiler writes it: alphabetical)
        for block in re.split(r"\n\s*- \.", notes):
            name = re.search(r"\.name:\s+(\S+)", block)
            scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            if name and scratch:
                out[name.group(1)] = int(scratch.group(1))
    return out


def test_quad_step_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    scratch = _kernel_scratch(tmp_path)
    quad = {k: v for k, v in scratch.items() if "k_step_quad" in k}
    assert len(quad) == 2, sorted(scratch)[:20]          # k_step_quad<double, false> and <double, true>
    assert all(v == 0 for v in quad.values()), quad
