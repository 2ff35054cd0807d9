"""Compare the gfx950 device code of two builds of libtactile_gym_hip.so kernel by kernel (no GPU needed).

    TG_OUT=/tmp/lib_a bash tactile_gym_amd/csrc/build.sh        # in a checkout of commit A
    TG_OUT=/tmp/lib_b bash tactile_gym_amd/csrc/build.sh        # in a checkout of commit B
    python tools/dev/compare_device_code.py /tmp/lib_a/libtactile_gym_hip.so /tmp/lib_b/libtactile_gym_hip.so

The library's .hip_fatbin section holds one clang offload bundle per translation unit (as tests/test_kstep_quad_resources_cpu.py reads it).
Per kernel (and per device function that is called, not inlined) it compares the machine code - the symbol's bytes in .text; where they differ,
the disassembly with every PC-relative reference to another symbol replaced by the symbol's name, since the order inside a code object may
differ - and the metadata of the kernel's note record (VGPRs, SGPRs, LDS, private segment, kernarg size, spills).  Prints the kernel count and "all identical", or the
kernels that differ; exit status 1 then.  For a host-only refactor: the two sets must be equal."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size",
        ".vgpr_spill_count", ".sgpr_spill_count", ".max_flat_workgroup_size", ".wavefront_size")


def tool(name):
    return os.path.join(LLVM, name)


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def code_objects(lib, tmp):
    fatbin = os.path.join(tmp, "fatbin")
    subprocess.run([tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fatbin}", lib, os.path.join(tmp, "stripped")], check=True)
    data = open(fatbin, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    for k, s in enumerate(starts):
        chunk, co = os.path.join(tmp, f"b{k}"), os.path.join(tmp, f"b{k}.co")
        open(chunk, "wb").write(data[s:starts[k + 1] if k + 1 < len(starts) else len(data)])
        r = subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={chunk}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--output={co}"], capture_output=True)
        if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co) > 0:
            yield co


def normalised(co, sym, symbols):
    """Disassembly of one function without addresses, the PC-relative address of another symbol (s_getpc_b64, then s_add_u32 / s_addc_u32 with the
    linker's displacement) replaced by that symbol's name: where a callee or a table sits in the code object does not matter"""
    lines = []
    for line in run(tool("llvm-objdump"), "-d", "--no-show-raw-insn", f"--disassemble-symbols={sym}", co).splitlines():
        m = re.match(r"\s+(\S.*?)\s+// ([0-9A-F]+):", line)
        if m:
            lines.append([m.group(1), int(m.group(2), 16)])
    for i, (ins, addr) in enumerate(lines):
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", ins)
        if not m:
            continue
        lo, hi, disp = f"s{m.group(1)}", f"s{m.group(2)}", [None, None]
        for j in range(i + 1, min(i + 4, len(lines))):
            for k, (op, reg) in enumerate((("s_add_u32", lo), ("s_addc_u32", hi))):
                mm = re.match(rf"{op} {reg}, {reg}, (0x[0-9a-f]+|-?\d+)$", lines[j][0])
                if mm:
                    disp[k] = (j, int(mm.group(1), 0) & 0xFFFFFFFF)
        if disp[0] and disp[1]:
            off = disp[0][1] | (disp[1][1] << 32)
            target = (addr + 4 + (off - (1 << 64) if off >> 63 else off)) & ((1 << 64) - 1)
            # (the low word's relocation is sym@rel32@lo + 4, taken at the literal 8 bytes behind the getpc: target = sym address exactly)
            if target not in symbols:   # a place inside this function (a long branch): the displacement is position independent, it stays
                continue
            name = symbols[target]
            lines[disp[0][0]][0] = f"s_add_u32 {lo}, {lo}, lo({name})"
            lines[disp[1][0]][0] = f"s_addc_u32 {hi}, {hi}, hi({name})"
    return [ins for ins, _ in lines]


def kernels(lib, tmp):
    """{function symbol: [(code bytes, normalised disassembly, metadata), ...]} over every gfx950 code object in the library: the kernels, and
    the device functions they call without inlining (no metadata).  The disassembly is filled in by main() only where the bytes differ."""
    out = {}
    for co in code_objects(lib, tmp):
        blob = open(co, "rb").read()
        text = None
        for line in run(tool("llvm-readelf"), "-S", "-W", co).splitlines():
            m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
            if m:
                text = (int(m.group(1), 16), int(m.group(2), 16))   # address, file offset
        meta = {}
        for block in re.split(r"\n\s*- \.", run(tool("llvm-readelf"), "--notes", co)):
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and ".private_segment_fixed_size" in block:
                meta[name.group(1)] = sorted((k, (re.search(re.escape(k) + r":\s+(\S+)", block) or [None, None])[1]) for k in META)
        seen, symbols = set(), {}                                   # (.dynsym and .symtab both list a kernel)
        table = [line.split() for line in run(tool("llvm-readelf"), "-s", "-W", co).splitlines()]
        for f in table:
            if len(f) == 8 and f[3] in ("FUNC", "OBJECT"):
                symbols.setdefault(int(f[1], 16), f[7])
        for f in table:
            if len(f) == 8 and f[3] == "FUNC" and f[7] not in seen:
                seen.add(f[7])
                off = text[1] + int(f[1], 16) - text[0]
                out.setdefault(f[7], []).append([blob[off:off + int(f[2])], (co, symbols), meta.get(f[7])])
    return {k: sorted(v, key=lambda e: e[0]) for k, v in out.items()}   # (a template kernel used by several translation units has a copy in each)


def main(a, b):
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:   # (the code objects stay until the disassembly below is done)
        return compare(a, b, kernels(a, ta), kernels(b, tb))


def compare(a, b, ka, kb):
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    diff_code, moved, diff_meta = [], [], []
    for k in sorted(set(ka) & set(kb)):
        if len(ka[k]) != len(kb[k]):
            diff_code.append(k)
            continue
        for (ca, (coa, sa), ma), (cb, (cob, sb), mb) in zip(ka[k], kb[k]):
            if ca != cb:
                same = len(ca) == len(cb) and normalised(coa, k, sa) == normalised(cob, k, sb)
                (moved if same else diff_code).append(k)
            if ma != mb:
                diff_meta.append(k)
    for lib, ks in ((a, ka), (b, kb)):
        n_k = sum(1 for v in ks.values() if v[0][2] is not None)
        print(f"{lib}: {n_k} kernels and {len(ks) - n_k} device functions, {sum(len(e[0]) for v in ks.values() for e in v)} bytes of code")
    for title, names in (("only in the first", only_a), ("only in the second", only_b), ("machine code differs", diff_code), ("metadata differs", diff_meta)):
        for k in names:
            print(f"{title}: {k}")
    if only_a or only_b or diff_code or diff_meta:
        return 1
    print(f"same symbols; metadata (VGPRs, SGPRs, AGPRs, LDS, private segment, kernarg size, spills) of every kernel identical; machine code byte-identical in "
          f"{len(set(ka)) - len(set(moved))} functions, and in {len(set(moved))} identical but for the PC-relative displacement to a symbol that sits elsewhere in the code "
          f"object (same instructions, same symbol)")
    for k in sorted(set(moved)):
        print(f"  displacement only: {k}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
