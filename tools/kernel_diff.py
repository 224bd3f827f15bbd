#!/usr/bin/env python
"""Compare the gfx950 kernels of two versions of kernels.hip, per kernel.

    python tools/kernel_diff.py OLD/kernels.hip NEW/kernels.hip

Each file is compiled for the device alone with the flags of
acg_amd/ops/build.py, the gfx950 code object is unbundled, and for every
kernel symbol the tool compares a hash of the code bytes at the symbol and
the resource metadata of the code object's notes (VGPR / SGPR / AGPR
counts, scratch and LDS size).  No instruction is inspected.  Comparing
whole files does not work: a change in the order of instantiation reorders
.text while every kernel body stays the same.

Prints the kernels found in one file only, those whose code differs and
those whose metadata differs; exit status 0 only if all three are empty.
CPU only -- needs hipcc and its LLVM tools, no GPU.
"""

from __future__ import annotations

import hashlib
import re
import shutil
import struct
import subprocess
import sys
import sysconfig
import tempfile
from pathlib import Path

ARCH = "gfx950"
META = ("vgpr_count", "sgpr_count", "agpr_count",
        "private_segment_fixed_size", "group_segment_fixed_size")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name: str) -> str:
    if shutil.which("hipcc") is None:
        raise RuntimeError("hipcc is not on PATH")
    hipcc = Path(shutil.which("hipcc")).resolve()
    for d in (hipcc.parents[1] / "lib" / "llvm" / "bin", hipcc.parents[1] / "llvm" / "bin"):
        if (d / name).exists():
            return str(d / name)
    return name


def _run(cmd) -> str:
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f"{cmd[0]} failed:\n{r.stderr[-2000:]}")
    return r.stdout


def code_object(src: Path, tmp: Path) -> Path:
    """Device-only compile of ``src``; returns the gfx950 ELF."""
    import pybind11

    obj = tmp / "dev.o"
    _run(["hipcc", f"--offload-arch={ARCH}", "-O3", "-std=c++17",
          "--cuda-device-only", "-c", f"-I{pybind11.get_include()}",
          f"-I{sysconfig.get_paths()['include']}", str(src), "-o", str(obj)])
    if not obj.read_bytes().startswith(BUNDLE_MAGIC):
        return obj
    elf = tmp / "dev.elf"
    _run([_tool("clang-offload-bundler"), "--type=o", "--unbundle",
          f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}",
          f"--input={obj}", f"--output={elf}"])
    return elf


def code_hashes(elf: bytes) -> dict[str, str]:
    """sha256 of the bytes at every kernel symbol (a function symbol NAME
    that has a kernel descriptor NAME.kd)."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    # (name, type, flags, addr, offset, size, link, info, align, entsize)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize)
            for i in range(shnum)]
    symtab = next(s for s in secs if s[1] == 2)  # SHT_SYMTAB
    stroff = secs[symtab[6]][4]
    funcs, names = {}, set()
    for i in range(symtab[5] // 24):
        noff, info, _, shndx, value, size = struct.unpack_from(
            "<IBBHQQ", elf, symtab[4] + 24 * i)
        name = elf[stroff + noff:elf.index(b"\0", stroff + noff)].decode()
        names.add(name)
        if info & 0xF == 2 and 0 < shndx < 0xFF00:  # STT_FUNC, defined
            off = secs[shndx][4] + value - secs[shndx][3]
            funcs[name] = hashlib.sha256(elf[off:off + size]).hexdigest()
    return {n: h for n, h in funcs.items() if n + ".kd" in names}


def metadata(elf: Path) -> dict[str, dict[str, int]]:
    """Resource fields of every kernel in the AMDGPU metadata note."""
    out, cur, indent = {}, None, -1
    for line in _run([_tool("llvm-readobj"), "--notes", str(elf)]).splitlines():
        m = re.match(r"^(\s*)(- )?\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        lead, dash, key, val = m.groups()
        if dash and key == "agpr_count":  # first (sorted) key of a kernel entry
            cur, indent = {}, len(lead) + 2
        if cur is None or len(lead) + len(dash or "") != indent:
            continue
        if key == "name":
            out[val] = cur
        elif key in META:
            cur[key] = int(val)
    return out


def kernels(src: Path) -> dict[str, tuple[str, dict[str, int]]]:
    with tempfile.TemporaryDirectory() as tmp:
        elf = code_object(src, Path(tmp))
        code, meta = code_hashes(elf.read_bytes()), metadata(elf)
    if set(code) != set(meta):
        raise RuntimeError(f"{src}: symbols and metadata name different kernels: "
                           f"{sorted(set(code) ^ set(meta))[:5]}")
    return {n: (code[n], meta[n]) for n in code}


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    a, b = kernels(Path(argv[1])), kernels(Path(argv[2]))
    only = sorted(set(a) ^ set(b))
    both = sorted(set(a) & set(b))
    code = [n for n in both if a[n][0] != b[n][0]]
    meta = [n for n in both if a[n][1] != b[n][1]]
    print(f"kernels: {len(a)} vs {len(b)}, {len(both)} in both")
    for title, names in (("only in one file", only), ("code bytes differ", code),
                         ("resource metadata differs", meta)):
        print(f"{title}: {len(names)}")
        for n in names:
            where = "" if n in both else (" (first)" if n in a else " (second)")
            print(f"  {n}{where}")
    return 1 if (only or code or meta) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
