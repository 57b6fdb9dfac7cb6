#!/usr/bin/env python3
"""Per-symbol digest of a .hip file's gfx950 device code: python tools/kernel_digest.py FILE.hip [...] > digest.txt

Compiles each file device-only with build_native.py's flags, unbundles the code object and prints, per function
symbol, the SHA-256 of its code bytes in .text and, per kernel, the SHA-256 of its 64-byte .kd descriptor with the
entry-offset field (bytes 16-23) zeroed. Host-only edits move functions inside .text (template instantiation
order), which changes that field and the file hash but nothing printed here: `diff` of two outputs (two revisions of
one file) is empty exactly when the device code is the same. Raw bytes only, no disassembly."""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import build_native as bn  # noqa: E402

FLAGS = [f"--offload-arch={bn.ARCH}", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-mcode-object-version=5",
         "-Wno-unused-result", "-munsafe-fp-atomics", "--offload-device-only"]


def code_object(src, tmp):
    out = os.path.join(tmp, "dev.o")
    bn._run([bn.HIPCC] + FLAGS + ["-I", os.path.dirname(os.path.abspath(src)), "-c", src, "-o", out])
    if open(out, "rb").read(24) == b"__CLANG_OFFLOAD_BUNDLE__":
        co = os.path.join(tmp, "dev.co")
        bn._run([os.path.join(bn.ROCM, "llvm", "bin", "clang-offload-bundler"), "--unbundle", "--type=o",
                 f"--targets=hipv4-amdgcn-amd-amdhsa--{bn.ARCH}", f"--input={out}", f"--output={co}"])
        out = co
    return open(out, "rb").read()


def digest(elf):
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    # per section: type, addr, offset, size, link
    secs = [struct.unpack_from("<4xI8xQQQI", elf, shoff + i * shentsize) for i in range(shnum)]
    symtab = next(s for s in secs if s[0] == 2)
    strs = secs[symtab[4]]
    rows = []
    for o in range(symtab[2], symtab[2] + symtab[3], 24):
        name, info, shndx, value, size = struct.unpack_from("<IBxHQQ", elf, o)
        end = elf.index(b"\0", strs[2] + name)
        name = elf[strs[2] + name:end].decode()
        if shndx == 0 or shndx >= shnum or size == 0:
            continue
        at = secs[shndx][2] + value - secs[shndx][1]
        data = bytearray(elf[at:at + size])
        if name.endswith(".kd") and size == 64:
            data[16:24] = bytes(8)
        elif info & 15 != 2:     # STT_FUNC
            continue
        rows.append(f"{name} {size} {hashlib.sha256(data).hexdigest()}")
    return sorted(rows)


if __name__ == "__main__":
    for src in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            rows = digest(code_object(src, tmp))
        print(f"# {os.path.basename(src)}: {len(rows)} symbols")
        print("\n".join(rows))
