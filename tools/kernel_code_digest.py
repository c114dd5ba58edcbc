"""One line per device kernel of libddpm_ood_hip.so: what a refactor that must not touch kernel code is held to.
    python tools/kernel_code_digest.py [path/to/libddpm_ood_hip.so] > kernels.txt
Without a path it takes the in-tree library and builds it first if it is missing.  Two such lists, of a commit and of its parent,
compare with diff(1): a kernel whose body was not edited keeps its line.

Fields, tab-separated: demangled name; vgpr / agpr / sgpr counts, LDS bytes and scratch bytes from the code object's metadata;
instruction count; SHA-256 (first 16 hex digits) of the kernel function's instruction bytes.  The digest is taken over the
encoded instructions only -- not over the kernel descriptor or the argument metadata -- so it moves exactly when the machine code
does.  The tool compares nothing itself and looks at no particular instruction."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
LLVM = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def run(*cmd):
    return subprocess.run([str(c) for c in cmd], check=True, capture_output=True, text=True).stdout


def code_objects(lib: Path):
    """The gfx950 ELF of every translation unit: the library's .hip_fatbin is a row of offload bundles, one per unit."""
    blob = lib.read_bytes()
    at = blob.find(MAGIC)
    while at >= 0:
        (entries,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(entries):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + len(MAGIC))


def kernels_of(elf: Path):
    """Per kernel (by mangled name) its metadata entry, its demangled name and its instruction words."""
    meta, cur = {}, None
    for line in run(LLVM / "llvm-readelf", "--notes", elf).splitlines():
        m = re.match(r"\s+(- )?\.(\w+):\s+(\S+)$", line)
        if line.startswith("  - "):  # a new entry of amdhsa.kernels
            cur = {}
        if m and cur is not None and len(line) - len(line.lstrip()) <= 4:  # (the kernel's own keys, not those of .args)
            cur[m.group(2)] = m.group(3).strip("'")
            if m.group(2) == "name":
                meta[cur["name"]] = cur
    size = {}
    for line in run(LLVM / "llvm-readelf", "-sW", "--dyn-syms", elf).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = (int(f[1], 16), int(f[2]))
    pretty = {}
    for line in run(LLVM / "llvm-readelf", "-sW", "-C", "--dyn-syms", elf).splitlines():
        f = line.split(None, 7)
        if len(f) == 8 and f[3] == "FUNC":
            pretty[int(f[1], 16)] = f[7]
    for name, k in meta.items():
        k["pretty"] = pretty[size[name][0]]
    words, sym = {}, None
    for line in run(LLVM / "llvm-objdump", "-d", elf).splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym = m.group(1) if m.group(1) in size else sym
            continue
        m = re.search(r"// ([0-9A-F]{12}): ((?:[0-9A-F]{8} ?)+)$", line)
        if m and sym:
            lo, n = size[sym]
            if lo <= int(m.group(1), 16) < lo + n:  # (not the padding behind the function)
                words.setdefault(sym, []).append(m.group(2).strip())
    return meta, words


def main():
    lib = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "ddpm_ood_amd" / "libddpm_ood_hip.so"
    if len(sys.argv) == 1 and not lib.exists():
        subprocess.run(["bash", str(ROOT / "ddpm_ood_amd" / "csrc" / "build.sh")], check=True, stdout=sys.stderr)
    rows = []
    with tempfile.TemporaryDirectory() as t:
        tmp = Path(t)
        for i, co in enumerate(code_objects(lib)):
            elf = tmp / f"co{i}.elf"
            elf.write_bytes(co)
            meta, words = kernels_of(elf)
            for name, k in meta.items():
                w = words[name]
                digest = hashlib.sha256("\n".join(w).encode()).hexdigest()[:16]
                rows.append((k["pretty"], k["vgpr_count"], k["agpr_count"], k["sgpr_count"], k["group_segment_fixed_size"],
                             k["private_segment_fixed_size"], str(len(w)), digest))
    for r in sorted(rows):
        print("\t".join((r[0], f"vgpr={r[1]}", f"agpr={r[2]}", f"sgpr={r[3]}", f"lds={r[4]}", f"scratch={r[5]}", f"insts={r[6]}",
                         f"sha256={r[7]}")))


if __name__ == "__main__":
    main()
