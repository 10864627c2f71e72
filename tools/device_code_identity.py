#!/usr/bin/env python3
"""Per-symbol identity of two device code objects (refactors that must not touch device code).

  hipcc <CXXFLAGS of csrc/Makefile> --cuda-device-only --no-gpu-bundle-output -c X.hip -o X.dev.o     (once per tree)
  python tools/device_code_identity.py parent/X.dev.o new/X.dev.o

Two builds of one source differ in .note / .dynsym, and a changed instantiation order permutes .text: so the bytes of every FUNC symbol and
of every kernel descriptor (OBJECT symbol *.kd) are compared by name.  A descriptor holds ONE position-dependent field, the 8 bytes at offset 16
(kernel_code_entry_byte_offset: entry address minus descriptor address), which moves with the kernel's place in .text: it is checked to
point at the FUNC symbol of the same name and left out of the descriptor's hash; the number of descriptors whose field moved is printed.  Prints the symbol counts, a sha256 over the sorted (name, sha256 of
the bytes) list of each side and the verdict; exit status 1 when they differ.  With --text only the hash of .text is compared (files that
were not edited)."""
import hashlib
import re
import subprocess
import sys

READELF = "/opt/rocm/llvm/bin/llvm-readelf"


def _sections(path):
    out = subprocess.run([READELF, "-SW", path], check=True, capture_output=True, text=True).stdout
    secs = {}
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S*)\s+(\S+)\s+([0-9a-f]{16})\s+([0-9a-f]{6,})\s+([0-9a-f]{6,})", out, re.M):
        secs[int(m.group(1))] = (m.group(2), int(m.group(4), 16), int(m.group(5), 16), int(m.group(6), 16))   # name, addr, offset, size
    return secs


def symbols(path):
    """{name: (type, sha256 of its bytes)} for FUNC symbols and *.kd objects."""
    secs, data = _sections(path), open(path, "rb").read()
    out = subprocess.run([READELF, "-sW", path], check=True, capture_output=True, text=True).stdout
    syms, where = {}, {}
    for line in out.splitlines():
        f = line.split()
        if len(f) < 8 or not f[0].rstrip(":").isdigit() or not f[6].isdigit():
            continue
        value, size, typ, ndx, name = int(f[1], 16), int(f[2], 0), f[3], int(f[6]), f[7]
        if not (typ == "FUNC" or (typ == "OBJECT" and name.endswith(".kd"))):
            continue
        _, addr, off, _ = secs[ndx]
        start = off + value - addr
        raw = data[start:start + size]
        where[name] = value
        if typ == "OBJECT":
            where[name] = value + int.from_bytes(raw[16:24], "little", signed=True)      # the entry it points at
            raw = raw[:16] + raw[24:]
        syms[name] = (typ, hashlib.sha256(raw).hexdigest(), data[start + 16:start + 24] if typ == "OBJECT" else b"")
    for name in syms:
        if name.endswith(".kd"):
            assert where[name] == where[name[:-3]], f"{name} does not point at its kernel"
    return syms


def text_hash(path):
    secs, data = _sections(path), open(path, "rb").read()
    for name, _, off, size in secs.values():
        if name == ".text":
            return hashlib.sha256(data[off:off + size]).hexdigest()
    return "no .text"


def list_hash(syms):
    return hashlib.sha256("\n".join(f"{n} {h}" for n, (_, h, _) in sorted(syms.items())).encode()).hexdigest()


def main(argv):
    if argv[0] == "--text":
        a, b = text_hash(argv[1]), text_hash(argv[2])
        print(f".text sha256 {a[:16]} / {b[:16]}: {'IDENTICAL' if a == b else 'DIFFERENT'}  ({argv[2]})")
        return int(a != b)
    a, b = symbols(argv[0]), symbols(argv[1])
    for side, s in (("parent", a), ("new", b)):
        print(f"{side}: {sum(v[0] == 'FUNC' for v in s.values())} FUNC + {sum(v[0] == 'OBJECT' for v in s.values())} .kd symbols, list sha256 {list_hash(s)}")
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(n for n in set(a) & set(b) if a[n][:2] != b[n][:2])
    moved = sum(a[n][2] != b[n][2] for n in set(a) & set(b))
    for tag, names in (("only in parent", only_a), ("only in new", only_b), ("bytes differ", differ)):
        for n in names:
            print(f"  {tag}: {n}")
    same = not (only_a or only_b or differ)
    print(f"descriptors whose entry offset moved (kernel at another place in .text; each still points at its own kernel): {moved}")
    print("verdict:", "IDENTICAL per symbol (same names, equal bytes)" if same else "DIFFERENT")
    return int(not same)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
