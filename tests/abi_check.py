"""The public headers under include/ against their ctypes bindings: one parser, one checker, written over the rows of _lib.ABIS.

A wrong argtype or field order is memory corruption, not an error, so every family's host test calls check_binding on its row and
check_families_apart on the whole registry.  A helper module like tests/guarded.py: no tests are collected from it."""
import ctypes as C
import os
import re
import shutil
import subprocess

import tav_amd  # noqa: F401
from tav_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

_SCALARS = {"int": "int32", "int32_t": "int32", "int64_t": "int64", "uint64_t": "uint64", "float": "float", "double": "double"}
_CTYPES = {C.c_int32: "int32", C.c_int64: "int64", C.c_uint64: "uint64", C.c_float: "float", C.c_double: "double"}
# Words of one family that the headers of the families before it must not carry (a family's entry points live in its own header).
_BANNED_BEFORE = {"tavhip_align.h": ("ctc",), "tavhip_rnn.h": ("lstm", "logsigmoid"), "tavhip_conv.h": ("conv3d", "flat_linear", "tav_sigmoid")}
_COUNTS = {"tavhip.h": 92, "tavhip_align.h": 5, "tavhip_rnn.h": 7, "tavhip_conv.h": 14}
_VERSIONS = {"tavhip.h": 7, "tavhip_align.h": 1, "tavhip_rnn.h": 1, "tavhip_conv.h": 1}


def abi(header):
    """The row of _lib.ABIS for a header."""
    return next(a for a in _lib.ABIS if a.header == header)


def header_text(name, comments=False):
    src = open(os.path.join(INCLUDE, name)).read()
    return src if comments else re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_names(src):
    """Every tav_* name followed by a parenthesis in a header's text (comments removed)."""
    return set(re.findall(r"\b(tav_[a-z0-9_]+)\s*\(", src))


def _c_class(decl):
    """Class of a C type as the header writes it: pointer, char*, int32, int64, uint64, float, double."""
    t = " ".join(decl.replace("const", " ").split())
    if "*" in t:
        return "char*" if t.replace(" ", "") == "char*" else "pointer"
    if t not in _SCALARS:
        raise ValueError(f"unknown C type {decl.strip()!r}")
    return _SCALARS[t]


def _ctypes_class(t):
    if t is C.c_char_p:
        return "char*"
    if t is C.c_void_p or hasattr(t, "contents") or isinstance(t, type(C.POINTER(C.c_int))):
        return "pointer"
    return _CTYPES[t]


def parse_header_text(src):
    """(structs, protos) of a header's text, comments removed.  structs: name -> [(field, class, array length or 0)]; protos: name ->
    (result class, [(argument class, pointed-to struct or None)]).  A declaration it cannot read raises ValueError."""
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.match(r"(.*?[\s\*])(\w+(?:\[\d+\])?(?:\s*,\s*\w+(?:\[\d+\])?)*)$", decl, flags=re.S)
            if not m:
                raise ValueError(f"{name}: cannot read the field declaration {decl!r}")
            for item in m.group(2).split(","):
                fname, _, dim = item.strip().partition("[")
                fields.append((fname, _c_class(m.group(1)), int(dim[:-1]) if dim else 0))
        structs[name] = fields
    if len(structs) != len(re.findall(r"\bstruct\b", src)):
        raise ValueError("a struct that is not `typedef struct [tag] { ... } name;`")
    protos = {}
    for res, name, args in re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(tav_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = [a.strip() for a in args.split(",")]
        kinds = []
        for a in ([] if args == ["void"] else args):
            m = re.match(r"(.*?[\s\*])(\w+)$", a, flags=re.S)             # type, then the parameter's name
            if not m:
                raise ValueError(f"{name}: cannot read the parameter {a!r}")
            kinds.append((_c_class(m.group(1)), next((s for s in structs if re.search(r"\b%s\b" % s, m.group(1))), None)))
        protos[name] = (_c_class(res), kinds)
    unread = declared_names(src) - set(protos)
    if unread:
        raise ValueError(f"cannot read the prototypes of {sorted(unread)}")
    return structs, protos


def parse_header(name):
    return parse_header_text(header_text(name))


def _laid_out(header, structs, tmp_path):
    """sizeof of every struct and offsetof of every field as a host C compiler lays them out: {"name": n, "name.field": n}."""
    cc = next((p for p in (shutil.which(c) for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang")) if p), None)
    assert cc is not None, "no host C compiler: the library was built here, so one exists"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', 'int main(void) {']
    for cname, fields in structs.items():
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _, _ in fields]
    lines += ['    return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", INCLUDE, str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def check_binding(abi, tmp_path, unbound=()):
    """One row of _lib.ABIS against its header: every prototype against abi.sigs (the same names, result class, arity, the class of every
    argument, which struct a struct pointer points to), every struct against its ctypes Structure (field names, order, classes, array
    lengths; sizeof / offsetof as a C compiler lays them out), the version function, and every name on the loaded library.  `unbound`
    names the structs that the header declares and the binding passes as an opaque pointer.  Returns the prototypes."""
    structs, protos = parse_header(abi.header)
    assert set(protos) == set(abi.sigs), set(protos) ^ set(abi.sigs)
    for name, (res, args) in protos.items():
        cres, cargs = abi.sigs[name]
        assert _ctypes_class(cres) == res, f"{name}: result {cres} vs {res}"
        assert len(cargs) == len(args), f"{name}: {len(cargs)} argtypes, {len(args)} parameters"
        for k, (ct, (kind, struct)) in enumerate(zip(cargs, args)):
            assert _ctypes_class(ct) == kind, f"{name}: argument {k} is {ct}, the header says {kind}"
            if struct in abi.structs:
                assert ct._type_ is abi.structs[struct], f"{name}: argument {k} points to {ct._type_}, the header says {struct}"
            else:
                assert struct is None or (struct in unbound and ct is C.c_void_p), f"{name}: argument {k} points to {struct}, which is not bound"
    assert set(structs) == set(abi.structs) | set(unbound) and set(abi.structs).isdisjoint(unbound), set(structs) ^ set(abi.structs)
    bound = {cname: structs[cname] for cname in abi.structs}
    for cname, cls in abi.structs.items():
        assert [f[0] for f in cls._fields_] == [f[0] for f in bound[cname]], cname
        for (fname, ct), (_, kind, dim) in zip(cls._fields_, bound[cname]):
            if dim:
                assert ct._length_ == dim and _ctypes_class(ct._type_) == kind, f"{cname}.{fname}"
            else:
                assert _ctypes_class(ct) == kind, f"{cname}.{fname}"
    laid = _laid_out(abi.header, bound, tmp_path)
    for cname, cls in abi.structs.items():
        assert C.sizeof(cls) == laid[cname], f"sizeof({cname})"
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == laid[f"{cname}.{f}"], f"offsetof({cname}, {f})"
    h = _lib.lib()
    assert getattr(h, abi.version_fn)() == abi.version == getattr(_lib, abi.version_const)
    for name in abi.sigs:
        assert hasattr(h, name), f"{name} declared in include/{abi.header} but not exported by libtavhip.so"
    return protos


def check_families_apart():
    """The families do not leak into each other: each header declares exactly the names of its own table, in the recorded numbers; the
    tables are pairwise disjoint; the versions, as constants and as the loaded library returns them, are the recorded ones; and no
    header carries the words of a family that came after it."""
    h = _lib.lib()
    assert [a.header for a in _lib.ABIS] == list(_COUNTS)
    assert _lib.ABIS[0].sigs is _lib._SIGS and set(_lib.declared_symbols()) == set(_lib._SIGS)
    for k, a in enumerate(_lib.ABIS):
        assert declared_names(header_text(a.header)) == set(a.sigs) and len(a.sigs) == _COUNTS[a.header], a.header
        assert a.version == getattr(_lib, a.version_const) == getattr(h, a.version_fn)() == _VERSIONS[a.header], a.header
        text = header_text(a.header, comments=True)
        for b in _lib.ABIS[k + 1:]:
            assert set(a.sigs).isdisjoint(b.sigs), (a.header, b.header)
            for word in _BANNED_BEFORE[b.header]:
                assert word not in text, f"{word!r} in include/{a.header}"
