"""capi/_abi.py against include/aos2.h, without a device and without the built library: one C program, generated from _abi and compiled
with the host C compiler against the header, prints sizeof and offsetof of every field of every mirrored struct and the value of every
mirrored constant; they have to equal ctypes', the numpy record dtypes' and Python's.  The header's own text gives the order of the
fields, the set of structs and the prototype of every function (count and kind of the parameters, kind of the return value)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_capi_cpu import declared_symbols  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def abi(pkg):
    return pkg.capi._abi


@pytest.fixture(scope="module")
def header():
    """the header without comments, preprocessor lines and the extern "C" brace"""
    src = open(os.path.join(INCLUDE, "aos2.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"(?m)^\s*#.*$", "", src)
    return src.replace('extern "C" {', "")


def header_structs(header):
    """C type -> field names in order, of every `typedef struct { ... } aos2_*_t;`"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(aos2_\w+_t)\s*;", header, flags=re.S):
        assert name not in out, name
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                for part in decl.split(","):
                    fields.append(re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", part.strip()).group(1))
        out[name] = fields
    return out


def c_kind(text, named):
    """kind of a C return type or of a parameter declaration (`named`: its last word is the parameter's name)"""
    if "*" in text or "[" in text:
        return "pointer"
    words = [w for w in text.split() if w != "const"]
    if named and len(words) > 1:
        words = words[:-1]
    for names, kind in ((("size_t",), "size_t"), (("int64_t", "uint64_t"), "int64"), (("int", "int32_t", "uint32_t", "unsigned"), "int32"),
                        (("float",), "float"), (("double",), "double"), (("void",), "void")):
        if any(w in names for w in words):
            return kind
    raise AssertionError("unknown C type: %r" % text)


def header_prototypes(header):
    """function -> (kind of the return value, kinds of the parameters)"""
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*aos2_\w+_t\s*;", ";", header, flags=re.S)
    out = {}
    for stmt in text.split(";"):
        m = re.match(r"\s*([\w\s\*]+?)\b(aos2_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if not m:
            assert "(" not in stmt, stmt   # no statement with a parameter list escapes the expression
            continue
        ret, name, params = m.groups()
        assert name not in out and "(" not in params, name
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        out[name] = (c_kind(ret, False), [c_kind(p, True) for p in params])
    return out


def ctypes_kind(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    return {C.c_int: "int32", C.c_uint: "int32", C.c_int64: "int64", C.c_size_t: "size_t", C.c_float: "float", C.c_double: "double"}[t]


@pytest.fixture(scope="module")
def measured(abi, tmp_path_factory):
    """what the C compiler says: (("S", type) -> size, ("F", type, field) -> (offset, size), ("C", macro) -> value)"""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "aos2.h"', "int main(void) {"]
    layouts = [(s._c_name_, [abi.RENAMED_FIELDS.get(f[0], f[0]) for f in s._fields_]) for s in abi.STRUCTS]
    layouts += [(name, list(dt.names)) for name, dt in abi.RECORD_DTYPES.items()]
    for name, fields in layouts:
        lines.append('printf("S %s %%zu\\n", sizeof(%s));' % (name, name))
        for f in fields:
            lines.append('printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f))
    for macro in abi.CONSTANTS:
        lines.append('printf("C %s %%lld\\n", (long long)(%s));' % (macro, macro))
    lines += ["return 0;", "}"]
    d = tmp_path_factory.mktemp("layout")
    (d / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", INCLUDE, "-o", str(d / "layout"), str(d / "layout.c")], check=True)
    out = {}
    for row in subprocess.run([str(d / "layout")], check=True, capture_output=True, text=True).stdout.split("\n"):
        w = row.split()
        if w:
            out[tuple(w[:{"S": 2, "F": 3, "C": 2}[w[0]]])] = tuple(int(x) for x in w[{"S": 2, "F": 3, "C": 2}[w[0]]:])
    return out


def test_every_struct_of_the_header_is_declared_once_with_its_fields_in_order(abi, header):
    want = header_structs(header)
    declared = [s._c_name_ for s in abi.STRUCTS] + list(abi.RECORD_DTYPES)
    assert sorted(declared) == sorted(want) and len(set(declared)) == len(declared)
    assert abi.RENAMED_FIELDS == {"lam": "lambda"}
    for s in abi.STRUCTS:
        assert [abi.RENAMED_FIELDS.get(f[0], f[0]) for f in s._fields_] == want[s._c_name_], s._c_name_
    for name, dt in abi.RECORD_DTYPES.items():
        assert list(dt.names) == want[name], name


def test_sizes_and_offsets_equal_the_compilers(abi, measured):
    n_fields = 0
    for s in abi.STRUCTS:
        assert measured["S", s._c_name_] == (C.sizeof(s),), s._c_name_
        for f in s._fields_:
            d = getattr(s, f[0])
            assert measured["F", s._c_name_, abi.RENAMED_FIELDS.get(f[0], f[0])] == (d.offset, d.size), (s._c_name_, f[0])
            n_fields += 1
    for name, dt in abi.RECORD_DTYPES.items():
        assert measured["S", name] == (dt.itemsize,), name
        for f in dt.names:
            assert measured["F", name, f] == (dt.fields[f][1], dt.fields[f][0].itemsize), (name, f)
            n_fields += 1
    assert n_fields == sum(k[0] == "F" for k in measured) > 600


def test_constants_equal_the_headers(abi, measured):
    assert len(abi.CONSTANTS) >= 45
    for macro, value in abi.CONSTANTS.items():
        assert measured["C", macro] == (value,), macro


def test_prototypes_equal_the_headers(abi, header):
    want = header_prototypes(header)
    assert sorted(want) == declared_symbols()   # (233 today) a prototype that the expression misses shows here
    assert sorted(abi.PROTOTYPES) == sorted(want)
    for name, (restype, argtypes) in abi.PROTOTYPES.items():
        assert (ctypes_kind(restype), [ctypes_kind(t) for t in argtypes]) == want[name], name
