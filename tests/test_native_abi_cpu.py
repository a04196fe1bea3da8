"""The boundary between Python and the native libraries, held on CPU (the libraries load without
a GPU): the three plain-C headers under csrc/include/mp4x are the ABI, and

* each library's ctypes table (mp4x/ops/hip_sigs.py, mp4x/ops/host_sigs.py) names exactly the
  functions its headers declare, with the same return and argument kinds — a ``c_int`` where C
  takes ``int64_t``, or a dropped argument, fails here instead of corrupting a launch on the GPU;
* each built library exports exactly the declared functions (release, and the device-assert debug
  build where built);
* ``FastAr`` is laid out in ctypes as the host compiler lays out the C struct;
* the enums and error codes of ops.h equal their Python mirrors.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "csrc", "include")
HEADERS = {"hip": ("ops.h", "runtime.h"), "host": ("host.h",)}

# C type -> kind; a pointer of any type is "ptr".  Anything else fails the parse.
SCALARS = {"int": "int", "int64_t": "i64", "size_t": "size", "uint32_t": "u32", "uint64_t": "u64", "float": "f32",
           "double": "f64", "void": "void"}
CTYPES_KIND = {ctypes.c_int: "int", ctypes.c_int64: "i64", ctypes.c_size_t: "size", ctypes.c_uint32: "u32",
               ctypes.c_uint64: "u64", ctypes.c_float: "f32", ctypes.c_double: "f64", None: "void",
               ctypes.c_void_p: "ptr", ctypes.c_char_p: "ptr"}
# where size_t / uint64_t are one ctypes class, the table cannot tell them apart either
_ALIAS = {"size": "u64"} if ctypes.c_size_t is ctypes.c_uint64 else {}

_PROTO = re.compile(r"([\w\s\*]+?)\b(mp4x_\w+)\s*\(([^()]*)\)")


def _strip(text):
    """Header text without comments, preprocessor lines, the extern "C" wrapper, enums, struct
    bodies and typedefs: what is left is prototypes."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"\benum\b[^{;]*\{[^}]*\}\s*;", " ", text)
    text = re.sub(r"\btypedef\s+struct\b[^{;]*\{[^}]*\}[^;]*;", " ", text)
    text = re.sub(r"\btypedef\b[^{;]*;", " ", text)
    return text


def _kind(ctype):
    """Kind of one C type (a parameter with its name already removed)."""
    if "*" in ctype:
        return "ptr"
    words = [w for w in ctype.split() if w != "const"]
    if len(words) != 1 or words[0] not in SCALARS:
        raise ValueError(f"unknown C type {ctype!r}")
    return SCALARS[words[0]]


def parse_prototypes(text):
    """{name: (return kind, [argument kinds])} of a flat C header.  Every statement must be a
    prototype of an ``mp4x_`` function: anything the regex cannot read raises."""
    out = {}
    for stmt in _strip(text).split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):            # "}" closes the extern "C" wrapper
            continue
        m = _PROTO.fullmatch(stmt)
        if not m:
            raise ValueError(f"not a prototype: {stmt!r}")
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if name in out:
            raise ValueError(f"{name} declared twice")
        kinds = []
        if args != "void":
            for a in args.split(","):
                pm = re.fullmatch(r"(.*?)(\w+)", a.strip(), flags=re.S)
                if not pm or not pm.group(1).strip():
                    raise ValueError(f"{name}: parameter without a name or type: {a!r}")
                kinds.append(_kind(pm.group(1)))
        out[name] = (_kind(ret), kinds)
    if not out:
        raise ValueError("no prototype found")
    return out


def table_kinds(sigs):
    def kind(t):
        if t in CTYPES_KIND:
            return CTYPES_KIND[t]
        if isinstance(t, type) and issubclass(t, ctypes._Pointer):
            return "ptr"
        raise ValueError(f"ctypes type {t!r} has no C kind")
    return {name: (kind(res), [kind(a) for a in args]) for name, (res, args) in sigs.items()}


def mismatches(declared, table):
    """Every disagreement between a header's prototypes and a ctypes table, as readable lines."""
    norm = lambda sig: (_ALIAS.get(sig[0], sig[0]), [_ALIAS.get(k, k) for k in sig[1]])   # noqa: E731
    bad = [f"{n}: declared in the header, not in the ctypes table" for n in sorted(set(declared) - set(table))]
    bad += [f"{n}: in the ctypes table, not declared in the header" for n in sorted(set(table) - set(declared))]
    for n in sorted(set(declared) & set(table)):
        if norm(declared[n]) != norm(table[n]):
            bad.append(f"{n}: header {declared[n]} != ctypes {table[n]}")
    return bad


def _read(name):
    with open(os.path.join(INCLUDE, "mp4x", name)) as f:
        return f.read()


def _declared(lib):
    out = {}
    for h in HEADERS[lib]:
        protos = parse_prototypes(_read(h))
        dup = set(out) & set(protos)
        assert not dup, f"declared in two headers: {sorted(dup)}"
        out.update(protos)
    return out


def _table(lib):
    if lib == "hip":
        from mp4x.ops.hip_sigs import HIP_SIGS
        return HIP_SIGS
    from mp4x.ops.host_sigs import HOST_SIGS
    return HOST_SIGS


# ---------------------------------------------------------------- the parser itself
_GOOD = """
// a comment with a semicolon; and a prototype: int mp4x_not_this(int x);
#pragma once
extern "C" {
enum mp4x_kind { MP4X_A = 0, MP4X_B = 1, };
typedef struct mp4x_opaque mp4x_opaque;
typedef struct Box { const uint32_t* w[8]; int32_t a, b; mp4x_opaque* o; } Box;
int mp4x_f(int a, int64_t n, const void* const* ins, float s, void* stream);
size_t mp4x_g(void);
/* block comment */ void mp4x_h(const Box* b, double t,
                                uint32_t e);
}
"""


def test_parser_reads_the_flat_style():
    assert parse_prototypes(_GOOD) == {"mp4x_f": ("int", ["int", "i64", "ptr", "f32", "ptr"]), "mp4x_g": ("size", []),
                                       "mp4x_h": ("void", ["ptr", "f64", "u32"])}


def test_parser_catches_a_wrong_type_and_a_missing_name():
    declared = parse_prototypes(_GOOD)
    good = {"mp4x_f": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p), ctypes.c_float,
                                      ctypes.c_void_p]),
            "mp4x_g": (ctypes.c_size_t, []),
            "mp4x_h": (None, [ctypes.c_void_p, ctypes.c_double, ctypes.c_uint32])}
    assert mismatches(declared, table_kinds(good)) == []
    narrow = dict(good, mp4x_f=(ctypes.c_int, [ctypes.c_int, ctypes.c_int, *good["mp4x_f"][1][2:]]))
    assert [m.split(":")[0] for m in mismatches(declared, table_kinds(narrow))] == ["mp4x_f"]
    dropped = dict(good, mp4x_h=(None, good["mp4x_h"][1][:-1]))
    assert [m.split(":")[0] for m in mismatches(declared, table_kinds(dropped))] == ["mp4x_h"]
    missing = {k: v for k, v in good.items() if k != "mp4x_g"}
    assert mismatches(declared, table_kinds(missing)) == ["mp4x_g: declared in the header, not in the ctypes table"]
    extra = dict(good, mp4x_x=(ctypes.c_int, []))
    assert mismatches(declared, table_kinds(extra)) == ["mp4x_x: in the ctypes table, not declared in the header"]


@pytest.mark.parametrize("text", [
    "int mp4x_f(long n);",                       # a C type outside the ABI's vocabulary
    "int mp4x_f(int);",                          # a parameter without a name
    "int mp4x_f(int (*cb)(int), void* s);",      # a function-pointer parameter
    "MP4X_API int mp4x_f(int a)\nint mp4x_g(int b);",   # a macro / a missing `;` between prototypes
    "int mp4x_f(int a); int mp4x_f(int a);",     # declared twice
    "static int helper(int a);",                 # not an mp4x_ entry point
    "// int mp4x_f(int a);",                     # matches nothing at all
])
def test_parser_refuses_what_it_cannot_read(text):
    with pytest.raises(ValueError):
        parse_prototypes(text)


# ---------------------------------------------------------------- headers <-> ctypes tables
@pytest.mark.parametrize("lib", ["hip", "host"])
def test_ctypes_table_equals_the_headers(lib):
    bad = mismatches(_declared(lib), table_kinds(_table(lib)))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- headers <-> built libraries
def _lib_path(lib, debug=False):
    from mp4x.ops import native
    if lib == "host":
        return native.HOST_LIB
    rel = os.path.join(native.NATIVE_DIR, "libmp4x_hip.so")
    return rel.replace("libmp4x_hip.so", "libmp4x_hip_debug.so") if debug else rel


@pytest.mark.parametrize("debug", [False, True])
def test_every_bound_symbol_exists(debug):
    """Every bound symbol exists in the release library and, where built, in the debug library."""
    pytest.importorskip("torch")       # libmp4x_hip.so resolves the HIP runtime torch ships
    path = _lib_path("hip", debug)
    if not os.path.exists(path):
        pytest.skip(f"{path} not built")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    missing = sorted(k for k in _table("hip") if not hasattr(lib, k))
    assert not missing, f"{os.path.basename(path)} lacks {missing}"


def test_every_bound_host_symbol_exists():
    path = _lib_path("host")
    if not os.path.exists(path):
        pytest.skip(f"{path} not built")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    missing = sorted(k for k in _table("host") if not hasattr(lib, k))
    assert not missing, f"{os.path.basename(path)} lacks {missing}"


@pytest.mark.parametrize("lib,debug", [("hip", False), ("hip", True), ("host", False)])
def test_library_exports_exactly_the_declared_functions(lib, debug):
    path = _lib_path(lib, debug)
    if not os.path.exists(path):
        pytest.skip(f"{path} not built")
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm on this machine: undeclared exports are not checked here (that every declared "
                    "function exists is test_every_bound_*_symbol_exists, through the tables)")
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("mp4x_")}
    declared = set(_declared(lib))
    assert exported == declared, (f"exported but not declared: {sorted(exported - declared)}; "
                                  f"declared but not exported: {sorted(declared - exported)}")


# ---------------------------------------------------------------- FastAr
_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mp4x/runtime.h"
#define F(f) printf(#f " %zu\n", offsetof(FastAr, f))
int main(void) {
  printf("sizeof %zu\n", sizeof(FastAr));
  F(herr); F(epoch); F(data_ptrs); F(signal_ptrs); F(rank); F(p); F(slot_base); F(slot_vecs); F(order); F(own_err);
  return 0;
}
"""


def test_fastar_layout_equals_the_c_struct(tmp_path):
    from mp4x.parallel.ipc import FastAr
    cc = next((c for c in ("cc", "gcc", "clang", "g++") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host compiler")
    src = tmp_path / "fastar_layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "fastar_layout"
    subprocess.run([cc, "-x", "c", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    c_layout = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    py_layout = {"sizeof": ctypes.sizeof(FastAr)}
    py_layout.update({name: getattr(FastAr, name).offset for name, _ in FastAr._fields_})
    assert py_layout == c_layout
    # the struct text names the same fields in the same order (the program above cannot see a
    # field it was not told about)
    body = re.search(r"typedef\s+struct\s+FastAr\s*\{(.*?)\}\s*FastAr\s*;", _strip_comments(_read("runtime.h")), re.S)
    names = [n for decl in body.group(1).split(";") if decl.strip()
             for n in re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == [name for name, _ in FastAr._fields_]


def _strip_comments(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


# ---------------------------------------------------------------- enums and codes
def _enums(text):
    """{enum name or "": {enumerator: value}} of a header (explicit values only)."""
    out = {}
    for m in re.finditer(r"\benum\b\s*(\w*)\s*\{([^}]*)\}", _strip_comments(text)):
        items = [i.strip() for i in m.group(2).split(",") if i.strip()]
        out.setdefault(m.group(1), {}).update({k.strip(): int(v) for k, v in (i.split("=") for i in items)})
    return out


def test_enums_and_error_codes_equal_their_python_mirrors():
    from mp4x import operators
    from mp4x.ops import native
    from mp4x.parallel import sparse
    e = _enums(_read("ops.h"))
    assert {k[len("MP4X_"):]: v for k, v in e["mp4x_dtype"].items()} == {m.name: int(m) for m in operators.DType}
    # MP4X_FIRST is no operator of the reference's table (operators.OpCode): the sparse map merge
    # alone passes it
    py_ops = {m.name: int(m) for m in operators.OpCode}
    py_ops["FIRST"] = sparse.OP_FIRST
    assert {k[len("MP4X_"):]: v for k, v in e["mp4x_op"].items()} == py_ops
    py_codes = {k: v for k, v in vars(native).items() if k.startswith("E_")}
    assert {k[len("MP4X_"):]: v for k, v in e[""].items()} == py_codes and len(py_codes) == 5
    for code, msg in ((native.E_BADARG, "bad argument"), (native.E_UNSUPPORTED, "unsupported")):
        with pytest.raises(native.NativeError, match=msg):
            native.check(code, "x")
    from mp4x.ops import device_ops
    assert int(re.search(r"^#define MP4X_MAX_NIN (\d+)$", _read("ops.h"), re.M).group(1)) == device_ops.MAX_NIN
