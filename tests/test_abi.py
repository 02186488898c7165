"""CPU (-m "not gpu"): the C ABI of libgmamd.so is written down twice -- include/gm_amd.h (which the kernels themselves compile against, csrc/gm_common.h) and
the ctypes mirror generativemodels_amd/_native.py -- and these tests hold the two to each other: the export list, every struct's layout as a C compiler lays
the header out, every field's and every argument's type, the limits ops.py repeats, and that no kernel file declares a symbol by hand any more.
No compute call is made -- there is no GPU here."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from generativemodels_amd import _build, _native, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "generativemodels_amd", "csrc")

SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double, "unsigned": ctypes.c_uint,
           "unsigned int": ctypes.c_uint, "unsigned char": ctypes.c_ubyte, "char": ctypes.c_char}
_BASE = r"(?:const\s+)?(?:unsigned char|unsigned int|unsigned|long long|int|float|double|void|char|Gm\w+)\b"
_PTRS = r"(?:\*\s*(?:const\b\s*)?)*"


# ---- the header, parsed --------------------------------------------------------------------------------------------------------------------------
def _header_source():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "gm_amd.h")).read(), flags=re.S)


def _header_functions():
    return sorted(set(re.findall(r"\b(gm_[a-z0-9_]+)\s*\(", _header_source())))


def _header_structs():
    """name -> [(field, base type, pointer depth, array length or None)] in declaration order, for every `typedef struct` of the header."""
    out = {}
    for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", _header_source(), flags=re.S):
        fields = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            m = re.match(r"(%s)\s*(.*)$" % _BASE, stmt, flags=re.S)
            assert m, (name, stmt)
            base = re.sub(r"^const\s+", "", m.group(1))
            for decl in m.group(2).split(","):
                d = re.fullmatch(r"\s*(%s)\s*(\w+)\s*(?:\[(\d+)\])?\s*" % _PTRS, decl)
                assert d, (name, stmt, decl)
                fields.append((d.group(2), base, d.group(1).count("*"), int(d.group(3)) if d.group(3) else None))
        out[name] = fields
    return out


def _header_prototypes():
    """name -> (return (base, pointer depth), [(base, pointer depth) per argument]) for every function the header declares."""
    src = re.sub(r"typedef struct (\w+) \{.*?\} \1;", "", _header_source(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M).replace('extern "C" {', "")
    out = {}
    for stmt in filter(None, (s.strip() for s in src.split(";"))):
        if stmt == "}":  # the closing brace of the extern "C" block
            continue
        m = re.fullmatch(r"(%s)\s*(%s)\s*(gm_\w+)\s*\((.*)\)" % (_BASE, _PTRS), stmt, flags=re.S)
        assert m, "not a prototype: %r" % stmt
        args = []
        if m.group(4).strip() not in ("", "void"):
            for a in m.group(4).split(","):
                d = re.fullmatch(r"\s*(%s)\s*(%s)\s*\w+\s*" % (_BASE, _PTRS), a, flags=re.S)
                assert d, (m.group(3), a)
                args.append((re.sub(r"^const\s+", "", d.group(1)), d.group(2).count("*")))
        assert m.group(3) not in out, m.group(3)
        out[m.group(3)] = ((re.sub(r"^const\s+", "", m.group(1)), m.group(2).count("*")), args)
    return out


# ---- the comparisons: each returns the list of disagreements it found ---------------------------------------------------------------------------
def _allowed(base, nptr, classes):
    """The ctypes types that may stand for the C type `base` + nptr stars."""
    if nptr == 0:
        return {SCALARS[base]}
    if base.startswith("Gm"):
        assert nptr == 1, base
        return {ctypes.POINTER(classes[base])}
    ok = {ctypes.c_void_p}
    if nptr > 1 or base != "void":  # ... or a typed pointer to what it points at
        ok |= {ctypes.POINTER(t) for t in _allowed(base, nptr - 1, classes)}
    return ok


def _prototype_problems(header, mirror, classes):
    bad = []
    for name in sorted(set(header) | set(mirror)):
        if name not in header or name not in mirror:
            bad.append(f"{name}: declared on one side only")
            continue
        (rbase, rptr), hargs = header[name]
        res, args = mirror[name]
        want = {None} if (rbase, rptr) == ("void", 0) else {ctypes.c_char_p} if (rbase, rptr) == ("char", 1) else _allowed(rbase, rptr, classes)
        if res not in want:
            bad.append(f"{name}: restype {res} for {rbase}{'*' * rptr}")
        if len(args) != len(hargs):
            bad.append(f"{name}: {len(args)} argtypes for {len(hargs)} parameters")
            continue
        for i, ((base, nptr), got) in enumerate(zip(hargs, args)):
            if got not in _allowed(base, nptr, classes):
                bad.append(f"{name}: argument {i} is {got} for {base}{'*' * nptr}")
    return bad


def _field_type_problems(structs, classes):
    bad = []
    for name, fields in structs.items():
        mirror = classes[name]._fields_
        if [f[0] for f in fields] != [f[0] for f in mirror]:
            bad.append(f"{name}: field names {[f[0] for f in mirror]} for {[f[0] for f in fields]}")
            continue
        for (fname, base, nptr, length), (_, got) in zip(fields, mirror):
            if length is not None:
                if getattr(got, "_length_", None) != length:
                    bad.append(f"{name}.{fname}: not an array of {length}")
                    continue
                got = got._type_
            if got not in _allowed(base, nptr, classes):
                bad.append(f"{name}.{fname}: {got} for {base}{'*' * nptr}")
    return bad


def _layout_problems(compiled, classes):
    """compiled: name -> (sizeof, [(field, offsetof, sizeof field)]) as the C compiler sees the header."""
    bad = []
    for name, (size, fields) in compiled.items():
        cls = classes[name]
        if ctypes.sizeof(cls) != size:
            bad.append(f"{name}: sizeof {ctypes.sizeof(cls)} for {size}")
        if [f[0] for f in fields] != [f[0] for f in cls._fields_]:
            bad.append(f"{name}: field names differ")
            continue
        for fname, off, fsize in fields:
            d = getattr(cls, fname)
            if (d.offset, d.size) != (off, fsize):
                bad.append(f"{name}.{fname}: offset {d.offset} size {d.size} for offset {off} size {fsize}")
    return bad


def _native_classes():
    return {n: c for n, c in vars(_native).items() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure}


def _c_compiler():
    """The host C compiler, else the clang of the ROCm installation hipcc belongs to."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    for cand in (os.environ.get("CC"), "cc", "gcc", "clang", os.path.join(rocm, "lib", "llvm", "bin", "clang"), os.path.join(rocm, "llvm", "bin", "clang")):
        path = cand and shutil.which(cand)
        if path:
            return path
    pytest.fail("no C compiler (cc, gcc, clang, ROCm's clang): the header's layout cannot be checked")


@pytest.fixture(scope="module")
def compiled_layout(tmp_path_factory):
    """sizeof / offsetof of every struct and field of gm_amd.h, printed by a C99 program generated from the header's struct list."""
    structs = _header_structs()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "gm_amd.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append(f'  printf("S {name} %lu\\n", (unsigned long)sizeof({name}));')
        for fname, *_ in fields:
            lines.append(f'  printf("F {name} {fname} %lu %lu\\n", (unsigned long)offsetof({name}, {fname}), (unsigned long)sizeof((({name}*)0)->{fname}));')
    lines += ["  return 0;", "}", ""]
    d = tmp_path_factory.mktemp("abi")
    (d / "layout.c").write_text("\n".join(lines))
    r = subprocess.run([_c_compiler(), "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", INCLUDE, str(d / "layout.c"), "-o", str(d / "layout")],
                       capture_output=True, text=True)
    assert r.returncode == 0, "include/gm_amd.h is not valid C99:\n" + r.stderr
    out = subprocess.run([str(d / "layout")], capture_output=True, text=True, check=True).stdout
    compiled = {}
    for line in out.splitlines():
        kind, name, *rest = line.split()
        if kind == "S":
            compiled[name] = (int(rest[0]), [])
        else:
            compiled[name][1].append((rest[0], int(rest[1]), int(rest[2])))
    return compiled


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_every_declared_symbol():
    path = _build.build_native()
    assert os.path.exists(path)
    handle = ctypes.CDLL(path)
    names = _header_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(handle, n), f"{n} declared in include/gm_amd.h but not exported by libgmamd.so"


def test_ctypes_prototypes_cover_the_header():
    assert sorted(_native.PROTOTYPES.keys()) == _header_functions()
    lib = _native.lib()
    assert lib.gm_abi_version() == 2


def test_struct_layouts_match_the_compiled_header(compiled_layout):
    structs, classes = _header_structs(), _native_classes()
    assert len(structs) == 12 and set(structs) == set(classes) == set(compiled_layout)  # nothing left out, on either side
    assert all(len(compiled_layout[n][1]) == len(structs[n]) > 0 for n in structs)
    assert _layout_problems(compiled_layout, classes) == []
    assert _field_type_problems(structs, classes) == []


def test_ctypes_prototypes_match_the_header_argument_by_argument():
    header = _header_prototypes()
    assert sorted(header) == _header_functions() == sorted(_native.PROTOTYPES)  # every prototype was parsed; nothing left out
    assert _prototype_problems(header, _native.PROTOTYPES, _native_classes()) == []


def test_the_checkers_report_a_doctored_prototype_and_a_doctored_field(compiled_layout):
    """A checker that matches nothing must not pass: one argument and one field changed on the ctypes side, each reported exactly once."""
    header, classes = _header_prototypes(), _native_classes()
    res, args = _native.PROTOTYPES["gm_gn_workspace_bytes"]
    assert args[0] is ctypes.c_int
    doctored = dict(_native.PROTOTYPES, gm_gn_workspace_bytes=(res, [ctypes.c_longlong] + args[1:]))
    assert _prototype_problems(header, doctored, classes) == ["gm_gn_workspace_bytes: argument 0 is %s for int" % ctypes.c_longlong]
    assert len(_prototype_problems(header, dict(doctored, gm_last_error=(ctypes.c_void_p, [])), classes)) == 2  # ... and a return type

    def with_field(cls, field, ftype):
        return type(cls.__name__, (ctypes.Structure,), {"_fields_": [(n, ftype if n == field else t) for n, t in cls._fields_]})

    wide = dict(classes, GmGnTables=with_field(_native.GmGnTables, "eps", ctypes.c_double))  # moves `groups` and grows the struct
    bad = _layout_problems(compiled_layout, wide)
    assert bad and all(b.startswith("GmGnTables") for b in bad) and any(b.startswith("GmGnTables.eps:") for b in bad)
    same_size = dict(classes, GmGnTables=with_field(_native.GmGnTables, "eps", ctypes.c_int))  # same layout, wrong type: the type check's to find
    # (GmRowsDesc.gn points at GmGnTables: the doctored set stays consistent, so that the one doctored field is the one report)
    same_size["GmRowsDesc"] = with_field(_native.GmRowsDesc, "gn", ctypes.POINTER(same_size["GmGnTables"]))
    assert _layout_problems(compiled_layout, same_size) == []
    assert _field_type_problems(_header_structs(), same_size) == ["GmGnTables.eps: %s for float" % ctypes.c_int]
    short = dict(classes, GmConvDesc=with_field(_native.GmConvDesc, "pre_S", ctypes.c_int * 3))
    assert _field_type_problems(_header_structs(), short) == ["GmConvDesc.pre_S: not an array of 2"]


def test_ops_limits_are_the_headers():
    k = {n: int(v) for n, v in re.findall(r"#define (GM_GN_[A-Z_]+) (\d+)", _header_source())}
    assert set(k) == {"GM_GN_SHORT_MAX_ROWS", "GM_GN_TABLE_MAX_CHANNELS"}
    assert ops.GN_IN_CONSUMER_MAX_ROWS == k["GM_GN_SHORT_MAX_ROWS"] == 128
    assert ops.GN_IN_CONSUMER_MAX_CHANNELS == k["GM_GN_TABLE_MAX_CHANNELS"] == 384


def test_no_kernel_file_declares_an_extern_c_symbol_by_hand():
    """Every extern "C" in a .hip / .cpp file is a definition: the declarations live in include/gm_amd.h and csrc/gm_internal.h, once each."""
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")))
    assert len(files) >= 24
    seen = 0
    for f in files:
        src = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(CSRC, f)).read(), flags=re.S)
        for m in re.finditer(r'extern\s+"C"\s*([^;{]*)([;{])', src):
            seen += 1
            assert m.group(2) == "{" and m.group(1).strip(), f"{f}: extern \"C\" {' '.join(m.group(1).split())}{m.group(2)} is not a definition"
    assert seen >= len(_header_functions())  # (the scan does see the definitions)


def test_pure_host_entry_points_run_without_a_gpu():
    lib = _native.lib()
    bm, bn = ctypes.c_int(), ctypes.c_int()
    assert lib.gm_conv_cfg_tile(0, ctypes.byref(bm), ctypes.byref(bn)) == 0 and (bm.value, bn.value) == (256, 64)
    assert lib.gm_packed_conv_weight_elems(64, 64, 3, 3, 3, 1) == 2 * 27 * 64 * 32
    assert lib.gm_gn_workspace_bytes(1, 128 ** 3, 64, 32, 1) > 0
    assert lib.gm_attention_max_head_dim() == 256
    for policy in (-1, 0, 16, 0):  # grid policy of the LDS-DMA convolutions: process-wide host state, no device call; leave the default (0)
        lib.gm_conv_dma_set_persistent(policy)
    lib.gm_attention_dma_set_variant(0, 0)
