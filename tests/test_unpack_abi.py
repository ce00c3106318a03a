"""CPU: packed typed columns as input in the C-ABI -- the four symbols in the header, in the library
and in the Python mirror's table, their exact signatures, clg_unpack_bad's layout (16 bytes) and
enum, the JNI shim, the Java native and method, the Python entry points, the kernels in the built
library; the version and the existing structs stay."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("clg_unpack_columns", "clg_unpack_columns_all_host", "clg_encode_columns_packed", "clg_append_columns_packed")
JDIR = ("jni", "java", "org", "apache", "flink", "runtime", "causal", "engine")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_in_header_library_and_mirror():
    from clonos_amd import _lib
    h = read("include", "clonos_engine.h")
    for sym in SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, h), sym
        assert sym in _lib.EXPORTED
        assert hasattr(_lib.lib, sym)
        assert getattr(_lib.lib, sym).argtypes is not None, sym  # a prototype in the table
    assert re.search(r"#define\s+CLG_ABI_VERSION\s+6\b", h)  # additions only: the version stays
    assert _lib.lib.clg_abi_version() == 6


def test_header_signatures():
    h = re.sub(r"\s+", " ", read("include", "clonos_engine.h"))
    assert "int clg_unpack_columns(clg_engine* e, const clg_packed* in, clg_columns* out, clg_unpack_bad* bad);" in h
    assert "int clg_unpack_columns_all_host(const clg_packed* in, clg_columns* out, clg_unpack_bad* bad);" in h
    assert ("int clg_encode_columns_packed(clg_engine* e, const clg_packed* narrow, const clg_columns_in* rest, "
            "clg_encoded* out, clg_unpack_bad* bad);") in h
    assert ("int clg_append_columns_packed(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans, "
            "const clg_packed* narrow, const clg_columns_in* rest, uint64_t* span_bytes, int32_t* status, "
            "clg_unpack_bad* bad);") in h
    for sym in SYMBOLS:  # every entry point carries its comment block
        assert re.search(r"\*/ (?:int \w+\([^;]*\); )*int %s\(" % sym, h), sym


def test_mirror_prototypes():
    from clonos_amd import _lib
    P, u32 = ctypes.c_void_p, ctypes.c_uint32
    col, pk, bad = ctypes.POINTER(_lib.Columns), ctypes.POINTER(_lib.Packed), ctypes.POINTER(_lib.UnpackBad)
    cin, enc = ctypes.POINTER(_lib.ColumnsIn), ctypes.POINTER(_lib.Encoded)
    want = {
        "clg_unpack_columns": [P, pk, col, bad],
        "clg_unpack_columns_all_host": [pk, col, bad],
        "clg_encode_columns_packed": [P, pk, cin, enc, bad],
        "clg_append_columns_packed": [P, P, P, u32, pk, cin, P, P, bad],
    }
    for sym, args in want.items():
        fn = getattr(_lib.lib, sym)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, sym


def test_unpack_bad_layout_enum_and_what_stays():
    from clonos_amd import _lib
    h = read("include", "clonos_engine.h")
    assert re.search(r"typedef struct clg_unpack_bad \{ uint32_t what; uint32_t stream; uint64_t block; \} clg_unpack_bad;", h)
    assert [(n, ctypes.sizeof(t)) for n, t in _lib.UnpackBad._fields_] == [("what", 4), ("stream", 4), ("block", 8)]
    assert ctypes.sizeof(_lib.UnpackBad) == 16 and _lib.UnpackBad.block.offset == 8
    assert "static_assert(sizeof(clg_unpack_bad) == 16" in read("clonos_amd", "csrc", "engine.cpp")
    for k, name in enumerate(("NONE", "LAYOUT", "BLOCK", "VALUE")):
        assert re.search(r"CLG_UNPACK_BAD_%s = %d\b" % (name, k), h) and getattr(_lib, "UNPACK_BAD_" + name) == k
    # not touched
    assert ctypes.sizeof(_lib.Packed) == 136 and ctypes.sizeof(_lib.Columns) == 232 and ctypes.sizeof(_lib.ColumnsIn) == 176
    eng = read("clonos_amd", "csrc", "engine.cpp")
    assert "static_assert(sizeof(clg_packed) == 136" in eng and "static_assert(sizeof(clg_columns) == 232" in eng


def test_the_input_rules_are_defined_once_for_host_and_device():
    hdr = read("clonos_amd", "csrc", "pack.h")
    for fn in ("pack_block_in_ok", "pack_range_inside", "pack_value_ok"):
        assert re.search(r"CLG_PACK_HD \w+ %s\(" % fn, hdr), fn
    for fn in ("pack_layout_in_ok", "pack_unpack_all_host", "pack_unpack_begin"):
        assert re.search(r"inline \w+ %s\(" % fn, hdr), fn
    assert "pos % 16" in hdr
    kern = read("clonos_amd", "csrc", "unpack.hip")
    assert "pack_block_in_ok(" in kern and "pack_range_inside(" in kern and "pack_value_ok(" in kern
    for user in (("clonos_amd", "csrc", "unpack.hip"), ("tests", "unpack_host.cpp")):
        assert re.search(r'#include ".*pack\.h"', read(*user)), user


def test_jni_shim_java_native_and_method():
    c = read("jni", "clonos_jni.c")
    java = read(*JDIR, "ClonosEngine.java")
    assert re.search(r"FN\(nAppendColumnsPacked\)", c) and re.search(r"\bclg_append_columns_packed\(ENG\(e\)", c)
    assert re.search(r"static native int nAppendColumnsPacked\(", java)
    assert re.search(r"public long\[\] appendColumnsPacked\(int\[\] logs, long\[\] epochs, EnginePackedColumns cols\)", java)
    assert "bad_what" in java and "bad_stream" in java and "bad_block" in java
    doc = read("INTEGRATION.md")
    assert "appendColumnsPacked(" in doc and "clg_append_columns_packed" in doc


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_shim_compiles_against_the_stub():
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                    "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "clonos_jni.c")], check=True)


def test_python_entry_points():
    import clonos_amd
    from clonos_amd import Engine, PackedColumns, _lib
    assert "unpack_packed_host" in clonos_amd.__all__ and callable(clonos_amd.unpack_packed_host)
    for m in ("unpack_columns", "unpack_columns_raw"):
        assert callable(getattr(Engine, m)), m
    assert list(inspect.signature(Engine.unpack_columns_raw).parameters) == ["self", "pin", "cols", "bad"]
    assert list(inspect.signature(Engine.unpack_columns).parameters) == ["self", "packed"]
    assert "PackedColumns" in inspect.getsource(Engine.encode_columns) and "PackedColumns" in inspect.getsource(Engine.append_columns)
    assert "clg_unpack_columns_host" in inspect.getsource(PackedColumns.unpack_stream)  # unpack() stays the host path
    assert hasattr(_lib, "UnpackBad")


def test_kernels_built_for_gfx950():
    from clonos_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_unpack_check", b"k_unpack_write"):
        assert k in blob, k
