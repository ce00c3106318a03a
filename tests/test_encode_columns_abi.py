"""CPU: the encode of typed columns in the C-ABI -- the three symbols in the header, in the library
and in the Python mirror's table, their exact signatures, both structs' layouts, the JNI shim and
the Java natives, the Python entry points, the kernels in the built library; the version and
clg_columns stay."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("clg_encode_columns", "clg_encode_columns_host", "clg_append_columns")


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
    assert "int clg_encode_columns(clg_engine* e, const clg_columns_in* in, clg_encoded* out);" in h
    assert "int clg_encode_columns_host(const clg_columns_in* in, clg_encoded* out);" in h
    assert ("int clg_append_columns(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans, "
            "const clg_columns_in* in, uint64_t* span_bytes, int32_t* status);") in h


def test_mirror_prototypes():
    from clonos_amd import _lib
    P, u32 = ctypes.c_void_p, ctypes.c_uint32
    cin, enc = ctypes.POINTER(_lib.ColumnsIn), ctypes.POINTER(_lib.Encoded)
    want = {
        "clg_encode_columns": [P, cin, enc],
        "clg_encode_columns_host": [cin, enc],
        "clg_append_columns": [P, P, P, u32, cin, P, P],
    }
    for sym, args in want.items():
        fn = getattr(_lib.lib, sym)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, sym


def header_fields(name):
    h = re.sub(r"/\*.*?\*/", "", read("include", "clonos_engine.h"), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
    ctype = {"uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    out = []
    for ty, star, fname, arr in re.findall(r"(?:const )?(\w+)(\*?)\s+(\w+)(\[\w+\])?;", body):
        t = ctypes.c_void_p if star else ctype[ty]
        out.append((fname, t * 5 if arr else t))
    return out


@pytest.mark.parametrize("name, mirror, size", [("clg_columns_in", "ColumnsIn", 176), ("clg_encoded", "Encoded", 56)])
def test_struct_layouts_mirror_the_header(name, mirror, size):
    from clonos_amd import _lib
    want = header_fields(name)
    got = list(getattr(_lib, mirror)._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and (a is ctypes.c_void_p) == (b is ctypes.c_void_p), n
    assert ctypes.sizeof(getattr(_lib, mirror)) == size
    assert "static_assert(sizeof(%s) == %d" % (name, size) in read("clonos_amd", "csrc", "engine.cpp")


def test_field_names_and_what_stays():
    from clonos_amd import _lib
    assert [n for n, _ in _lib.ColumnsIn._fields_] == [
        "tag", "order", "timestamp", "rng", "buffer_built", "w_rc", "w_v1", "w_var_len", "w_sub", "w_v0", "w_idx", "pos",
        "var", "span_base", "n_rec", "n_class", "n_var", "n_spans", "in_kind"]
    assert [n for n, _ in _lib.Encoded._fields_] == [
        "bytes", "cap", "out_kind", "reserved", "span_byte_base", "n_bytes", "bad_what", "reserved2", "bad_index"]
    assert "w_var_off" not in dict(_lib.ColumnsIn._fields_)  # it indexes bytes that are not there
    assert ctypes.sizeof(_lib.Columns) == 232 and ctypes.sizeof(_lib.Payloads) == 64  # not touched
    eng = read("clonos_amd", "csrc", "engine.cpp")
    assert "static_assert(sizeof(clg_columns) == 232" in eng
    h = read("include", "clonos_engine.h")
    for k, name in enumerate(("NONE", "TAG", "TOTALS", "SPAN", "ROW")):
        assert re.search(r"CLG_ENC_BAD_%s = %d\b" % (name, k), h) and getattr(_lib, "ENC_BAD_" + name) == k


def test_jni_shim_and_java_natives():
    c = read("jni", "clonos_jni.c")
    jdir = ("jni", "java", "org", "apache", "flink", "runtime", "causal", "engine")
    java = read(*jdir, "ClonosEngine.java")
    assert re.search(r"FN\(nEncodeColumns\)", c) and re.search(r"\bclg_encode_columns\(ENG\(e\)", c)
    assert re.search(r"FN\(nAppendColumns\)", c) and re.search(r"\bclg_append_columns\(ENG\(e\)", c)
    assert re.search(r"static native int nEncodeColumns\(", java) and re.search(r"static native int nAppendColumns\(", java)
    assert re.search(r"public long\[\] appendColumns\(int\[\] logs, long\[\] epochs, EngineDecodedColumns cols\)", java)
    assert re.search(r"public ByteBuffer encodeColumns\(EngineDecodedColumns cols\)", java)
    assert "appendColumns(" in read("INTEGRATION.md") and "clg_append_columns" in read("INTEGRATION.md")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_shim_compiles_against_the_stub():
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                    "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "clonos_jni.c")], check=True)


def test_python_entry_points():
    import clonos_amd
    from clonos_amd import Engine
    assert callable(clonos_amd.encode_columns_host) and "encode_columns_host" in clonos_amd.__all__
    for m in ("encode_columns", "encode_columns_raw", "append_columns"):
        assert callable(getattr(Engine, m)), m
    assert inspect.signature(Engine.encode_columns).parameters["per_span"].default is False
    assert inspect.signature(clonos_amd.encode_columns_host).parameters["per_span"].default is False
    assert list(inspect.signature(Engine.append_columns).parameters)[:4] == ["self", "logs", "epochs", "cols"]


def test_kernels_built_for_gfx950():
    from clonos_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_ecol_bytes", b"k_ecol_scan64", b"k_ecol_span", b"k_ecol_write", b"k_col_count", b"k_col_scan"):
        assert k in blob, k
