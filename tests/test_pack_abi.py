"""CPU: packed typed columns in the C-ABI -- the five symbols in the header, in the library and in
the Python mirror's table, their exact signatures, both structs' layouts (clg_pack_block is 32
bytes), the JNI shim, the Java natives and the block cursor, the Python entry points, the kernels
in the built library; the version and clg_columns stay."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("clg_pack_columns", "clg_decode_logs_columns_packed", "clg_decode_host_columns_packed",
           "clg_pack_columns_host", "clg_unpack_columns_host")
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
    assert "int clg_pack_columns(clg_engine* e, const clg_columns* in, clg_packed* out);" in h
    assert ("int clg_decode_logs_columns_packed(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, "
            "clg_columns* wide, clg_payloads* var, clg_packed* out);") in h
    assert ("int clg_decode_host_columns_packed(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, "
            "const uint64_t* span_len, uint32_t n, clg_columns* wide, clg_payloads* var, clg_packed* out);") in h
    assert "int clg_pack_columns_host(const clg_columns* in, clg_packed* out);" in h
    assert ("int clg_unpack_columns_host(const clg_packed* in, uint32_t stream, uint64_t first, uint64_t count, "
            "void* out);") in h


def test_mirror_prototypes():
    from clonos_amd import _lib
    P, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    col, pay, pk = ctypes.POINTER(_lib.Columns), ctypes.POINTER(_lib.Payloads), ctypes.POINTER(_lib.Packed)
    want = {
        "clg_pack_columns": [P, col, pk],
        "clg_decode_logs_columns_packed": [P, P, P, u32, col, pay, pk],
        "clg_decode_host_columns_packed": [P, P, P, P, u32, col, pay, pk],
        "clg_pack_columns_host": [col, pk],
        "clg_unpack_columns_host": [pk, u32, u64, u64, P],
    }
    for sym, args in want.items():
        fn = getattr(_lib.lib, sym)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, sym


def header_fields(name):
    h = re.sub(r"/\*.*?\*/", "", read("include", "clonos_engine.h"), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
    ctype = {"uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64,
             "clg_pack_block": None}
    count = {"CLG_PACK_STREAMS": 5, "CLG_PACK_STREAMS + 1": 6}
    out = []
    for ty, star, fname, arr in re.findall(r"(?:const )?(\w+)(\*?)\s+(\w+)(?:\[([\w +]+)\])?;", body):
        t = ctypes.c_void_p if star else ctype[ty]
        out.append((fname, t * count[arr] if arr else t))
    return out


@pytest.mark.parametrize("name, mirror, size", [("clg_pack_block", "PackBlock", 32), ("clg_packed", "Packed", 136)])
def test_struct_layouts_mirror_the_header(name, mirror, size):
    from clonos_amd import _lib
    want = header_fields(name)
    got = list(getattr(_lib, mirror)._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and (a is ctypes.c_void_p) == (b is ctypes.c_void_p), n
    assert ctypes.sizeof(getattr(_lib, mirror)) == size
    where = read("clonos_amd", "csrc", "engine.cpp") + read("clonos_amd", "csrc", "pack.h")
    assert "static_assert(sizeof(%s) == %d" % (name, size) in where


def test_field_names_constants_and_what_stays():
    from clonos_amd import _lib
    from clonos_amd.engine import PACK_BLOCK
    assert [n for n, _ in _lib.PackBlock._fields_] == ["ref", "first", "pos", "width", "count"]
    assert [n for n, _ in _lib.Packed._fields_] == ["desc", "bits", "cap_desc", "cap_bits", "out_kind", "reserved", "n_val",
                                                    "blk_base", "n_bits"]
    assert PACK_BLOCK.itemsize == 32 and list(PACK_BLOCK.names) == ["ref", "first", "pos", "width", "count"]
    for f in PACK_BLOCK.names:
        assert PACK_BLOCK.fields[f][1] == getattr(_lib.PackBlock, f).offset, f
    h = read("include", "clonos_engine.h")
    assert re.search(r"#define\s+CLG_PACK_STREAMS\s+5\b", h) and re.search(r"#define\s+CLG_PACK_BLOCK\s+1024\b", h)
    assert _lib.PACK_STREAMS == 5 and _lib.PACK_BLOCK == 1024
    for k, name in enumerate(("TAG", "ORDER", "TIMESTAMP", "RNG", "BUFFER_BUILT")):
        assert re.search(r"CLG_PACK_%s = %d\b" % (name, k), h) and getattr(_lib, "PACK_" + name) == k
    assert ctypes.sizeof(_lib.Columns) == 232 and ctypes.sizeof(_lib.Payloads) == 64  # not touched
    assert "static_assert(sizeof(clg_columns) == 232" in read("clonos_amd", "csrc", "engine.cpp")


def test_the_format_is_defined_once_for_host_and_device():
    hdr = read("clonos_amd", "csrc", "pack.h")
    assert "kPackBlock = CLG_PACK_BLOCK" in hdr and "__host__ __device__" in hdr
    for user in (("clonos_amd", "csrc", "pack.hip"), ("clonos_amd", "csrc", "engine_pack.cpp"), ("tests", "pack_host.cpp")):
        assert re.search(r'#include ".*pack\.h"', read(*user)), user


def test_jni_shim_java_natives_and_cursor():
    c = read("jni", "clonos_jni.c")
    java = read(*JDIR, "ClonosEngine.java")
    assert re.search(r"FN\(nDecodeLogsColumnsPacked\)", c) and re.search(r"\bclg_decode_logs_columns_packed\(ENG\(e\)", c)
    assert re.search(r"static native int nDecodeLogsColumnsPacked\(", java)
    assert re.search(r"public EnginePackedColumns decodeLogsColumnsPacked\(int\[\] logs, long\[\] startEpochs, "
                     r"boolean withPayloads\)", java)
    cur = read(*JDIR, "EnginePackedColumns.java")
    for sig in (r"public int nextTag\(\)", r"public byte nextChannel\(\)", r"public long nextTimestamp\(\)",
                r"public int nextInt\(\)", r"public int nextBufferSize\(\)", r"public Cursor cursor\(int s\)"):
        assert re.search(sig, cur), sig
    assert "LogReplayerImpl.java:61-119" in cur and "LogReplayerImpl.java:71-78" in cur
    assert "LogReplayerImpl.java:81-88" in cur and "ReplayingState.java:161-188" in cur
    assert "native" not in re.sub(r"nativeOrder", "", cur)  # the cursor is pure Java over direct buffers
    assert "decodeLogsColumnsPacked(" in read("INTEGRATION.md") and "clg_decode_logs_columns_packed" in read("INTEGRATION.md")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_shim_compiles_against_the_stub():
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                    "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "clonos_jni.c")], check=True)


def test_python_entry_points():
    import clonos_amd
    from clonos_amd import Engine, PackedColumns
    for name in ("PackedColumns", "pack_columns_host", "unpack_columns_host"):
        assert name in clonos_amd.__all__ and getattr(clonos_amd, name) is not None
    for m in ("pack_columns", "pack_columns_raw"):
        assert callable(getattr(Engine, m)), m
    assert inspect.signature(Engine.decode_logs_columns).parameters["packed"].default is False
    assert inspect.signature(Engine.decode_host_columns).parameters["packed"].default is False
    for m in ("unpack", "span", "unpack_stream", "payload"):
        assert callable(getattr(PackedColumns, m)), m
    assert isinstance(PackedColumns.n_bytes, property) and isinstance(clonos_amd.DecodedColumns.n_bytes, property)


def test_kernels_built_for_gfx950():
    from clonos_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_pack_measure", b"k_pack_scan_sums", b"k_pack_scan_top", b"k_pack_scan_apply", b"k_pack_write"):
        assert k in blob, k
