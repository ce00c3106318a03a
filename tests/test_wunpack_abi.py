"""CPU: packed wide rows as input in the C-ABI -- the four symbols in the header, in the library and
in the Python mirror's table, their exact signatures, the stream offset of a wide finding, the
Python entry points and their routing, the kernels in the built library; the version stays."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("clg_unpack_wide", "clg_encode_columns_packed_wide", "clg_append_columns_packed_wide",
           "clg_encode_columns_packed_wide_host")


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


def test_header_signatures_and_the_stream_offset():
    from clonos_amd import _lib
    h = re.sub(r"\s+", " ", read("include", "clonos_engine.h"))
    assert ("int clg_unpack_wide(clg_engine* e, const clg_packed_wide* in, clg_columns* out, uint64_t* pos, "
            "clg_unpack_bad* bad);") in h
    assert ("int clg_encode_columns_packed_wide(clg_engine* e, const clg_packed* narrow, const clg_packed_wide* wide, "
            "const clg_columns_in* rest, clg_encoded* out, clg_unpack_bad* bad);") in h
    assert ("int clg_append_columns_packed_wide(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans, "
            "const clg_packed* narrow, const clg_packed_wide* wide, const clg_columns_in* rest, uint64_t* span_bytes, "
            "int32_t* status, clg_unpack_bad* bad);") in h
    assert ("int clg_encode_columns_packed_wide_host(const clg_packed* narrow, const clg_packed_wide* wide, "
            "const clg_columns_in* rest, clg_encoded* out, clg_unpack_bad* bad);") in h
    assert re.search(r"#define CLG_UNPACK_WIDE_STREAM 32\b", h) and _lib.UNPACK_WIDE_STREAM == 32
    # the offset and the cross rule are defined once, for the host and the kernels
    fmt = read("clonos_amd", "csrc", "pack_wide.h")
    assert "kWPackBadStream = CLG_UNPACK_WIDE_STREAM" in fmt and "CLG_PACK_HD bool wpack_cross_ok(" in fmt
    assert "wpack_cross_ok(" in read("clonos_amd", "csrc", "unpack_wide.hip")
    assert "CLG_UNPACK_WIDE_STREAM" not in read("clonos_amd", "csrc", "engine_encode_columns.cpp")


def test_mirror_prototypes():
    from clonos_amd import _lib
    P, u32 = ctypes.c_void_p, ctypes.c_uint32
    col, cin, enc = ctypes.POINTER(_lib.Columns), ctypes.POINTER(_lib.ColumnsIn), ctypes.POINTER(_lib.Encoded)
    pk, wpk, bad = ctypes.POINTER(_lib.Packed), ctypes.POINTER(_lib.PackedWideC), ctypes.POINTER(_lib.UnpackBad)
    want = {
        "clg_unpack_wide": [P, wpk, col, P, bad],
        "clg_encode_columns_packed_wide": [P, pk, wpk, cin, enc, bad],
        "clg_append_columns_packed_wide": [P, P, P, u32, pk, wpk, cin, P, P, bad],
        "clg_encode_columns_packed_wide_host": [pk, wpk, cin, enc, bad],
    }
    for sym, args in want.items():
        fn = getattr(_lib.lib, sym)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, sym


def test_what_stays():
    from clonos_amd import _lib
    assert ctypes.sizeof(_lib.Columns) == 232 and ctypes.sizeof(_lib.PackedWideC) == 480 and ctypes.sizeof(_lib.Packed) == 136
    assert ctypes.sizeof(_lib.UnpackBad) == 16
    for sym in ("clg_unpack_wide_host", "clg_encode_columns_packed", "clg_append_columns_packed", "clg_unpack_columns"):
        assert hasattr(_lib.lib, sym), sym


def test_python_entry_points_and_routing():
    import numpy as np
    import clonos_amd
    from clonos_amd import Engine
    from _encode_util import host_columns
    assert "encode_columns_packed_wide_host" in clonos_amd.__all__ and callable(clonos_amd.encode_columns_packed_wide_host)
    for m in ("unpack_wide", "unpack_wide_raw"):
        assert callable(getattr(Engine, m)), m
    assert inspect.signature(Engine.unpack_wide).parameters["pos"].default is False
    for fn in (Engine.encode_columns, Engine.append_columns):
        assert inspect.signature(fn).parameters["wide"].default == "host"
    # "device" over anything but PackedColumns with wide_packed is a ValueError, before the engine is touched
    from clonos_amd import synth
    plain = host_columns([synth.random_log(20, np.random.default_rng(1), allow_serializable=True)])
    narrow_only = clonos_amd.pack_columns_host(plain)
    for cols in (plain, narrow_only):
        with pytest.raises(ValueError):
            Engine.encode_columns(None, cols, wide="device")
        with pytest.raises(ValueError):
            Engine.append_columns(None, [], [], cols, wide="device")
        with pytest.raises(ValueError):
            clonos_amd.encode_columns_packed_wide_host(cols)
    with pytest.raises(ValueError):
        Engine.encode_columns(None, plain, wide="gpu")


def test_jni_shim_java_native_and_method():
    c = read("jni", "clonos_jni.c")
    jdir = ("jni", "java", "org", "apache", "flink", "runtime", "causal", "engine")
    java = read(*jdir, "ClonosEngine.java")
    assert re.search(r"FN\(nAppendColumnsPackedWide\)", c) and re.search(r"\bclg_append_columns_packed_wide\(ENG\(e\)", c)
    assert re.search(r"static native int nAppendColumnsPackedWide\(", java)
    assert re.search(r"public long\[\] appendColumnsPackedWide\(int\[\] logs, long\[\] epochs, EnginePackedColumns cols, "
                     r"EnginePackedWide wide\)", java)
    # the native's parameters, in order, against the shim's
    m = re.search(r"static native int nAppendColumnsPackedWide\((.*?)\);", java, re.S)
    jtypes = [p.split()[0] for p in re.sub(r"\s+", " ", m.group(1)).split(", ")]
    m = re.search(r"FN\(nAppendColumnsPackedWide\)\(JNIEnv\* env, jclass cls, (.*?)\) \{", c, re.S)
    ctypes_ = [p.split()[0] for p in re.sub(r"\s+", " ", m.group(1)).split(", ")]
    to_c = {"long": "jlong", "int[]": "jintArray", "long[]": "jlongArray", "ByteBuffer": "jobject"}
    assert [to_c[t] for t in jtypes] == ctypes_
    assert "long nVar;" in read(*jdir, "EnginePackedWide.java")


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("nm") is None, reason="gcc or nm not available")
def test_shim_compiles_against_the_stub_and_defines_the_native(tmp_path):
    obj = str(tmp_path / "clonos_jni.o")
    subprocess.run(["gcc", "-c", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                    "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "clonos_jni.c"), "-o", obj], check=True)
    syms = subprocess.run(["nm", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    assert re.search(r" T \w*ClonosEngine_nAppendColumnsPackedWide$", syms, re.M), syms
    assert re.search(r" T \w*ClonosEngine_nAppendColumnsPacked$", syms, re.M)  # the existing native stays


def test_kernels_built_for_gfx950():
    from clonos_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_wunpack_check", b"k_wunpack_kind", b"k_wunpack_scan", b"k_wunpack_write", b"k_wunpack_merge",
              b"k_wunpack_tscan", b"k_wunpack_pos", b"k_unpack_check", b"k_unpack_write"):
        assert k in blob, k
