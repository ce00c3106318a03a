"""CPU: the payload column's additions to the C-ABI -- the five symbols in the header, in the
library and in the Python mirror's table, their exact signatures, clg_payloads' layout, the JNI
shim and the Java natives, the Python entry points, the kernels in the built library; the version
and clg_columns stay."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("clg_gather_payloads", "clg_gather_payloads_logs", "clg_decode_logs_columns_var",
           "clg_decode_host_columns_var", "clg_gather_payloads_host")


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
    assert ("int clg_gather_payloads(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, "
            "const uint64_t* span_len, uint32_t n_spans, const uint32_t* w_var_off, const uint32_t* w_var_len, "
            "const uint64_t* row_base, uint32_t in_kind, clg_payloads* out);") in h
    assert ("int clg_gather_payloads_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, "
            "const uint32_t* w_var_off, const uint32_t* w_var_len, const uint64_t* row_base, uint32_t in_kind, "
            "clg_payloads* out);") in h
    assert ("int clg_decode_logs_columns_var(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, "
            "clg_columns* out, clg_payloads* var);") in h
    assert ("int clg_decode_host_columns_var(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, "
            "const uint64_t* span_len, uint32_t n, clg_columns* out, clg_payloads* var);") in h
    assert ("int clg_gather_payloads_host(const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len, "
            "uint32_t n_spans, const uint32_t* w_var_off, const uint32_t* w_var_len, const uint64_t* row_base, "
            "clg_payloads* out);") in h


def test_mirror_prototypes():
    from clonos_amd import _lib
    P = ctypes.c_void_p
    u32 = ctypes.c_uint32
    pay, col = ctypes.POINTER(_lib.Payloads), ctypes.POINTER(_lib.Columns)
    want = {
        "clg_gather_payloads": [P, P, P, P, u32, P, P, P, u32, pay],
        "clg_gather_payloads_logs": [P, P, P, u32, P, P, P, u32, pay],
        "clg_decode_logs_columns_var": [P, P, P, u32, col, pay],
        "clg_decode_host_columns_var": [P, P, P, P, u32, col, pay],
        "clg_gather_payloads_host": [P, P, P, u32, P, P, P, pay],
    }
    for sym, args in want.items():
        fn = getattr(_lib.lib, sym)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, sym


def test_struct_layout_mirrors_the_header():
    """Field order and types of clg_payloads, read from the header, against the ctypes mirror."""
    from clonos_amd import _lib
    h = re.sub(r"/\*.*?\*/", "", read("include", "clonos_engine.h"), flags=re.S)
    body = re.search(r"typedef struct clg_payloads \{(.*?)\} clg_payloads;", h, re.S).group(1)
    fields = re.findall(r"(\w+)(\*?)\s+(\w+);", body)
    ctype = {"uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    want = [(name, ctypes.c_void_p if star else ctype[ty]) for ty, star, name in fields]
    got = list(_lib.Payloads._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    assert [n for n, _ in got] == ["var", "pos", "cap_var", "cap_pos", "out_kind", "reserved", "n_rows", "n_var", "bad_row"]
    for (n, a), (_, b) in zip(got, want):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and (a is ctypes.c_void_p) == (b is ctypes.c_void_p), n
    assert ctypes.sizeof(_lib.Payloads) == 64
    assert ctypes.sizeof(_lib.Columns) == 232  # clg_columns is not touched
    assert "static_assert(sizeof(clg_payloads) == 64" in read("clonos_amd", "csrc", "engine.cpp")


def test_jni_shim_and_java_natives():
    c = read("jni", "clonos_jni.c")
    jdir = ("jni", "java", "org", "apache", "flink", "runtime", "causal", "engine")
    java = read(*jdir, "ClonosEngine.java")
    assert re.search(r"FN\(nDecodeLogsColumnsVar\)", c) and re.search(r"\bclg_decode_logs_columns_var\(ENG\(e\)", c)
    assert re.search(r"static native int nDecodeLogsColumnsVar\(", java)
    assert re.search(r"public EngineDecodedColumns decodeLogsColumns\(int\[\] logs, long\[\] startEpochs, boolean withPayloads\)",
                     java)
    assert re.search(r"public ByteBuffer payload\(int k\)", read(*jdir, "EngineDecodedColumns.java"))
    assert "payload(" in read("INTEGRATION.md") and "clg_decode_logs_columns_var" in read("INTEGRATION.md")


def test_python_entry_points():
    import inspect

    import clonos_amd
    from clonos_amd import DecodedColumns, Engine
    assert callable(clonos_amd.gather_payloads_host)
    for m in ("gather_payloads", "gather_payloads_logs", "encode_columns"):
        assert callable(getattr(Engine, m)), m
    for f in (Engine.decode_logs_columns, Engine.decode_host_columns):
        assert inspect.signature(f).parameters["payloads"].default is False
    assert callable(DecodedColumns.payload)
    empty = [np.zeros(0, dt) for dt in ("u4", "u1", "i8", "u4", "i4", "i8", "u4", "u4", "u1")]
    c = clonos_amd.columnize_host(clonos_amd.DecodedBatch(*empty, [0, 0]))
    assert c.var is None and c.var_pos is None  # not asked for


def test_kernels_built_for_gfx950():
    from clonos_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_pay_size", b"k_pay_scan", b"k_pay_pos", b"k_pay_copy"):
        assert k in blob, k
