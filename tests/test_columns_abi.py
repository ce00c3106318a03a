"""CPU: the typed columns' additions to the C-ABI -- the four symbols in the header, in the
library and in the Python mirror's table, their exact signatures, the struct's layout, the JNI
shim and the Java native pair, the Python entry points; the version stays."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("clg_columnize", "clg_decode_logs_columns", "clg_decode_host_columns", "clg_columnize_host")


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
    assert ("int clg_columnize(clg_engine* e, const clg_decoded* in, const uint64_t* span_rec_base, uint32_t n_spans, "
            "clg_columns* out);") in h
    assert ("int clg_decode_logs_columns(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, "
            "clg_columns* out);") in h
    assert ("int clg_decode_host_columns(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, "
            "const uint64_t* span_len, uint32_t n, clg_columns* out);") in h
    assert ("int clg_columnize_host(const clg_decoded* in, const uint64_t* span_rec_base, uint32_t n_spans, "
            "clg_columns* out);") in h


def test_struct_layout_mirrors_the_header():
    """Field order and types of clg_columns, read from the header, against the ctypes mirror."""
    from clonos_amd import _lib
    h = re.sub(r"/\*.*?\*/", "", read("include", "clonos_engine.h"), flags=re.S)
    body = re.search(r"typedef struct clg_columns \{(.*?)\} clg_columns;", h, re.S).group(1)
    fields = re.findall(r"(\w+)(\*?)\s+(\w+)(?:\[(\w+)\])?;", body)
    ctype = {"uint8_t": ctypes.c_uint8, "int8_t": ctypes.c_int8, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
             "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
    want = []
    for ty, star, name, arr in fields:
        t = ctypes.c_void_p if star else ctype[ty]
        want.append((name, t * _lib.COL_CLASSES if arr else t))
    got = [(n, t) for n, t in _lib.Columns._fields_]
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and (a is ctypes.c_void_p) == (b is ctypes.c_void_p), n
    assert ctypes.sizeof(_lib.Columns) == 232
    assert re.search(r"#define CLG_COL_CLASSES (\d+)", h).group(1) == str(_lib.COL_CLASSES)


def test_jni_shim_and_java_natives():
    c = read("jni", "clonos_jni.c")
    jdir = ("jni", "java", "org", "apache", "flink", "runtime", "causal", "engine")
    java = read(*jdir, "ClonosEngine.java")
    assert re.search(r"FN\(nDecodeLogsColumns\)", c) and re.search(r"\bclg_decode_logs_columns\(ENG\(e\)", c)
    assert re.search(r"static native int nDecodeLogsColumns\(", java)
    assert re.search(r"public EngineDecodedColumns decodeLogsColumns\(", java)
    cols = read(*jdir, "EngineDecodedColumns.java")
    for view in (r"public ByteBuffer channels\(", r"public LongBuffer timestamps\(", r"public IntBuffer randomInts\(",
                 r"public IntBuffer bufferSizes\(", r"public ByteBuffer tags\("):
        assert re.search(view, cols), view
    assert "EngineDecodedColumns" in read("INTEGRATION.md")


def test_python_entry_points():
    import clonos_amd
    from clonos_amd import DecodedColumns, Engine
    from clonos_amd.replay import ColumnReplayer, ReplayOrderError
    assert callable(clonos_amd.columnize_host)
    assert callable(Engine.columnize) and callable(Engine.decode_logs_columns) and callable(Engine.decode_host_columns)
    for m in ("span", "to_soa", "determinants"):
        assert callable(getattr(DecodedColumns, m)), m
    for m in ("replayNextChannel", "replayNextTimestamp", "replayRandomInt", "replaySerializableDeterminant",
              "triggerAsyncEvent", "record_count_target", "isFinished"):
        assert callable(getattr(ColumnReplayer, m)), m
    assert issubclass(ReplayOrderError, AssertionError)


def test_kernels_built_for_gfx950():
    from clonos_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_col_count", b"k_col_scan", b"k_col_write", b"k_col_span_base", b"k_col_wide_v0"):
        assert k in blob, k
