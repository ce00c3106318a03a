"""CPU: packed wide rows in the C-ABI -- the five symbols in the header, in the library and in the
Python mirror's table, their exact signatures, clg_packed_wide's layout against the mirror, the JNI
shim, the Java native, method and row cursor, the Python entry points, the kernels in the built
library; the version and the existing structs stay."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("clg_pack_wide", "clg_pack_wide_host", "clg_unpack_wide_host", "clg_decode_logs_columns_packed_wide",
           "clg_decode_host_columns_packed_wide")
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
    assert "int clg_pack_wide(clg_engine* e, const clg_columns* in, clg_packed_wide* out);" in h
    assert "int clg_pack_wide_host(const clg_columns* in, clg_packed_wide* out);" in h
    assert "int clg_unpack_wide_host(const clg_packed_wide* in, clg_columns* out, clg_unpack_bad* bad);" in h
    assert ("int clg_decode_logs_columns_packed_wide(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, "
            "uint32_t n, clg_columns* sizes, clg_payloads* var, clg_packed* narrow, clg_packed_wide* wide);") in h
    assert ("int clg_decode_host_columns_packed_wide(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, "
            "const uint64_t* span_len, uint32_t n, clg_columns* sizes, clg_payloads* var, clg_packed* narrow, "
            "clg_packed_wide* wide);") in h


def test_mirror_prototypes():
    from clonos_amd import _lib
    P, u32 = ctypes.c_void_p, ctypes.c_uint32
    col, pay, pk = ctypes.POINTER(_lib.Columns), ctypes.POINTER(_lib.Payloads), ctypes.POINTER(_lib.Packed)
    wpk, bad = ctypes.POINTER(_lib.PackedWideC), ctypes.POINTER(_lib.UnpackBad)
    want = {
        "clg_pack_wide": [P, col, wpk],
        "clg_pack_wide_host": [col, wpk],
        "clg_unpack_wide_host": [wpk, col, bad],
        "clg_decode_logs_columns_packed_wide": [P, P, P, u32, col, pay, pk, wpk],
        "clg_decode_host_columns_packed_wide": [P, P, P, P, u32, col, pay, pk, wpk],
    }
    for sym, args in want.items():
        fn = getattr(_lib.lib, sym)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, sym


def header_fields(name):
    h = re.sub(r"/\*.*?\*/", "", read("include", "clonos_engine.h"), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
    ctype = {"uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64,
             "clg_pack_block": None}
    count = {"CLG_WPACK_STREAMS": 26, "CLG_WPACK_STREAMS + 1": 27}
    out = []
    for ty, star, fname, arr in re.findall(r"(?:const )?(\w+)(\*?)\s+(\w+)(?:\[([\w +]+)\])?;", body):
        t = ctypes.c_void_p if star else ctype[ty]
        out.append((fname, t * count[arr] if arr else t))
    return out


def test_struct_layout_mirrors_the_header():
    from clonos_amd import _lib
    want = header_fields("clg_packed_wide")
    got = list(_lib.PackedWideC._fields_)
    assert [n for n, _ in got] == [n for n, _ in want] == ["desc", "bits", "cap_desc", "cap_bits", "out_kind", "reserved",
                                                           "n_val", "blk_base", "n_bits", "bad_row"]
    for (n, a), (_, b) in zip(got, want):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and (a is ctypes.c_void_p) == (b is ctypes.c_void_p), n
    assert ctypes.sizeof(_lib.PackedWideC) == 480
    assert "static_assert(sizeof(clg_packed_wide) == 480" in read("clonos_amd", "csrc", "engine.cpp")


def test_constants_and_what_stays():
    from clonos_amd import _lib
    h = read("include", "clonos_engine.h")
    for name, value in (("KINDS", 4), ("FIELDS", 6), ("STREAMS", 26)):
        assert re.search(r"#define\s+CLG_WPACK_%s\s+%d\b" % (name, value), h) and getattr(_lib, "WPACK_" + name) == value
    for k, name in enumerate(("RC", "V1", "VAR_OFF", "VAR_LEN", "SUB", "V0")):
        assert re.search(r"CLG_WPACK_%s = %d\b" % (name, k), h) and getattr(_lib, "WPACK_" + name) == k
    assert re.search(r"CLG_WPACK_KIND = 0\b", h) and re.search(r"CLG_WPACK_IDX = 1\b", h)
    assert (_lib.WPACK_KIND, _lib.WPACK_IDX) == (0, 1)
    # not touched
    assert ctypes.sizeof(_lib.Columns) == 232 and ctypes.sizeof(_lib.Payloads) == 64 and ctypes.sizeof(_lib.Packed) == 136
    assert ctypes.sizeof(_lib.PackBlock) == 32 and ctypes.sizeof(_lib.UnpackBad) == 16
    assert re.search(r"#define\s+CLG_PACK_STREAMS\s+5\b", h) and re.search(r"#define\s+CLG_PACK_BLOCK\s+1024\b", h)


def test_the_format_is_defined_once_for_host_and_device():
    hdr = read("clonos_amd", "csrc", "pack_wide.h")
    assert "kWPackStreams = CLG_WPACK_STREAMS" in hdr and "constexpr WPackField kWPackField[kWPackFields]" in hdr
    assert '#include "pack.h"' in hdr  # a block is packed as pack.h packs it
    for user in (("clonos_amd", "csrc", "pack_wide.hip"), ("clonos_amd", "csrc", "engine_pack.cpp"), ("tests", "wpack_host.cpp")):
        assert re.search(r'#include ".*pack_wide\.h"', read(*user)), user
    # the three scan kernels are pack.hip's, launched for both families
    hip = read("clonos_amd", "csrc", "pack_wide.hip")
    assert "k_pack_scan" not in re.sub(r"//.*", "", hip) and "launch_pack_scan" in read("clonos_amd", "csrc", "engine_pack.cpp")


def test_jni_shim_java_native_method_and_cursor():
    c = read("jni", "clonos_jni.c")
    java = read(*JDIR, "ClonosEngine.java")
    assert re.search(r"FN\(nDecodeLogsColumnsPackedWide\)", c) and re.search(r"\bclg_decode_logs_columns_packed_wide\(ENG\(e\)", c)
    assert re.search(r"static native int nDecodeLogsColumnsPackedWide\(", java)
    assert re.search(r"public EnginePackedWide decodeLogsColumnsPackedWide\(int\[\] logs, long\[\] startEpochs, "
                     r"boolean withPayloads\)", java)
    cur = read(*JDIR, "EnginePackedWide.java")
    for sig in (r"public Cursor cursor\(int s\)", r"public Row next\(Row r\)", r"public Row next\(\)",
                r"public boolean isFinished\(\)", r"public ByteBuffer payload\(Row r\)",
                r"public static boolean isDelta\(int stream\)", r"public final EnginePackedColumns narrow"):
        assert re.search(sig, cur), sig
    for field in ("kind", "rc", "sub", "idx", "v1", "varOff", "varLen", "v0", "varPos"):
        assert re.search(r"\b%s\b" % field, re.search(r"class Row \{(.*?)\}", cur, re.S).group(1)), field
    assert "LogReplayerImpl.java:61-119" in cur
    assert "native" not in re.sub(r"nativeOrder", "", cur)  # the cursor is pure Java over direct buffers
    assert "decodeLogsColumnsPackedWide(" in read("INTEGRATION.md") and "clg_decode_logs_columns_packed_wide" in read("INTEGRATION.md")


def test_the_java_scheme_table_is_the_headers():
    """EnginePackedWide.isDelta, read from its source, against the library's packer: a stream is
    DELTA exactly when a block of climbing values packs to width 0 with a non-zero ref."""
    cur = read(*JDIR, "EnginePackedWide.java")
    assert "return stream == IDX;" in cur
    assert "return field == V1 || field == VAR_OFF || (field == V0 && kind != 0);" in cur
    import numpy as np
    from _wpack_util import Wide
    from clonos_amd import pack_wide_host
    n = 8
    ramp = np.arange(n) * 5 + 100
    cols = Wide(np.repeat(np.arange(4), n), w_rc=np.tile(ramp, 4), w_v1=np.tile(ramp, 4), w_var_off=np.tile(ramp, 4),
                w_var_len=np.tile(ramp, 4), w_sub=np.tile(ramp, 4), w_v0=np.tile(ramp, 4))
    packed = pack_wide_host(cols)
    delta = [int(packed.desc["width"][packed.blk_base[s]]) == 0 for s in range(26)]
    want = [False, True] + [f in (1, 2) or (f == 5 and k != 0) for k in range(4) for f in range(6)]
    assert delta == want


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("nm") is None, reason="gcc or nm not available")
def test_shim_compiles_against_the_stub_and_defines_the_native(tmp_path):
    obj = str(tmp_path / "clonos_jni.o")
    subprocess.run(["gcc", "-c", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                    "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "clonos_jni.c"), "-o", obj], check=True)
    syms = subprocess.run(["nm", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    assert re.search(r" T \w*ClonosEngine_nDecodeLogsColumnsPackedWide$", syms, re.M), syms
    assert re.search(r" T \w*ClonosEngine_nDecodeLogsColumnsPacked$", syms, re.M)  # the existing native stays


def test_python_entry_points():
    import clonos_amd
    from clonos_amd import Engine, PackedColumns, PackedWide
    for name in ("PackedWide", "pack_wide_host", "unpack_wide_host"):
        assert name in clonos_amd.__all__ and getattr(clonos_amd, name) is not None
    for m in ("pack_wide", "pack_wide_raw"):
        assert callable(getattr(Engine, m)), m
    for fn in (Engine.decode_logs_columns, Engine.decode_host_columns):
        p = inspect.signature(fn).parameters
        assert p["pack_wide"].default is False and p["packed"].default is False and p["payloads"].default is False
        assert p["partial"].default is False
    for m in ("unpack", "rows", "kinds"):
        assert callable(getattr(PackedWide, m)), m
    assert isinstance(PackedWide.n_bytes, property)
    assert inspect.signature(PackedColumns.__init__).parameters["wide_packed"].default is None
    with pytest.raises(ValueError):
        Engine.decode_host_columns(None, b"", pack_wide=True)  # meaningful with packed=True only


def test_kernels_built_for_gfx950():
    from clonos_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_wpack_kind", b"k_wpack_scan", b"k_wpack_split", b"k_wpack_measure", b"k_wpack_write",
              b"k_pack_scan_sums", b"k_pack_scan_top", b"k_pack_scan_apply"):
        assert k in blob, k
