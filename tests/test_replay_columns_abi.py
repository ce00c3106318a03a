"""CPU: the columns form of replay preparation in the C-ABI -- the two symbols in the header, in
the library and in the Python mirror's table, the struct's layout, the JNI shim and the Java
native, the Python entry point, the one-launch kernels in the code object; the version stays."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("clg_replay_prepare_columns", "clg_replay_prepare_columns_device")


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
    assert ("int clg_replay_prepare_columns(clg_engine* e, const clg_replay_vertex* v, uint32_t n, "
            "clg_replay_columns_out* out);") in h
    assert ("int clg_replay_prepare_columns_device(clg_engine* e, const clg_replay_vertex* v, uint32_t n, "
            "clg_replay_columns_out* out);") in h


def test_struct_layout_mirrors_the_header():
    """Field order and types of clg_replay_columns_out, read from the header, against the ctypes
    mirror; from buffer_sizes on the fields are clg_replay_out's."""
    from clonos_amd import _lib
    h = re.sub(r"/\*.*?\*/", "", read("include", "clonos_engine.h"), flags=re.S)

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
        return re.findall(r"(\w+)(\*?)\s+(\w+);", body)

    want = fields("clg_replay_columns_out")
    got = list(_lib.ReplayColumnsOut._fields_)
    assert [n for n, _ in got] == [n for _, _, n in want]
    for (n, t), (ty, star, _) in zip(got, want):
        assert ctypes.sizeof(t) == 8, n
        assert bool(star) == (t is not ctypes.c_uint64), n
        assert star or ty == "uint64_t", n
    assert [f[2] for f in want[:2]] == ["main", "var"] and [f[0] for f in want[:2]] == ["clg_columns", "clg_payloads"]
    assert want[2:] == fields("clg_replay_out")[2:]
    assert ctypes.sizeof(_lib.ReplayColumnsOut) == 72
    for k, (n, _) in enumerate(got):
        assert getattr(_lib.ReplayColumnsOut, n).offset == 8 * k, n
    assert [n for n, _ in _lib.ReplayOut._fields_][2:] == [n for n, _ in got][2:]


def test_jni_shim_and_java_natives():
    c = read("jni", "clonos_jni.c")
    jdir = ("jni", "java", "org", "apache", "flink", "runtime", "causal")
    java = read(*jdir, "engine", "ClonosEngine.java")
    assert re.search(r"FN\(nReplayPrepareColumns\)", c)
    body = c[c.index("FN(nReplayPrepareColumns)"):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"\bclg_replay_prepare_columns\(ENG\(e\)", body)
    assert re.search(r"static native int nReplayPrepareColumns\(", java)
    assert re.search(r"public EngineDecodedColumns replayPrepareColumns\(", java)
    prep = read(*jdir, "recovery", "EngineReplayPreparation.java")
    assert re.search(r"public static EngineReplayPreparation columns\(", prep)
    assert re.search(r"public EngineDecodedColumns mainColumns\(", prep)
    doc = read("INTEGRATION.md")
    assert "mainColumns" in doc and "EngineReplayPreparation.columns" in doc


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_shim_still_compiles_against_the_stub():
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                    "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "clonos_jni.c")], check=True)


def test_python_entry_point():
    import dataclasses
    from clonos_amd import replay
    assert callable(replay.prepare_replay_columns)
    assert dataclasses.is_dataclass(replay.ReplayColumns)
    names = [f.name for f in dataclasses.fields(replay.ReplayColumns)]
    assert names[:7] == ["main", "sizes", "base", "count", "status", "err_off", "err_tag"]
    assert callable(replay.ReplayColumns.replayer) and callable(replay.ReplayColumns.vertex)


def test_small_constants_keep_their_floors():
    col, pay = read("clonos_amd", "csrc", "columns.h"), read("clonos_amd", "csrc", "payload.h")

    def const(src, name):
        return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))

    assert const(col, "kColSmallRecords") >= 8 * const(col, "kColTile") + 1
    assert const(col, "kColSmallSpans") >= 64
    tile = const(pay, "kPayThreads") * const(pay, "kPayPerThread")
    rounds = const(pay, "kPayScanThreads") // const(pay, "kPayThreads") * tile
    assert const(pay, "kPaySmallRows") >= 2 * rounds + 1
    assert const(pay, "kPaySmallBytes") > 0


def test_kernels_built_for_gfx950():
    from clonos_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_col_small", b"k_pay_small"):
        assert k in blob, k
