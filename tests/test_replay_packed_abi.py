"""CPU: the packed form of replay preparation in the C-ABI -- the two symbols in the header, in the
library and in the Python mirror's table, the struct's layout, the JNI shim and the Java natives,
the Python entry point, the one-launch pack's constants and its kernel in the code object; the
version stays."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("clg_replay_prepare_columns_packed", "clg_replay_prepare_columns_packed_device")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_in_header_library_and_mirror():
    from clonos_amd import _lib
    h = read("include", "clonos_engine.h")
    flat = re.sub(r"\s+", " ", h)
    for sym in SYMBOLS:
        assert ("int %s(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_packed_out* out);" % sym) in flat
        assert sym in _lib.EXPORTED
        assert hasattr(_lib.lib, sym)
        assert getattr(_lib.lib, sym).argtypes is not None, sym  # a prototype in the table
    assert re.search(r"#define\s+CLG_ABI_VERSION\s+6\b", h)  # additions only: the version stays
    assert _lib.lib.clg_abi_version() == 6


def test_struct_layout_mirrors_the_header():
    """Field order and types of clg_replay_packed_out, read from the header, against the ctypes
    mirror; from buffer_sizes on the fields are clg_replay_out's."""
    from clonos_amd import _lib
    h = re.sub(r"/\*.*?\*/", "", read("include", "clonos_engine.h"), flags=re.S)

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
        return re.findall(r"(\w+)(\*?)\s+(\w+);", body)

    want = fields("clg_replay_packed_out")
    got = list(_lib.ReplayPackedOut._fields_)
    assert [n for n, _ in got] == [n for _, _, n in want]
    for (n, t), (ty, star, _) in zip(got, want):
        assert ctypes.sizeof(t) == 8, n
        assert bool(star) == (t is not ctypes.c_uint64), n
        assert star or ty == "uint64_t", n
    assert [(f[0], f[2]) for f in want[:4]] == [("clg_columns", "sizes"), ("clg_payloads", "var"), ("clg_packed", "narrow"),
                                                ("clg_packed_wide", "wide")]
    assert want[4:] == fields("clg_replay_out")[2:]
    assert ctypes.sizeof(_lib.ReplayPackedOut) == 88
    for k, (n, _) in enumerate(got):
        assert getattr(_lib.ReplayPackedOut, n).offset == 8 * k, n
    assert [n for n, _ in _lib.ReplayOut._fields_][2:] == [n for n, _ in got][4:]


def test_jni_shim_and_java_natives():
    c = read("jni", "clonos_jni.c")
    jdir = ("jni", "java", "org", "apache", "flink", "runtime", "causal")
    java = read(*jdir, "engine", "ClonosEngine.java")
    assert re.search(r"FN\(nReplayPrepareColumnsPacked\)", c)
    body = c[c.index("FN(nReplayPrepareColumnsPacked)"):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"\bclg_replay_prepare_columns_packed\(ENG\(e\)", body)
    assert re.search(r"static native int nReplayPrepareColumnsPacked\(", java)
    assert re.search(r"public EnginePackedWide replayPrepareColumnsPacked\(", java)
    prep = read(*jdir, "recovery", "EngineReplayPreparation.java")
    assert re.search(r"public static EngineReplayPreparation packed\(", prep)
    assert re.search(r"public EnginePackedColumns mainPacked\(", prep)
    assert re.search(r"public EnginePackedWide mainPackedWide\(", prep)
    doc = read("INTEGRATION.md")
    assert "mainPackedWide" in doc and "EngineReplayPreparation.packed" in doc and "clg_replay_prepare_columns_packed" in doc


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_shim_still_compiles_against_the_stub():
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                    "-I", os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "clonos_jni.c")], check=True)


def test_python_entry_point_takes_packed_and_pack_wide():
    from clonos_amd import replay
    p = inspect.signature(replay.prepare_replay_columns).parameters
    assert p["packed"].default is False and p["pack_wide"].default is False
    with pytest.raises(ValueError):
        replay.prepare_replay_columns(None, [], pack_wide=True)


def test_one_launch_constants_meet_their_floors():
    """kPackSmallBlocks holds the five streams of kColSmallRecords records (the tags' blocks and, for
    the four classes that share the records, one block a whole 1024 and one more each);
    kWPackSmallRows holds kPaySmallRows rows."""
    def const(header, name):
        return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, read("clonos_amd", "csrc", header)).group(1))

    records = const("columns.h", "kColSmallRecords")
    assert records == 32769
    assert const("pack.h", "kPackSmallBlocks") >= (records + 1023) // 1024 + records // 1024 + 4 == 69
    assert const("pack_wide.h", "kWPackSmallRows") >= const("payload.h", "kPaySmallRows") == 8193
    eng = read("clonos_amd", "csrc", "engine_pack.cpp")
    assert "static_assert(clg::kPackSmallBlocks >=" in eng and "static_assert(clg::kWPackSmallRows >= clg::kPaySmallRows" in eng
    assert "CLONOS_PACK_SMALL" in read("clonos_amd", "csrc", "engine_impl.h")


def test_kernel_built_for_gfx950():
    from clonos_amd import _lib
    assert b"k_pack_small" in open(_lib.LIB_PATH, "rb").read()
