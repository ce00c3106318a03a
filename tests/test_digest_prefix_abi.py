"""CPU: the prefix digests' additions to the C-ABI -- the three symbols in the header, in the
library, in the Python mirror's table and in the JNI shim; the version stays."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("clg_digest_prefixes", "clg_digest_epochs", "clg_digest_prefixes_host")


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


def test_header_signatures():
    h = re.sub(r"\s+", " ", read("include", "clonos_engine.h"))
    assert ("int clg_digest_prefixes(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, "
            "const uint64_t* cut_first, const uint32_t* cuts, clg_digest* out);") in h
    assert ("int clg_digest_epochs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, "
            "uint64_t cap, uint64_t* first, int64_t* epoch_id, clg_digest* out, uint64_t* total);") in h
    assert ("int clg_digest_prefixes_host(const uint8_t* bytes, uint64_t n, const uint32_t* cuts, uint32_t n_cuts, "
            "clg_digest* out);") in h


def test_jni_shim_and_java_natives():
    c = read("jni", "clonos_jni.c")
    java = read("jni", "java", "org", "apache", "flink", "runtime", "causal", "engine", "ClonosEngine.java")
    for native, sym in (("nDigestPrefixes", "clg_digest_prefixes"), ("nDigestEpochs", "clg_digest_epochs")):
        assert re.search(r"FN\(%s\)" % native, c) and re.search(r"\b%s\(ENG\(e\)" % sym, c), native
        assert re.search(r"static native int %s\(" % native, java), native
    assert re.search(r"public long\[\] digestPrefixes\(", java)
    assert re.search(r"public long\[\]\[\] digestEpochs\(", java)


def test_python_entry_points():
    import clonos_amd
    from clonos_amd import Engine
    from clonos_amd.dist import EngineIO
    assert callable(clonos_amd.digest_prefixes_host)
    assert callable(Engine.digest_prefixes) and callable(Engine.digest_epochs)
    assert callable(EngineIO.digest_prefixes)
