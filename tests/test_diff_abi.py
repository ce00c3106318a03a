"""CPU: the log comparison's additions to the C-ABI -- the clg_diff struct's size and layout as
the header declares it, and the new symbols in the library and the Python mirror."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "clonos_engine.h")) as f:
        return f.read()


def test_clg_diff_struct():
    from clonos_amd import DIFF, _lib
    m = re.search(r"typedef struct clg_diff \{(.*?)\} clg_diff;", header(), re.S)
    assert m, "clg_diff not declared"
    fields = re.findall(r"uint64_t\s+(\w+);", m.group(1))
    assert fields == ["lcp", "len_log", "len_ref"]
    assert C.sizeof(_lib.Diff) == 24 and [f[0] for f in _lib.Diff._fields_] == fields
    assert DIFF.itemsize == 24 and list(DIFF.names) == fields
    assert [DIFF.fields[n][1] for n in fields] == [0, 8, 16]


def test_symbols_present():
    from clonos_amd import _lib
    h = header()
    for sym in ("clg_diff_logs", "clg_lcp_host"):
        assert re.search(r"\bint %s\(" % sym, h), sym
        assert sym in _lib.EXPORTED
        assert hasattr(_lib.lib, sym)
    assert re.search(r"#define\s+CLG_ABI_VERSION\s+6\b", h)  # additions only: the version stays
