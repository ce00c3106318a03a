"""CPU: the packed payload column's ABI.  The header, the library and the ctypes mirror agree on
the four entry points, the struct and the two new constants, and nothing older moved: the ABI
version stays 6."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("clg_pack_payloads", "clg_pack_payloads_host", "clg_unpack_payloads", "clg_unpack_payloads_host")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_symbols_are_declared_exported_and_mirrored():
    from clonos_amd import _lib
    h = re.sub(r"/\*.*?\*/", "", read("include", "clonos_engine.h"), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, h), n
        assert hasattr(raw, n) and n in _lib.EXPORTED
    P, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    pp, pay, bad = ctypes.POINTER(_lib.PackedPayloadsC), ctypes.POINTER(_lib.Payloads), ctypes.POINTER(_lib.UnpackBad)
    want = {
        "clg_pack_payloads": [P, P, P, u64, u32, pp],
        "clg_pack_payloads_host": [P, P, u64, pp],
        "clg_unpack_payloads": [P, pp, P, u32, pay, bad],
        "clg_unpack_payloads_host": [pp, P, pay, bad],
    }
    for sym, args in want.items():
        fn = getattr(_lib.lib, sym)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, sym
    assert _lib.lib.clg_abi_version() == 6 and re.search(r"#define CLG_ABI_VERSION 6\b", h)


def test_struct_layout_and_constants():
    from clonos_amd import _lib
    h = read("include", "clonos_engine.h")
    body = re.search(r"typedef struct clg_packed_payloads \{(.*?)\} clg_packed_payloads;", h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(clg_pack_block\*|uint8_t\*|uint64_t|uint32_t)\s+(.*)", decl.strip(), flags=re.S)
        if m:
            fields += [(n.strip(), 8 if m.group(1) != "uint32_t" else 4) for n in m.group(2).split(",")]
    assert fields == [(n, ctypes.sizeof(t)) for n, t in _lib.PackedPayloadsC._fields_]
    assert [n for n, _ in fields] == ["desc", "bits", "tail", "cap_desc", "cap_bits", "cap_tail", "out_kind", "reserved",
                                      "n_rows", "n_var", "n_bits", "n_tail", "bad_row"]
    assert ctypes.sizeof(_lib.PackedPayloadsC) == 96
    assert "static_assert(sizeof(clg_packed_payloads) == 96" in read("clonos_amd", "csrc", "engine.cpp")
    assert re.search(r"#define CLG_PPAY_STREAM 64\b", h) and _lib.PPAY_STREAM == 64
    assert re.search(r"CLG_UNPACK_BAD_TOTAL = 4\b", h) and _lib.UNPACK_BAD_TOTAL == 4
    # not touched
    assert ctypes.sizeof(_lib.UnpackBad) == 16 and ctypes.sizeof(_lib.Payloads) == 64 and ctypes.sizeof(_lib.Packed) == 136
    assert ctypes.sizeof(_lib.PackedWideC) == 480


def test_the_format_is_defined_once_and_exported_from_the_package():
    import clonos_amd
    for name in ("PackedPayloads", "pack_payloads_host", "unpack_payloads_host"):
        assert name in clonos_amd.__all__ and hasattr(clonos_amd, name)
    for name in ("pack_payloads", "unpack_payloads"):
        assert callable(getattr(clonos_amd.Engine, name))
    hdr = read("clonos_amd", "csrc", "ppay.h")
    for fn in ("ppay_hash", "ppay_row_bad", "ppay_bits_bound", "ppay_tail_bound"):
        assert re.search(r"CLG_PACK_HD \w+ %s\(" % fn, hdr), fn
    for user in (("clonos_amd", "csrc", "ppay.hip"), ("clonos_amd", "csrc", "engine_pack.cpp"), ("tests", "ppay_host.cpp")):
        assert re.search(r'#include "(\.\./clonos_amd/csrc/)?ppay\.h"', read(*user)), user
    hip = re.sub(r"//.*", "", read("clonos_amd", "csrc", "ppay.hip"))
    for k in ("k_ppay_lcp", "k_ppay_scan", "k_ppay_write", "k_ppay_in", "k_ppay_in_scan", "k_ppay_out"):
        assert re.search(r"__global__[^;{]*\b%s\(" % k, hip), k
    # one anchor step for both directions; the device hash is the header's
    assert len(re.findall(r"\bppay_anchors\(", hip)) == 4 and "ppay_hash(" in hip
    from _ppay_util import HASH_MUL, HASH_SHIFT
    assert "0x%Xu" % HASH_MUL in hdr and "kPpayHashShift = %d" % HASH_SHIFT in hdr


def test_kernels_are_in_the_library():
    from clonos_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_ppay_lcp", b"k_ppay_scan", b"k_ppay_write", b"k_ppay_in", b"k_ppay_out"):
        assert k in blob, k
