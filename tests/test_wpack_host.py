"""CPU: packed wide rows on the host.  The header's functions (clonos_amd/csrc/pack_wide.h, compiled
with g++ into the stand-alone program tests/wpack_host.cpp, once plainly and once with
-fsanitize=address,undefined, and run directly), and clg_pack_wide_host / clg_unpack_wide_host of
the library through ctypes over the oracle's columns: the bytes are an independent numpy packer's
(tests/_wpack_util.py), the round trip gives the seven arrays back, and on config 3 the packed wide
rows are at most a third of the plain ones."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _columns_util import oracle_batch
from _wpack_util import (FIELDS, Wide, assert_round_trip, assert_wide_equals_numpy, plain_bytes, seeded_wide,
                         width_scene, widths_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "wpack_host.cpp")
FILL = 0xA5


def test_header_functions(tmp_path):
    exe = str(tmp_path / "wpack_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 50000, r.stdout


def test_header_functions_sanitized(tmp_path):
    """The same program with the address and undefined-behaviour sanitizers, run directly (their
    runtimes linked into the program: it needs nothing preloaded)."""
    exe = str(tmp_path / "wpack_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok (\d+)\n", r.stdout), r.stdout


def span_sets():
    from clonos_amd import synth
    rng = np.random.default_rng(0x9AC)
    a = synth.random_log(1500, rng, allow_serializable=True)
    b = synth.random_log(300, rng, allow_serializable=False)
    c = bytes(synth.config3_epoch(3000, rng)[0])
    d = bytes(synth.config2_log(5000, rng)[0])
    return {
        "random_log": [a],
        "config3": [c],
        "config2": [d],
        "empty_first_middle_last": [b"", a, b"", b"", b, c, d, b""],
        "all_empty": [b"", b"", b""],
    }


SPANS = span_sets()
_COLS = {}


def columns_of(name):
    """The oracle's columns of a span set, computed once and left unchanged."""
    from clonos_amd import columnize_host
    if name not in _COLS:
        _COLS[name] = columnize_host(oracle_batch(SPANS[name]))
    return _COLS[name]


@pytest.mark.parametrize("name", sorted(SPANS))
def test_bytes_are_the_numpy_packers_and_the_round_trip_is_the_input(name):
    from clonos_amd import pack_wide_host
    cols = columns_of(name)
    packed = pack_wide_host(cols)
    assert_wide_equals_numpy(packed, cols)
    assert_round_trip(packed, cols)
    assert packed.n_wide == len(cols.w_idx)
    kinds = cols.tag[cols.w_idx] - 3
    assert (packed.kinds() == kinds).all()
    for t in range(4):
        rows = packed.rows(t)
        for k in ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0"):
            assert (rows[k] == getattr(cols, k)[kinds == t]).all(), (t, k)
    with pytest.raises(IndexError):
        packed.rows(4)


def test_every_width_against_the_numpy_packer():
    """Every width 0..64 on the i64 fields, 0..32 on RC, VAR_OFF and VAR_LEN, 0..8 on SUB, in every
    kind."""
    from clonos_amd import pack_wide_host
    for w in range(65):
        cols = width_scene(w, n=260)
        packed = pack_wide_host(cols)
        assert_wide_equals_numpy(packed, cols)
        for t in range(4):
            assert widths_of(packed, t) == [min(w, 32), w, min(w, 32), min(w, 32), min(w, 8), w], (w, t)
        assert_round_trip(packed, cols)


def test_a_kind_without_rows_and_a_field_of_zeros_cost_a_descriptor_a_block():
    from clonos_amd import pack_wide_host
    cols = Wide(np.full(2049, 2, np.uint8))  # every field zero
    packed = pack_wide_host(cols)
    assert_wide_equals_numpy(packed, cols)
    assert packed.n_val == [2049, 2049] + [0] * 12 + [2049] * 6 + [0] * 6
    assert set(packed.desc["width"][packed.blk_base[2]:]) == {0}
    # KIND is constant (width 0); IDX climbs by a constant step (width 0): no payload byte at all
    assert packed.bits.size == 0 and packed.desc.size == 3 * 8
    assert_round_trip(packed, cols)


def wide_out(nb, nbits):
    """clg_packed_wide over exactly sized host arrays filled with FILL."""
    from clonos_amd.engine import PACK_BLOCK, _packed_wide_struct
    desc, bits = np.full(nb * 32, FILL, np.uint8), np.full(nbits, FILL, np.uint8)
    return _packed_wide_struct(desc.view(PACK_BLOCK), bits), desc, bits


def test_sizes_only_and_both_capacity_errors_with_the_outputs_untouched():
    from clonos_amd import _lib, pack_wide_host
    from clonos_amd.engine import _pack_wide_in
    cols = columns_of("config3")
    want = pack_wide_host(cols)
    cin, keep = _pack_wide_in(cols)
    p = _lib.PackedWideC()
    assert _lib.lib.clg_pack_wide_host(C.byref(cin), C.byref(p)) == _lib.CLG_OK
    assert list(p.blk_base) == want.blk_base and p.n_bits == want.bits.size and list(p.n_val) == want.n_val
    assert p.bad_row == 2 ** 64 - 1
    for short in ("desc", "bits"):
        p, desc, bits = wide_out(want.desc.size - (short == "desc"), want.bits.size - (short == "bits"))
        assert _lib.lib.clg_pack_wide_host(C.byref(cin), C.byref(p)) == _lib.CLG_E_CAPACITY
        assert list(p.blk_base) == want.blk_base and p.n_bits == want.bits.size and list(p.n_val) == want.n_val
        assert (desc == FILL).all() and (bits == FILL).all()


def test_bad_row_is_the_lowest_of_several():
    from clonos_amd import ClonosError, _lib, pack_wide_host
    from clonos_amd.engine import _pack_wide_in
    cols = seeded_wide(np.arange(3000) % 4, 5)
    want = pack_wide_host(cols)
    cols.w_idx = cols.w_idx.copy()
    cols.tag = cols.tag.copy()
    cols.w_idx[2900] = cols.tag.size       # w_idx == n_rec
    cols.w_idx[1500] = cols.tag.size + 9
    cols.tag[cols.w_idx[41]] = 1           # a narrow tag
    cols.tag[cols.w_idx[1024]] = 7
    with pytest.raises(ClonosError) as ei:
        pack_wide_host(cols)
    assert ei.value.status == _lib.CLG_E_INVALID_ARG and ei.value.bad_row == 41
    cin, keep = _pack_wide_in(cols)
    p, desc, bits = wide_out(want.desc.size + 8, want.bits.size + 1024)
    assert _lib.lib.clg_pack_wide_host(C.byref(cin), C.byref(p)) == _lib.CLG_E_INVALID_ARG
    assert p.bad_row == 41 and p.n_bits == 0 and (desc == FILL).all() and (bits == FILL).all()
    keep[0][cols.w_idx[41]] = 3
    assert _lib.lib.clg_pack_wide_host(C.byref(cin), C.byref(p)) == _lib.CLG_E_INVALID_ARG and p.bad_row == 1024
    keep[0][cols.w_idx[1024]] = 5
    assert _lib.lib.clg_pack_wide_host(C.byref(cin), C.byref(p)) == _lib.CLG_E_INVALID_ARG and p.bad_row == 1500


def unpack_raw(packed, n_rows):
    """clg_unpack_wide_host into exactly sized arrays filled with FILL: status, bad, untouched?"""
    from clonos_amd import _lib
    from _wpack_util import WIDE, WIDE_DT
    c = _lib.Columns()
    arrs = []
    for name, dt in zip(WIDE, WIDE_DT):
        a = np.full(n_rows * np.dtype(dt).itemsize, FILL, np.uint8)
        arrs.append(a)
        setattr(c, name, a.ctypes.data)
    c.cap_wide = n_rows
    bad = _lib.UnpackBad()
    st = _lib.lib.clg_unpack_wide_host(C.byref(packed), C.byref(c), C.byref(bad))
    return st, (int(bad.what), int(bad.stream), int(bad.block)), all((a == FILL).all() for a in arrs)


def test_every_rejection_of_the_unpack_leaves_the_output_untouched():
    from clonos_amd import _lib, pack_wide_host
    cols = seeded_wide(np.random.default_rng(3).integers(0, 4, 2500), 7)
    good = pack_wide_host(cols)
    n = 2500
    L, B, V = _lib.UNPACK_BAD_LAYOUT, _lib.UNPACK_BAD_BLOCK, _lib.UNPACK_BAD_VALUE
    assert all(x % 1024 > 1 for x in good.n_val)  # (a length moved by one keeps its block count)

    def rejected(what, stream, block, p=None):
        st, bad, untouched = unpack_raw(p or good._struct(), n)
        assert st == _lib.CLG_E_INVALID_ARG and bad == (what, stream, block) and untouched, (st, bad, untouched)

    def layout(stream, **poke):
        p = good._struct()
        for k, (i, d) in poke.items():
            getattr(p, k)[i] += d
        rejected(L, stream, 0, p)

    st, bad, untouched = unpack_raw(good._struct(), n)
    assert st == _lib.CLG_OK and bad == (_lib.UNPACK_BAD_NONE, 0, 2 ** 64 - 1) and not untouched
    # every LAYOUT rule
    layout(0, blk_base=(0, 1))
    layout(6, blk_base=(7, 1))            # blk_base[7] - blk_base[6] is no longer stream 6's blocks
    layout(9, n_val=(9, 1024))
    layout(1, n_val=(1, -1))              # n_val[KIND] != n_val[IDX]
    layout(2 + 3, n_val=(2 + 3, -1))      # kind 0: VAR_LEN shorter than RC
    layout(2 + 18 + 5, n_val=(2 + 18 + 5, 1))
    p = good._struct()
    p.n_val[0] -= 1
    p.n_val[1] -= 1
    rejected(L, 0, 0, p)                  # the kinds' n_val no longer sum to n_val[KIND]
    p = good._struct()
    p.cap_desc -= 1
    rejected(L, 0, 0, p)
    p = good._struct()
    p.n_bits = p.cap_bits + 16
    rejected(L, 0, 0, p)
    # a block rule, and that it comes before a value finding in a lower stream
    desc = good.desc
    for field, value, stream, block in (("width", 65, 1, 2), ("count", 1023, 0, 0), ("pos", 8, 4, 0)):
        good.desc = desc.copy()
        good.desc[field][good.blk_base[stream] + block] = value
        rejected(B, stream, block)
    good.desc = desc.copy()
    good.desc["ref"][good.blk_base[0]] = 3        # kinds up to 6
    good.desc["width"][good.blk_base[20]] = 99
    rejected(B, 20, 0)
    # a KIND of 4
    good.desc = desc.copy()
    good.desc["ref"][good.blk_base[0] + 1] = 1    # block 1's kinds become 1 .. 4
    rejected(V, 0, 1)
    # a histogram mismatch: every KIND is a kind, one row's is another kind's
    good.desc = desc
    bits = good.bits
    good.bits = bits.copy()
    good.bits[0] = (int(bits[0]) & 0xFC) | ((int(bits[0]) + 1) & 3)
    rejected(V, 0, 0)
    good.bits = bits
    # a u32 out of range, either side, in VAR_OFF (DELTA: through first) and VAR_LEN (FOR: through ref)
    for stream, field, value in ((2 + 6 + 2, "first", 2 ** 32 - 4), (2 + 6 + 2, "first", -1), (2 + 12 + 3, "ref", 2 ** 32 - 1),
                                 (2 + 12 + 3, "ref", -1), (1, "first", 2 ** 32)):
        good.desc = desc.copy()
        good.desc[field][good.blk_base[stream]] = value
        rejected(V, stream, 0)
    # ... and the other elements' bounds
    for stream, value in ((2 + 0, 2 ** 31 - 5), (2 + 0, -2 ** 31 - 1), (2 + 18 + 4, 255)):
        good.desc = desc.copy()
        good.desc["ref"][good.blk_base[stream]] = value
        rejected(V, stream, 0)
    good.desc = desc
    # a capacity one short: the rows are filled and nothing is written
    st, bad, untouched = unpack_raw(good._struct(), n - 1)
    assert st == _lib.CLG_E_CAPACITY and untouched


def test_config3_wide_rows_pack_to_at_most_a_third():
    """The format's point.  Three spans of synth.config3_epoch(60000), seed 1: the packed wide rows
    against the plain seven arrays at 33 B a row.  Measured 0.218 with an independent packer when the
    format was designed; the bound of one third leaves room for the generator's w_rc, which it draws
    at random over 31 bits (real record counts are counters).  The value this test sees is recorded
    in DESIGN.md 4.8."""
    from clonos_amd import columnize_host, pack_wide_host, synth
    rng = np.random.default_rng(1)
    cols = columnize_host(oracle_batch([bytes(synth.config3_epoch(60000, rng)[0]) for _ in range(3)]))
    packed = pack_wide_host(cols)
    plain = plain_bytes(cols)
    ratio = packed.n_bytes / plain
    rc = sum(int(np.asarray(packed.desc["width"][packed.blk_base[2 + FIELDS * t]:packed.blk_base[3 + FIELDS * t]],
                            np.int64).sum()) * 128 for t in range(4))
    print(f"config 3, 3 x 60000 records: {len(cols.w_idx)} wide rows, packed {packed.n_bytes} B, plain {plain} B, "
          f"ratio {ratio:.4f}; w_rc's streams about {rc} B")
    assert ratio <= 1 / 3
    assert_round_trip(packed, cols)
