"""CPU: packed typed columns on the host.  The header's functions (clonos_amd/csrc/pack.h, compiled
with g++ into the stand-alone program tests/pack_host.cpp, once plainly and once with
-fsanitize=address,undefined, and run directly), and clg_pack_columns_host /
clg_unpack_columns_host of the library through ctypes over the oracle's columns: the bytes are an
independent numpy packer's (tests/_pack_util.py), the round trip gives the columns back, and a
ColumnReplayer over PackedColumns.span(s) yields the oracle's determinants."""
import os
import re
import subprocess

import numpy as np
import pytest

from _columns_util import assert_columns_equal, oracle_batch
from _pack_util import STREAMS, Narrow, assert_packed_equals_numpy, values_of_width

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pack_host.cpp")


def test_header_functions(tmp_path):
    exe = str(tmp_path / "pack_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 100000, r.stdout


def test_header_functions_sanitized(tmp_path):
    """The same program with the address and undefined-behaviour sanitizers, run directly (their
    runtimes linked into the program: it needs nothing preloaded)."""
    exe = str(tmp_path / "pack_host_san")
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
        batch = oracle_batch(SPANS[name])
        _COLS[name] = (columnize_host(batch), batch)
    return _COLS[name]


@pytest.mark.parametrize("name", sorted(SPANS))
def test_bytes_are_the_numpy_packers_and_the_round_trip_is_the_input(name):
    from clonos_amd import pack_columns_host
    cols, _ = columns_of(name)
    packed = pack_columns_host(cols)
    assert_packed_equals_numpy(packed, cols)
    assert_columns_equal(packed.unpack(), cols)
    assert packed.n_rec == cols.n_rec and packed.n_spans == cols.n_spans
    assert packed.n_val == [cols.n_rec] + [len(getattr(cols, k)) for k, _, _ in STREAMS[1:]]


def test_every_width_against_the_numpy_packer():
    from clonos_amd import pack_columns_host
    rng = np.random.default_rng(0x51DE)
    for w in range(65):
        cols = Narrow(tag=values_of_width(rng, np.uint8, min(w, 3), 2049, vmin=0, vmax=7),
                      order=values_of_width(rng, np.int8, min(w, 8), 1025),
                      timestamp=values_of_width(rng, np.int64, w, 1024, delta=True),
                      rng=values_of_width(rng, np.int32, min(w, 32), 1023),
                      buffer_built=values_of_width(rng, np.int32, min(w, 32), 3))
        packed = pack_columns_host(cols)
        assert_packed_equals_numpy(packed, cols)
        assert packed.desc["width"][packed.blk_base[2]] == w
        back = packed.unpack()
        for name, _, _ in STREAMS:
            assert (getattr(back, name) == getattr(cols, name)).all(), (w, name)


@pytest.mark.parametrize("name", ["empty_first_middle_last", "config3"])
def test_span_views_unpack_only_their_ranges(name):
    from clonos_amd import pack_columns_host
    cols, _ = columns_of(name)
    packed = pack_columns_host(cols)
    for s in range(cols.n_spans):
        got, want = packed.span(s), cols.span(s)
        for f in ("tag", "order", "timestamp", "rng", "buffer_built"):
            a, b = getattr(got, f), getattr(want, f)
            assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (s, f)
        assert (got.w0, got.n_wide) == (want.w0, want.n_wide)
    with pytest.raises(IndexError):
        packed.span(cols.n_spans)


def test_a_span_view_reads_no_block_outside_its_ranges():
    """Every descriptor outside the blocks of one span's ranges is made malformed: the span's view
    still unpacks, the whole unpack does not."""
    from clonos_amd import pack_columns_host
    cols, _ = columns_of("empty_first_middle_last")
    s = 5  # the config 3 span
    packed = pack_columns_host(cols)
    want = packed.span(s)
    a, b = cols.span_base[s].astype(np.int64), cols.span_base[s + 1].astype(np.int64)
    cut = [(int(a.sum()), int(b.sum()))] + [(int(a[c]), int(b[c])) for c in range(4)]
    desc = packed.desc.copy()
    for c, (lo, hi) in enumerate(cut):
        keep = set(range(lo // 1024, (hi - 1) // 1024 + 1)) if hi > lo else set()
        for blk in range(packed.blk_base[c + 1] - packed.blk_base[c]):
            if blk not in keep:
                desc["width"][packed.blk_base[c] + blk] = 99
    packed.desc = desc
    got = packed.span(s)
    for f in ("tag", "order", "timestamp", "rng", "buffer_built"):
        assert (getattr(got, f) == getattr(want, f)).all(), f
    from clonos_amd import ClonosError
    with pytest.raises(ClonosError):
        packed.unpack()


def drive(rep, D):
    got = []
    while not rep.isFinished():
        t = rep.next_tag()
        if t == D.ORDER:
            got.append(D.OrderDeterminant(rep.replayNextChannel()))
        elif t == D.TIMESTAMP:
            got.append(D.TimestampDeterminant(rep.replayNextTimestamp()))
        elif t == D.RNG:
            got.append(D.RNGDeterminant(rep.replayRandomInt()))
        elif t == D.BUFFER_BUILT:
            got.append(D.BufferBuiltDeterminant(rep.replayNextBufferSize()))
        elif t == D.SERIALIZABLE:
            got.append(D.SerializableDeterminant(rep.replaySerializableDeterminant()))
        else:
            got.append(rep.triggerAsyncEvent(rep.record_count_target()))
    return got


@pytest.mark.parametrize("name", ["random_log", "empty_first_middle_last"])
def test_column_replayer_over_packed_spans_yields_the_oracles_determinants(name):
    from clonos_amd import determinants as D
    from clonos_amd import pack_columns_host
    from clonos_amd.replay import ColumnReplayer
    cols, batch = columns_of(name)
    packed = pack_columns_host(cols)
    for s in range(cols.n_spans):
        assert drive(ColumnReplayer(packed, s), D) == batch.determinants(s)


def test_sizes_only_capacity_and_rejections_through_ctypes():
    import ctypes as C
    from clonos_amd import _lib, pack_columns_host
    from clonos_amd.engine import PACK_BLOCK, _pack_in, _packed_struct
    cols, _ = columns_of("config3")
    want = pack_columns_host(cols)
    cin, keep = _pack_in(cols)
    p = _lib.Packed()
    assert _lib.lib.clg_pack_columns_host(C.byref(cin), C.byref(p)) == _lib.CLG_OK
    assert list(p.blk_base) == want.blk_base and p.n_bits == want.bits.size and list(p.n_val) == want.n_val
    for short in ("desc", "bits"):
        desc = np.full((want.desc.size - (short == "desc")) * 32, 0xA5, np.uint8)
        bits = np.full(want.bits.size - (short == "bits"), 0xA5, np.uint8)
        p = _packed_struct(desc.view(PACK_BLOCK), bits)
        assert _lib.lib.clg_pack_columns_host(C.byref(cin), C.byref(p)) == _lib.CLG_E_CAPACITY
        assert list(p.blk_base) == want.blk_base and p.n_bits == want.bits.size
        assert (desc == 0xA5).all() and (bits == 0xA5).all()
    # the unpack validates what it reads
    out = np.zeros(want.n_val[3], np.int32)
    good = want._struct()
    assert _lib.lib.clg_unpack_columns_host(C.byref(good), 3, 0, out.size, out.ctypes.data) == _lib.CLG_OK
    assert (out == cols.rng).all()
    assert _lib.lib.clg_unpack_columns_host(C.byref(good), 3, 1, out.size, out.ctypes.data) == _lib.CLG_E_INVALID_ARG
    assert _lib.lib.clg_unpack_columns_host(C.byref(good), 5, 0, 0, out.ctypes.data) == _lib.CLG_E_INVALID_ARG
    bad = want.desc.copy()
    bad["ref"][want.blk_base[3]] = (1 << 31) - 1  # values past int32
    want.desc = bad
    p = want._struct()
    assert _lib.lib.clg_unpack_columns_host(C.byref(p), 3, 0, out.size, out.ctypes.data) == _lib.CLG_E_INVALID_ARG


def test_config2_delivers_under_a_fifth_of_the_plain_columns():
    """The format's point: on config 2 the packed form is 0.091 of the plain columns (tags 1 bit,
    channels 2 bits, timestamps 3 bits from their deltas, 32 bytes a block).  The cap guards the
    format, not a speed."""
    from clonos_amd import columnize_host, pack_columns_host, synth
    rng = np.random.default_rng(2)
    cols = columnize_host(oracle_batch([bytes(synth.config2_log(1 << 20, rng)[0])]))
    packed = pack_columns_host(cols)
    ratio = packed.n_bytes / cols.n_bytes
    print(f"config 2, 1 M records: packed {packed.n_bytes} B, plain {cols.n_bytes} B, ratio {ratio:.4f}")
    assert ratio < 0.2
    w = packed.desc["width"]
    assert set(w[packed.blk_base[0]:packed.blk_base[1]]) == {1} and set(w[packed.blk_base[1]:packed.blk_base[2]]) == {2}
    assert set(w[packed.blk_base[2]:packed.blk_base[3]]) == {3}
    assert (packed.unpack_stream(2) == cols.timestamp).all()
