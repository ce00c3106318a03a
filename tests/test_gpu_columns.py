"""GPU: typed replay columns (clg_columnize, clg_decode_logs_columns, clg_decode_host_columns).
Every result is compared element for element with columnize_host on the same decoded batch, and
through to_soa() with the plain decode of the same logs, which the rest of the suite holds to
the oracle.  T = kColTile (records per tile), S = the scan workgroup's threads (columns.h)."""
import re
import os

import numpy as np
import pytest

from _columns_util import (COLS, GuardedColumns, assert_columns_equal, exact_caps, made_batch, oracle_batch,
                           to_device)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    src = open(os.path.join(ROOT, "clonos_amd", "csrc", "columns.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


T = _header_constant("kColTile")
S = _header_constant("kColScanThreads")
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)


@pytest.fixture(scope="module")
def eng():
    from clonos_amd import Engine
    e = Engine(segment_bytes=4096, pool_segments=4096, timing=True)
    yield e
    e.close()


def pattern_tags(pattern, n, rng):
    if pattern == "alternate":
        return (np.arange(n) & 1).astype(np.uint8)
    if pattern == "order_then_timestamps":  # the i8 column's tile bases fall at every residue mod 16
        t = np.ones(n, np.uint8)
        t[:1] = 0
        return t
    if pattern == "wide":
        return rng.integers(3, 7, n).astype(np.uint8)
    return np.full(n, {"order": 0, "timestamp": 1, "rng": 2, "buffer_built": 7}[pattern], np.uint8)


def run_columnize(eng, batch, kind="device", caps=None):
    """clg_columnize of the uploaded batch into guarded columns; returns (status, GuardedColumns)."""
    from clonos_amd import _lib
    d, keep = to_device(batch)
    n_spans = len(batch.span_rec_base) - 1
    if caps is None:  # exact capacities, from a sizes-only call
        c = _lib.Columns()
        sb = np.zeros((n_spans + 1) * 5, np.uint64)
        c.span_base = sb.ctypes.data
        eng.columnize(d, batch.span_rec_base, c)
        assert int(c.n_rec) == batch.n_rec
        caps = exact_caps(batch.n_rec, c.n_class)
    g = GuardedColumns(kind, caps, n_spans)
    base = np.ascontiguousarray(batch.span_rec_base, np.uint64)
    st = _lib.lib.clg_columnize(eng.handle, d, base.ctypes.data, n_spans, g.c)
    del keep
    return st, g


def check_against_host(eng, batch, kind="device"):
    from clonos_amd import columnize_host
    want = columnize_host(batch)
    st, g = run_columnize(eng, batch, kind)
    try:
        assert st == 0
        assert g.guards_intact()
        got = g.result()
        assert_columns_equal(got, want)
        back = got.to_soa()
        assert (back.tag == batch.tag).all() and (back.v0 == batch.v0).all()
        assert (back.span_rec_base == np.asarray(batch.span_rec_base)).all()
        return got
    finally:
        g.free()


@pytest.mark.parametrize("pattern", ["order", "timestamp", "rng", "buffer_built", "wide", "alternate",
                                     "order_then_timestamps"])
def test_columnize_patterns_at_every_size(eng, pattern):
    rng = np.random.default_rng(len(pattern))
    for n in SIZES:
        check_against_host(eng, made_batch(pattern_tags(pattern, n, rng), rng))


def test_order_column_bases_at_every_residue(eng):
    """k Orders, then only Timestamps, then Orders again in later tiles: the i8 column's tile bases
    fall at every residue mod 16."""
    rng = np.random.default_rng(16)
    for k in range(16):
        t = np.ones(3 * T + 9, np.uint8)
        t[:k] = 0
        t[T + 5:T + 40] = 0
        t[2 * T + 1:] = 0
        check_against_host(eng, made_batch(t, rng))


def test_spans(eng):
    rng = np.random.default_rng(7)
    n = 2 * T + 200 + 3 * T + 5
    base = [0, 0, 0]                                   # empty spans first
    base += [T - 1, T, T + 1]                          # a boundary on a tile edge, and one record either side
    base += [T + 1, T + 1]                             # empty spans in the middle
    base += list(range(T + 10, T + 10 + 70))           # more than 64 one-record spans inside one tile
    base += [2 * T + 200]                              # then one span over 3T + 5 records
    base += [n, n, n]                                  # empty spans last
    tag = rng.integers(0, 8, n).astype(np.uint8)
    got = check_against_host(eng, made_batch(tag, rng, base))
    assert got.n_spans == len(base) - 1
    assert got.span(0).tag.size == 0 and got.span(got.n_spans - 1).tag.size == 0
    s = base.index(2 * T + 200)
    assert got.span(s).tag.size == 3 * T + 5


def test_more_tiles_than_one_scan_round(eng):
    rng = np.random.default_rng(99)
    n = (S + 3) * T + 7
    tag = rng.choice(np.arange(8, dtype=np.uint8), n, p=[.3, .3, .1, .02, .02, .03, .03, .2])
    base = [0, 5, S * T - 1, S * T, S * T + 1, n]
    check_against_host(eng, made_batch(tag, rng, base))


@pytest.mark.parametrize("kind", ["device", "mapped", "host"])
def test_output_kinds_give_identical_columns(eng, kind):
    rng = np.random.default_rng(3)
    tag = rng.integers(0, 8, 2 * T + 1).astype(np.uint8)
    check_against_host(eng, made_batch(tag, rng, [0, 7, T, 2 * T + 1]), kind)


def test_mapped_input(eng):
    """The decoded batch itself in registered host memory (in.out_kind CLG_MEM_MAPPED)."""
    import mmap
    from clonos_amd import _lib, columnize_host
    rng = np.random.default_rng(4)
    b = made_batch(rng.integers(0, 8, T + 77).astype(np.uint8), rng)
    region = np.frombuffer(mmap.mmap(-1, 1 << 20), np.uint8)
    _lib.check(_lib.lib.clg_host_register(region.ctypes.data, region.size))
    try:
        d, at = _lib.Decoded(), 0
        for k in ("tag", "v0", "w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub"):
            a = np.ascontiguousarray(getattr(b, k)).view(np.uint8)
            region[at:at + a.size] = a
            setattr(d, k, region.ctypes.data + at)
            at = (at + a.size + 63) & ~63
        d.n_rec, d.n_wide, d.out_kind = b.n_rec, len(b.w_idx), _lib.CLG_MEM_MAPPED
        assert_columns_equal(eng.columnize(d, b.span_rec_base), columnize_host(b))
    finally:
        _lib.lib.clg_host_unregister(region.ctypes.data)


def test_capacity_and_sizes_only(eng):
    from clonos_amd import _lib, columnize_host
    rng = np.random.default_rng(5)
    tag = rng.integers(0, 8, T + 300).astype(np.uint8)
    b = made_batch(tag, rng, [0, 100, T + 300])
    want = columnize_host(b)
    totals = [len(want.order), len(want.timestamp), len(want.rng), len(want.buffer_built), len(want.w_idx)]
    # sizes only: the totals and span_base, no column
    d, keep = to_device(b)
    c = _lib.Columns()
    sb = np.zeros(15, np.uint64)
    c.span_base = sb.ctypes.data
    eng.columnize(d, b.span_rec_base, c)
    assert int(c.n_rec) == b.n_rec and [int(x) for x in c.n_class] == totals
    assert (sb.reshape(3, 5) == want.span_base).all()
    # one element short in each column in turn
    for name, _, _, _ in COLS:
        caps = exact_caps(b.n_rec, totals)
        caps[name] -= 1
        for kind in ("device", "host"):
            st, g = run_columnize(eng, b, kind, caps)
            try:
                assert st == _lib.CLG_E_CAPACITY, (name, kind, st)
                assert int(g.c.n_rec) == b.n_rec and [int(x) for x in g.c.n_class] == totals
                assert (g.base.reshape(3, 5) == want.span_base).all()
                assert g.untouched(), (name, kind)  # every guard, and nothing past any capacity
            finally:
                g.free()


def test_bad_tag_gives_its_lowest_index(eng):
    from clonos_amd import ClonosError, _lib
    rng = np.random.default_rng(6)
    n = 3 * T + 50
    for where in ([int(rng.integers(0, n))], [T + 17, T + 900], [5, 2 * T + 3], [n - 1], [T - 1, T]):
        tag = rng.integers(0, 8, n).astype(np.uint8)
        b = made_batch(tag, rng, [0, T, T + 20, n])  # (side rows as for the good tags)
        bad_tag = b.tag.copy()
        bad_tag[where] = 9
        b.tag = bad_tag
        st, g = run_columnize(eng, b, "device", exact_caps(n, [n] * 5))
        try:
            assert st == _lib.CLG_E_INVALID_ARG
            assert g.c.err_status == _lib.CLG_E_INVALID_ARG and g.c.err_off == min(where) and g.c.err_tag == 9
            assert g.c.err_span == (0 if min(where) < T else 1 if min(where) < T + 20 else 2)
            assert g.untouched()
        finally:
            g.free()
        d, keep = to_device(b)
        with pytest.raises(ClonosError) as ei:
            eng.columnize(d, b.span_rec_base)
        assert ei.value.status == _lib.CLG_E_INVALID_ARG and ei.value.err_off == min(where)


def test_kernel_stats_entry(eng):
    rng = np.random.default_rng(8)
    eng.kernel_stats_reset()
    check_against_host(eng, made_batch(rng.integers(0, 8, 1000).astype(np.uint8), rng))
    st = eng.kernel_stats()
    assert "decode_columns" in st and st["decode_columns"]["launches"] > 0 and st["decode_columns"]["bytes"] > 0


# ---- the decode entry points, on real logs -------------------------------------------------------
def open_logs(engine, spans):
    from clonos_amd import CausalLogID
    logs = []
    for i, b in enumerate(spans):
        lg = engine.open_log(CausalLogID.main(i))
        if len(b):
            lg.appendDeterminant(bytes(b), 0)
        logs.append(lg)
    return logs


def real_spans(name):
    from clonos_amd import job as J
    from clonos_amd import synth
    rng = np.random.default_rng({"config2": 2, "config3": 3, "config4": 4}[name])
    if name == "config2":
        return [synth.config2_log(n, rng)[0] for n in (9000, 0, 4097)]
    if name == "config3":  # Serializable records included
        return [synth.config3_epoch(n, rng)[0] for n in (2500, 900)]
    table = J.LogTable(J.dag(3, 12))  # 36 main logs and 288 subpartition logs: several hundred spans
    data, offs = synth.config4_epoch(table, np.arange(len(table)), rng, main_records=150, sub_records=16)
    return [data[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]


@pytest.mark.parametrize("name", ["config2", "config3", "config4"])
def test_decode_logs_columns(engine, name):
    from clonos_amd import columnize_host
    spans = real_spans(name)
    logs = open_logs(engine, spans)
    dec = engine.decode_logs(logs, [0] * len(logs))
    want = columnize_host(dec)
    got = engine.decode_logs_columns(logs, [0] * len(logs), keep_bytes=True)
    assert_columns_equal(got, want)
    back = got.to_soa()
    for k in ("tag", "v0", "w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "span_rec_base"):
        assert (getattr(back, k) == getattr(dec, k)).all(), k
    if name == "config3":
        assert (dec.tag == 3).any()
        dk = engine.decode_logs(logs, [0] * len(logs), keep_bytes=True)
        assert got.determinants(1) == dk.determinants(1)
    # the same bytes from host memory
    data = np.concatenate([np.frombuffer(bytes(b), np.uint8) for b in spans])
    offs = np.concatenate([[0], np.cumsum([len(b) for b in spans])])
    host = engine.decode_host_columns(data, [(int(o), len(b)) for o, b in zip(offs, spans)])
    assert_columns_equal(host, want)
    # a second call reuses the kept scratch
    assert_columns_equal(engine.decode_logs_columns(logs, [0] * len(logs)), want)


def test_decode_error_cuts_one_span(engine):
    from clonos_amd import ClonosError, columnize_host, synth
    rng = np.random.default_rng(11)
    good = [synth.random_log(300, rng, allow_serializable=False) for _ in range(3)]
    cut = synth.random_log(120, rng, allow_serializable=False) + b"\x09" + synth.random_log(40, rng, allow_serializable=False)
    spans = [good[0], cut, good[1], good[2]]
    logs = open_logs(engine, spans)
    with pytest.raises(ClonosError) as ex:
        engine.decode_logs(logs, [0] * 4)
    want_batch, err = oracle_batch(spans, allow_errors=True)
    assert err is not None and err[1] == 1
    with pytest.raises(ClonosError) as ec:
        engine.decode_logs_columns(logs, [0] * 4)
    for e in (ex.value, ec.value):
        assert (e.status, e.err_span, e.err_off, e.err_tag) == err
    got = engine.decode_logs_columns(logs, [0] * 4, partial=True)
    assert got.error is not None and got.error.status == err[0]
    assert (got.error.err_span, got.error.err_off, got.error.err_tag) == err[1:]
    assert_columns_equal(got, columnize_host(want_batch))  # every span's records up to its first error
    assert got.span(1).tag.size == 120


@pytest.mark.parametrize("kind", ["device", "mapped", "host"])
def test_decode_logs_columns_output_kinds(eng, kind):
    from clonos_amd import _lib, columnize_host
    spans = real_spans("config3")
    from clonos_amd import CausalLogID
    logs = []
    for i, b in enumerate(spans):
        lg = eng.open_log(CausalLogID.sub(900 + i, 1, 2, {"device": 0, "mapped": 1, "host": 2}[kind]))
        lg.appendDeterminant(bytes(b), 0)
        logs.append(lg)
    h = np.array([l.handle for l in logs], np.uint32)
    ep = np.zeros(len(logs), np.int64)
    want = columnize_host(eng.decode_logs(logs, [0] * len(logs)))
    c = _lib.Columns()
    sb = np.zeros((len(logs) + 1) * 5, np.uint64)
    c.span_base = sb.ctypes.data
    assert eng.decode_logs_columns_raw(h, ep, c) == 0  # sizes only
    assert (sb.reshape(-1, 5) == want.span_base).all()
    g = GuardedColumns(kind, exact_caps(int(c.n_rec), c.n_class), len(logs))
    try:
        assert eng.decode_logs_columns_raw(h, ep, g.c) == 0
        assert g.guards_intact()
        assert_columns_equal(g.result(), want)
    finally:
        g.free()
    for lg in logs:
        lg.close()
