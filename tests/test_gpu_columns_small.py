"""GPU: the one-launch form of the typed columns (k_col_small) against the multi-kernel form.

Two engines: one with the small path on, one with it turned off by CLONOS_COLUMNS_SMALL=0 (read
when the engine opens).  Every scene runs on both, against columnize_host, into guarded columns;
the count-only stat `columns_small` proves which path ran.  T = kColTile, R = one round of the
small kernel (four tiles), M = kColSmallRecords, P = kColSmallSpans (columns.h)."""
import os
import re

import numpy as np
import pytest

from _columns_util import COLS, GuardedColumns, assert_columns_equal, exact_caps, made_batch, to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    src = open(os.path.join(ROOT, "clonos_amd", "csrc", "columns.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


T = _header_constant("kColTile")
M = _header_constant("kColSmallRecords")
P = _header_constant("kColSmallSpans")
R = 4 * T
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, R - 1, R, R + 1, 2 * R + 1, M - 1, M, M + 1)
BOTH = ("small", "multi")


def test_constants_reach_the_carry_between_rounds():
    assert M >= 8 * T + 1 and M >= 2 * R + 1 and P >= 64


@pytest.fixture(scope="module")
def engines():
    from clonos_amd import Engine
    small = Engine(segment_bytes=4096, pool_segments=4096, timing=True)
    old = os.environ.get("CLONOS_COLUMNS_SMALL")
    os.environ["CLONOS_COLUMNS_SMALL"] = "0"
    try:
        multi = Engine(segment_bytes=4096, pool_segments=4096, timing=True)
    finally:
        if old is None:
            del os.environ["CLONOS_COLUMNS_SMALL"]
        else:
            os.environ["CLONOS_COLUMNS_SMALL"] = old
    yield {"small": small, "multi": multi}
    small.close()
    multi.close()


def taken(eng):
    """Calls that took the one-launch columns path so far."""
    return eng.kernel_stats().get("columns_small", {"launches": 0})["launches"]


def pattern_tags(pattern, n, rng):
    if pattern == "alternate":
        return (np.arange(n) & 1).astype(np.uint8)
    if pattern == "order_then_timestamps":
        t = np.ones(n, np.uint8)
        t[:1] = 0
        return t
    if pattern == "wide":
        return rng.integers(3, 7, n).astype(np.uint8)
    return np.full(n, {"order": 0, "timestamp": 1, "rng": 2, "buffer_built": 7}[pattern], np.uint8)


def columnize_into(eng, d, batch, g):
    from clonos_amd import _lib
    base = np.ascontiguousarray(batch.span_rec_base, np.uint64)
    return _lib.lib.clg_columnize(eng.handle, d, base.ctypes.data, len(base) - 1, g.c)


def check(engines, batch, want=None, kind="device", small=True):
    """clg_columnize of `batch` on both engines into guarded columns of exactly the batch's sizes
    (from columnize_host): equal to columnize_host, guards intact, to_soa() gives the batch back.
    small: whether the small-path engine must have taken the one-launch kernel."""
    from clonos_amd import columnize_host
    if want is None:
        want = columnize_host(batch)
    n_class = [len(want.order), len(want.timestamp), len(want.rng), len(want.buffer_built), len(want.w_idx)]
    d, keep = to_device(batch)
    for which in BOTH:
        eng = engines[which]
        before = taken(eng)
        g = GuardedColumns(kind, exact_caps(batch.n_rec, n_class), len(batch.span_rec_base) - 1)
        try:
            assert columnize_into(eng, d, batch, g) == 0, which
            assert taken(eng) - before == (1 if which == "small" and small else 0), which
            assert g.guards_intact(), which
            got = g.result()
            assert_columns_equal(got, want)
            back = got.to_soa()
            assert (back.tag == batch.tag).all() and (back.v0 == batch.v0).all()
            assert (back.span_rec_base == np.asarray(batch.span_rec_base)).all()
        finally:
            g.free()
    del keep
    return want


@pytest.mark.parametrize("pattern", ["order", "timestamp", "rng", "buffer_built", "wide", "alternate",
                                     "order_then_timestamps"])
def test_patterns_at_every_size(engines, pattern):
    rng = np.random.default_rng(len(pattern) + 100)
    for n in SIZES:
        check(engines, made_batch(pattern_tags(pattern, n, rng), rng), small=n <= M)


def test_mixed_classes_at_every_size(engines):
    rng = np.random.default_rng(41)
    for n in SIZES:
        check(engines, made_batch(rng.integers(0, 8, n).astype(np.uint8), rng), small=n <= M)


def test_order_column_bases_at_every_residue_over_two_rounds(engines):
    """k Orders, then only Timestamps, then Orders again in later tiles of both rounds: the i8
    column's tile bases fall at every residue mod 16, and the second round's come from the carry."""
    rng = np.random.default_rng(16)
    for k in range(16):
        t = np.ones(R + 2 * T + 9, np.uint8)
        t[:k] = 0
        t[T + 5:T + 40] = 0
        t[R - 3:R + 11] = 0
        t[R + T + 1:] = 0
        check(engines, made_batch(t, rng))


def test_spans(engines):
    rng = np.random.default_rng(7)
    n = R + 2 * T + 77
    assert n <= M
    base = [0, 0, 0]                                   # empty spans first
    base += [T - 1, T, T + 1]                          # a boundary on a tile edge, and one record either side
    base += [T + 1, T + 1]                             # empty spans in the middle
    base += list(range(T + 10, T + 10 + 70))           # more than 64 one-record spans inside one tile
    base += [R - 1, R, R + 1]                          # a boundary on a round's edge
    base += [R + T + 200]
    base += [n, n, n]                                  # empty spans last
    assert len(base) - 1 <= P
    got = check(engines, made_batch(rng.integers(0, 8, n).astype(np.uint8), rng, base))
    assert got.n_spans == len(base) - 1
    assert got.span(0).tag.size == 0 and got.span(got.n_spans - 1).tag.size == 0


@pytest.mark.parametrize("n_spans,small", [(P, True), (P + 1, False)])
def test_span_count_at_the_limit(engines, n_spans, small):
    rng = np.random.default_rng(n_spans)
    n = T + 500
    base = np.sort(rng.integers(0, n + 1, n_spans + 1))
    base[0], base[-1] = 0, n
    check(engines, made_batch(rng.integers(0, 8, n).astype(np.uint8), rng, base.tolist()), small=small)


@pytest.mark.parametrize("kind", ["device", "mapped", "host"])
def test_output_kinds(engines, kind):
    rng = np.random.default_rng(3)
    tag = rng.integers(0, 8, R + T + 1).astype(np.uint8)
    check(engines, made_batch(tag, rng, [0, 7, T, R, R + T + 1]), kind=kind)
    check(engines, made_batch(np.zeros(0, np.uint8), rng, [0, 0]), kind=kind)


# ---- errors: nothing written -----------------------------------------------------------------
def test_bad_tag_gives_its_lowest_index_and_writes_nothing(engines):
    from clonos_amd import _lib
    rng = np.random.default_rng(6)
    n = R + T + 50
    for where in ([0], [R - 1], [R], [n - 1], [R + 5, 3], [R, R - 1], [n - 1, T + 17]):
        b = made_batch(rng.integers(0, 8, n).astype(np.uint8), rng, [0, T, T + 20, n])
        bad_tag = b.tag.copy()
        bad_tag[where] = 9
        b.tag = bad_tag
        d, keep = to_device(b)
        for which in BOTH:
            for kind in ("device", "host"):
                g = GuardedColumns(kind, exact_caps(n, [n] * 5), 3)
                try:
                    before = taken(engines[which])
                    assert columnize_into(engines[which], d, b, g) == _lib.CLG_E_INVALID_ARG
                    assert taken(engines[which]) - before == (which == "small")
                    assert g.c.err_status == _lib.CLG_E_INVALID_ARG and g.c.err_off == min(where) and g.c.err_tag == 9
                    assert g.c.err_span == (0 if min(where) < T else 1 if min(where) < T + 20 else 2)
                    assert g.untouched(), (which, kind, where)
                finally:
                    g.free()
        del keep


def test_capacity_n_wide_and_sizes_only(engines):
    from clonos_amd import _lib, columnize_host
    rng = np.random.default_rng(5)
    n = R + 300
    b = made_batch(rng.integers(0, 8, n).astype(np.uint8), rng, [0, 100, R, n])
    want = columnize_host(b)
    totals = [len(want.order), len(want.timestamp), len(want.rng), len(want.buffer_built), len(want.w_idx)]
    d, keep = to_device(b)
    base = np.ascontiguousarray(b.span_rec_base, np.uint64)
    for which in BOTH:
        eng = engines[which]
        # sizes only: the totals and span_base, no column
        c = _lib.Columns()
        sb = np.zeros(20, np.uint64)
        c.span_base = sb.ctypes.data
        before = taken(eng)
        assert _lib.lib.clg_columnize(eng.handle, d, base.ctypes.data, 3, c) == 0
        assert taken(eng) - before == (which == "small")
        assert int(c.n_rec) == n and [int(x) for x in c.n_class] == totals
        assert (sb.reshape(4, 5) == want.span_base).all()
        # one element short in each column in turn
        for name, _, _, _ in COLS:
            caps = exact_caps(n, totals)
            caps[name] -= 1
            for kind in ("device", "host"):
                g = GuardedColumns(kind, caps, 3)
                try:
                    assert columnize_into(eng, d, b, g) == _lib.CLG_E_CAPACITY, (which, name, kind)
                    assert int(g.c.n_rec) == n and [int(x) for x in g.c.n_class] == totals
                    assert (g.base.reshape(4, 5) == want.span_base).all()
                    assert g.untouched(), (which, name, kind)
                finally:
                    g.free()
        # n_wide off by one, either way
        for dn in (-1, 1):
            d2, keep2 = to_device(b)
            d2.n_wide = d.n_wide + dn
            caps = exact_caps(n, [t + 1 for t in totals])
            g = GuardedColumns("device", caps, 3)
            try:
                assert columnize_into(eng, d2, b, g) == _lib.CLG_E_INVALID_ARG, (which, dn)
                assert g.untouched(), (which, dn)
            finally:
                g.free()
            del keep2
    del keep


# ---- the decode entry points ------------------------------------------------------------------
def test_decode_entry_points_agree(engines):
    from clonos_amd import CausalLogID, columnize_host, synth
    rng = np.random.default_rng(33)
    spans = [synth.config3_epoch(k, rng)[0] for k in (700, 1, 300)]
    data = np.concatenate([np.frombuffer(bytes(b), np.uint8) for b in spans])
    offs = np.concatenate([[0], np.cumsum([len(b) for b in spans])])
    res = {}
    for which in BOTH:
        eng = engines[which]
        logs = []
        for i, b in enumerate(spans):
            lg = eng.open_log(CausalLogID.main(500 + i))
            lg.appendDeterminant(bytes(b), 0)
            logs.append(lg)
        want = columnize_host(eng.decode_logs(logs, [0] * 3))
        before = taken(eng)
        a = eng.decode_logs_columns(logs, [0] * 3)
        h = eng.decode_host_columns(data, [(int(o), len(b)) for o, b in zip(offs, spans)])
        assert taken(eng) - before == (2 if which == "small" else 0)
        assert_columns_equal(a, want)
        assert_columns_equal(h, want)
        res[which] = a
        for lg in logs:
            lg.close()
    assert_columns_equal(res["small"], res["multi"])
