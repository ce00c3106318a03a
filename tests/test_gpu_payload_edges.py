"""GPU: the payload column's kernels (clg_gather_payloads) at every alignment and length edge.
The expected column is plain numpy slicing of the span bytes (_payload_util.expected).
T = kPayTile (rows per tile), S = the scan workgroup's threads, W = the wave-copy threshold
(payload.h)."""
import os
import re

import numpy as np
import pytest

from _payload_util import FILL, NO_ROW, GuardedPayloads, expected, upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    src = open(os.path.join(ROOT, "clonos_amd", "csrc", "payload.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


THREADS = _header_constant("kPayThreads")
PER = _header_constant("kPayPerThread")
T = THREADS * PER
S = _header_constant("kPayScanThreads")
W = _header_constant("kPayWaveRow")
SPAN = 4096
LENGTHS = list(range(0, 81)) + [127, 128, 129, 255, 256, 257, 1023, 1024, 1025]


@pytest.fixture(scope="module")
def eng():
    from clonos_amd import Engine
    e = Engine(segment_bytes=4096, pool_segments=256, timing=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    return np.random.default_rng(0xBEEF).integers(0, 256, SPAN, dtype=np.uint8)


@pytest.fixture(scope="module")
def edge_rows(data):
    """Every source residue 0-15 x every length of LENGTHS, each group (one residue, every length)
    preceded by a filler row of length 0-15, and every (filler, residue) pair: 256 groups.  The
    expected column once, shared and left unchanged."""
    rng = np.random.default_rng(16)
    wo, wl = [], []
    lens = np.array(LENGTHS)
    for filler in range(16):
        for r in range(16):
            wo.append(int(rng.integers(0, SPAN - 16)))
            wl.append(filler)
            q = (rng.random(lens.size) * ((SPAN - lens - r) // 16 + 1)).astype(np.int64)
            wo += (16 * q + r).tolist()
            wl += LENGTHS
    for L in (1, 17, W - 1, W, W + 1, 1025):  # rows that end on the span's last byte
        wo.append(SPAN - L)
        wl.append(L)
    wo, wl = np.array(wo, np.uint32), np.array(wl, np.uint32)
    assert ((wo.astype(np.int64) + wl) <= SPAN).all()
    var, pos = expected([data], wo, wl, [0, wo.size])
    # every destination residue meets every source residue on both sides of the wave-copy split
    m = wl > 0
    seen = set(zip((pos[:-1][m] % 16).tolist(), (wo[m] % 16).tolist(), (wl[m] >= W).tolist()))
    assert len(seen) == 16 * 16 * 2
    var.setflags(write=False)
    pos.setflags(write=False)
    return wo, wl, var, pos


def gather(eng, d_bytes, spans, wo, wl, rb, g, host_rows=None):
    """clg_gather_payloads over device bytes and rows into the clg_payloads g.p; returns the status."""
    so = np.array([s[0] for s in spans], np.uint64)
    sl = np.array([s[1] for s in spans], np.uint64)
    d_wo, d_wl = upload(wo), upload(wl)
    try:
        return eng.gather_payloads(d_bytes.p.value, so, sl, d_wo.p.value if wo.size else 0, d_wl.p.value if wl.size else 0,
                                   rb, device=True, out=g.p if isinstance(g, GuardedPayloads) else g)
    finally:
        d_wo.free()
        d_wl.free()


def test_every_residue_and_length_in_every_output_kind(eng, data, edge_rows):
    wo, wl, want, want_pos = edge_rows
    d = upload(data)
    outs = {}
    try:
        for kind in ("device", "mapped", "host"):
            g = GuardedPayloads(kind, want.size, wo.size + 1)
            try:
                assert gather(eng, d, [(0, SPAN)], wo, wl, [0, wo.size], g) == 0
                assert (int(g.p.n_rows), int(g.p.n_var), int(g.p.bad_row)) == (wo.size, want.size, NO_ROW)
                assert g.guards_intact(), kind
                outs[kind] = g.result()
            finally:
                g.free()
            var, pos = outs[kind]
            assert (pos == want_pos).all(), kind
            bad = np.nonzero(var != want)[0]
            assert bad.size == 0, (kind, int(bad[0]), int(np.searchsorted(want_pos, bad[0], side="right") - 1))
        assert (outs["device"][0] == outs["mapped"][0]).all() and (outs["device"][0] == outs["host"][0]).all()
        assert (outs["device"][1] == outs["mapped"][1]).all() and (outs["device"][1] == outs["host"][1]).all()
        # the same rows and bytes from host memory (staged)
        var, pos = eng.gather_payloads(data, [0], [SPAN], wo, wl, [0, wo.size])
        assert (pos == want_pos).all() and (var == want).all()
    finally:
        d.free()


def test_unaligned_row_arrays_and_destination(eng, data, edge_rows):
    """Row arrays that are not 16-byte aligned (the per-row loads) and var at every residue."""
    wo, wl, _, _ = edge_rows
    n = 2 * T + 77
    wo, wl = wo[:n], wl[:n]
    want, want_pos = expected([data], wo, wl, [0, n])
    d = upload(data)
    d_wo, d_wl = upload(np.concatenate([[0], wo]).astype(np.uint32)), upload(np.concatenate([[0, 0, 0], wl]).astype(np.uint32))
    so, sl = np.array([0], np.uint64), np.array([SPAN], np.uint64)
    try:
        for shift in (1, 7, 15):
            g = GuardedPayloads("device", want.size + 16, n + 1)
            try:
                g.p.var += shift
                g.p.cap_var = want.size
                assert eng.gather_payloads(d.p.value, so, sl, d_wo.p.value + 4, d_wl.p.value + 12, [0, n], device=True,
                                           out=g.p) == 0
                raw = g.raw("var")
                assert (raw[64 + shift:64 + shift + want.size] == want).all()
                assert (raw[:64 + shift] == FILL).all() and (raw[64 + shift + want.size:] == FILL).all()
                assert (g.result()[1] == want_pos).all()
            finally:
                g.free()
    finally:
        for b in (d, d_wo, d_wl):
            b.free()


def test_no_rows_writes_only_pos0(eng, data):
    d = upload(data)
    try:
        for kind in ("device", "mapped", "host"):
            for spans, rb in (([(0, SPAN)], [0, 0]), ([(0, 0), (5, 9)], [0, 0, 0]), ([], [0])):
                g = GuardedPayloads(kind, 32, 4)
                try:
                    assert gather(eng, d, spans, np.zeros(0, np.uint32), np.zeros(0, np.uint32), rb, g) == 0
                    assert (int(g.p.n_rows), int(g.p.n_var), int(g.p.bad_row)) == (0, 0, NO_ROW)
                    assert g.guards_intact() and g.result()[1].tolist() == [0]
                    v, q = g.after_result()
                    assert (v == FILL).all() and (q == FILL).all()  # only pos[0] was written
                finally:
                    g.free()
    finally:
        d.free()


def test_several_spans_some_empty(eng):
    rng = np.random.default_rng(21)
    lens = [0, 700, 0, 0, 1, 2000, 64, 0, 3000, 0]
    offs, at = [], 3
    for L in lens:
        offs.append(at)
        at += L + int(rng.integers(0, 5))
    buf = rng.integers(0, 256, at, dtype=np.uint8)
    wo, wl, rb = [], [], [0]
    for s, L in enumerate(lens):
        rows = 0 if s in (3, 6) else int(rng.integers(T // 3, 2 * T // 3))  # (spans without rows too)
        for r in range(rows):
            if L == 0:
                o, l = 0, 0
            elif r == 0:  # ends on the span's last byte
                l = int(rng.integers(1, min(L, 300) + 1))
                o = L - l
            else:
                o = int(rng.integers(0, L))
                l = int(rng.integers(0, min(L - o, 200) + 1)) if r % 3 else 0
            wo.append(o)
            wl.append(l)
        rb.append(len(wo))
    wo, wl = np.array(wo, np.uint32), np.array(wl, np.uint32)
    assert len(wo) > 2 * T
    spans = [buf[o:o + L] for o, L in zip(offs, lens)]
    want, want_pos = expected(spans, wo, wl, rb)
    d = upload(buf)
    g = GuardedPayloads("device", want.size, wo.size + 1)
    try:
        assert gather(eng, d, list(zip(offs, lens)), wo, wl, rb, g) == 0
        assert g.guards_intact()
        var, pos = g.result()
        assert (pos == want_pos).all() and (var == want).all()
    finally:
        g.free()
        d.free()
    var, pos = eng.gather_payloads(buf, offs, lens, wo, wl, rb)  # host input, staged
    assert (pos == want_pos).all() and (var == want).all()


@pytest.fixture(scope="module")
def many_rows(data):
    """More tiles than one scan round and a partial tile, lengths 0-3."""
    rng = np.random.default_rng(33)
    n = T * S + 2 * T + 301
    wl = rng.integers(0, 4, n).astype(np.uint32)
    wo = rng.integers(0, SPAN - 3, n).astype(np.uint32)
    want, want_pos = expected([data], wo, wl, [0, n])
    return wo, wl, want, want_pos


@pytest.fixture(scope="module")
def round_rows(data):
    """2 * T * S + 1 rows, lengths 0-3: the scan's rounds are S tiles, so the prefixes of T * S,
    T * S + 1, 2 * T * S and 2 * T * S + 1 rows end exactly one full round, one tile into the second,
    exactly two rounds and one tile into the third.  The expected column once; a prefix of the rows
    has a prefix of it."""
    rng = np.random.default_rng(34)
    n = 2 * T * S + 1
    wl = rng.integers(0, 4, n).astype(np.uint32)
    wo = rng.integers(0, SPAN - 3, n).astype(np.uint32)
    want, want_pos = expected([data], wo, wl, [0, n])
    for a in (wo, wl, want, want_pos):
        a.setflags(write=False)
    return wo, wl, want, want_pos


def gathers_as_expected(eng, data, wo, wl, want, want_pos):
    d = upload(data)
    g = GuardedPayloads("device", want.size, wo.size + 1)
    try:
        assert gather(eng, d, [(0, SPAN)], wo, wl, [0, wo.size], g) == 0
        assert (int(g.p.n_rows), int(g.p.n_var)) == (wo.size, want.size)
        assert g.guards_intact()
        var, pos = g.result()
        assert (pos == want_pos).all() and (var == want).all()
    finally:
        g.free()
        d.free()


def test_more_tiles_than_one_scan_round(eng, data, many_rows):
    gathers_as_expected(eng, data, *many_rows)


@pytest.mark.parametrize("n", [T * S, T * S + 1, 2 * T * S, 2 * T * S + 1])
def test_the_scan_round_edges(eng, data, round_rows, n):
    """The one-workgroup scan's carry and partial last round (k_pay_scan, the cheapest instance of
    the family's shared scan) at its round edges."""
    wo, wl, want, want_pos = round_rows
    gathers_as_expected(eng, data, wo[:n], wl[:n], want[:int(want_pos[n])], want_pos[:n + 1])


def test_bad_row_in_the_middle_tile_gives_its_lowest_index(eng, data, many_rows):
    """Rejected by the size pass, before any load of the range; nothing is written."""
    from clonos_amd import _lib
    wo, wl, want, _ = many_rows
    n = 3 * T + 50
    d = upload(data)
    try:
        for where in ([T + 17, T + 900], [T + 5, 2 * T + 3], [2 * T - 1, 2 * T], [n - 1], [0, T + 1]):
            wo2, wl2 = wo[:n].copy(), wl[:n].copy()
            for i, k in enumerate(where):
                wo2[k], wl2[k] = ((SPAN - 1, 2), (0xFFFFFFFF, 2), (SPAN, 1))[(i + k) % 3]
            counted = int(wl[:n].sum()) - int(wl[:n][where].sum())
            for kind in ("device", "host"):
                g = GuardedPayloads(kind, int(wl[:n].sum()) + 64, n + 1)
                try:
                    assert gather(eng, d, [(0, SPAN)], wo2, wl2, [0, n], g) == _lib.CLG_E_INVALID_ARG
                    assert (int(g.p.bad_row), int(g.p.n_rows), int(g.p.n_var)) == (min(where), n, counted)
                    assert g.untouched()
                finally:
                    g.free()
    finally:
        d.free()


def test_sizes_only_and_capacity_failures_leave_the_outputs_untouched(eng, data, edge_rows):
    from clonos_amd import _lib
    wo, wl, want, _ = edge_rows
    n = 2 * T + 9
    wo, wl = wo[:n], wl[:n]
    nv = int(wl.sum())
    d = upload(data)
    try:
        p = _lib.Payloads()  # var and pos null: sizes only
        assert gather(eng, d, [(0, SPAN)], wo, wl, [0, n], p) == 0
        assert (int(p.n_rows), int(p.n_var), int(p.bad_row)) == (n, nv, NO_ROW)
        for kind in ("device", "mapped", "host"):
            for cv, cp in ((nv - 1, n + 1), (nv, n)):
                g = GuardedPayloads(kind, cv, cp)
                try:
                    assert gather(eng, d, [(0, SPAN)], wo, wl, [0, n], g) == _lib.CLG_E_CAPACITY
                    assert (int(g.p.n_rows), int(g.p.n_var)) == (n, nv)
                    assert g.untouched(), (kind, cv, cp)
                finally:
                    g.free()
    finally:
        d.free()


def test_kernel_stats_entry(eng, data, edge_rows):
    wo, wl, want, want_pos = edge_rows
    eng.kernel_stats_reset()
    var, pos = eng.gather_payloads(data, [0], [SPAN], wo[:500], wl[:500], [0, 500])
    assert (var == want[:int(want_pos[500])]).all()
    st = eng.kernel_stats()
    assert "decode_payloads" in st and st["decode_payloads"]["launches"] > 0 and st["decode_payloads"]["bytes"] > 0
