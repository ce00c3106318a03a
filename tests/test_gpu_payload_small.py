"""GPU: the one-launch form of the payload column (k_pay_small) against the multi-kernel form.

Two engines with segment_bytes=256 (rows cross segment ends): one with the small path on, one
with it turned off by CLONOS_COLUMNS_SMALL=0.  Every scene runs on both, against plain numpy
slicing of the span bytes (_payload_util.expected, which gather_payloads_host is held to
elsewhere) and against gather_payloads_host itself; the count-only stat `payloads_small` proves
which path ran.  RW = one round of the small kernel's workgroup (four tiles of rows),
MR = kPaySmallRows, MB = kPaySmallBytes (payload.h)."""
import os
import re

import numpy as np
import pytest

from _payload_util import NO_ROW, GuardedPayloads, expected, upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    src = open(os.path.join(ROOT, "clonos_amd", "csrc", "payload.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


T = _header_constant("kPayThreads") * _header_constant("kPayPerThread")
RW = _header_constant("kPayScanThreads") // _header_constant("kPayThreads") * T
MR = _header_constant("kPaySmallRows")
MB = _header_constant("kPaySmallBytes")
SEG = 256
SPAN = 8192
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4096)
BOTH = ("small", "multi")


def test_constants_reach_the_carry_between_rounds():
    assert MR >= 2 * RW + 1


@pytest.fixture(scope="module")
def engines():
    from clonos_amd import Engine
    small = Engine(segment_bytes=SEG, pool_segments=16384, timing=True)
    old = os.environ.get("CLONOS_COLUMNS_SMALL")
    os.environ["CLONOS_COLUMNS_SMALL"] = "0"
    try:
        multi = Engine(segment_bytes=SEG, pool_segments=16384, timing=True)
    finally:
        if old is None:
            del os.environ["CLONOS_COLUMNS_SMALL"]
        else:
            os.environ["CLONOS_COLUMNS_SMALL"] = old
    yield {"small": small, "multi": multi}
    small.close()
    multi.close()


def taken(eng):
    return eng.kernel_stats().get("payloads_small", {"launches": 0})["launches"]


@pytest.fixture(scope="module")
def data():
    return np.random.default_rng(0xFEED).integers(0, 256, SPAN, dtype=np.uint8)


@pytest.fixture(scope="module")
def edge_rows(data):
    """Every source residue 0-15 x every length of LENGTHS, a filler row of length 0-15 before each
    residue's group, so the destinations fall at many residues too.  Expected once, shared."""
    rng = np.random.default_rng(12)
    wo, wl = [], []
    for r in range(16):
        wo.append(int(rng.integers(0, SPAN - 16)))
        wl.append(int(rng.integers(0, 16)))
        for L in LENGTHS:
            q = int(rng.integers(0, (SPAN - L - r) // 16 + 1))
            wo.append(16 * q + r)
            wl.append(L)
    for L in (1, 17, 64, 4096):  # rows that end on the span's last byte
        wo.append(SPAN - L)
        wl.append(L)
    wo, wl = np.array(wo, np.uint32), np.array(wl, np.uint32)
    var, pos = expected([data], wo, wl, [0, wo.size])
    var.setflags(write=False)
    pos.setflags(write=False)
    return wo, wl, var, pos


def gather(eng, d_bytes, spans, wo, wl, rb, out):
    so = np.array([s[0] for s in spans], np.uint64)
    sl = np.array([s[1] for s in spans], np.uint64)
    d_wo, d_wl = upload(wo), upload(wl)
    try:
        return eng.gather_payloads(d_bytes.p.value, so, sl, d_wo.p.value if wo.size else 0, d_wl.p.value if wl.size else 0,
                                   rb, device=True, out=out)
    finally:
        d_wo.free()
        d_wl.free()


def check(engines, buf, spans, wo, wl, rb, want, want_pos, kinds=("device", "host"), small=True):
    """clg_gather_payloads of device bytes and rows on both engines into guarded outputs of exactly
    the expected sizes."""
    d = upload(buf)
    try:
        for which in BOTH:
            for kind in kinds:
                g = GuardedPayloads(kind, want.size, len(wo) + 1)
                try:
                    before = taken(engines[which])
                    assert gather(engines[which], d, spans, wo, wl, rb, g.p) == 0, (which, kind)
                    assert taken(engines[which]) - before == (1 if which == "small" and small else 0), (which, kind)
                    assert (int(g.p.n_rows), int(g.p.n_var), int(g.p.bad_row)) == (len(wo), want.size, NO_ROW)
                    assert g.guards_intact(), (which, kind)
                    var, pos = g.result()
                    assert (pos == want_pos).all(), (which, kind)
                    bad = np.nonzero(var != want)[0]
                    assert bad.size == 0, (which, kind, int(bad[0]))
                finally:
                    g.free()
    finally:
        d.free()


def test_every_length_and_source_alignment_contiguous(engines, data, edge_rows):
    from clonos_amd import gather_payloads_host
    wo, wl, want, want_pos = edge_rows
    hv, hp = gather_payloads_host(data, [0], [SPAN], wo, wl, [0, wo.size])
    assert (hv == want).all() and (hp == want_pos).all()
    check(engines, data, [(0, SPAN)], wo, wl, [0, wo.size], want, want_pos, kinds=("device", "mapped", "host"))
    for which in BOTH:  # the same rows and bytes from host memory (staged)
        var, pos = engines[which].gather_payloads(data, [0], [SPAN], wo, wl, [0, wo.size])
        assert (pos == want_pos).all() and (var == want).all()


def test_every_length_and_source_alignment_in_pool_segments(engines, data, edge_rows):
    """The same rows over a log in 256-byte segments, the range starting mid-segment: rows cross
    one and many segment ends."""
    from clonos_amd import CausalLogID
    wo, wl, want, want_pos = edge_rows
    for which in BOTH:
        eng = engines[which]
        lg = eng.open_log(CausalLogID.main(7))
        lg.appendDeterminant(bytes(100), 0)
        lg.appendDeterminant(data.tobytes(), 1)
        d_wo, d_wl = upload(wo), upload(wl)
        try:
            for kind in ("device", "host"):
                g = GuardedPayloads(kind, want.size, wo.size + 1)
                try:
                    before = taken(eng)
                    assert eng.gather_payloads_logs([lg.handle], [1], d_wo.p.value, d_wl.p.value, [0, wo.size], device=True,
                                                    out=g.p) == 0
                    assert taken(eng) - before == (which == "small")
                    assert g.guards_intact()
                    var, pos = g.result()
                    assert (pos == want_pos).all() and (var == want).all(), (which, kind)
                finally:
                    g.free()
        finally:
            d_wo.free()
            d_wl.free()
            lg.close()


def test_several_spans_some_empty(engines):
    rng = np.random.default_rng(21)
    lens = [0, 700, 0, 0, 1, 2000, 64, 0, 3000, 0]
    offs, at = [], 3
    for L in lens:
        offs.append(at)
        at += L + int(rng.integers(0, 5))
    buf = rng.integers(0, 256, at, dtype=np.uint8)
    wo, wl, rb = [], [], [0]
    for s, L in enumerate(lens):
        rows = 0 if s in (3, 6) else int(rng.integers(RW // 7, RW // 5))  # (spans without rows too)
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
    assert RW < len(wo) <= MR
    want, want_pos = expected([buf[o:o + L] for o, L in zip(offs, lens)], wo, wl, rb)
    check(engines, buf, list(zip(offs, lens)), wo, wl, rb, want, want_pos)


@pytest.mark.parametrize("n", sorted({1, T - 1, T, T + 1, RW - 1, RW, RW + 1, 2 * RW - 1, 2 * RW, 2 * RW + 1, MR - 1, MR,
                                       MR + 1}))
def test_row_counts_around_the_rounds_and_the_limit(engines, data, n):
    rng = np.random.default_rng(n)
    wl = rng.integers(0, 4, n).astype(np.uint32)
    wl[rng.integers(0, n, 3)] = 70  # a few rows for the wave copy
    wo = rng.integers(0, SPAN - 70, n).astype(np.uint32)
    want, want_pos = expected([data], wo, wl, [0, n])
    check(engines, data, [(0, SPAN)], wo, wl, [0, n], want, want_pos, kinds=("device",), small=n <= MR)


def test_bad_row_gives_its_lowest_index_and_writes_nothing(engines, data):
    from clonos_amd import _lib
    rng = np.random.default_rng(5)
    n = RW + T + 50
    wl = rng.integers(0, 80, n).astype(np.uint32)
    wo = rng.integers(0, SPAN - 80, n).astype(np.uint32)
    d = upload(data)
    try:
        for where in ([0], [RW - 1, RW + 3], [RW, n - 1], [n - 1], [T + 5, 0]):
            wo2, wl2 = wo.copy(), wl.copy()
            for k in where:  # one byte past the span's end
                wl2[k] = 9
                wo2[k] = SPAN - 8
            counted = int(wl.sum()) - int(wl[where].sum())
            for which in BOTH:
                for kind in ("device", "host"):
                    g = GuardedPayloads(kind, int(wl.sum()) + 64, n + 1)
                    try:
                        before = taken(engines[which])
                        assert gather(engines[which], d, [(0, SPAN)], wo2, wl2, [0, n], g.p) == _lib.CLG_E_INVALID_ARG
                        assert taken(engines[which]) - before == (which == "small")
                        assert (int(g.p.bad_row), int(g.p.n_rows), int(g.p.n_var)) == (min(where), n, counted)
                        assert g.untouched(), (which, kind, where)
                    finally:
                        g.free()
    finally:
        d.free()


def test_sizes_only_and_capacity_failures_leave_the_outputs_untouched(engines, data, edge_rows):
    from clonos_amd import _lib
    wo, wl, want, _ = edge_rows
    n, nv = wo.size, int(wl.sum())
    d = upload(data)
    try:
        for which in BOTH:
            eng = engines[which]
            p = _lib.Payloads()  # var and pos null: sizes only
            before = taken(eng)
            assert gather(eng, d, [(0, SPAN)], wo, wl, [0, n], p) == 0
            assert taken(eng) - before == (which == "small")
            assert (int(p.n_rows), int(p.n_var), int(p.bad_row)) == (n, nv, NO_ROW)
            for kind in ("device", "mapped", "host"):
                for cv, cp in ((nv - 1, n + 1), (nv, n)):
                    g = GuardedPayloads(kind, cv, cp)
                    try:
                        assert gather(eng, d, [(0, SPAN)], wo, wl, [0, n], g.p) == _lib.CLG_E_CAPACITY
                        assert (int(g.p.n_rows), int(g.p.n_var)) == (n, nv)
                        assert g.untouched(), (which, kind, cv, cp)
                    finally:
                        g.free()
    finally:
        d.free()


@pytest.mark.parametrize("span_bytes,small", [(MB, True), (MB + 1, False)])
def test_span_bytes_at_the_limit(engines, span_bytes, small):
    rng = np.random.default_rng(span_bytes & 0xFFFF)
    buf = rng.integers(0, 256, span_bytes, dtype=np.uint8)
    n = 300
    wl = rng.integers(0, 300, n).astype(np.uint32)
    wo = rng.integers(0, span_bytes - 300, n).astype(np.uint32)
    wo[-1], wl[-1] = span_bytes - 100, 100  # ends on the span's last byte
    want, want_pos = expected([buf], wo, wl, [0, n])
    check(engines, buf, [(0, span_bytes)], wo, wl, [0, n], want, want_pos, kinds=("device",), small=small)
