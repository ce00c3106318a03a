"""CPU: the payload column on the host.  The header's function (clonos_amd/csrc/payload.h, compiled
with g++ into the stand-alone program tests/payload_host.cpp, once plainly and once with
-fsanitize=address,undefined, and run directly), and clg_gather_payloads_host of the library
through ctypes against plain slicing of the span bytes: sizes only, each capacity failure with the
outputs untouched, the lowest bad row, and the Python views built on it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _columns_util import oracle_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "payload_host.cpp")
FILL = 0xA5
NO_ROW = 0xFFFFFFFFFFFFFFFF


def test_header_function(tmp_path):
    exe = str(tmp_path / "payload_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 100000, r.stdout


def test_header_function_sanitized(tmp_path):
    """The same program with the address and undefined-behaviour sanitizers, run directly (their
    runtimes linked into the program: it needs nothing preloaded)."""
    exe = str(tmp_path / "payload_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok (\d+)\n", r.stdout), r.stdout


def seeded(rng, n_spans=9, max_rows=30, max_span=400):
    """Spans of one buffer (some empty, gaps between them) and rows inside them: zero-length rows,
    and in every non-empty span with rows one that ends on the span's last byte."""
    so, sl, wo, wl, rb, at = [], [], [], [], [0], 0
    for s in range(n_spans):
        L = 0 if s % 4 == 1 else int(rng.integers(1, max_span))
        at += int(rng.integers(0, 7))
        so.append(at)
        sl.append(L)
        at += L
        for r in range(int(rng.integers(0, max_rows + 1))):
            if L == 0:
                o, l = 0, 0
            elif r == 0:
                l = int(rng.integers(1, L + 1))
                o = L - l
            elif r % 4 == 1:
                o, l = int(rng.integers(0, L + 1)), 0
            else:
                o = int(rng.integers(0, L))
                l = int(rng.integers(0, L - o + 1))
            wo.append(o)
            wl.append(l)
        rb.append(len(wo))
    data = rng.integers(0, 256, at, dtype=np.uint8)
    return (data, np.array(so, np.uint64), np.array(sl, np.uint64), np.array(wo, np.uint32), np.array(wl, np.uint32),
            np.array(rb, np.uint64))


def sliced(data, so, sl, wo, wl, rb):
    """The expected column by plain slicing."""
    parts, pos = [], [0]
    for s in range(len(so)):
        span = data[int(so[s]):int(so[s]) + int(sl[s])]
        for k in range(int(rb[s]), int(rb[s + 1])):
            parts.append(span[int(wo[k]):int(wo[k]) + int(wl[k])])
            assert len(parts[-1]) == int(wl[k])
            pos.append(pos[-1] + int(wl[k]))
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), np.array(pos, np.uint64)


def raw_call(case, var, pos, cap_var=None, cap_pos=None):
    """clg_gather_payloads_host into var[64:-64] / pos[8:-8] (guards either side); returns (status, struct)."""
    from clonos_amd import _lib
    data, so, sl, wo, wl, rb = case
    p = _lib.Payloads()
    if var is not None:
        p.var, p.pos = var.ctypes.data + 64, pos.ctypes.data + 64
        p.cap_var = var.size - 128 if cap_var is None else cap_var
        p.cap_pos = pos.size - 16 if cap_pos is None else cap_pos
    st = _lib.lib.clg_gather_payloads_host(data.ctypes.data if data.size else None, so.ctypes.data, sl.ctypes.data, so.size,
                                           wo.ctypes.data if wo.size else None, wl.ctypes.data if wl.size else None,
                                           rb.ctypes.data, C.byref(p))
    return st, p


def guarded(n_var, n_pos):
    return np.full(n_var + 128, FILL, np.uint8), np.full(n_pos + 16, 0xA5A5A5A5A5A5A5A5, np.uint64)


@pytest.mark.parametrize("seed", range(6))
def test_library_against_slicing(seed):
    from clonos_amd import _lib, gather_payloads_host
    rng = np.random.default_rng(seed)
    case = seeded(rng)
    want, want_pos = sliced(*case)
    n = len(want_pos) - 1
    got, got_pos = gather_payloads_host(*case)
    assert got.dtype == np.uint8 and got_pos.dtype == np.uint64
    assert (got_pos == want_pos).all() and (got == want).all()
    # sizes only
    st, p = raw_call(case, None, None)
    assert st == 0 and (p.n_rows, p.n_var, p.bad_row) == (n, want.size, NO_ROW)
    # exact capacities: the guards either side stay
    var, pos = guarded(want.size, n + 1)
    st, p = raw_call(case, var, pos)
    assert st == 0 and (p.n_rows, p.n_var, p.bad_row) == (n, want.size, NO_ROW)
    assert (var[:64] == FILL).all() and (var[-64:] == FILL).all() and (var[64:-64] == want).all()
    assert (pos[:8] == 0xA5A5A5A5A5A5A5A5).all() and (pos[-8:] == 0xA5A5A5A5A5A5A5A5).all() and (pos[8:-8] == want_pos).all()
    # each capacity one short: the results filled, nothing written
    for cv, cp in ((want.size - 1, n + 1), (want.size, n)):
        var, pos = guarded(want.size, n + 1)
        st, p = raw_call(case, var, pos, cv, cp)
        assert st == _lib.CLG_E_CAPACITY and (p.n_rows, p.n_var) == (n, want.size)
        assert (var == FILL).all() and (pos == 0xA5A5A5A5A5A5A5A5).all()


def test_bad_row_gives_its_lowest_index():
    from clonos_amd import ClonosError, _lib, gather_payloads_host
    rng = np.random.default_rng(77)
    case = seeded(rng)
    data, so, sl, wo, wl, rb = case
    want, want_pos = sliced(*case)
    n = len(want_pos) - 1
    span_of = np.searchsorted(rb, np.arange(n), side="right") - 1
    for where in ([n // 2], [3, n - 1], [n - 1], [0, 1]):
        wo2, wl2 = wo.copy(), wl.copy()
        for i, k in enumerate(where):
            if i % 2 == 0:
                wo2[k], wl2[k] = sl[span_of[k]], 1       # one byte past the span's last
            else:
                wo2[k], wl2[k] = 0xFFFFFFFF, 2           # off + len wraps in 32 bits
        var, pos = guarded(want.size + 8, n + 1)
        st, p = raw_call((data, so, sl, wo2, wl2, rb), var, pos)
        assert st == _lib.CLG_E_INVALID_ARG and p.bad_row == min(where) and p.n_rows == n
        assert p.n_var == want.size - int(wl[where].sum())  # a bad row counts as length 0
        assert (var == FILL).all() and (pos == 0xA5A5A5A5A5A5A5A5).all()
        with pytest.raises(ClonosError) as ei:
            gather_payloads_host(data, so, sl, wo2, wl2, rb)
        assert ei.value.status == _lib.CLG_E_INVALID_ARG and ei.value.bad_row == min(where)


def test_no_rows_and_bad_row_base():
    from clonos_amd import ClonosError, _lib, gather_payloads_host
    var, pos = gather_payloads_host(b"abc", [0, 3], [3, 0], [], [], [0, 0, 0])
    assert var.size == 0 and pos.tolist() == [0]
    var, pos = gather_payloads_host(b"", [], [], [], [], [0])
    assert var.size == 0 and pos.tolist() == [0]
    for rb in ([1, 1, 2], [0, 2, 1]):
        with pytest.raises(ClonosError) as ei:
            gather_payloads_host(b"abcdef", [0, 3], [3, 3], [0, 0], [1, 1], rb)
        assert ei.value.status == _lib.CLG_E_INVALID_ARG


def test_columns_views_over_a_payload_column():
    """DecodedColumns with var / var_pos from the host call: payload(k), determinants(), to_soa()
    and ColumnReplayer read the packed column, ahead of spans_bytes."""
    from clonos_amd import columnize_host, gather_payloads_host, synth
    from clonos_amd import determinants as D
    from clonos_amd.replay import ColumnReplayer
    rng = np.random.default_rng(5)
    spans = [synth.random_log(200, rng), b"", synth.config3_epoch(300, rng)[0],
             D.encode(D.TimerTriggerDeterminant(5, 1000, D.INTERNAL, b"PTS")) + D.encode(D.SerializableDeterminant(b"\xac\xed\x00\x05t\x00\x01x"))]
    b = oracle_batch(spans)
    c = columnize_host(b)
    data = np.concatenate([np.frombuffer(bytes(s), np.uint8) for s in spans])
    offs = np.concatenate([[0], np.cumsum([len(s) for s in spans])]).astype(np.uint64)
    c.var, c.var_pos = gather_payloads_host(data, offs[:-1], np.diff(offs), c.w_var_off, c.w_var_len, c.span_base[:, 4])
    assert int(c.var_pos[-1]) == int(c.w_var_len.sum()) == c.var.size and c.var.size > 0
    for s in range(c.n_spans):
        sp = c.span(s)
        raw = bytes(spans[s])
        for k in range(sp.w0, sp.w0 + sp.n_wide):
            o, l = int(c.w_var_off[k]), int(c.w_var_len[k])
            assert c.payload(k) == raw[o:o + l]
    want = [b.determinants(s) for s in range(c.n_spans)]
    c.spans_bytes = None  # nothing but the columns
    for s in range(c.n_spans):
        assert c.determinants(s) == want[s]
        assert c.to_soa().determinants(s) == want[s]
        rep, got = ColumnReplayer(c, s), []
        while not rep.isFinished():
            t = rep.next_tag()
            if t == D.SERIALIZABLE:
                got.append(D.SerializableDeterminant(rep.replaySerializableDeterminant()))
            elif t in (D.TIMER_TRIGGER, D.SOURCE_CHECKPOINT, D.IGNORE_CHECKPOINT):
                got.append(rep.triggerAsyncEvent(rep.record_count_target()))
            else:
                got.append({D.ORDER: lambda: D.OrderDeterminant(rep.replayNextChannel()),
                            D.TIMESTAMP: lambda: D.TimestampDeterminant(rep.replayNextTimestamp()),
                            D.RNG: lambda: D.RNGDeterminant(rep.replayRandomInt()),
                            D.BUFFER_BUILT: lambda: D.BufferBuiltDeterminant(rep.replayNextBufferSize())}[t]())
        assert got == want[s]
    with pytest.raises(IndexError):
        c.payload(len(c.w_idx))
    with pytest.raises(ValueError):
        columnize_host(b).payload(0)
