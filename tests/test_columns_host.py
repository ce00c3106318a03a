"""CPU: typed replay columns on the host.  The header's one-pass function (clonos_amd/csrc/columns.h,
compiled with g++ into the stand-alone program tests/columns_host.cpp, once plainly and once with
-fsanitize=address,undefined, and run directly), and clg_columnize_host of the library on the
oracle's decode of synthetic logs: every column equals v0[tag == t] narrowed, to_soa() gives the
input back, DecodedColumns.determinants equals DecodedBatch.determinants, and ColumnReplayer walks
a span as LogReplayerImpl walks its log."""
import os
import re
import subprocess

import numpy as np
import pytest

from _columns_util import oracle_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "columns_host.cpp")


@pytest.fixture(scope="module")
def batches():
    from clonos_amd import job as J
    from clonos_amd import synth
    rng = np.random.default_rng(0xC0105)
    out = {}
    out["random"] = oracle_batch([synth.random_log(n, rng) for n in (300, 0, 1, 257, 0)])
    out["config2"] = oracle_batch([synth.config2_log(n, rng)[0] for n in (5000, 4096, 1)])
    out["config3"] = oracle_batch([synth.config3_epoch(n, rng)[0] for n in (3000, 700)])
    table = J.LogTable(J.dag(2, 4))
    gids = np.arange(len(table))
    data, offs = synth.config4_epoch(table, gids, rng, main_records=300, sub_records=16)
    out["config4"] = oracle_batch([data[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])])
    return out


NAMES = ("random", "config2", "config3", "config4")


def test_header_one_pass_function(tmp_path):
    exe = str(tmp_path / "columns_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 100000, r.stdout


def test_header_one_pass_function_sanitized(tmp_path):
    """The same program with the address and undefined-behaviour sanitizers, run directly (their
    runtimes linked into the program: it needs nothing preloaded)."""
    exe = str(tmp_path / "columns_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok (\d+)\n", r.stdout), r.stdout


@pytest.mark.parametrize("name", NAMES)
def test_columns_equal_the_filtered_soa(batches, name):
    from clonos_amd import columnize_host
    b = batches[name]
    c = columnize_host(b)
    assert b.n_rec > 0 and c.n_rec == b.n_rec
    assert c.tag.dtype == np.uint8 and (c.tag == b.tag).all()
    for t, col, dt in ((0, c.order, np.int8), (1, c.timestamp, np.int64), (2, c.rng, np.int32),
                       (7, c.buffer_built, np.int32)):
        want = b.v0[b.tag == t]
        assert col.dtype == dt and len(col) == len(want)
        assert (col == want.astype(dt)).all() and (col.astype(np.int64) == want).all()  # narrowed without loss
    wide = (b.tag >= 3) & (b.tag <= 6)
    assert (c.w_v0 == b.v0[wide]).all() and (c.w_idx == np.nonzero(wide)[0]).all()
    for k in ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub"):
        assert (getattr(c, k) == getattr(b, k)).all(), k
    # the span bases: class counts before every span, the totals last
    cls = np.array([0, 1, 2, 4, 4, 4, 4, 3])[b.tag]
    for s, r in enumerate(b.span_rec_base):
        assert c.span_base[s].tolist() == [int((cls[:int(r)] == k).sum()) for k in range(5)], s
    assert (c.span_rec_base == b.span_rec_base).all()
    # the inverse
    back = c.to_soa()
    assert back.off is None
    for k in ("tag", "v0", "w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "span_rec_base"):
        assert (getattr(back, k) == getattr(b, k)).all(), k


@pytest.mark.parametrize("name", NAMES)
def test_span_views_and_determinants(batches, name):
    from clonos_amd import columnize_host
    b = batches[name]
    c = columnize_host(b)
    assert c.n_spans == len(b.span_rec_base) - 1
    for s in range(c.n_spans):
        sl = b.span_slice(s)
        sp = c.span(s)
        assert (sp.tag == b.tag[sl]).all()
        assert (sp.order == b.v0[sl][b.tag[sl] == 0]).all() and (sp.timestamp == b.v0[sl][b.tag[sl] == 1]).all()
        assert (sp.rng == b.v0[sl][b.tag[sl] == 2]).all() and (sp.buffer_built == b.v0[sl][b.tag[sl] == 7]).all()
        assert sp.n_wide == int(((b.tag[sl] >= 3) & (b.tag[sl] <= 6)).sum())
        assert c.determinants(s) == b.determinants(s)


def drive(rep, D):
    """Walk a ColumnReplayer by its tag sequence, as the task's calls would; returns the
    determinants it yielded and the record-count targets seen before each record."""
    got, targets = [], []
    while not rep.isFinished():
        t = rep.next_tag()
        targets.append(rep.record_count_target())
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
            got.append(rep.triggerAsyncEvent(targets[-1]))
    return got, targets


@pytest.mark.parametrize("name", NAMES)
def test_column_replayer_follows_the_log(batches, name):
    from clonos_amd import columnize_host
    from clonos_amd import determinants as D
    from clonos_amd.replay import ColumnReplayer
    b = batches[name]
    c = columnize_host(b)
    for s in range(c.n_spans):
        want = b.determinants(s)
        got, targets = drive(ColumnReplayer(c, s), D)
        assert got == want
        assert targets == [getattr(d, "record_count", None) if not isinstance(d, D.SerializableDeterminant) else None
                           for d in want]


def test_column_replayer_raises_on_a_wrong_call(batches):
    from clonos_amd import columnize_host
    from clonos_amd import determinants as D
    from clonos_amd.replay import ColumnReplayer, ReplayOrderError
    spans = [D.encode(D.OrderDeterminant(3)) + D.encode(D.TimestampDeterminant(77)) +
             D.encode(D.TimerTriggerDeterminant(5, 1000, D.INTERNAL, b"PTS")) + D.encode(D.RNGDeterminant(-9))]
    c = columnize_host(oracle_batch(spans))
    rep = ColumnReplayer(c, 0)
    with pytest.raises(ReplayOrderError) as ei:
        rep.replayNextTimestamp()
    assert ei.value.position == 0 and ei.value.asked == "TIMESTAMP" and ei.value.found == "ORDER"
    assert "0" in str(ei.value) and "TIMESTAMP" in str(ei.value) and "ORDER" in str(ei.value)
    assert rep.replayNextChannel() == 3  # (the failed call consumed nothing)
    with pytest.raises(ReplayOrderError):
        rep.triggerAsyncEvent(5)
    assert rep.record_count_target() is None
    assert rep.replayNextTimestamp() == 77
    assert rep.record_count_target() == 5  # the next determinant is async: its record count
    with pytest.raises(ReplayOrderError):
        rep.replayRandomInt()
    with pytest.raises(RuntimeError, match="Current record count is not the determinants record count") as ei:
        rep.triggerAsyncEvent(4)
    assert not isinstance(ei.value, ReplayOrderError)
    d = rep.triggerAsyncEvent(5)  # (the mismatch consumed nothing)
    assert d == D.TimerTriggerDeterminant(5, 1000, D.INTERNAL, b"PTS")
    assert not rep.isFinished() and rep.replayRandomInt() == -9 and rep.isFinished()
    with pytest.raises(ReplayOrderError) as ei:
        rep.replayNextChannel()
    assert ei.value.position == 4


def test_host_error_rules(batches):
    from clonos_amd import ClonosError, DecodedBatch, _lib, columnize_host
    b = batches["random"]
    tag = b.tag.copy()
    tag[[41, 200]] = (9, 200)
    bad = DecodedBatch(b.off, tag, b.v0, b.w_idx, b.w_rc, b.w_v1, b.w_var_off, b.w_var_len, b.w_sub, b.span_rec_base)
    with pytest.raises(ClonosError) as ei:
        columnize_host(bad)
    assert ei.value.status == _lib.CLG_E_INVALID_ARG and ei.value.err_off == 41 and ei.value.err_tag == 9
    assert ei.value.err_span == 0
    empty = DecodedBatch(*[np.zeros(0, dt) for dt in (np.uint32, np.uint8, np.int64, np.uint32, np.int32, np.int64,
                                                      np.uint32, np.uint32, np.uint8)], np.zeros(3, np.uint64))
    c = columnize_host(empty)
    assert c.n_rec == 0 and c.n_spans == 2 and not c.span_base.any() and c.determinants(1) == []
