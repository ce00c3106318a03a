"""GPU: the payload column of logs in the segment pool (clg_decode_logs_columns_var,
clg_decode_host_columns_var, clg_gather_payloads_logs).  Logs are built from determinants.encode
so that payloads meet the segment boundaries in every way; the expected bytes are the oracle's
w_var_off / w_var_len sliced out of the span bytes in Python.

With 256-byte segments a row of under 64 bytes can cross one boundary at most, so the short rows
that straddle more run on an engine with 16-byte segments (the smallest the engine takes), through
gather_payloads_logs (append and gather only).  There 63 bytes cross four boundaries at most, so
the short rows cover one, two and four; five boundaries are covered by long rows only."""
import numpy as np
import pytest

from _columns_util import assert_columns_equal, oracle_batch

pytestmark = pytest.mark.gpu

C = 256
SHORT = 64  # kPayWaveRow: rows of under 64 bytes are copied by one lane


def ascii_bytes(rng, n):
    return bytes(rng.integers(97, 123, n, dtype=np.uint8))


def payload_record(kind, payload, i):
    """(determinant, offset of the payload in its record, payload bytes as the decode reports them)."""
    from clonos_amd import determinants as D
    if kind == "timer":       # [tag][rc i32][ts i64][type][len i32][name]
        return D.TimerTriggerDeterminant(100 + i, 5000 + i, D.INTERNAL, payload), 18, payload
    if kind == "source":      # [tag][rc i32][id i64][ts i64][type][has ref][len i32][ref]
        return D.SourceCheckpointDeterminant(200 + i, 7 + i, 9000 + i, D.CHECKPOINT, payload), 27, payload
    stream = D.jser_string(payload.decode())  # [tag][AC ED 00 05 74][len u16][chars]: the stream is the payload
    return D.SerializableDeterminant(stream), 1, stream


def padding(p):
    """p bytes of short records (ORDER 2 B, RNG 5 B); p is 0, 2, or at least 4."""
    from clonos_amd import determinants as D
    assert p >= 0 and p not in (1, 3)
    out = b""
    if p % 2:
        out += D.encode(D.RNGDeterminant(p))
        p -= 5
    return out + D.encode(D.OrderDeterminant(3)) * (p // 2)


def placed(prefix, wants, seg, rng):
    """prefix, then for each (kind, start mod seg, payload length) a record whose payload starts at
    that physical residue (padding records before it).  Returns the bytes."""
    from clonos_amd import determinants as D
    buf = bytearray(prefix)
    for i, (kind, start_mod, length) in enumerate(wants):
        plen = length if kind != "serial" else length - 7  # (a TC_STRING stream is 7 bytes + its chars)
        det, rel, payload = payload_record(kind, ascii_bytes(rng, plen), i)
        assert len(payload) == length
        pad = (start_mod - rel - len(buf)) % seg
        if pad in (1, 3):
            pad += seg
        buf += padding(pad) + D.encode(det)
        assert (len(buf) - length) % seg == start_mod
    return bytes(buf)


def boundaries(start, length, seg):
    return (start + length - 1) // seg - start // seg if length else 0


# (kind, payload start mod 256, payload length)
WANTS_256 = [
    ("timer", 255, 20), ("source", 255, 100), ("serial", 255, 300),   # start on a segment's last byte
    ("timer", 236, 20), ("serial", 156, 100), ("source", 0, 256),     # end exactly at a segment's end
    ("source", 250, 40), ("timer", 230, 63),                           # short, one boundary
    ("timer", 200, 100), ("serial", 200, 400), ("source", 100, 1300),  # long: one, two, five boundaries
    ("timer", 17, 0), ("timer", 40, 1), ("source", 255, 1), ("timer", 1, 64), ("serial", 129, 65),
]


@pytest.fixture(scope="module")
def placed_logs():
    """Three logs: one whose decoded range starts mid-segment (start_epoch 1 after 300 bytes of epoch
    0, so run.phys != 0), one from epoch 0, one empty.  (log bytes per epoch, start epochs, spans)."""
    from clonos_amd import synth
    rng = np.random.default_rng(0x9A7)
    first = synth.random_log(60, rng, allow_serializable=False)
    first += padding((300 - len(first)) % C + (C if (300 - len(first)) % C in (1, 3) else 0))
    a = placed(first, WANTS_256, C, rng)
    b = placed(b"", list(reversed(WANTS_256)), C, rng)
    logs = [((first, a[len(first):]), 1), ((b, b""), 0), ((b"", b""), 0)]
    spans = [a[len(first):], b, b""]
    assert len(first) % C not in (0,)  # the range starts mid-segment
    return logs, spans, len(first)


def open_placed(engine, logs, base=0):
    from clonos_amd import CausalLogID
    out = []
    for i, ((e0, e1), _) in enumerate(logs):
        lg = engine.open_log(CausalLogID.main(base + i))
        if e0:
            lg.appendDeterminant(e0, 0)
        if e1:
            lg.appendDeterminant(e1, 1)
        out.append(lg)
    return out


def open_logs(engine, spans):
    from clonos_amd import CausalLogID
    logs = []
    for i, b in enumerate(spans):
        lg = engine.open_log(CausalLogID.main(i))
        if len(b):
            lg.appendDeterminant(bytes(b), 0)
        logs.append(lg)
    return logs


def want_payloads(batch):
    """Every wide row's payload by slicing its span's bytes (the oracle's offsets)."""
    out = []
    raws = [bytes(b) for b in batch.spans_bytes]
    span_of = np.searchsorted(np.asarray(batch.span_rec_base), batch.w_idx, side="right") - 1
    for s, o, l in zip(span_of.tolist(), batch.w_var_off.tolist(), batch.w_var_len.tolist()):
        assert o + l <= len(raws[s])
        out.append(raws[s][o:o + l])
    return out


def check_payloads(cols, want):
    assert cols.var is not None and len(cols.var_pos) == len(want) + 1
    assert int(cols.var_pos[-1]) == len(cols.var) == sum(len(w) for w in want)
    for k, w in enumerate(want):
        assert cols.payload(k) == w, k


def test_geometry_of_the_placed_logs(placed_logs):
    """The test's own premise: the payloads meet the boundaries as the cases ask."""
    _, spans, phys0 = placed_logs
    b = oracle_batch(spans[:1])
    starts = (phys0 + b.w_var_off[b.w_var_len > 0]).astype(np.int64)
    lens = b.w_var_len[b.w_var_len > 0].astype(np.int64)
    short, long_ = lens < SHORT, lens >= SHORT
    assert ((starts % C == C - 1) & short).any() and ((starts % C == C - 1) & long_).any()
    assert (((starts + lens) % C == 0) & short).any() and (((starts + lens) % C == 0) & long_).any()
    cross = np.array([boundaries(int(s), int(l), C) for s, l in zip(starts, lens)])
    assert {1} <= set(cross[short].tolist()) and {1, 2, 5} <= set(cross[long_].tolist())
    assert phys0 % C != 0


def test_decode_logs_columns_with_payloads(engine, placed_logs):
    logs, spans, _ = placed_logs
    lgs = open_placed(engine, logs)
    eps = [ep for _, ep in logs]
    # first call of all: the logs' tails are still unflushed
    engine.kernel_stats_reset()
    got = engine.decode_logs_columns(lgs, eps, payloads=True)
    st = engine.kernel_stats()
    assert "decode_payloads" in st and st["decode_payloads"]["launches"] > 0 and st["decode_payloads"]["bytes"] > 0
    plain = engine.decode_logs_columns(lgs, eps)
    assert plain.var is None and plain.var_pos is None
    assert_columns_equal(got, plain)
    batch = oracle_batch(spans)
    check_payloads(got, want_payloads(batch))
    assert [got.determinants(s) for s in range(3)] == [batch.determinants(s) for s in range(3)]
    for s, lg in enumerate(lgs):
        assert lg.getDeterminants(eps[s]) == spans[s]
    # the same bytes from host memory
    data = np.frombuffer(b"".join(spans), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in spans])])
    host = engine.decode_host_columns(data, [(int(o), len(s)) for o, s in zip(offs, spans)], payloads=True)
    assert_columns_equal(host, plain)
    check_payloads(host, want_payloads(batch))
    assert (host.var == got.var).all() and (host.var_pos == got.var_pos).all()
    # the raw entry point over the columns' rows gives the same column
    h = np.array([l.handle for l in lgs], np.uint32)
    var, pos = engine.gather_payloads_logs(h, eps, got.w_var_off, got.w_var_len, got.span_base[:, 4])
    assert (var == got.var).all() and (pos == got.var_pos).all()


def test_encode_columns_gives_the_log_back(engine, placed_logs):
    logs, spans, _ = placed_logs
    lgs = open_placed(engine, logs)
    for s in (0, 1):
        cols = engine.decode_logs_columns([lgs[s]], [logs[s][1]], payloads=True)
        assert engine.encode_columns(cols) == lgs[s].getDeterminants(logs[s][1]) == spans[s]
    with pytest.raises(ValueError):
        engine.encode_columns(engine.decode_logs_columns([lgs[0]], [1]))


def test_column_replayer_over_hbm_logs_needs_only_the_columns(engine, placed_logs):
    from clonos_amd import determinants as D
    from clonos_amd.replay import ColumnReplayer
    logs, spans, _ = placed_logs
    lgs = open_placed(engine, logs)
    cols = engine.decode_logs_columns(lgs, [ep for _, ep in logs], payloads=True)
    assert cols.spans_bytes is None
    batch = oracle_batch(spans)
    for s in range(3):
        want = [d for d in batch.determinants(s) if isinstance(d, (D.TimerTriggerDeterminant, D.SourceCheckpointDeterminant,
                                                                    D.SerializableDeterminant))]
        rep, got = ColumnReplayer(cols, s), []
        while not rep.isFinished():
            t = rep.next_tag()
            if t == D.SERIALIZABLE:
                got.append(D.SerializableDeterminant(rep.replaySerializableDeterminant()))
            elif t in (D.TIMER_TRIGGER, D.SOURCE_CHECKPOINT):
                got.append(rep.triggerAsyncEvent(rep.record_count_target()))
            elif t == D.ORDER:
                rep.replayNextChannel()
            elif t == D.RNG:
                rep.replayRandomInt()
            elif t == D.TIMESTAMP:
                rep.replayNextTimestamp()
            elif t == D.BUFFER_BUILT:
                rep.replayNextBufferSize()
            else:
                rep.triggerAsyncEvent(rep.record_count_target())
        assert got == want and (s == 2 or len(want) >= len(WANTS_256))


def test_decode_error_keeps_the_rows_before_it(engine):
    from clonos_amd import synth
    rng = np.random.default_rng(11)
    good = [synth.random_log(300, rng, allow_serializable=False) for _ in range(3)]
    cut = synth.random_log(120, rng, allow_serializable=False) + b"\x09" + synth.random_log(40, rng, allow_serializable=False)
    spans = [good[0], cut, good[1], good[2]]
    lgs = open_logs(engine, spans)
    want_batch, err = oracle_batch(spans, allow_errors=True)
    assert err is not None and err[1] == 1
    got = engine.decode_logs_columns(lgs, [0] * 4, partial=True, payloads=True)
    plain = engine.decode_logs_columns(lgs, [0] * 4, partial=True)
    assert got.error is not None and got.error.status == err[0]
    assert (got.error.err_span, got.error.err_off, got.error.err_tag) == err[1:]
    assert_columns_equal(got, plain)
    assert got.span(1).tag.size == 120
    want = want_payloads(want_batch)
    assert any(len(w) for w in want)
    check_payloads(got, want)


@pytest.fixture(params=["auto", "robust", "one_pass"])
def engine4k(request, monkeypatch):
    """The conftest engine fixture's decode variants on 4 KiB segments."""
    from clonos_amd import Engine
    if request.param == "one_pass":
        monkeypatch.setenv("CLONOS_ONE_PASS", "2")
        e = Engine(segment_bytes=4096, pool_segments=1 << 12, timing=True, decode="three_pass")
        monkeypatch.delenv("CLONOS_ONE_PASS")
    else:
        e = Engine(segment_bytes=4096, pool_segments=1 << 12, timing=True, decode=request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def config3_spans():
    from clonos_amd import synth
    rng = np.random.default_rng(3)
    spans = [bytes(synth.config3_epoch(n, rng)[0]) for n in (20000, 19000, 21000)]
    batch = oracle_batch(spans)
    return spans, batch, want_payloads(batch)


def test_config3_mix(engine4k, config3_spans):
    spans, batch, want = config3_spans
    assert (batch.tag == 3).any() and len(want) > 3000
    lgs = open_logs(engine4k, spans)
    got = engine4k.decode_logs_columns(lgs, [0] * len(lgs), payloads=True)
    assert_columns_equal(got, engine4k.decode_logs_columns(lgs, [0] * len(lgs)))
    check_payloads(got, want)
    assert got.determinants(1) == batch.determinants(1)


def test_short_rows_across_several_boundaries():
    """16-byte segments: rows of under 64 bytes that straddle one, two and four boundaries (the most
    63 bytes can), start on
    a segment's last byte and end exactly at a segment's end; the range starts mid-segment."""
    from clonos_amd import CausalLogID, Engine
    seg = 16
    rng = np.random.default_rng(0x16)
    wants = [("timer", 15, 10), ("timer", 10, 6), ("source", 9, 20), ("timer", 5, 40), ("source", 3, 63), ("timer", 15, 62),
             ("serial", 4, 12 + 16 * 3), ("timer", 0, 16), ("timer", 7, 0), ("source", 15, 1), ("serial", 15, 200)]
    first = padding(24)
    full = placed(first, wants, seg, rng)
    span = full[len(first):]
    b = oracle_batch([span])
    starts = (len(first) + b.w_var_off).astype(np.int64)
    lens = b.w_var_len.astype(np.int64)
    cross = {boundaries(int(s), int(l), seg) for s, l in zip(starts, lens) if 0 < l < SHORT}
    assert {1, 2, 4} <= cross and len(first) % seg != 0
    want = want_payloads(b)
    with Engine(segment_bytes=seg, pool_segments=256, timing=True) as eng:
        lg = eng.open_log(CausalLogID.main(1))
        lg.appendDeterminant(first, 0)
        lg.appendDeterminant(span, 1)
        var, pos = eng.gather_payloads_logs([lg.handle], [1], b.w_var_off, b.w_var_len, [0, len(want)])
        assert pos.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
        for k, w in enumerate(want):
            assert var[int(pos[k]):int(pos[k + 1])].tobytes() == w, k
        assert lg.getDeterminants(1) == span
