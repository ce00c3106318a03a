"""GPU: typed columns appended to logs on the device (clg_append_columns).  Every log that takes a
span of columns has a twin that takes the same bytes through appendDeterminant; the pairs must
agree on everything the log interface shows, and a decode of the appended logs must be the
oracle's decode of the bytes."""
import numpy as np
import pytest

from _encode_util import host_columns
from test_gpu_decode import assert_span_equal

pytestmark = pytest.mark.gpu


def five_spans():
    """Five spans: two with Serializable records, one empty."""
    from clonos_amd import synth
    rng = np.random.default_rng(0xAC)
    return [synth.random_log(200, rng, allow_serializable=True), synth.random_log(150, rng, allow_serializable=False), b"",
            bytes(synth.config3_epoch(700, rng)[0]), synth.random_log(40, rng, allow_serializable=False)]


SPANS = five_spans()


def open_pairs(eng, n, base=0):
    from clonos_amd import CausalLogID
    return ([eng.open_log(CausalLogID.main(base + i)) for i in range(n)],
            [eng.open_log(CausalLogID.main(base + 1000 + i)) for i in range(n)])


def assert_same(a, b, epochs=(0,)):
    for e in epochs:
        assert a.getDeterminants(e) == b.getDeterminants(e)
    assert a.logLength() == b.logLength()
    assert a.state() == b.state()


@pytest.fixture
def eng():
    from clonos_amd import Engine
    e = Engine(segment_bytes=256, pool_segments=1 << 12, timing=True)
    yield e
    e.close()


def test_twin_logs(eng):
    cols = host_columns(SPANS)
    logs, twins = open_pairs(eng, 5)
    epochs = [0, 0, 3, 1, 0]
    nb = eng.append_columns(logs, epochs, cols)
    assert nb.tolist() == [len(s) for s in SPANS]
    for t, s, e in zip(twins, SPANS, epochs):
        t.appendDeterminant(s, e)
    for a, b, s, e in zip(logs, twins, SPANS, epochs):
        assert_same(a, b, (0, e))
        assert a.getDeterminants(e) == s
    st = eng.kernel_stats()
    assert st["append_columns_scatter"]["launches"] == 1 and st["append_columns_scatter"]["bytes"] == 2 * sum(map(len, SPANS))


def test_pending_host_bytes_keep_their_order(eng):
    cols = host_columns(SPANS[:2])
    logs, twins = open_pairs(eng, 2)
    for lg in (logs[0], twins[0]):
        lg.appendDeterminant(SPANS[4], 0)  # staged on the host, not flushed
    eng.append_columns(logs, [0, 0], cols)
    twins[0].appendDeterminant(SPANS[0], 0)
    twins[1].appendDeterminant(SPANS[1], 0)
    assert logs[0].getDeterminants(0) == SPANS[4] + SPANS[0]
    for a, b in zip(logs, twins):
        assert_same(a, b)
    logs[0].appendDeterminant(SPANS[4], 0)  # and host appends go on behind the device's bytes
    twins[0].appendDeterminant(SPANS[4], 0)
    assert_same(logs[0], twins[0])


def test_one_log_twice(eng):
    cols = host_columns([SPANS[0], SPANS[3]])
    (lg,), (tw,) = open_pairs(eng, 1)
    eng.append_columns([lg, lg], [0, 1], cols)
    tw.appendDeterminant(SPANS[0], 0)
    tw.appendDeterminant(SPANS[3], 1)
    assert_same(lg, tw, (0, 1))
    assert lg.getDeterminants(0) == SPANS[0] + SPANS[3] and lg.getDeterminants(1) == SPANS[3]


def test_skipped_and_unknown_logs(eng):
    from clonos_amd import CausalLogID, _lib
    cols = host_columns(SPANS[:4])
    off = eng.open_job((0xC, 0xD), sharing_depth=0)  # logging switched off for this job
    lz = eng.open_log(CausalLogID.main(77), off)
    (a, b), (ta, tb) = open_pairs(eng, 2)
    before = lz.state()
    nb, st = eng.append_columns([a, lz, 9999, b], [0, 0, 0, 0], cols, statuses=True)
    assert st.tolist() == [0, 0, _lib.CLG_E_NO_LOG, 0]
    assert nb.tolist() == [len(s) for s in SPANS[:4]]
    assert lz.state() == before and lz.logLength() == 0
    ta.appendDeterminant(SPANS[0], 0)
    tb.appendDeterminant(SPANS[3], 0)
    assert_same(a, ta)
    assert_same(b, tb)
    with pytest.raises(_lib.ClonosError) as ex:
        eng.append_columns([a, lz, 9999, b], [1, 1, 1, 1], cols)
    assert ex.value.status == _lib.CLG_E_NO_LOG and ex.value.span == 2


def test_pool_exhaustion_leaves_the_log_unchanged():
    from clonos_amd import Engine, _lib
    from clonos_amd import determinants as D
    with Engine(segment_bytes=256, pool_segments=8) as eng:
        small = D.encode(D.OrderDeterminant(3)) * 50 + D.encode(D.TimestampDeterminant(9)) * 10
        assert len(SPANS[0]) > 8 * 256 and len(small) <= 256
        cols = host_columns([small, SPANS[0], small])
        (a, big, c), (ta, _, tc) = open_pairs(eng, 3)
        before = big.state()
        nb, st = eng.append_columns([a, big, c], [0, 0, 0], cols, statuses=True)
        assert st.tolist() == [0, _lib.CLG_E_NOSPACE, 0]
        assert big.state() == before and big.logLength() == 0 and big.getDeterminants(0) == b""
        ta.appendDeterminant(small, 0)
        tc.appendDeterminant(small, 0)
        assert_same(a, ta)
        assert_same(c, tc)


def test_invalid_columns_change_no_log(eng):
    from clonos_amd import _lib
    cols = host_columns(SPANS[:2])
    cols.tag = cols.tag.copy()
    cols.tag[len(cols.tag) - 1] = 9
    logs, _ = open_pairs(eng, 2)
    before = [lg.state() for lg in logs]
    with pytest.raises(_lib.ClonosError) as ex:
        eng.append_columns(logs, [0, 0], cols)
    assert ex.value.status == _lib.CLG_E_INVALID_ARG
    assert [lg.state() for lg in logs] == before


def test_later_operations_behave_as_on_the_twins(eng):
    ch = (1, 2)
    (lg,), (tw,) = open_pairs(eng, 1)
    eng.append_columns([lg], [0], host_columns([SPANS[0]]))
    tw.appendDeterminant(SPANS[0], 0)
    for x in (lg, tw):
        assert x.hasDeltaForConsumer(ch, 0)
    assert lg.getDeltaForConsumer(ch, 0) == tw.getDeltaForConsumer(ch, 0) == SPANS[0]
    eng.append_columns([lg], [1], host_columns([SPANS[3]]))  # a second append, in a new epoch
    tw.appendDeterminant(SPANS[3], 1)
    assert_same(lg, tw, (0, 1))
    for x in (lg, tw):
        assert x.hasDeltaForConsumer(ch, 1)
    assert lg.getDeltaForConsumer(ch, 1) == tw.getDeltaForConsumer(ch, 1)
    assert lg.consumer_state(ch) == tw.consumer_state(ch)
    for x in (lg, tw):
        x.notifyCheckpointComplete(1)  # the first epoch goes
    assert_same(lg, tw, (1,))
    assert lg.getDeterminants(1) == SPANS[3]
    eng.append_columns([lg], [2], host_columns([SPANS[1]]))
    tw.appendDeterminant(SPANS[1], 2)
    assert_same(lg, tw, (1, 2))


@pytest.mark.parametrize("side", [True, False], ids=["sidecar", "scan"])
def test_decode_of_appended_logs(monkeypatch, side):
    """decode_logs of logs that only ever took columns: the oracle's decode.  With the sidecar the
    Serializable length tables come from the lists the scatter's writer filled (no fallback)."""
    from clonos_amd import Engine
    monkeypatch.setenv("CLONOS_SIDECAR", "1" if side else "0")
    with Engine(segment_bytes=256, pool_segments=1 << 12, timing=True) as eng:
        logs, _ = open_pairs(eng, len(SPANS))
        eng.append_columns(logs, [0] * len(SPANS), host_columns(SPANS))
        for _ in range(2):  # the first batch learns that the logs hold Serializable records
            eng.kernel_stats_reset()
            dec = eng.decode_logs(logs, [0] * len(SPANS))
            for s, b in enumerate(SPANS):
                assert_span_equal(dec, s, b)
        ks = eng.kernel_stats()
        assert "decode_fallback" not in ks and "decode_span_fallback" not in ks, sorted(ks)
        if side:
            assert ks["decode_jser"]["launches"] >= 1, sorted(ks)
