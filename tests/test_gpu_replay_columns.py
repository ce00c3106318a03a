"""GPU: replay preparation that delivers typed columns and the payload column
(clg_replay_prepare_columns, replay.prepare_replay_columns).

The scene is test_gpu_replay.py's config-5 one at a quarter of its size: 4 failed vertices, 2
subpartitions each, at most 400 records an epoch, two or three responders whose engine logs
went through checkpoint truncation, one subpartition log that no responder holds.  Checked
against prepare_replay on the same jobs (the main batch through columnize_host, every
subpartition field), against the response oracle's spans for the payload bytes, and against the
decode oracle's determinants for the replayer."""
import os
import struct
import sys

import numpy as np
import pytest

import _oracle as O
from _columns_util import assert_columns_equal, oracle_batch
from clonos_amd import CausalLogID, ClonosError, Engine, _lib, columnize_host, job, synth
from clonos_amd import determinants as D
from clonos_amd.replay import DeterminantResponseEvent, accumulate, prepare_replay, prepare_replay_columns, prepare_replay_raw

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import response_ref as R  # noqa: E402  (checker)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SUB = 2


def _bb(rng, n):
    return b"".join(b"\x07" + struct.pack(">i", int(x)) for x in rng.integers(-(1 << 31), 1 << 31, n))


def _rid(lid):
    if lid.is_main:
        return R.LogId.main(lid.vertex_id)
    return R.LogId.subpartition(lid.vertex_id, lid.irp_lower, lid.irp_upper, lid.subpartition)


def taken(eng):
    return eng.kernel_stats().get("columns_small", {"launches": 0})["launches"]


@pytest.fixture(scope="module")
def eng():
    e = Engine(segment_bytes=4096, pool_segments=4096, timing=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def scene(eng):
    """(failed vertices, their subpartition tables, the responses' wire bytes per vertex)."""
    rng = np.random.default_rng(0xC1050005)
    graph = job.dag(5, 8)
    ids = [vid for _, _, vid in graph.all_vertex_ids()]
    failed = sorted(int(x) for x in rng.choice(ids, size=4, replace=False))
    copies, table = {}, {}
    for v in failed:
        subs = [CausalLogID.sub(v, 1000 + v, 7, j) for j in range(N_SUB)]
        table[v] = subs
        copies[v] = []
        for r in range(int(rng.integers(2, 4))):
            held = {}
            for lid in [CausalLogID.main(v)] + subs:
                log = eng.open_log(CausalLogID(lid.vertex_id + 2000 * (r + 1), lid.is_main, lid.irp_lower, lid.irp_upper,
                                               lid.subpartition))
                for ep in range(3):
                    n = int(rng.integers(0, 400))
                    data = synth.config3_epoch(n, rng, ep)[0].tobytes() if lid.is_main else _bb(rng, n)
                    if data:
                        log.appendDeterminant(data, ep)
                held[lid] = log
            copies[v].append(held)
    assert eng.truncate_all(1)
    wires = {}
    for v in failed:
        wires[v] = []
        for r, held in enumerate(copies[v]):
            ev = DeterminantResponseEvent(True, v, int(rng.integers(0, 1 << 62)))
            for lid, log in held.items():
                if v == failed[0] and lid == table[v][1]:
                    continue  # a subpartition log that no responder holds
                if lid.is_main or rng.random() < 0.8:
                    ev.put(lid, log.getDeterminants(int(rng.integers(1, 3))))
            wires[v].append(ev.write())
    return failed, table, wires


def make_jobs(scene):
    failed, table, wires = scene
    return [(v, accumulate(v, [DeterminantResponseEvent.read(w)[0] for w in wires[v]]), table[v]) for v in failed]


def main_spans(scene):
    failed, table, wires = scene
    return [R.replay_spans(R.accumulate(v, wires[v]), v, [_rid(s) for s in table[v]])[0] for v in failed]


def check_sub_fields(rc, raw):
    for k in ("base", "count", "status", "err_off", "err_tag"):
        assert (getattr(rc, k) == getattr(raw, k)).all(), k
    for j in range(len(raw.count)):
        a, c = int(raw.base[j]), int(raw.count[j])
        assert (rc.sizes[a:a + c] == raw.sizes[a:a + c]).all(), j


def check_payloads(cols, spans):
    """payload(k) is the slice of row k's span at its w_var_off / w_var_len."""
    assert cols.var is not None and len(cols.var_pos) == len(cols.w_idx) + 1
    wb = np.asarray(cols.span_base).reshape(-1, 5)[:, 4]
    n_payload = 0
    for s, raw in enumerate(spans):
        for k in range(int(wb[s]), int(wb[s + 1])):
            o, l = int(cols.w_var_off[k]), int(cols.w_var_len[k])
            assert cols.payload(k) == bytes(raw[o:o + l]), (s, k)
            n_payload += l > 0
    return n_payload


def replay_all(rep):
    """Every record of the replayer's span through the call its tag asks for."""
    out = []
    while not rep.isFinished():
        t = rep.next_tag()
        if t == D.ORDER:
            out.append((t, rep.replayNextChannel()))
        elif t == D.TIMESTAMP:
            out.append((t, rep.replayNextTimestamp()))
        elif t == D.RNG:
            out.append((t, rep.replayRandomInt()))
        elif t == D.BUFFER_BUILT:
            out.append((t, rep.replayNextBufferSize()))
        elif t == D.SERIALIZABLE:
            out.append((t, D.SerializableDeterminant(rep.replaySerializableDeterminant())))
        else:
            out.append((t, rep.triggerAsyncEvent(rep.record_count_target())))
    return out


def test_columns_payloads_replayer_and_subpartitions(eng, scene):
    failed, table, wires = scene
    jobs = make_jobs(scene)
    main, res = prepare_replay(eng, jobs)
    raw = prepare_replay_raw(eng, [(v, a, np.ascontiguousarray(_table_array(t))) for v, a, t in jobs])
    before = taken(eng)
    rc = prepare_replay_columns(eng, jobs)
    assert taken(eng) - before == 1  # (a batch of this size takes the one-launch columns)
    assert rc.main.error is None
    assert_columns_equal(rc.main, columnize_host(main))
    spans = main_spans(scene)
    assert check_payloads(rc.main, spans) > 0
    # the replayer of every vertex replays the oracle's determinant sequence
    for i, raw_span in enumerate(spans):
        b = oracle_batch([raw_span])
        dets = b.determinants(0)
        got = replay_all(rc.replayer(i))
        assert len(got) == len(dets) == b.n_rec
        for k, (t, val) in enumerate(got):
            assert t == int(b.tag[k])
            if t in (D.ORDER, D.TIMESTAMP, D.RNG, D.BUFFER_BUILT):
                assert val == int(b.v0[k]), (i, k)
            else:
                assert val == dets[k], (i, k)
    # every subpartition field is prepare_replay's
    check_sub_fields(rc, raw)
    absent = False
    for i in range(len(jobs)):
        want = res[i].subpartitions
        got = rc.vertex(i)
        assert len(got) == len(want) == N_SUB
        for a, b_ in zip(got, want):
            assert a.log_id == b_.log_id and (a.status, a.err_off, a.err_tag) == (b_.status, b_.err_off, b_.err_tag)
            assert (a.buffer_sizes == b_.buffer_sizes).all()
        absent = absent or (i == 0 and len(got[1].buffer_sizes) == 0)
    assert absent


def _table_array(subs):
    from clonos_amd.replay import log_id_array
    return log_id_array(list(subs))


def test_table_as_log_id_array_and_without_payloads(eng, scene):
    jobs = make_jobs(scene)
    a = prepare_replay_columns(eng, jobs)
    b = prepare_replay_columns(eng, [(v, acc, _table_array(t)) for v, acc, t in jobs], payloads=False)
    assert b.main.var is None and b.main.var_pos is None
    assert_columns_equal(a.main, b.main)
    check_sub_fields(a, b)


def test_device_input_equals_host_input(eng, scene):
    from _devbuf import DeviceBuf
    failed, table, wires = scene
    jobs = make_jobs(scene)
    host = prepare_replay_columns(eng, jobs)
    # the same responses in device memory, 16 bytes of margin either side of every entry
    total = sum(16 + ((len(b) + 15) & ~15) + 16 for _, acc, _ in jobs for b in acc.getDeterminants().values())
    buf = DeviceBuf(total + 64, fill=0xEE)
    stage = np.full(total + 64, 0xEE, np.uint8)
    at, djobs = 0, []
    for v, acc, t in jobs:
        ev = DeterminantResponseEvent(True, v)
        for lid, data in acc.getDeterminants().items():
            at += 16
            stage[at:at + len(data)] = np.frombuffer(data, np.uint8)
            ev.put_device(lid, buf.p.value + at, len(data), keep=buf)
            at += ((len(data) + 15) & ~15) + 16
        djobs.append((v, ev, t))
    import ctypes
    assert buf.hip.hipMemcpy(buf.p, ctypes.c_void_p(stage.ctypes.data), ctypes.c_size_t(stage.size), 1) == 0
    try:
        dev = prepare_replay_columns(eng, djobs, device_input=True)
        assert_columns_equal(dev.main, host.main)
        assert (dev.main.var == host.main.var).all() and (dev.main.var_pos == host.main.var_pos).all()
        check_sub_fields(dev, host)
    finally:
        buf.free()


def test_invalid_record_in_one_main_log(eng):
    rng = np.random.default_rng(11)
    good = [synth.random_log(300, rng, allow_serializable=False) for _ in range(3)]
    cut = synth.random_log(120, rng, allow_serializable=False) + b"\x09" + synth.random_log(40, rng, allow_serializable=False)
    mains = [good[0], cut, good[1], good[2]]
    jobs = []
    for v, m in enumerate(mains):
        ev = DeterminantResponseEvent(True, v)
        ev.put(CausalLogID.main(v), m)
        ev.put(CausalLogID.sub(v, 5, 6, 0), _bb(rng, 50 + v))
        jobs.append((v, accumulate(v, [ev]), [CausalLogID.sub(v, 5, 6, 0)]))
    with pytest.raises(ClonosError) as ex:
        prepare_replay(eng, jobs)
    want_batch, err = oracle_batch(mains, allow_errors=True)
    assert err is not None and err[1] == 1
    assert (ex.value.status, ex.value.err_span, ex.value.err_off, ex.value.err_tag) == err
    rc = prepare_replay_columns(eng, jobs)
    e = rc.main.error
    assert e is not None and (e.status, e.err_span, e.err_off, e.err_tag) == err
    assert_columns_equal(rc.main, columnize_host(want_batch))  # every vertex's records up to its first error
    assert rc.main.span(1).tag.size == 120 and rc.main.span(3).tag.size == 300
    assert check_payloads(rc.main, mains) > 0
    # the subpartition outputs are complete
    for v in range(4):
        (sp,) = rc.vertex(v)
        assert sp.status == _lib.CLG_OK and len(sp.buffer_sizes) == 50 + v


def test_absent_main_log_and_no_vertices(eng):
    rng = np.random.default_rng(12)
    m = synth.random_log(200, rng, allow_serializable=True)
    jobs = []
    for v in range(3):
        ev = DeterminantResponseEvent(True, v)
        if v != 1:
            ev.put(CausalLogID.main(v), m)
        ev.put(CausalLogID.sub(v, 5, 6, 0), _bb(rng, 10))
        jobs.append((v, accumulate(v, [ev]), [CausalLogID.sub(v, 5, 6, 0)]))
    rc = prepare_replay_columns(eng, jobs)
    assert_columns_equal(rc.main, columnize_host(oracle_batch([m, b"", m])))
    assert rc.main.span(1).tag.size == 0 and rc.replayer(1).isFinished()
    assert rc.main.span(2).tag.size == rc.main.span(0).tag.size > 0
    check_payloads(rc.main, [m, b"", m])
    none = prepare_replay_columns(eng, [])
    assert none.main.n_rec == 0 and len(none.count) == 0 and len(none.main.var) == 0


def test_a_batch_past_the_small_limit_takes_the_multi_kernel_form(eng):
    src = open(os.path.join(ROOT, "clonos_amd", "csrc", "columns.h")).read()
    import re
    limit = int(re.search(r"constexpr uint32_t kColSmallRecords = (\d+);", src).group(1))
    rng = np.random.default_rng(13)
    n = limit + 1
    m = np.zeros((n, 2), np.uint8)  # Order records: tag 0, one channel byte
    m[:, 1] = rng.integers(0, 128, n)
    m = m.tobytes()
    ev = DeterminantResponseEvent(True, 9)
    ev.put(CausalLogID.main(9), m)
    before = taken(eng)
    rc = prepare_replay_columns(eng, [(9, accumulate(9, [ev]), [])])
    assert taken(eng) == before
    assert rc.main.n_rec == n and len(rc.main.order) == n
    assert (rc.main.order == np.frombuffer(m, np.uint8)[1::2].astype(np.int8)).all()
    st, r, _, _ = O.decode(m[:200])
    assert st == 0 and (r["tag"] == 0).all()  # (the premise: these bytes are Order records)
