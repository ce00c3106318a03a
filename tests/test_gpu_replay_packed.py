"""GPU: replay preparation that delivers packed typed columns (clg_replay_prepare_columns_packed,
replay.prepare_replay_columns(packed=True[, pack_wide=True])).

Two engines, one opened under CLONOS_PACK_SMALL=0.  Every scene runs on both, with the narrow
columns packed and with the wide rows packed as well, against prepare_replay_columns() on the same
jobs: main.unpack() is the plain columns array for array, var is equal, desc / bits are
pack_columns_host / pack_wide_host of those columns byte for byte, the six subpartition arrays are
equal, and a ColumnReplayer driven to isFinished() over each gives the same sequence."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from _columns_util import assert_columns_equal
from _pack_util import assert_same_packed
from _wpack_util import assert_same_wide
from clonos_amd import CausalLogID, Engine, _lib, pack_columns_host, pack_wide_host, synth
from clonos_amd import determinants as D
from clonos_amd.replay import DeterminantResponseEvent, accumulate, log_id_array, prepare_replay_columns

pytestmark = pytest.mark.gpu

BOTH = ("small", "multi")


@pytest.fixture(scope="module")
def engines():
    small = Engine(segment_bytes=4096, pool_segments=4096, timing=True)
    old = os.environ.get("CLONOS_PACK_SMALL")
    os.environ["CLONOS_PACK_SMALL"] = "0"
    try:
        multi = Engine(segment_bytes=4096, pool_segments=4096, timing=True)
    finally:
        if old is None:
            del os.environ["CLONOS_PACK_SMALL"]
        else:
            os.environ["CLONOS_PACK_SMALL"] = old
    yield {"small": small, "multi": multi}
    small.close()
    multi.close()


def taken(eng):
    return eng.kernel_stats().get("pack_small", {"launches": 0})["launches"]


def _bb(rng, n):
    return b"".join(b"\x07" + struct.pack(">i", int(x)) for x in rng.integers(-(1 << 31), 1 << 31, n))


def jobs_of(mains, rng, subs=1):
    """A job per main log (None: the response holds no main log), `subs` subpartition logs each."""
    jobs = []
    for v, m in enumerate(mains):
        ev = DeterminantResponseEvent(True, v)
        if m is not None:
            ev.put(CausalLogID.main(v), m)
        table = [CausalLogID.sub(v, 5, 6, j) for j in range(subs)]
        for j, lid in enumerate(table):
            ev.put(lid, _bb(rng, 10 + v + j))
        jobs.append((v, accumulate(v, [ev]), table))
    return jobs


def replay_all(rep):
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


def error_of(cols):
    e = cols.error
    return None if e is None else (e.status, e.err_span, e.err_off, e.err_tag)


def compare(engines, jobs, small=True, device_jobs=None, replay=True):
    """Both packed forms on both engines against the plain columns call; returns the plain result."""
    plain = None
    for which in BOTH:
        eng = engines[which]
        plain = prepare_replay_columns(eng, jobs)
        want_seq = [replay_all(plain.replayer(i)) for i in range(len(jobs))] if replay else None
        for pack_wide in (False, True):
            before = taken(eng)
            if device_jobs is not None:
                got = prepare_replay_columns(eng, device_jobs, device_input=True, packed=True, pack_wide=pack_wide)
            else:
                got = prepare_replay_columns(eng, jobs, packed=True, pack_wide=pack_wide)
            assert taken(eng) - before == (1 if which == "small" and small else 0), (which, pack_wide)
            assert error_of(got.main) == error_of(plain.main)
            assert (got.main.wide_packed is not None) == pack_wide
            assert_same_packed(got.main, pack_columns_host(plain.main))
            if pack_wide:
                assert_same_wide(got.main.wide_packed, pack_wide_host(plain.main))
            assert got.main.var.tobytes() == plain.main.var.tobytes()
            assert (np.asarray(got.main.span_base) == np.asarray(plain.main.span_base)).all()
            assert_columns_equal(got.main.unpack(), plain.main)
            for k in ("sizes", "base", "count", "status", "err_off", "err_tag"):
                a, b = getattr(got, k), getattr(plain, k)
                n = int(plain.base[-1] + plain.count[-1]) if k == "sizes" and len(plain.count) else len(b)
                assert (a[:n] == b[:n]).all(), k
            if replay:
                for i in range(len(jobs)):
                    assert replay_all(got.replayer(i)) == want_seq[i], (which, pack_wide, i)
    return plain


def config1_jobs():
    """Config 1's epoch: every vertex of the job failed, its subpartition logs in its table."""
    graph, logs = synth.config1_job(np.random.default_rng(0xC1))
    by_vertex = {}
    for lid, data in logs.items():
        by_vertex.setdefault(lid.vertex_id, []).append((lid, bytes(data)))
    jobs = []
    for v, held in sorted(by_vertex.items()):
        ev = DeterminantResponseEvent(True, v)
        for lid, data in held:
            ev.put(lid, data)
        jobs.append((v, accumulate(v, [ev]), [lid for lid, _ in held if not lid.is_main]))
    return jobs


def test_config1_epoch_takes_the_one_launch_forms(engines):
    jobs = config1_jobs()
    plain = compare(engines, jobs)
    assert plain.main.n_rec > 1000 and len(plain.main.w_idx) > 100 and len(plain.count) > 0


def test_no_vertices(engines):
    for which in BOTH:
        for pack_wide in (False, True):
            none = prepare_replay_columns(engines[which], [], packed=True, pack_wide=pack_wide)
            assert none.main.n_rec == 0 and len(none.count) == 0 and len(none.main.var) == 0
            assert none.main.n_val == [0] * 5 and len(none.main.desc) == 0


def test_absent_main_log_a_vertex_without_wide_rows_and_empty_logs(engines):
    rng = np.random.default_rng(12)
    wide = synth.random_log(300, rng, allow_serializable=True)
    narrow = np.zeros((500, 2), np.uint8)  # Order records only: no wide row
    narrow[:, 1] = rng.integers(0, 100, 500)
    plain = compare(engines, jobs_of([wide, None, narrow.tobytes(), wide], rng, subs=2))
    assert plain.main.span(1).tag.size == 0 and plain.main.span(2).tag.size == 500
    plain = compare(engines, jobs_of([narrow.tobytes()], rng))
    assert len(plain.main.w_idx) == 0
    plain = compare(engines, jobs_of([b"", None, b""], rng))
    assert plain.main.n_rec == 0


def test_a_main_log_cut_inside_a_record(engines):
    """The decode's status, that vertex's records up to the error, the subpartition outputs complete."""
    rng = np.random.default_rng(11)
    good = [synth.random_log(300, rng, allow_serializable=False) for _ in range(3)]
    whole = synth.random_log(120, rng, allow_serializable=False) + b"\x01" + bytes(8)  # a Timestamp record last
    jobs = jobs_of([good[0], whole[:-3], good[1], good[2]], rng)
    plain = compare(engines, jobs)
    e = plain.main.error
    assert e is not None and e.status != _lib.CLG_OK and e.err_span == 1
    assert plain.main.span(1).tag.size == 120 and plain.main.span(3).tag.size == 300
    for which in BOTH:
        got = prepare_replay_columns(engines[which], jobs, packed=True, pack_wide=True)
        for v in range(4):
            (sp,) = got.vertex(v)
            assert sp.status == _lib.CLG_OK and len(sp.buffer_sizes) == 10 + v


def test_sizes_cap_one_short_comes_first(engines):
    rng = np.random.default_rng(5)
    jobs = jobs_of([synth.random_log(200, rng, allow_serializable=True)] * 2, rng, subs=2)
    n = len(jobs)
    vs = (_lib.ReplayVertex * n)()
    tables = [log_id_array(list(t)) for _, _, t in jobs]
    for i, (vid, acc, _) in enumerate(jobs):
        vs[i] = _lib.ReplayVertex(C.pointer(acc._c), C.cast(tables[i].ctypes.data, C.POINTER(_lib.CausalLogIdC)), len(tables[i]),
                                  vid, 0)
    n_sub = sum(len(t) for t in tables)
    need = sum(10 + v + j for v in range(2) for j in range(2))
    for which in BOTH:
        for cap, want in ((need, _lib.CLG_OK), (need - 1, _lib.CLG_E_CAPACITY)):
            sizes = np.full(need, -7, np.int32)
            sbase, cnt, soff = np.zeros(n_sub + 1, np.uint64), np.zeros(n_sub, np.uint64), np.zeros(n_sub, np.int64)
            sst, stag = np.zeros(n_sub, np.int32), np.zeros(n_sub, np.int32)
            c, pk, wpk = _lib.Columns(), _lib.Packed(), _lib.PackedWideC()
            out = _lib.ReplayPackedOut(C.pointer(c), None, C.pointer(pk), C.pointer(wpk), sizes.ctypes.data, cap,
                                       sbase.ctypes.data, cnt.ctypes.data, sst.ctypes.data, soff.ctypes.data, stag.ctypes.data)
            before = taken(engines[which])
            assert _lib.lib.clg_replay_prepare_columns_packed(engines[which].handle, vs, n, C.byref(out)) == want, (which, cap)
            assert int(sbase[-1]) == need
            if want == _lib.CLG_OK:  # the sizes-only call of both packed forms
                assert c.n_rec == 400 and pk.n_val[0] == 400 and pk.n_bits > 0 and wpk.n_bits > 0 and int(cnt.sum()) == need
                assert taken(engines[which]) - before == (1 if which == "small" else 0)
            else:  # nothing ran: no main log was decoded, no size written
                assert c.n_rec == 0 and pk.n_bits == 0 and list(pk.n_val) == [0] * 5 and (sizes == -7).all()
                assert taken(engines[which]) == before


def test_device_input(engines):
    from _devbuf import DeviceBuf
    rng = np.random.default_rng(21)
    jobs = jobs_of([synth.random_log(400, rng, allow_serializable=True), bytes(synth.config3_epoch(300, rng)[0])], rng)
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
    assert buf.hip.hipMemcpy(buf.p, C.c_void_p(stage.ctypes.data), C.c_size_t(stage.size), 1) == 0
    try:
        compare(engines, jobs, device_jobs=djobs)
    finally:
        buf.free()


def test_three_large_vertices_take_the_multi_kernel_forms(engines):
    """About 14 000 records each: past kColSmallRecords and kPackSmallBlocks on both engines."""
    rng = np.random.default_rng(13)
    mains = []
    for _ in range(3):
        m = np.zeros((13000, 2), np.uint8)  # Order records, and wide records behind them
        m[:, 1] = rng.integers(0, 128, 13000)
        mains.append(m.tobytes() + synth.random_log(1000, rng, allow_serializable=True))
    plain = compare(engines, jobs_of(mains, rng), small=False, replay=False)
    assert plain.main.n_rec == 3 * 14000 and len(plain.main.w_idx) > 0
