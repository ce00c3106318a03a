"""GPU: the subpartition recovery buffers of replay preparation (k_bufsizes and
k_bufsizes_classify, replay.hip) at their edges, bit-exact against the reference loop
(oracle/response_ref.buffer_sizes: decodeNext until the buffer ends, anything but a BufferBuilt
is an error): the sizes before the end or the error, status, err_off and err_tag.

What is swept (the scenes are in _bufsizes_scenes.py; test_bufsizes_edges_scene.py checks their
coverage without a GPU):
  1. values: every buffer starts with the ends of the int32 range, -1, 0, 1, 0x01020304, the sign
     bit alone and sizes with a single byte set; the rest is drawn from the whole range.
  2. lengths: 0 bytes, 1..4 bytes (a partial record alone), 1, 2, 255, 256, 257 and 512 records,
     256 records and a tail of 1..4 bytes, 513 records and 3 bytes; the tails as a cut BufferBuilt
     and as an Order -- each span alone, and all as the subpartitions of one call (host input and
     device input), where the bases into buffer_sizes are no multiple of anything.
  3. the first bad record: a corrupt tag, an Order and a TimerTrigger with a bad enum before
     record 0, 255, 256, 257 and the last; corrupt tags on the 5-byte grid at k1 < k2 in two
     chunks, in one chunk and in every chunk; bad spans between clean ones.
  4. 63, 64 and 65 subpartitions over several partitions, the last one bad.
  5. sizes_cap exactly sizes_base[ns], and one less (CLG_E_CAPACITY).
"""
import ctypes as C

import numpy as np
import pytest

import _bufsizes_scenes as S
from _devbuf import DeviceBuf
from clonos_amd import CausalLogID, Engine, _lib
from clonos_amd._lib import lib
from clonos_amd.replay import DeterminantResponseEvent, ReplayArrays, log_id_array, prepare_replay_raw

pytestmark = pytest.mark.gpu

VERTEX = 3
MAIN = b"\x00\x01" + b"\x02\x00\x00\x00\x05" + b"\x01" + bytes(8)  # an Order, an RNG, a Timestamp


@pytest.fixture(scope="module")
def eng():
    e = Engine(segment_bytes=16384, pool_segments=64)
    yield e
    e.close()


def table_of(ns):
    return [CausalLogID.sub(VERTEX, *S.sub_id(j)) for j in range(ns)]


def response(spans, dbuf=None):
    """The accumulated response: a small main log and span j under subpartition id j (None: the
    table names it, the response does not hold it).  dbuf: every entry's bytes in device memory,
    back to back."""
    ev = DeterminantResponseEvent(True, VERTEX, capacity=len(spans) + 1)
    at = 0
    for lid, b in [(CausalLogID.main(VERTEX), MAIN)] + list(zip(table_of(len(spans)), spans)):
        if b is None:
            continue
        if dbuf is None:
            ev.put(lid, b)
        else:
            ev.put_device(lid, dbuf.at(at), len(b), keep=dbuf)
            at += len(b)
    return ev


def run(eng, spans, device=False):
    """prepare_replay_raw over one vertex whose subpartitions are `spans`."""
    dbuf = None
    if device:
        data = np.frombuffer(b"".join([MAIN] + [b for b in spans if b is not None]), np.uint8)
        dbuf = DeviceBuf(data.size + 1)
        assert dbuf.hip.hipMemcpy(dbuf.p, C.c_void_p(data.ctypes.data), C.c_size_t(data.size), 1) == 0
        assert dbuf.hip.hipDeviceSynchronize() == 0
    try:
        acc = response(spans, dbuf)
        res = prepare_replay_raw(eng, [(VERTEX, acc, log_id_array(table_of(len(spans))))], device_input=device)
        assert res.main.tag.tolist() == [0, 2, 1] and res.main.v0.tolist() == [1, 5, 0]
        return res
    finally:
        if dbuf is not None:
            dbuf.free()


def check(res, spans, names):
    """Every span's sizes, status, err_off and err_tag are the reference's; the bases are the
    whole records before each span."""
    at = 0
    for j, (b, name) in enumerate(zip(spans, names)):
        sizes, st, off, tag = S.expected(b or b"")
        assert int(res.base[j]) == at, name
        got = res.sizes[at:at + int(res.count[j])]
        assert (int(res.status[j]), int(res.err_off[j]), int(res.err_tag[j])) == (st, off, tag), name
        assert int(res.count[j]) == len(sizes), name
        np.testing.assert_array_equal(got, np.array(sizes, np.int64).astype(np.int32), err_msg=name)
        at += len(b or b"") // 5


def test_each_length_alone(eng):
    for name, b in S.length_spans():
        check(run(eng, [b]), [b], [name])


@pytest.mark.parametrize("device", [False, True])
def test_all_lengths_in_one_call(eng, device):
    names, spans = zip(*S.length_spans())
    check(run(eng, list(spans), device), spans, names)


def test_absent_between_lengths(eng):
    """A subpartition the response does not hold is an empty buffer; its neighbours keep theirs."""
    names, spans = zip(*S.length_spans()[:6])
    spans = list(spans[:3]) + [None] + list(spans[3:])
    check(run(eng, spans), spans, list(names[:3]) + ["absent"] + list(names[3:]))


def test_first_bad_record_alone(eng):
    for name, b in S.bad_spans():
        check(run(eng, [b]), [b], [name])


def test_bad_spans_between_clean_ones(eng):
    names, spans = [], []
    for j, (name, b) in enumerate(S.bad_spans()):
        names += [name, f"clean_{j}"]
        spans += [b, S.good(S.CHUNK + j, 400 + j)]
    res = run(eng, spans)
    check(res, spans, names)
    assert (res.status[1::2] == 0).all() and (res.status[0::2] != 0).all()


@pytest.mark.parametrize("ns", S.SPAN_COUNTS)
def test_many_spans(eng, ns):
    spans = S.many_spans(ns)
    res = run(eng, spans)
    check(res, spans, [f"span_{j}" for j in range(ns)])
    assert (res.status[:-1] == 0).all() and res.status[-1] == _lib.CLG_E_NOT_BUFFER_BUILT


def test_sizes_capacity(eng):
    """sizes_cap == sizes_base[ns] succeeds, one less is CLG_E_CAPACITY (with sizes_base filled)."""
    names, spans = zip(*S.length_spans())
    n_sizes = sum(len(b) // 5 for b in spans)
    acc = response(spans)
    table = log_id_array(table_of(len(spans)))
    ids = C.cast(table.ctypes.data, C.POINTER(_lib.CausalLogIdC))
    vs = (_lib.ReplayVertex * 1)(_lib.ReplayVertex(C.pointer(acc._c), ids, len(table), VERTEX, 0))
    ns = len(spans)
    for cap, want in ((n_sizes, _lib.CLG_OK), (n_sizes - 1, _lib.CLG_E_CAPACITY)):
        d, arrs, _ = eng._pooled_outputs(len(MAIN), len(MAIN))
        base = np.zeros(2, np.uint64)
        sizes = np.full(n_sizes + 8, 0x5A5A5A5A, np.int32)
        sbase, cnt = np.zeros(ns + 1, np.uint64), np.zeros(ns, np.uint64)
        sst, soff, stag = np.zeros(ns, np.int32), np.zeros(ns, np.int64), np.zeros(ns, np.int32)
        out = _lib.ReplayOut(C.pointer(d), base.ctypes.data, sizes.ctypes.data, cap, sbase.ctypes.data, cnt.ctypes.data,
                             sst.ctypes.data, soff.ctypes.data, stag.ctypes.data)
        try:
            st = lib.clg_replay_prepare(eng.handle, vs, 1, C.byref(out))
        finally:
            eng._slot_done(arrs)
        assert st == want and int(sbase[ns]) == n_sizes
        assert (sizes[n_sizes:] == 0x5A5A5A5A).all()
        if st == _lib.CLG_OK:
            check(ReplayArrays(None, sizes, sbase, cnt, sst, soff, stag), spans, names)
        else:
            assert (sizes == 0x5A5A5A5A).all()
