"""GPU: packed typed columns encoded and appended on the device (clg_encode_columns_packed,
clg_append_columns_packed): logs -> packed -> columns -> log bytes -> logs.  Every comparison is
exact against the logs' own bytes and encode_columns_host; there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_decode import assert_span_equal

pytestmark = pytest.mark.gpu


def spans():
    from clonos_amd import synth
    rng = np.random.default_rng(0x7AC)
    return [b"", synth.random_log(1500, rng, allow_serializable=True), b"", bytes(synth.config3_epoch(3000, rng)[0]),
            bytes(synth.config2_log(5000, rng)[0]), b""]


SPANS = spans()
N = len(SPANS)


@pytest.fixture
def eng():
    from clonos_amd import Engine
    e = Engine(segment_bytes=256, pool_segments=1 << 12, timing=True)
    yield e
    e.close()


def open_logs(eng, n, base):
    from clonos_amd import CausalLogID
    return [eng.open_log(CausalLogID.main(base + i)) for i in range(n)]


def source_packed(eng, spans=SPANS):
    """Source logs holding `spans`, and their packed columns with payloads."""
    src = open_logs(eng, len(spans), 0)
    for lg, s in zip(src, spans):
        if s:
            lg.appendDeterminant(s, 0)
    packed = eng.decode_logs_columns(src, [0] * len(spans), packed=True, payloads=True)
    from clonos_amd import PackedColumns
    assert isinstance(packed, PackedColumns)
    return src, packed


def states(logs):
    return [(lg.logLength(), lg.getDeterminants(0), lg.state()) for lg in logs]


def test_encode_gives_each_logs_bytes(eng):
    from clonos_amd import encode_columns_host
    src, packed = source_packed(eng)
    got = eng.encode_columns(packed, per_span=True)
    assert got == [lg.getDeterminants(0) for lg in src] == SPANS
    assert got == encode_columns_host(packed.unpack(), per_span=True)
    assert eng.encode_columns(packed) == b"".join(SPANS)
    st = eng.kernel_stats()
    assert st["unpack_columns"]["launches"] >= 2 and st["encode_columns"]["launches"] >= 2


def test_append_rebuilds_the_logs(eng):
    src, packed = source_packed(eng)
    dst = open_logs(eng, N, 500)
    epochs = [0, 0, 2, 1, 0, 0]
    nb = eng.append_columns(dst, epochs, packed)
    assert nb.tolist() == [len(s) for s in SPANS]
    for a, b, e in zip(src, dst, epochs):
        assert b.getDeterminants(e) == a.getDeterminants(0) and b.logLength() == a.logLength()
    hs, hd = [lg.handle for lg in src], [lg.handle for lg in dst]
    ds, dd = eng.digest_logs(hs, [0] * N), eng.digest_logs(hd, epochs)
    assert (ds["hash"] == dd["hash"]).all() and (ds["len"] == dd["len"]).all()
    for _ in range(2):  # a decode of the destinations is the oracle's: the Serializable sidecar was filled
        eng.kernel_stats_reset()  # (the first batch learns that the logs hold Serializable records)
        dec = eng.decode_logs(dst, epochs)
        for s, b in enumerate(SPANS):
            assert_span_equal(dec, s, b)
    ks = eng.kernel_stats()
    assert "decode_fallback" not in ks and "decode_span_fallback" not in ks, sorted(ks)


def test_one_log_twice_applies_its_spans_in_order(eng):
    _, packed = source_packed(eng, [SPANS[1], SPANS[3]])
    (lg,) = open_logs(eng, 1, 500)
    eng.append_columns([lg, lg], [0, 1], packed)
    assert lg.getDeterminants(0) == SPANS[1] + SPANS[3] and lg.getDeterminants(1) == SPANS[3]


def test_an_unknown_handle_fails_its_span_only(eng):
    from clonos_amd import _lib
    _, packed = source_packed(eng, [SPANS[1], SPANS[3], SPANS[4]])
    a, b = open_logs(eng, 2, 500)
    nb, st = eng.append_columns([a, 99999, b], [0, 0, 0], packed, statuses=True)
    assert st.tolist() == [0, _lib.CLG_E_NO_LOG, 0]
    assert nb.tolist() == [len(SPANS[1]), len(SPANS[3]), len(SPANS[4])]
    assert a.getDeterminants(0) == SPANS[1] and b.getDeterminants(0) == SPANS[4]


def test_one_bad_block_fails_the_call_and_changes_no_log(eng):
    from clonos_amd import ClonosError, _lib
    _, packed = source_packed(eng)
    dst = open_logs(eng, N, 500)
    dst[1].appendDeterminant(SPANS[3], 0)
    eng.sync()
    before = states(dst)
    desc = packed.desc.copy()
    b = packed.blk_base[2] + 1
    desc["pos"][b] += 8
    packed.desc = desc
    with pytest.raises(ClonosError) as ei:
        eng.append_columns(dst, [0] * N, packed)
    e = ei.value
    assert (e.status, e.bad_what, e.bad_stream, e.bad_block) == (_lib.CLG_E_INVALID_ARG, _lib.UNPACK_BAD_BLOCK, 2, 1)
    assert states(dst) == before
    with pytest.raises(ClonosError) as ei:
        eng.encode_columns(packed)
    e = ei.value
    assert (e.bad_what, e.bad_stream, e.bad_block, e.enc_bad_what) == (_lib.UNPACK_BAD_BLOCK, 2, 1, 0)
    # the raw call: every status stays CLG_OK
    from clonos_amd.engine import _columns_in
    pk, (rest, keep), bad = packed._struct(), _columns_in(packed), _lib.UnpackBad()
    h, ep = np.array([lg.handle for lg in dst], np.uint32), np.zeros(N, np.int64)
    nb, st = np.full(N, 7, np.uint64), np.full(N, 7, np.int32)
    rc = _lib.lib.clg_append_columns_packed(eng.handle, h.ctypes.data, ep.ctypes.data, N, C.byref(pk), C.byref(rest),
                                            nb.ctypes.data, st.ctypes.data, C.byref(bad))
    assert rc == _lib.CLG_E_INVALID_ARG and (st == _lib.CLG_OK).all() and (bad.what, bad.stream, bad.block) == (2, 2, 1)
    assert states(dst) == before


def test_a_clean_unpack_with_a_tag_of_8_is_the_encodes_error(eng):
    from clonos_amd import ClonosError, _lib, pack_columns_host
    _, packed = source_packed(eng)
    cols = packed.unpack()
    at = cols.n_rec - 3
    cols.tag = cols.tag.copy()
    cols.tag[at] = 8
    bad_tags = pack_columns_host(cols)  # a well-formed packed input whose tag stream holds an 8
    dst = open_logs(eng, N, 500)
    before = states(dst)
    with pytest.raises(ClonosError) as ei:
        eng.encode_columns(bad_tags)
    e = ei.value
    assert (e.status, e.bad_what, e.bad_index) == (_lib.CLG_E_INVALID_ARG, _lib.ENC_BAD_TAG, at)
    with pytest.raises(ClonosError) as ei:
        eng.append_columns(dst, [0] * N, bad_tags)
    e = ei.value
    assert e.status == _lib.CLG_E_INVALID_ARG and e.bad_what == _lib.UNPACK_BAD_NONE and "bad tag, index %d" % at in str(e)
    assert states(dst) == before


def test_rest_must_leave_the_narrow_columns_out_and_agree_with_n_val(eng):
    from clonos_amd import _lib
    from clonos_amd.engine import _columns_in
    _, packed = source_packed(eng)
    pk = packed._struct()

    def call(rest):
        enc, bad = _lib.Encoded(), _lib.UnpackBad(9, 9, 9)
        st = _lib.lib.clg_encode_columns_packed(eng.handle, C.byref(pk), C.byref(rest), C.byref(enc), C.byref(bad))
        return st, bad.what, bad.stream, bad.block, enc.bad_what

    rest, keep = _columns_in(packed)
    assert call(rest)[0] == _lib.CLG_OK
    tags = np.zeros(packed.n_rec, np.uint8)
    rest.tag = tags.ctypes.data
    assert call(rest) == (_lib.CLG_E_INVALID_ARG, 0, 0, 2 ** 64 - 1, 0)
    rest.tag = None
    rest.n_class[2] += 1
    assert call(rest) == (_lib.CLG_E_INVALID_ARG, _lib.UNPACK_BAD_LAYOUT, 3, 0, 0)
    rest.n_rec -= 1
    assert call(rest) == (_lib.CLG_E_INVALID_ARG, _lib.UNPACK_BAD_LAYOUT, 0, 0, 0)


def test_the_packed_input_in_device_memory_gives_the_same_logs(eng):
    from clonos_amd import _lib
    from clonos_amd.engine import _columns_in
    from test_gpu_unpack_columns import PackedIn
    src, packed = source_packed(eng)
    dst = open_logs(eng, N, 500)
    pin = PackedIn(packed.desc, packed.bits, packed._struct(), "device")
    rest, keep = _columns_in(packed)
    bad = _lib.UnpackBad()
    h, ep = np.array([lg.handle for lg in dst], np.uint32), np.zeros(N, np.int64)
    nb, st = np.zeros(N, np.uint64), np.zeros(N, np.int32)
    try:
        rc = _lib.lib.clg_append_columns_packed(eng.handle, h.ctypes.data, ep.ctypes.data, N, C.byref(pin.p), C.byref(rest),
                                                nb.ctypes.data, st.ctypes.data, C.byref(bad))
        assert rc == _lib.CLG_OK and (st == 0).all() and nb.tolist() == [len(s) for s in SPANS] and bad.what == 0
        for a, b in zip(src, dst):
            assert b.getDeterminants(0) == a.getDeterminants(0)
    finally:
        pin.free()
