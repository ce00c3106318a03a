"""GPU: clg_encode_columns_packed_wide / clg_append_columns_packed_wide, the device route of the
wide rows (Engine.encode_columns / append_columns with wide="device").  Every comparison is exact,
against clg_encode_columns_packed_wide_host (which tests/test_wunpack_host.py holds to the plain
host encode): bytes, statuses and (what, stream, block) alike.  The scene is
tests/test_gpu_decode_packed_wide.py's; the cross rule and the rejections run over
tests/test_wunpack_host.py's larger one, whose wide rows fill more than two tiles."""
import ctypes as C

import numpy as np
import pytest

from _wunpack_util import FILL, WIDE_STREAM, host_rows_untouched, raw_host, swap_two_wide_tags, with_tags
from test_gpu_decode_packed_wide import make_spans, open_logs
from test_gpu_unpack_columns import PackedIn
from test_gpu_unpack_wide import WideIn
from test_wunpack_host import SPANS as BIG_SPANS, fresh, scene as big_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from clonos_amd import Engine
    with Engine(segment_bytes=256, pool_segments=1 << 15, timing=True) as e:
        yield e


@pytest.fixture(scope="module")
def scene(eng):
    spans = make_spans()
    logs = open_logs(eng, spans, 100)
    return spans, logs


def decoded(eng, logs):
    return eng.decode_logs_columns(logs, [0] * len(logs), packed=True, pack_wide=True, payloads=True)


def fresh_logs(eng, n, first_vertex):
    from clonos_amd import CausalLogID
    return [eng.open_log(CausalLogID.main(first_vertex + i)) for i in range(n)]


def handles(logs):
    return np.array([l.handle for l in logs], np.uint32)


def test_encode_gives_the_logs_bytes_and_the_host_twins(eng, scene):
    from clonos_amd import encode_columns_packed_wide_host
    spans, logs = scene
    got = decoded(eng, logs)
    assert got.wide_packed.n_wide > 0 and got.var.size > 0
    eng.kernel_stats_reset()
    whole = eng.encode_columns(got, wide="device")
    assert eng.kernel_stats()["unpack_wide"]["launches"] >= 2
    assert whole == b"".join(spans) == encode_columns_packed_wide_host(got)
    per = eng.encode_columns(got, per_span=True, wide="device")
    assert per == [bytes(s) for s in spans] == encode_columns_packed_wide_host(got, per_span=True)
    assert host_rows_untouched(got)  # the host unpack never ran


def test_the_larger_scene_across_tiles(eng):
    cols, got = big_scene()
    assert got.wide_packed.n_wide > 2048
    assert eng.encode_columns(got, wide="device") == b"".join(BIG_SPANS)
    assert host_rows_untouched(got)


def test_append_into_fresh_logs_gives_the_sources_bytes_and_digests(eng, scene):
    spans, logs = scene
    got = decoded(eng, logs)
    dst = fresh_logs(eng, len(spans), 300)
    nb = eng.append_columns(dst, [0] * len(dst), got, wide="device")
    assert list(nb) == [len(s) for s in spans]
    for s, lg in zip(spans, dst):
        assert lg.getDeterminants(0) == bytes(s)
    ep = np.zeros(len(dst), np.int64)
    a, b = eng.digest_logs(handles(dst), ep), eng.digest_logs(handles(logs), ep)
    assert (a["hash"] == b["hash"]).all() and (a["len"] == b["len"]).all()
    assert host_rows_untouched(got)


def test_one_log_twice_and_an_unknown_handle(eng, scene):
    from clonos_amd import _lib
    spans, logs = scene
    got = decoded(eng, logs)
    dst = fresh_logs(eng, 2, 400)
    # spans 1 and 3 into one log, in order; span 4 to a handle that does not exist
    h = [dst[1].handle] * len(spans)
    h[1] = h[3] = dst[0].handle
    h[4] = 99999
    nb, st = eng.append_columns(h, [0] * len(spans), got, statuses=True, wide="device")
    assert list(nb) == [len(s) for s in spans]
    assert [int(x) for x in st] == [_lib.CLG_E_NO_LOG if s == 4 else _lib.CLG_OK for s in range(len(spans))]
    assert dst[0].getDeterminants(0) == bytes(spans[1]) + bytes(spans[3])
    assert dst[1].getDeterminants(0) == b"".join(bytes(s) for i, s in enumerate(spans) if i not in (1, 3, 4))


def raw_append(eng, logs, narrow, wide, rest):
    from clonos_amd import _lib
    ns = max(int(rest.n_spans), 1)
    h, ep = handles(logs), np.zeros(len(logs), np.int64)
    nb, st, bad = np.zeros(ns, np.uint64), np.full(ns, 77, np.int32), _lib.UnpackBad()
    rc = _lib.lib.clg_append_columns_packed_wide(eng._h, h.ctypes.data, ep.ctypes.data, ns, C.byref(narrow), C.byref(wide),
                                                 C.byref(rest), nb.ctypes.data, st.ctypes.data, C.byref(bad))
    return rc, (int(bad.what), int(bad.stream), int(bad.block)), nb, st


def test_packed_inputs_in_device_memory_give_the_same_logs(eng, scene):
    from clonos_amd import _lib
    from clonos_amd.engine import _rest_in
    spans, logs = scene
    got = decoded(eng, logs)
    pin = PackedIn(got.desc, got.bits, got._struct(), "device")
    win = WideIn(got.wide_packed, "device", exact=True)
    rest, keep = _rest_in(got)
    dst = fresh_logs(eng, len(spans), 500)
    try:
        rc, bad, nb, st = raw_append(eng, dst, pin.p, win.p, rest)
        assert rc == _lib.CLG_OK and bad == (0, 0, 2 ** 64 - 1) and not st.any()
        assert list(nb) == [len(s) for s in spans]
        for s, lg in zip(spans, dst):
            assert lg.getDeterminants(0) == bytes(s)
    finally:
        pin.free()
        win.free()


def states(logs):
    return [l.state() for l in logs]


def rejected_like_the_host(eng, g, dst, rest_poke=None):
    """g fails clg_append_columns_packed_wide as the host twin fails: the same triple, every log's
    state unchanged, every status CLG_OK; and the encode writes nothing."""
    from clonos_amd import _lib
    from clonos_amd.engine import _rest_in
    hst, hbad, henc, hbuf = raw_host(g, rest_poke=rest_poke)
    assert hst == _lib.CLG_E_INVALID_ARG and henc.bad_what == 0
    rest, keep = _rest_in(g)
    if rest_poke:
        rest_poke(rest)
    before = states(dst)
    rc, bad, nb, st = raw_append(eng, dst, g._struct(), g.wide_packed._struct(), rest)
    assert rc == hst and bad == hbad, (rc, bad, hbad)
    assert states(dst) == before and not st.any()
    buf = np.full(1 << 20, FILL, np.uint8)
    enc, ebad = _lib.Encoded(), _lib.UnpackBad()
    enc.bytes, enc.cap, enc.out_kind = buf.ctypes.data, buf.size, _lib.CLG_MEM_HOST
    rc = _lib.lib.clg_encode_columns_packed_wide(eng._h, C.byref(g._struct()), C.byref(g.wide_packed._struct()), C.byref(rest),
                                                 C.byref(enc), C.byref(ebad))
    assert rc == hst and (int(ebad.what), int(ebad.stream), int(ebad.block)) == hbad
    assert enc.bad_what == 0 and (buf == FILL).all()
    return hbad


@pytest.fixture(scope="module")
def big_dst(eng):
    """Destination logs for the larger scene, with something in them already."""
    dst = fresh_logs(eng, len(BIG_SPANS), 600)
    for lg in dst[::2]:
        lg.appendDeterminant(bytes(BIG_SPANS[5]), 0)
    return dst


def test_one_bad_block_in_narrow(eng, big_dst):
    from clonos_amd import _lib
    g = fresh()
    g.desc["width"][g.blk_base[_lib.PACK_TIMESTAMP] + 1] = 70
    g.wide_packed.desc["width"][1] = 65  # (a wide finding as well: the narrow one is reported)
    assert rejected_like_the_host(eng, g, big_dst) == (_lib.UNPACK_BAD_BLOCK, _lib.PACK_TIMESTAMP, 1)


def test_one_bad_block_in_wide(eng, big_dst):
    from clonos_amd import _lib
    g = fresh()
    w = g.wide_packed
    w.desc["pos"][w.blk_base[2 + 6 + 1]] += 8
    assert rejected_like_the_host(eng, g, big_dst) == (_lib.UNPACK_BAD_BLOCK, WIDE_STREAM + 2 + 6 + 1, 0)
    g = fresh()
    g.wide_packed.desc["width"][g.wide_packed.blk_base[1] + 2] = 65
    assert rejected_like_the_host(eng, g, big_dst) == (_lib.UNPACK_BAD_BLOCK, WIDE_STREAM + 1, 2)


def test_a_histogram_mismatch_and_a_value(eng, big_dst):
    from clonos_amd import _lib
    g = fresh()
    w = g.wide_packed
    at = int(w.desc["pos"][0])
    w.bits[at] = (int(w.bits[at]) & 0xFC) | ((int(w.bits[at]) + 1) & 3)
    assert rejected_like_the_host(eng, g, big_dst) == (_lib.UNPACK_BAD_VALUE, WIDE_STREAM, 0)
    g = fresh()
    w = g.wide_packed
    w.desc["first"][w.blk_base[2 + 12 + 2]] = -1
    assert rejected_like_the_host(eng, g, big_dst) == (_lib.UNPACK_BAD_VALUE, WIDE_STREAM + 2 + 12 + 2, 0)


def test_the_cross_rule_in_the_first_and_the_last_tile(eng, big_dst):
    from clonos_amd import ClonosError, _lib, pack_columns_host
    cols, good = big_scene()
    n = good.wide_packed.n_wide
    tag_last, k_last = swap_two_wide_tags(cols, (n - 1) // 1024 * 1024 + 3, n)
    tag_both, k_first = swap_two_wide_tags(with_tags(cols, tag_last), 40, 1024)
    for tag, row in ((tag_last, k_last), (tag_both, k_first)):
        g = fresh()
        pk = pack_columns_host(with_tags(cols, tag))
        g.desc, g.bits, g.n_val, g.blk_base = pk.desc, pk.bits, pk.n_val, pk.blk_base
        assert rejected_like_the_host(eng, g, big_dst) == (_lib.UNPACK_BAD_VALUE, WIDE_STREAM + _lib.WPACK_IDX, row // 1024)
        with pytest.raises(ClonosError) as ei:
            eng.encode_columns(g, wide="device")
        assert (ei.value.bad_what, ei.value.bad_stream, ei.value.bad_block) == (3, 33, row // 1024)
        with pytest.raises(ClonosError) as ei:
            eng.append_columns(big_dst, [0] * len(big_dst), g, wide="device")
        assert (ei.value.bad_what, ei.value.bad_stream, ei.value.bad_block) == (3, 33, row // 1024)
    assert k_last // 1024 == (n - 1) // 1024 >= 2 and k_first // 1024 == 0


def test_rest_with_a_wide_pointer_or_pos_is_rejected(eng, big_dst):
    from clonos_amd import _lib
    from clonos_amd.engine import _rest_in
    cols, got = big_scene()
    spare = np.zeros(1 << 16, np.uint64)
    before = states(big_dst)
    for name in ("w_rc", "pos", "w_idx", "tag"):
        rest, keep = _rest_in(got)
        setattr(rest, name, spare.ctypes.data)
        rc, bad, nb, st = raw_append(eng, big_dst, got._struct(), got.wide_packed._struct(), rest)
        assert rc == _lib.CLG_E_INVALID_ARG and bad[0] == _lib.UNPACK_BAD_NONE and not st.any(), name
    assert states(big_dst) == before


def test_a_mismatch_of_n_class_4_is_a_layout_finding(eng, big_dst):
    from clonos_amd import _lib

    def one_row_fewer(rest):
        rest.n_class[4] -= 1
    assert rejected_like_the_host(eng, fresh(), big_dst, one_row_fewer) == (_lib.UNPACK_BAD_LAYOUT, WIDE_STREAM, 0)
    g = fresh()
    g.wide_packed.n_val[2 + 3] -= 1
    assert rejected_like_the_host(eng, g, big_dst) == (_lib.UNPACK_BAD_LAYOUT, WIDE_STREAM + 2 + 3, 0)


def test_a_tag_of_8_after_a_clean_unpack_is_the_encodes_finding(eng):
    from clonos_amd import ClonosError, _lib, pack_columns_host
    cols, good = big_scene()
    at = int(np.flatnonzero(cols.tag == 2)[7])
    tag = np.array(cols.tag)
    tag[at] = 8
    g = fresh()
    pk = pack_columns_host(with_tags(cols, tag))
    g.desc, g.bits, g.n_val, g.blk_base = pk.desc, pk.bits, pk.n_val, pk.blk_base
    with pytest.raises(ClonosError) as ei:
        eng.encode_columns(g, wide="device")
    assert ei.value.status == _lib.CLG_E_INVALID_ARG and ei.value.bad_what == _lib.ENC_BAD_TAG and ei.value.bad_index == at
    hst, hbad, henc, hbuf = raw_host(g)
    assert (hst, henc.bad_what, henc.bad_index) == (_lib.CLG_E_INVALID_ARG, _lib.ENC_BAD_TAG, at)


def test_no_wide_rows_launch_nothing_of_the_wide_unpack(eng):
    from clonos_amd import synth
    spans = [bytes(synth.config2_log(1200, np.random.default_rng(2))[0]), b""]
    logs = open_logs(eng, spans, 700)
    got = decoded(eng, logs)
    assert got.wide_packed.n_wide == 0
    eng.kernel_stats_reset()
    assert eng.encode_columns(got, wide="device") == b"".join(spans)
    assert eng.kernel_stats().get("unpack_wide", {}).get("launches", 0) == 0
    dst = fresh_logs(eng, 2, 720)
    eng.append_columns(dst, [0, 0], got, wide="device")
    assert dst[0].getDeterminants(0) == spans[0] and dst[1].getDeterminants(0) == b""
