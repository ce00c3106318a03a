"""GPU: clg_decode_logs_columns_packed_wide / clg_decode_host_columns_packed_wide.  The narrow part
is the existing packed call's clg_packed, byte for byte; the wide part is pack_wide_host of the plain
call's columns, byte for byte; the payload bytes are the plain call's and come without pos, which
the prefix sum of w_var_len gives back.  Span_base, the error fields and the status pass through as
the existing packed call delivers them."""
import ctypes as C

import numpy as np
import pytest

from _columns_util import assert_columns_equal, oracle_batch
from _pack_util import assert_same_packed
from _wpack_util import assert_same_wide

pytestmark = pytest.mark.gpu

FILL = 0xA5
WIDE = ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0")


def make_spans():
    """Empty spans first, in the middle and last; config 3, config 2 and random logs (wide rows of
    every kind, with payloads); spans that cross 256-byte segments and blocks of 1024 values."""
    from clonos_amd import synth
    rng = np.random.default_rng(0xDEC0DE)
    return [b"", bytes(synth.config3_epoch(1500, rng)[0]), b"", synth.random_log(700, rng, allow_serializable=True),
            bytes(synth.config2_log(3000, rng)[0]), synth.random_log(5, rng, allow_serializable=False), b""]


@pytest.fixture(scope="module")
def eng():
    from clonos_amd import Engine
    with Engine(segment_bytes=256, pool_segments=1 << 14, timing=True) as e:
        yield e


def open_logs(eng, spans, first_vertex):
    from clonos_amd import CausalLogID
    logs = []
    for i, b in enumerate(spans):
        lg = eng.open_log(CausalLogID.main(first_vertex + i))
        if len(b):
            lg.appendDeterminant(bytes(b), 0)
        logs.append(lg)
    return logs


@pytest.fixture(scope="module")
def scene(eng):
    """The spans, their logs, the oracle's batch, and the two existing calls' results, computed once."""
    spans = make_spans()
    logs = open_logs(eng, spans, 100)
    plain = eng.decode_logs_columns(logs, [0] * len(logs), payloads=True)
    packed = eng.decode_logs_columns(logs, [0] * len(logs), packed=True, payloads=True)
    return spans, logs, oracle_batch(spans), plain, packed


def same_as_the_existing_calls(got, plain, packed):
    from clonos_amd import pack_wide_host
    assert_same_packed(got, packed)                             # the narrow part
    assert got.wide_packed is not None
    assert_same_wide(got.wide_packed, pack_wide_host(plain))    # the wide part
    assert (np.asarray(got.span_base) == np.asarray(plain.span_base)).all()
    if plain.var is not None:
        assert "var_pos" not in got.__dict__                    # pos was not delivered
        assert got.var.tobytes() == plain.var.tobytes()
        pos = np.concatenate([[0], np.cumsum(got.wide_packed.unpack()["w_var_len"], dtype=np.uint64)])
        assert (pos == plain.var_pos).all() and (got.var_pos == plain.var_pos).all()
    assert_columns_equal(got.unpack(), plain)


def test_narrow_wide_and_payloads_are_the_existing_calls(eng, scene):
    spans, logs, batch, plain, packed = scene
    assert plain.w_v0.size > 0 and plain.var.size > 0 and set(plain.tag[plain.w_idx]) == {3, 4, 5, 6}
    eng.kernel_stats_reset()
    got = eng.decode_logs_columns(logs, [0] * len(logs), packed=True, pack_wide=True, payloads=True)
    assert eng.kernel_stats()["pack_wide"]["launches"] >= 3
    delivered = got.n_bytes
    same_as_the_existing_calls(got, plain, packed)
    assert got.n_bytes == delivered < packed.n_bytes           # (unpacking for the checks delivers nothing more)
    assert got.n_spans == len(spans) and got.n_rec == batch.n_rec


def test_without_the_payload_column(eng, scene):
    spans, logs, _, plain, packed = scene
    got = eng.decode_logs_columns(logs, [0] * len(logs), packed=True, pack_wide=True)
    assert got.var is None and got.var_pos is None
    from clonos_amd import pack_wide_host
    assert_same_packed(got, packed)
    assert_same_wide(got.wide_packed, pack_wide_host(plain))
    for k in WIDE:
        assert (getattr(got, k) == getattr(plain, k)).all(), k


def test_host_input_twin(eng, scene):
    spans, logs, _, plain, packed = scene
    data = np.frombuffer(b"".join(spans), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in spans])])
    at = [(int(o), len(s)) for o, s in zip(offs, spans)]
    got = eng.decode_host_columns(data, at, packed=True, pack_wide=True, payloads=True)
    same_as_the_existing_calls(got, plain, packed)


def raw_call(eng, logs, sizes, var, pk, wpk):
    from clonos_amd import _lib
    h = np.array([l.handle for l in logs], np.uint32)
    ep = np.zeros(len(logs), np.int64)
    return _lib.lib.clg_decode_logs_columns_packed_wide(eng._h, h.ctypes.data, ep.ctypes.data, len(logs), C.byref(sizes),
                                                        C.byref(var) if var is not None else None, C.byref(pk), C.byref(wpk))


def test_any_column_pointer_in_sizes_is_rejected(eng, scene):
    from clonos_amd import _lib
    _, logs, _, _, _ = scene
    spare = np.zeros(1 << 16, np.int64)
    for name in ("tag", "order", "timestamp", "rng", "buffer_built") + WIDE:
        sizes, pk, wpk = _lib.Columns(), _lib.Packed(), _lib.PackedWideC()
        setattr(sizes, name, spare.ctypes.data)
        sizes.cap_tag = sizes.cap_order = sizes.cap_timestamp = sizes.cap_rng = sizes.cap_buffer_built = sizes.cap_wide = 1 << 16
        assert raw_call(eng, logs, sizes, None, pk, wpk) == _lib.CLG_E_INVALID_ARG, name
    assert not spare.any()


def test_sizes_only_then_pos_alone_is_still_short(eng, scene):
    """Every pointer NULL: all sizes.  var NULL with pos given keeps its meaning: var is too small."""
    from clonos_amd import _lib
    from clonos_amd.engine import _payloads_struct
    _, logs, _, plain, packed = scene
    want = eng.decode_logs_columns(logs, [0] * len(logs), packed=True, pack_wide=True, payloads=True)
    sizes, pk, wpk, pv = _lib.Columns(), _lib.Packed(), _lib.PackedWideC(), _lib.Payloads()
    assert raw_call(eng, logs, sizes, pv, pk, wpk) == _lib.CLG_OK
    assert sizes.n_rec == plain.n_rec and sizes.n_class[4] == plain.w_v0.size
    assert list(pk.n_val) == packed.n_val and pk.n_bits == packed.bits.size
    assert list(wpk.n_val) == want.wide_packed.n_val and list(wpk.blk_base) == want.wide_packed.blk_base
    assert wpk.n_bits == want.wide_packed.bits.size and wpk.bad_row == 2 ** 64 - 1
    assert pv.n_rows == plain.w_v0.size and pv.n_var == plain.var.size
    pos = np.full(plain.w_v0.size + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    pv = _payloads_struct(None, pos)
    assert raw_call(eng, logs, sizes, pv, pk, wpk) == _lib.CLG_E_CAPACITY
    assert (pos == 0xA5A5A5A5A5A5A5A5).all()


@pytest.mark.parametrize("short", ["desc", "bits", "wdesc", "wbits", "var"])
def test_a_capacity_failure_fills_every_size_and_writes_nothing(eng, scene, short):
    from clonos_amd import _lib
    from clonos_amd.engine import PACK_BLOCK, _packed_struct, _packed_wide_struct, _payloads_struct
    _, logs, _, plain, packed = scene
    want = eng.decode_logs_columns(logs, [0] * len(logs), packed=True, pack_wide=True, payloads=True)
    nb, nbits, nvar = packed.desc.size, packed.bits.size, plain.var.size
    wnb, wnbits = want.wide_packed.desc.size, want.wide_packed.bits.size
    assert min(nb, nbits, wnb, wnbits, nvar) > 0
    desc, bits = np.full((nb - (short == "desc")) * 32, FILL, np.uint8), np.full(nbits - (short == "bits"), FILL, np.uint8)
    wdesc = np.full((wnb - (short == "wdesc")) * 32, FILL, np.uint8)
    wbits = np.full(wnbits - (short == "wbits"), FILL, np.uint8)
    var = np.full(nvar - (short == "var"), FILL, np.uint8)
    base = np.zeros((len(logs) + 1) * 5, np.uint64)
    sizes = _lib.Columns()
    sizes.span_base = base.ctypes.data
    pk = _packed_struct(desc.view(PACK_BLOCK), bits)
    wpk = _packed_wide_struct(wdesc.view(PACK_BLOCK), wbits)
    pv = _payloads_struct(var, None)
    assert raw_call(eng, logs, sizes, pv, pk, wpk) == _lib.CLG_E_CAPACITY
    assert sizes.n_rec == plain.n_rec and sizes.n_class[4] == plain.w_v0.size
    assert list(pk.n_val) == packed.n_val and list(pk.blk_base) == packed.blk_base and pk.n_bits == nbits
    assert list(wpk.n_val) == want.wide_packed.n_val and list(wpk.blk_base) == want.wide_packed.blk_base
    assert wpk.n_bits == wnbits and pv.n_rows == plain.w_v0.size and pv.n_var == nvar
    assert (base.reshape(-1, 5) == plain.span_base).all()
    for a in (desc, bits, wdesc, wbits, var):
        assert (a == FILL).all()


def test_decode_error_in_one_span_passes_through(eng):
    from clonos_amd import ClonosError, pack_wide_host, synth
    rng = np.random.default_rng(11)
    good = [synth.random_log(300, rng, allow_serializable=True) for _ in range(3)]
    cut = synth.random_log(120, rng, allow_serializable=False) + b"\x09" + synth.random_log(40, rng, allow_serializable=False)
    spans = [good[0], cut, good[1], good[2]]
    logs = open_logs(eng, spans, 200)
    _, err = oracle_batch(spans, allow_errors=True)
    assert err is not None and err[1] == 1
    with pytest.raises(ClonosError) as ei:
        eng.decode_logs_columns(logs, [0] * 4, packed=True, pack_wide=True)
    assert (ei.value.status, ei.value.err_span, ei.value.err_off, ei.value.err_tag) == err
    got = eng.decode_logs_columns(logs, [0] * 4, packed=True, pack_wide=True, partial=True, payloads=True)
    plain = eng.decode_logs_columns(logs, [0] * 4, partial=True, payloads=True)
    packed = eng.decode_logs_columns(logs, [0] * 4, packed=True, partial=True, payloads=True)
    assert got.error is not None and got.error.status == err[0] == plain.error.status
    assert (got.error.err_span, got.error.err_off, got.error.err_tag) == err[1:]
    same_as_the_existing_calls(got, plain, packed)
    assert got.span(1).tag.size == 120  # span 1 is packed up to its first error


def test_column_replayer_over_unpacked_columns_yields_the_oracles_determinants(eng, scene):
    from clonos_amd import determinants as D
    from clonos_amd.replay import ColumnReplayer
    spans, logs, batch, _, _ = scene
    got = eng.decode_logs_columns(logs, [0] * len(logs), packed=True, pack_wide=True, payloads=True)
    for cols in (got.unpack(), got):  # the plain columns, and the packed ones through their span views
        for s in range(len(spans)):
            rep, out = ColumnReplayer(cols, s), []
            while not rep.isFinished():
                t = rep.next_tag()
                if t == D.ORDER:
                    out.append(D.OrderDeterminant(rep.replayNextChannel()))
                elif t == D.TIMESTAMP:
                    out.append(D.TimestampDeterminant(rep.replayNextTimestamp()))
                elif t == D.RNG:
                    out.append(D.RNGDeterminant(rep.replayRandomInt()))
                elif t == D.BUFFER_BUILT:
                    out.append(D.BufferBuiltDeterminant(rep.replayNextBufferSize()))
                elif t == D.SERIALIZABLE:
                    out.append(D.SerializableDeterminant(rep.replaySerializableDeterminant()))
                else:
                    out.append(rep.triggerAsyncEvent(rep.record_count_target()))
            assert out == batch.determinants(s)


def test_encode_of_wide_packed_columns_gives_the_logs_bytes(eng, scene):
    """The _columns_in path: the rows go through clg_unpack_wide_host and var_pos is rebuilt."""
    spans, logs, _, _, _ = scene
    got = eng.decode_logs_columns(logs, [0] * len(logs), packed=True, pack_wide=True, payloads=True)
    assert eng.encode_columns(got) == b"".join(spans)
