"""GPU: clg_decode_logs_columns_packed / clg_decode_host_columns_packed.  The packed call's
unpacked columns are the plain call's, array for array, and its packed bytes are pack_columns_host's
of those columns, byte for byte; the wide rows, span_base, the payload column, the error fields and
the status pass through as clg_decode_logs_columns_var delivers them."""
import ctypes as C

import numpy as np
import pytest

from _columns_util import assert_columns_equal, oracle_batch
from _pack_util import assert_same_packed

pytestmark = pytest.mark.gpu

FILL = 0xA5
WIDE = ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0")
WIDE_DT = (np.uint32, np.int32, np.int64, np.uint32, np.uint32, np.uint8, np.int64)


def make_spans():
    """Empty spans first, in the middle and last; spans that cross 256-byte segments and blocks of
    1024 values (the tag stream runs over every span boundary); wide rows with payloads."""
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
    spans = make_spans()
    return spans, open_logs(eng, spans, 100), oracle_batch(spans)


def same_columns(packed, plain):
    from clonos_amd import pack_columns_host
    assert_columns_equal(packed.unpack(), plain)
    assert_same_packed(packed, pack_columns_host(plain))
    assert packed.n_bytes < plain.n_bytes


def test_unpacked_columns_are_the_plain_ones(eng, scene):
    spans, logs, batch = scene
    eng.kernel_stats_reset()
    packed = eng.decode_logs_columns(logs, [0] * len(logs), packed=True)
    assert eng.kernel_stats()["pack_columns"]["launches"] >= 2
    plain = eng.decode_logs_columns(logs, [0] * len(logs))
    same_columns(packed, plain)
    assert packed.var is None and packed.n_spans == len(spans) and packed.n_rec == batch.n_rec


def test_with_the_payload_column(eng, scene):
    spans, logs, _ = scene
    packed = eng.decode_logs_columns(logs, [0] * len(logs), packed=True, payloads=True)
    plain = eng.decode_logs_columns(logs, [0] * len(logs), payloads=True)
    same_columns(packed, plain)
    assert plain.var.size > 0
    assert (packed.var == plain.var).all() and (packed.var_pos == plain.var_pos).all()


def test_host_input_twin(eng, scene):
    spans, logs, _ = scene
    data = np.frombuffer(b"".join(spans), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in spans])])
    at = [(int(o), len(s)) for o, s in zip(offs, spans)]
    packed = eng.decode_host_columns(data, at, packed=True, payloads=True)
    plain = eng.decode_host_columns(data, at, payloads=True)
    same_columns(packed, plain)
    assert (packed.var == plain.var).all() and (packed.var_pos == plain.var_pos).all()
    assert_same_packed(packed, eng.decode_logs_columns(logs, [0] * len(logs), packed=True))


def test_a_batch_past_the_one_launch_forms(eng):
    """40000 records: the multi-kernel columnize and decode, 79 blocks."""
    from clonos_amd import synth
    rng = np.random.default_rng(0xB16)
    spans = [bytes(synth.config2_log(25000, rng)[0]), bytes(synth.config2_log(15000, rng)[0])]
    logs = open_logs(eng, spans, 300)
    packed = eng.decode_logs_columns(logs, [0, 0], packed=True)
    same_columns(packed, eng.decode_logs_columns(logs, [0, 0]))
    assert packed.n_rec == 40000


def test_decode_error_in_one_span_passes_through(eng):
    from clonos_amd import ClonosError, synth
    rng = np.random.default_rng(11)
    good = [synth.random_log(300, rng, allow_serializable=False) for _ in range(3)]
    cut = synth.random_log(120, rng, allow_serializable=False) + b"\x09" + synth.random_log(40, rng, allow_serializable=False)
    spans = [good[0], cut, good[1], good[2]]
    logs = open_logs(eng, spans, 200)
    _, err = oracle_batch(spans, allow_errors=True)
    assert err is not None and err[1] == 1
    with pytest.raises(ClonosError) as ei:
        eng.decode_logs_columns(logs, [0] * 4, packed=True)
    assert (ei.value.status, ei.value.err_span, ei.value.err_off, ei.value.err_tag) == err
    packed = eng.decode_logs_columns(logs, [0] * 4, packed=True, partial=True, payloads=True)
    plain = eng.decode_logs_columns(logs, [0] * 4, partial=True, payloads=True)
    assert packed.error is not None and packed.error.status == err[0] == plain.error.status
    assert (packed.error.err_span, packed.error.err_off, packed.error.err_tag) == err[1:]
    same_columns(packed, plain)
    assert packed.span(1).tag.size == 120
    assert (packed.var == plain.var).all() and (packed.var_pos == plain.var_pos).all()


def raw_call(eng, logs, wide, var, pk):
    from clonos_amd import _lib
    h = np.array([l.handle for l in logs], np.uint32)
    ep = np.zeros(len(logs), np.int64)
    return _lib.lib.clg_decode_logs_columns_packed(eng._h, h.ctypes.data, ep.ctypes.data, len(logs), C.byref(wide),
                                                   C.byref(var) if var is not None else None, C.byref(pk))


def test_narrow_pointers_in_wide_are_rejected(eng, scene):
    from clonos_amd import _lib
    _, logs, _ = scene
    spare = np.zeros(1 << 16, np.int64)
    for name in ("tag", "order", "timestamp", "rng", "buffer_built"):
        wide, pk = _lib.Columns(), _lib.Packed()
        setattr(wide, name, spare.ctypes.data)
        setattr(wide, "cap_" + name, spare.size)
        assert raw_call(eng, logs, wide, None, pk) == _lib.CLG_E_INVALID_ARG
    assert not spare.any()


@pytest.mark.parametrize("short", ["wide", "desc", "bits", "var"])
def test_a_capacity_failure_fills_every_size_and_writes_nothing(eng, scene, short):
    from clonos_amd import _lib
    from clonos_amd.engine import PACK_BLOCK, _packed_struct, _payloads_struct
    _, logs, _ = scene
    want = eng.decode_logs_columns(logs, [0] * len(logs), packed=True, payloads=True)
    nw, nb, nbits, nvar = want.w_v0.size, want.desc.size, want.bits.size, want.var.size
    assert min(nw, nb, nbits, nvar) > 0
    arrs = {k: np.full((nw - (short == "wide")) * np.dtype(dt).itemsize, FILL, np.uint8) for k, dt in zip(WIDE, WIDE_DT)}
    desc, bits = np.full((nb - (short == "desc")) * 32, FILL, np.uint8), np.full(nbits - (short == "bits"), FILL, np.uint8)
    var, pos = np.full(nvar - (short == "var"), FILL, np.uint8), np.full((nw + 1) * 8, FILL, np.uint8)
    base = np.zeros((len(logs) + 1) * 5, np.uint64)
    wide = _lib.Columns()
    for k in WIDE:
        setattr(wide, k, arrs[k].ctypes.data)
    wide.cap_wide, wide.span_base = nw - (short == "wide"), base.ctypes.data
    pk = _packed_struct(desc.view(PACK_BLOCK), bits)
    pv = _payloads_struct(var, pos.view(np.uint64))
    assert raw_call(eng, logs, wide, pv, pk) == _lib.CLG_E_CAPACITY
    assert wide.n_rec == want.n_rec and wide.n_class[4] == nw
    assert list(pk.n_val) == want.n_val and list(pk.blk_base) == want.blk_base and pk.n_bits == nbits
    assert pv.n_rows == nw and pv.n_var == nvar
    assert (base.reshape(-1, 5) == want.span_base).all()
    for a in list(arrs.values()) + [desc, bits, var, pos]:
        assert (a.view(np.uint8) == FILL).all()


def test_column_replayer_over_packed_spans(eng, scene):
    from clonos_amd import determinants as D
    from clonos_amd.replay import ColumnReplayer
    spans, logs, batch = scene
    packed = eng.decode_logs_columns(logs, [0] * len(logs), packed=True, payloads=True)
    for s in range(len(spans)):
        rep, got = ColumnReplayer(packed, s), []
        while not rep.isFinished():
            t = rep.next_tag()
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
                got.append(rep.triggerAsyncEvent(rep.record_count_target()))
        assert got == batch.determinants(s)
