"""Shared by the tests of the calls that take both packed forms: host columns given as a
PackedColumns whose wide rows are packed too (what decode_logs_columns(packed=True, pack_wide=True,
payloads=True) delivers), the raw host call, and copies with one descriptor or payload byte
changed."""
import ctypes as C

import numpy as np

from _encode_util import host_columns

FILL = 0xA5
WIDE_STREAM = 32


def packed_both(cols):
    """Both packed forms of host columns that carry their payload column; var is attached, var_pos
    and the w_* arrays are not there (they stay unbuilt until something reads them)."""
    from clonos_amd import PackedColumns, pack_columns_host, pack_wide_host
    pk = pack_columns_host(cols)
    out = PackedColumns(np.array(pk.desc), np.array(pk.bits), pk.n_val, pk.blk_base, *[None] * 7, cols.span_base,
                        wide_packed=pack_wide_host(cols))
    out.var = cols.var
    return out


def packed_spans(spans):
    cols = host_columns(spans)
    return cols, packed_both(cols)


def host_rows_untouched(got) -> bool:
    """No w_* array and no var_pos was built on the host."""
    return "w_idx" not in got.__dict__ and "var_pos" not in got.__dict__


def swap_two_wide_tags(cols, lo, hi):
    """A copy of cols' tags in which the first two neighbouring wide records of different kinds among
    rows [lo, hi) have their tags swapped, and the lower of the two rows."""
    tag = np.array(cols.tag)
    idx = np.asarray(cols.w_idx)
    for k in range(lo, hi - 1):
        if tag[idx[k]] != tag[idx[k + 1]]:
            tag[idx[k]], tag[idx[k + 1]] = tag[idx[k + 1]], tag[idx[k]]
            return tag, k
    raise AssertionError("no two neighbouring wide records of different kinds")


def with_tags(cols, tag):
    """cols with other tags (the narrow pack reads nothing else of them)."""
    import copy
    out = copy.copy(cols)
    out.tag = tag
    return out


def raw_host(got, cap=None, rest_poke=None):
    """clg_encode_columns_packed_wide_host into `cap` bytes of FILL: status, (what, stream, block),
    the clg_encoded, the buffer."""
    from clonos_amd import _lib
    from clonos_amd.engine import _rest_in
    pk, pw, (rest, keep), bad = got._struct(), got.wide_packed._struct(), _rest_in(got), _lib.UnpackBad()
    if rest_poke:
        rest_poke(rest)
    buf = np.full(cap if cap is not None else 1 << 20, FILL, np.uint8)
    enc = _lib.Encoded()
    enc.bytes, enc.cap, enc.out_kind = buf.ctypes.data, buf.size, _lib.CLG_MEM_HOST
    st = _lib.lib.clg_encode_columns_packed_wide_host(C.byref(pk), C.byref(pw), C.byref(rest), C.byref(enc), C.byref(bad))
    return st, (int(bad.what), int(bad.stream), int(bad.block)), enc, buf
