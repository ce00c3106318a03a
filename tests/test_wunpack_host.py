"""CPU: both packed forms back to log bytes on the host.  The header's functions
(clonos_amd/csrc/pack_wide.h's wpack_unpack_both_host and its parts, compiled with g++ into the
stand-alone program tests/wunpack_host.cpp, once plainly and once with
-fsanitize=address,undefined, and run directly), and clg_encode_columns_packed_wide_host of the
library through ctypes: its bytes are encode_columns_host's of the plain columns, that is the spans'
own; every check comes in its order; the output is untouched on every rejection."""
import os
import re
import subprocess

import numpy as np
import pytest

from _encode_util import host_columns
from _wunpack_util import (FILL, WIDE_STREAM, host_rows_untouched, packed_both, packed_spans, raw_host, swap_two_wide_tags,
                           with_tags)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "wunpack_host.cpp")


def test_header_functions(tmp_path):
    exe = str(tmp_path / "wunpack_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 50000, r.stdout


def test_header_functions_sanitized(tmp_path):
    """The same program with the address and undefined-behaviour sanitizers, run directly (their
    runtimes linked into the program: it needs nothing preloaded)."""
    exe = str(tmp_path / "wunpack_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok (\d+)\n", r.stdout), r.stdout


def make_spans():
    """Empty spans first, in the middle and last; config 3, config 2 and random logs: wide rows of
    every kind with payloads, over more than two tiles of 1024 rows."""
    from clonos_amd import synth
    rng = np.random.default_rng(0xDEC0DE)
    return [b"", bytes(synth.config3_epoch(3000, rng)[0]), b"", synth.random_log(6000, rng, allow_serializable=True),
            bytes(synth.config2_log(3000, rng)[0]), synth.random_log(5, rng, allow_serializable=False), b""]


SPANS = make_spans()
_SCENE = []


def scene():
    """The plain host columns and both their packed forms, computed once and left unchanged."""
    if not _SCENE:
        _SCENE.extend(packed_spans(SPANS))
    return _SCENE


def test_the_twin_equals_the_plain_host_encode():
    from clonos_amd import encode_columns_host, encode_columns_packed_wide_host
    cols, got = scene()
    assert got.wide_packed.n_wide > 2048 and set(cols.tag[cols.w_idx]) == {3, 4, 5, 6} and cols.var.size > 0
    whole = encode_columns_packed_wide_host(got)
    assert whole == encode_columns_host(cols) == b"".join(SPANS)
    assert encode_columns_packed_wide_host(got, per_span=True) == encode_columns_host(cols, per_span=True) == [bytes(s) for s in SPANS]
    assert host_rows_untouched(got)  # neither the rows nor var_pos were built in Python


def test_no_wide_rows_and_no_records():
    from clonos_amd import encode_columns_packed_wide_host, synth
    spans = [bytes(synth.config2_log(1200, np.random.default_rng(2))[0]), b""]
    cols, got = packed_spans(spans)
    assert got.wide_packed.n_wide == 0
    assert encode_columns_packed_wide_host(got) == b"".join(spans)
    cols, got = packed_spans([b"", b""])
    assert encode_columns_packed_wide_host(got) == b""


def rejected(got, what, stream, block, rest_poke=None):
    from clonos_amd import _lib
    st, bad, enc, buf = raw_host(got, rest_poke=rest_poke)
    assert st == _lib.CLG_E_INVALID_ARG and bad == (what, stream, block), (st, bad)
    assert (buf == FILL).all() and enc.bad_what == 0 and enc.n_bytes == 0


def fresh():
    """A copy of the scene's packed columns whose descriptors, bits and sizes may be changed."""
    import copy
    cols, got = scene()
    out = copy.copy(got)
    out.desc, out.bits, out.n_val, out.blk_base = got.desc.copy(), got.bits.copy(), list(got.n_val), list(got.blk_base)
    out.wide_packed = copy.copy(got.wide_packed)
    w = out.wide_packed
    w.desc, w.bits, w.n_val, w.blk_base = w.desc.copy(), w.bits.copy(), list(w.n_val), list(w.blk_base)
    return out


def test_every_check_in_its_order():
    from clonos_amd import _lib
    L, B, V = _lib.UNPACK_BAD_LAYOUT, _lib.UNPACK_BAD_BLOCK, _lib.UNPACK_BAD_VALUE
    W = WIDE_STREAM
    assert W == _lib.UNPACK_WIDE_STREAM
    st, bad, enc, buf = raw_host(scene()[1])
    assert st == _lib.CLG_OK and bad == (_lib.UNPACK_BAD_NONE, 0, 2 ** 64 - 1)
    assert buf[:enc.n_bytes].tobytes() == b"".join(SPANS) and (buf[enc.n_bytes:] == FILL).all()
    # 1. narrow's layout, then its totals, both before wide's layout
    g = fresh()
    g.blk_base[3] += 1
    g.wide_packed.blk_base[7] += 1
    rejected(g, L, 2, 0)
    g.blk_base[3] -= 1

    def one_more_timestamp(rest):
        rest.n_class[1] += 1
    rejected(g, L, 2, 0, one_more_timestamp)
    # 2. wide's layout, with the offset: the family's own rules too
    rejected(g, L, W + 6, 0)
    g.wide_packed.blk_base[7] -= 1
    g.wide_packed.n_val[1] -= 1
    rejected(g, L, W + 1, 0)
    g.wide_packed.n_val[1] += 1
    g.wide_packed.n_val[2 + 6 + 3] -= 1
    rejected(g, L, W + 2 + 6 + 3, 0)
    # 3. the rows against rest's n_class[4]

    def one_row_fewer(rest):
        rest.n_class[4] -= 1
    rejected(fresh(), L, W, 0, one_row_fewer)
    # 4. a narrow finding (a value, the later kind) comes before 5. a wide one (a block, the earlier kind)
    g = fresh()
    g.wide_packed.desc["width"][1] = 65
    g.desc["ref"][g.blk_base[_lib.PACK_RNG]] = 1 << 40
    rejected(g, V, _lib.PACK_RNG, 0)
    g.desc["width"][g.blk_base[_lib.PACK_TAG] + 1] = 99
    rejected(g, B, _lib.PACK_TAG, 1)
    g = fresh()
    g.wide_packed.desc["width"][1] = 65
    g.wide_packed.desc["ref"][0] = 3
    rejected(g, B, W, 1)                                    # BLOCK before VALUE inside wide
    g.wide_packed.desc["width"][1] = scene()[1].wide_packed.desc["width"][1]
    rejected(g, V, W, 0)                                    # a KIND above 3
    g = fresh()
    w = g.wide_packed
    assert w.desc["width"][0] == 2
    w.bits[int(w.desc["pos"][0])] = (int(w.bits[int(w.desc["pos"][0])]) & 0xFC) | ((int(w.bits[int(w.desc["pos"][0])]) + 1) & 3)
    w.desc["first"][w.blk_base[2 + 12 + 2]] = -1            # a later stream's value: the histogram comes first
    rejected(g, V, W, 0)
    g = fresh()
    w = g.wide_packed
    w.desc["first"][w.blk_base[2 + 12 + 2]] = -1
    w.desc["pos"][w.blk_base[2 + 18 + 5]] += 8              # pos % 16
    rejected(g, B, W + 2 + 18 + 5, 0)
    w.desc["pos"][w.blk_base[2 + 18 + 5]] -= 8
    rejected(g, V, W + 2 + 12 + 2, 0)


def test_rest_must_not_carry_what_the_packed_forms_give():
    from clonos_amd import _lib
    cols, got = scene()
    spare = np.zeros(1 << 16, np.uint64)
    for name in ("tag", "order", "timestamp", "rng", "buffer_built", "w_rc", "w_v1", "w_var_len", "w_sub", "w_v0", "w_idx", "pos"):
        st, bad, enc, buf = raw_host(got, rest_poke=lambda rest: setattr(rest, name, spare.ctypes.data))
        assert st == _lib.CLG_E_INVALID_ARG and bad[0] == _lib.UNPACK_BAD_NONE and (buf == FILL).all(), name


def test_the_cross_rule_in_the_first_and_the_last_tile():
    """The wide rows packed from consistent columns, the narrow columns from tags in which two wide
    records of different kinds are swapped.  The expected row comes from numpy on the packed kinds
    and the tags; the lowest row wins."""
    from clonos_amd import ClonosError, _lib, encode_columns_packed_wide_host, pack_columns_host
    cols, good = scene()
    n = good.wide_packed.n_wide
    kinds = good.wide_packed.kinds()
    idx = np.asarray(cols.w_idx)

    def expect(tag):
        return int(np.flatnonzero(tag[idx].astype(np.int64) - 3 != kinds)[0])

    tag_last, k_last = swap_two_wide_tags(cols, (n - 1) // 1024 * 1024 + 3, n)
    tag_both, k_first = swap_two_wide_tags(with_tags(cols, tag_last), 40, 1024)
    assert k_first < 1024 <= 2048 <= k_last and expect(tag_last) == k_last and expect(tag_both) == k_first
    for tag, row in ((tag_last, k_last), (tag_both, k_first)):
        g = fresh()
        pk = pack_columns_host(with_tags(cols, tag))
        g.desc, g.bits, g.n_val, g.blk_base = pk.desc, pk.bits, pk.n_val, pk.blk_base
        rejected(g, _lib.UNPACK_BAD_VALUE, WIDE_STREAM + _lib.WPACK_IDX, row // 1024)
        with pytest.raises(ClonosError) as ei:
            encode_columns_packed_wide_host(g)
        assert (ei.value.bad_what, ei.value.bad_stream, ei.value.bad_block) == (3, 33, row // 1024)
        assert ei.value.enc_bad_what == 0


def test_a_tag_of_8_at_a_narrow_position_is_the_encodes_finding():
    from clonos_amd import _lib, pack_columns_host
    cols, good = scene()
    at = int(np.flatnonzero(cols.tag == 2)[7])
    tag = np.array(cols.tag)
    tag[at] = 8
    g = fresh()
    pk = pack_columns_host(with_tags(cols, tag))
    g.desc, g.bits, g.n_val, g.blk_base = pk.desc, pk.bits, pk.n_val, pk.blk_base
    st, bad, enc, buf = raw_host(g)
    assert st == _lib.CLG_E_INVALID_ARG and bad[0] == _lib.UNPACK_BAD_NONE
    assert enc.bad_what == _lib.ENC_BAD_TAG and enc.bad_index == at and (buf == FILL).all()
