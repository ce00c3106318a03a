"""CPU: typed columns back to log bytes on the host.  The header's function
(clonos_amd/csrc/encode_columns.h, compiled with g++ into the stand-alone program
tests/encode_columns_host.cpp, once plainly and once with -fsanitize=address,undefined, and run
directly), and clg_encode_columns_host of the library through ctypes over columnize_host of the
oracle's decode with the payload column from gather_payloads_host: the result is the spans' own
bytes and the oracle's encode of the same batch."""
import os
import re
import subprocess

import numpy as np
import pytest

import _oracle as O
from _encode_util import (FILL, NONE, arrays_of, columns_in, encoded, host_columns, placed_spans, span_lengths)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "encode_columns_host.cpp")


def test_header_function(tmp_path):
    exe = str(tmp_path / "encode_columns_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 100000, r.stdout


def test_header_function_sanitized(tmp_path):
    """The same program with the address and undefined-behaviour sanitizers, run directly (their
    runtimes linked into the program: it needs nothing preloaded)."""
    exe = str(tmp_path / "encode_columns_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"ok (\d+)\n", r.stdout), r.stdout


def span_sets():
    from clonos_amd import synth
    rng = np.random.default_rng(0xEC0)
    a = synth.random_log(300, rng, allow_serializable=True)
    b = synth.random_log(300, rng, allow_serializable=False)
    c = bytes(synth.config3_epoch(400, rng)[0])
    return {
        "random_serializable": [a],
        "random_plain": [b],
        "config3": [c],
        "placed": placed_spans(),
        "empty_first_middle_last": [b"", a, b"", b"", b, c, b""],
        "all_empty": [b"", b""],
    }


SPANS = span_sets()


@pytest.mark.parametrize("name", sorted(SPANS))
def test_bytes_are_the_spans(name):
    from clonos_amd import encode_columns_host
    spans = SPANS[name]
    cols = host_columns(spans)
    whole = b"".join(spans)
    assert encode_columns_host(cols) == whole
    assert encode_columns_host(cols, per_span=True) == [bytes(s) for s in spans]
    b = cols.to_soa()
    assert whole == O.encode_soa(b.tag, b.v0, b.w_idx, b.w_rc, b.w_v1, b.w_var_off, b.w_var_len, b.w_sub, cols.var.tobytes())


def run_host(cin, enc):
    from clonos_amd import _lib
    import ctypes as C
    return _lib.lib.clg_encode_columns_host(C.byref(cin), C.byref(enc))


def test_sizes_only_and_span_byte_base():
    from clonos_amd import _lib
    spans = SPANS["empty_first_middle_last"]
    cols = host_columns(spans)
    cin, keep = columns_in(arrays_of(cols), cols.span_base)
    enc, sbb = encoded(None, 0, len(spans))
    assert run_host(cin, enc) == _lib.CLG_OK
    assert enc.n_bytes == sum(len(s) for s in spans) and enc.bad_what == 0 and enc.bad_index == NONE
    assert (sbb == span_lengths(spans)).all()
    # one span without span_base
    cin, keep = columns_in(arrays_of(cols), None)
    enc, sbb = encoded(None, 0, 1)
    assert run_host(cin, enc) == _lib.CLG_OK
    assert list(sbb) == [0, enc.n_bytes] and enc.n_bytes == sum(len(s) for s in spans)


def test_capacity_fills_results_and_writes_nothing():
    from clonos_amd import _lib
    spans = SPANS["placed"]
    cols = host_columns(spans)
    total = sum(len(s) for s in spans)
    cin, keep = columns_in(arrays_of(cols), cols.span_base)
    buf = np.full(total + 128, FILL, np.uint8)
    enc, sbb = encoded(buf.ctypes.data + 64, total - 1, len(spans))
    assert run_host(cin, enc) == _lib.CLG_E_CAPACITY
    assert enc.n_bytes == total and (sbb == span_lengths(spans)).all()
    assert (buf == FILL).all()
    enc, sbb = encoded(buf.ctypes.data + 64, total, len(spans))
    assert run_host(cin, enc) == _lib.CLG_OK
    assert buf[64:64 + total].tobytes() == b"".join(spans)
    assert (buf[:64] == FILL).all() and (buf[64 + total:] == FILL).all()


def bad(cin, total):
    """(status, bad_what, bad_index) of a call with an output buffer that must stay untouched."""
    buf = np.full(total + 16, FILL, np.uint8)
    enc, _ = encoded(buf.ctypes.data, total + 16, max(int(cin.n_spans), 1))
    st = run_host(cin, enc)
    assert (buf == FILL).all()
    return st, int(enc.bad_what), int(enc.bad_index)


def payload_rows(cols):
    """The wide rows whose format carries a payload of at least one byte."""
    tags = np.asarray(cols.tag)[np.asarray(cols.w_idx)]
    sub = np.asarray(cols.w_sub)
    pay = (tags == 3) | ((tags == 4) & (sub == 6)) | ((tags == 5) & (sub & 0x80 != 0))
    return np.nonzero(pay & (np.asarray(cols.w_var_len) > 0))[0]


def test_every_error_kind_reports_the_lowest_index():
    from clonos_amd import _lib
    spans = SPANS["empty_first_middle_last"]
    cols = host_columns(spans)
    total = sum(len(s) for s in spans)
    E = _lib.CLG_E_INVALID_ARG
    n = cols.n_rec

    a = arrays_of(cols)
    a["tag"] = a["tag"].copy()
    a["tag"][[n // 3, n - 2]] = [8, 200]
    assert bad(columns_in(a, cols.span_base)[0], total) == (E, _lib.ENC_BAD_TAG, n // 3)

    for cls in range(5):
        cin, keep = columns_in(arrays_of(cols), cols.span_base)
        cin.n_class[cls] -= 1  # (the arrays hold one more than stated: nothing is read past a length)
        assert bad(cin, total) == (E, _lib.ENC_BAD_TOTALS, cls)

    rows = payload_rows(cols)
    assert len(rows) >= 4
    a = arrays_of(cols)
    a["pos"] = a["pos"].copy()
    a["pos"][rows[-1]] = a["var"].size               # one byte past the end
    a["pos"][rows[1]] = 0xFFFFFFFFFFFFFFFF - 2       # pos + len wraps in 64 bits
    assert bad(columns_in(a, cols.span_base)[0], total) == (E, _lib.ENC_BAD_ROW, int(rows[1]))

    a = arrays_of(cols)
    a["w_idx"] = a["w_idx"].copy()
    a["w_idx"][[2, 5]] += 1
    assert bad(columns_in(a, cols.span_base)[0], total) == (E, _lib.ENC_BAD_ROW, 2)
    cin, keep = columns_in(a, cols.span_base, idx=False)  # not given: not checked
    enc, _ = encoded(None, 0, len(spans))
    assert run_host(cin, enc) == _lib.CLG_OK and enc.n_bytes == total

    sb = np.array(cols.span_base, np.uint64)
    dec = sb.copy()
    dec[5] = 0  # row 4 (the counts of the first log) is above it
    assert bad(columns_in(arrays_of(cols), dec)[0], total) == (E, _lib.ENC_BAD_SPAN, 4)
    last = sb.copy()
    last[-1, 0] += 1
    assert bad(columns_in(arrays_of(cols), last)[0], total) == (E, _lib.ENC_BAD_SPAN, len(spans))
    moved = sb.copy()  # row 5's sum stays and the rows still do not decrease, but its counts are not the tags'
    frm = int(np.nonzero(moved[5] > moved[4])[0][0])
    to = int([k for k in range(5) if k != frm and moved[5][k] < moved[6][k]][0])
    moved[5, frm] -= 1
    moved[5, to] += 1
    assert bad(columns_in(arrays_of(cols), moved)[0], total) == (E, _lib.ENC_BAD_SPAN, 5)


def test_rows_without_a_payload_are_not_read_as_one():
    """pos and w_var_len of a row whose format carries no payload may hold anything."""
    from clonos_amd import _lib
    spans = SPANS["config3"]
    cols = host_columns(spans)
    a = arrays_of(cols)
    none = np.setdiff1d(np.arange(len(cols.w_v0)), payload_rows(cols))
    tags = np.asarray(cols.tag)[np.asarray(cols.w_idx)][none]
    sub = np.asarray(cols.w_sub)[none]
    none = none[(tags == 6) | ((tags == 4) & (sub != 6)) | ((tags == 5) & (sub & 0x80 == 0))]
    assert len(none)
    a["pos"], a["w_var_len"] = a["pos"].copy(), a["w_var_len"].copy()
    a["pos"][none] = 0xFFFFFFFFFFFFFFFF
    a["w_var_len"][none] = 0xFFFFFFFF
    total = len(spans[0])
    buf = np.zeros(total, np.uint8)
    cin, keep = columns_in(a, None)
    enc, _ = encoded(buf.ctypes.data, total, 1)
    assert run_host(cin, enc) == _lib.CLG_OK
    assert buf.tobytes() == bytes(spans[0])


def test_columns_without_a_payload_column_raise():
    from clonos_amd import columnize_host, encode_columns_host
    from _columns_util import oracle_batch
    with pytest.raises(ValueError):
        encode_columns_host(columnize_host(oracle_batch(SPANS["random_plain"])))
