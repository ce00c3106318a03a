"""CPU: the windowed dispatch order of a batched slice's runs (clonos_amd/csrc/slice_order.h).

Compiled for the host with g++ (tests/slice_order_host.cpp).  window_order cuts each run at
multiples of W segments of the log's physical offset and emits the sub-runs by log, window,
consumer.  Checked on random run sets (1-9 runs per log, requests of the logs interleaved,
starts and ends inside a segment, on its boundary and one byte either side): the pieces the
device expansion (k_expand_pieces, restated here) makes of the new runs are the pieces of the
original runs, no sub-run crosses a window boundary, the order is log, window, consumer,
`first` is the exclusive prefix of the piece counts, and a batch in which no log has two runs
comes back untouched.
"""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN = np.dtype([("segtab_off", "<u8"), ("phys", "<u4"), ("len", "<u4"), ("dst", "<u8"), ("first", "<u4"),
                 ("pad", "<u4")])
BIG_W = 1 << 20  # more segments than any log here (W * C passes 2^32 with C = 4096 and up: 64-bit window bytes)


@pytest.fixture(scope="module")
def so(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("slice_order") / "libslice_order.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", path,
                    os.path.join(ROOT, "tests", "slice_order_host.cpp")], check=True)
    lib = C.CDLL(path)
    lib.so_window_order.restype = C.c_int64
    lib.so_window_order.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                    C.POINTER(C.c_int32)]
    lib.so_span_bytes.restype = C.c_uint32
    lib.so_default_window.restype = C.c_uint32
    lib.so_default_window.argtypes = [C.c_uint32]
    assert lib.so_span_bytes() == SPAN.itemsize
    return lib


def window_order(lib, runs, seg, w):
    runs = np.ascontiguousarray(runs, SPAN)
    cap = int(sum(n_pieces(r, seg) for r in runs)) + 1  # a sub-run holds at least one piece
    out = np.zeros(cap, SPAN)
    changed = C.c_int32(-1)
    n = lib.so_window_order(runs.ctypes.data, len(runs), seg, w, out.ctypes.data, cap, C.byref(changed))
    assert n >= 0
    return out[:n], bool(changed.value)


def n_pieces(r, seg):
    return (int(r["phys"]) + int(r["len"]) - 1) // seg - int(r["phys"]) // seg + 1


def pieces(runs, seg):
    """k_expand_pieces: (segment table entry, offset in the segment, dst, len) per piece, in order."""
    out = []
    for r in runs:
        phys, ln, dst, tab = int(r["phys"]), int(r["len"]), int(r["dst"]), int(r["segtab_off"])
        for w in range(phys // seg, (phys + ln - 1) // seg + 1):
            s0, e1 = max(w * seg, phys), min((w + 1) * seg, phys + ln)
            out.append((tab + w, s0 - w * seg, dst + s0 - phys, e1 - s0))
    return out


def edge_offset(rng, seg, n_seg):
    """A byte offset in [0, n_seg * seg]: inside a segment, on a boundary, or one byte either side."""
    b = int(rng.integers(0, n_seg + 1)) * seg
    o = b + int(rng.choice([0, 0, -1, 1, int(rng.integers(1, seg))]))
    return min(max(o, 0), n_seg * seg)


def random_runs(rng, seg, n_logs, max_runs=9, suffixes=False):
    """Runs as clg_slice_batch plans them: requests of the logs interleaved, a log's segtab_off
    handed out when it first appears (rising), dst packed in request order, pad = the request."""
    n_seg = [int(rng.integers(1, 24)) for _ in range(n_logs)]
    owner = [l for l in range(n_logs) for _ in range(int(rng.integers(1, max_runs + 1)))]
    owner = [owner[j] for j in rng.permutation(len(owner))]
    tab_of, tab_top, rows, dst, first = {}, 0, [], 0, 0
    for i, l in enumerate(owner):
        total = n_seg[l] * seg
        if suffixes:  # a consumer's suffix of the log, as the slice's runs are
            a, b = edge_offset(rng, seg, n_seg[l]), total
        else:
            a, b = sorted((edge_offset(rng, seg, n_seg[l]), edge_offset(rng, seg, n_seg[l])))
        if a == b:  # the planner makes no run of an empty delta
            continue
        if l not in tab_of:
            tab_of[l] = tab_top
            tab_top += n_seg[l]
        rows.append((tab_of[l], a, b - a, dst, first, i))
        first += (b - 1) // seg - a // seg + 1
        dst += b - a
    return np.array(rows, SPAN)


@pytest.mark.parametrize("seg", [64, 256])
@pytest.mark.parametrize("w", [1, 2, 5, BIG_W])
def test_same_pieces_in_window_order(so, seg, w):
    rng = np.random.default_rng(seg * 31 + w % 1000)
    for it in range(60):
        runs = random_runs(rng, seg, int(rng.integers(1, 6)), suffixes=it % 2 == 0)
        got, changed = window_order(so, runs, seg, w)
        shared = len(set(runs["segtab_off"].tolist())) < len(runs)
        assert changed == shared
        if not shared:
            assert got.tobytes() == runs.tobytes()
            continue
        # the same pieces, each once
        assert Counter(pieces(got, seg)) == Counter(pieces(runs, seg))
        assert (got["len"] > 0).all()
        win = w * seg
        lo, hi = got["phys"].astype(np.int64) // win, (got["phys"].astype(np.int64) + got["len"] - 1) // win
        assert (lo == hi).all()  # no sub-run crosses a window boundary
        # log (in order of first appearance: rising segtab_off), then window, then consumer;
        # strictly rising: a consumer has one sub-run per window
        keys = list(zip(got["segtab_off"].tolist(), lo.tolist(), got["pad"].tolist()))
        assert all(a < b for a, b in zip(keys, keys[1:]))
        # first: the exclusive prefix of the piece counts
        cnt = [n_pieces(r, seg) for r in got]
        assert got["first"].tolist() == [sum(cnt[:i]) for i in range(len(cnt))]
        assert sum(cnt) == sum(n_pieces(r, seg) for r in runs)
        # a sub-run lies in its request's run, at the dst that run gives its bytes
        by_req = {int(r["pad"]): r for r in runs}
        for s in got:
            r = by_req[int(s["pad"])]
            assert s["segtab_off"] == r["segtab_off"] and s["phys"] >= r["phys"]
            assert int(s["phys"]) + int(s["len"]) <= int(r["phys"]) + int(r["len"])
            assert int(s["dst"]) - int(r["dst"]) == int(s["phys"]) - int(r["phys"])
        if w == BIG_W:  # one window: the runs themselves, grouped by log
            assert len(got) == len(runs)


@pytest.mark.parametrize("seg", [64, 256])
@pytest.mark.parametrize("w", [0, 1, 2, 5, BIG_W])
def test_no_shared_log_is_untouched(so, seg, w):
    rng = np.random.default_rng(seg + w % 1000)
    for _ in range(20):
        runs = random_runs(rng, seg, int(rng.integers(1, 40)), max_runs=1)
        got, changed = window_order(so, runs, seg, w)
        assert not changed and got.tobytes() == runs.tobytes()


def test_window_zero_is_request_order(so):
    rng = np.random.default_rng(3)
    runs = random_runs(rng, 64, 4)
    got, changed = window_order(so, runs, 64, 0)
    assert not changed and got.tobytes() == runs.tobytes()
    got, changed = window_order(so, runs[:0], 64, 2)
    assert not changed and len(got) == 0


def test_default_window_is_two_mib_of_log(so):
    assert [so.so_default_window(c) for c in (64, 256, 16384, 65536, 2 << 20, 4 << 20, 0)] == [
        32768, 8192, 128, 32, 1, 1, 1]


def test_cut_at_the_window_boundary_exactly(so):
    """Two consumers of one log of 8 segments of 64 bytes, W = 2 (windows of 128 bytes): one
    starts on a window boundary, one a byte before it."""
    runs = np.array([(0, 128, 384, 0, 0, 0), (0, 127, 385, 384, 6, 1)], SPAN)
    got, changed = window_order(so, runs, 64, 2)
    assert changed
    assert [(int(s["phys"]), int(s["len"]), int(s["dst"]), int(s["first"]), int(s["pad"])) for s in got] == [
        (127, 1, 384, 0, 1),
        (128, 128, 0, 1, 0), (128, 128, 385, 3, 1),
        (256, 128, 128, 5, 0), (256, 128, 513, 7, 1),
        (384, 128, 256, 9, 0), (384, 128, 641, 11, 1)]
