"""Helpers shared by the GPU decode tests: the raw decode of a batch of host spans with its
per-span record bases and first error, and its comparison with the CPU oracle span by span."""
import numpy as np

import _oracle as O

REC_FIELDS = ("off", "tag", "v0")
WIDE_FIELDS = ("w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub")


def _raw_decode(eng, blob, spans):
    from clonos_amd import Engine, _lib
    from clonos_amd._lib import lib
    from clonos_amd.engine import _np_ptr
    buf = np.frombuffer(blob, np.uint8)
    so = np.array([s[0] for s in spans], np.uint64)
    sl = np.array([s[1] for s in spans], np.uint64)
    cap, wcap = int(sl.sum()) // 2 + len(spans) + 1, int(sl.sum()) // 6 + len(spans) + 1
    d, arrs = Engine._host_outputs(cap, wcap)
    base = np.zeros(len(spans) + 1, np.uint64)
    st = lib.clg_decode_host(eng.handle, _np_ptr(buf), _np_ptr(so), _np_ptr(sl), len(spans), _lib.C.byref(d),
                             _np_ptr(base))
    nr, nw = d.n_rec, d.n_wide
    return (st, d.err_status, d.err_span, d.err_off, d.err_tag, nr, nw,
            {k: v[:nr if k in ("off", "tag", "v0") else nw].copy() for k, v in arrs.items()}, base.copy())


def check_spans_oracle(a, spans_b, key):
    rec0, recs = a[8], a[7]
    widx = recs["w_idx"].astype(np.int64)
    for s, b in enumerate(spans_b):
        st, rr, eo, _ = O.decode(b)
        lo, hi = int(rec0[s]), int(rec0[s + 1])
        assert hi - lo == len(rr["tag"]), (key, s, st)
        for f in ("off", "tag", "v0"):
            np.testing.assert_array_equal(recs[f][lo:hi], rr[f], err_msg=f"{key} span {s} {f}")
        w = (widx >= lo) & (widx < hi)
        np.testing.assert_array_equal(widx[w] - lo, rr["w_idx"].astype(np.int64), err_msg=f"{key} span {s} w_idx")
        for f in ("w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub"):
            np.testing.assert_array_equal(recs[f][w], rr[f], err_msg=f"{key} span {s} {f}")


def oracle_batch(spans_b):
    """O.decode of every span of a batch, once: what a decode of the batch must return -- each
    span's records up to its first error back to back, the wide rows' record indices moved to
    the batch's, the spans' record bases, and the first error of the lowest bad span (status,
    span, offset, tag; status 0 and span 0, offset -1 when every span is good)."""
    recs = {f: [] for f in REC_FIELDS + ("w_idx",) + WIDE_FIELDS}
    base, err = [0], None
    for s, b in enumerate(spans_b):
        st, rr, eo, et = O.decode(b)
        for f in REC_FIELDS + WIDE_FIELDS:
            recs[f].append(rr[f])
        recs["w_idx"].append(rr["w_idx"].astype(np.int64) + base[-1])
        base.append(base[-1] + len(rr["tag"]))
        if st != 0 and err is None:
            err = (st, s, eo, et)
    return {"recs": {f: np.concatenate(v) if v else np.zeros(0) for f, v in recs.items()},
            "base": np.array(base, np.uint64), "err": err, "spans": spans_b}


def check_batch_oracle(a, exp, key):
    """A raw decode result (`_raw_decode`'s tuple) against `oracle_batch`: the whole batch's
    arrays at once, which is every span's comparison of check_spans_oracle together with the
    record bases; on a difference, check_spans_oracle names the span."""
    recs, e = a[7], exp["recs"]
    same = a[5] == len(e["tag"]) and a[6] == len(e["w_idx"]) and np.array_equal(a[8], exp["base"])
    same = same and all(np.array_equal(recs[f], e[f]) for f in REC_FIELDS + WIDE_FIELDS)
    same = same and np.array_equal(recs["w_idx"].astype(np.int64), e["w_idx"])
    if not same:
        check_spans_oracle(a, exp["spans"], key)
        np.testing.assert_array_equal(a[8], exp["base"], err_msg=f"{key} span_rec_base")
        raise AssertionError(f"{key}: batch arrays differ from the oracle's")
    if exp["err"] is None:
        assert a[0] == 0 and a[1] == 0, (key, a[:5])
    else:
        assert a[0] != 0 and tuple(int(x) for x in a[1:5]) == exp["err"], (key, a[:5], exp["err"])


def as_raw(dec):
    """A DecodedBatch (decode_logs) in `_raw_decode`'s form."""
    recs = {f: getattr(dec, f) for f in REC_FIELDS + ("w_idx",) + WIDE_FIELDS}
    return (0, 0, 0, -1, 0, dec.n_rec, len(dec.w_idx), recs, np.asarray(dec.span_rec_base, np.uint64))
