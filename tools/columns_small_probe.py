"""Developer probe: the one-launch columns and payload kernels (k_col_small, k_pay_small) against
the multi-kernel pipelines, and replay preparation as columns against the SoA form.  One process,
the compared calls alternating, 20 repeats after 5 warm-up rounds, each figure as median
(min - max) of the host clock around a call that ends in a synchronise.

  (a) crossover   clg_columnize and clg_gather_payloads, device in and device out, at record / row
                  counts in powers of two from 1 Ki, through up to four libraries:
                    parent  the parent commit's library (PROBE_PARENT_LIB, default ab/libparent.so,
                            from `tools/ab_build.sh parent HEAD~1` or the like): the multi-kernel form
                    off     this tree's library with CLONOS_COLUMNS_SMALL=0: the same form, to confirm
                    on      this tree's library: the small path up to the constants in columns.h /
                            payload.h, the multi-kernel form past them
                    wide    (PROBE_WIDE_LIB, default ab/libwide.so) this tree built from a copy whose
                            kColSmallRecords / kPaySmallRows / kPaySmallBytes are raised past every
                            probed size (`tools/ab_build.sh wide <that copy>`): the small path at
                            every size, which is what sets the constants
                  A library that is not there is left out and reported as not measured.
  (b) replay-prep clg_replay_prepare (SoA) against clg_replay_prepare_columns with the small paths
                  on and off, into plain host arrays, on config 5's shape (16 main logs of ~45 KB,
                  4 subpartition buffers each) and config 1's epoch (44 main logs in ~73 KB); wall
                  time and bytes delivered.
  (c) host outputs  only one delivery for CLG_MEM_HOST was built (device scratch, one copy into
                  pinned memory after the result block is read): its time at config 5's size, host
                  outputs against device outputs.

Writes profiles/columns_small_probe.json and prints it."""
import ctypes as C
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (the engine binds torch's HIP runtime)
from clonos_amd import CausalLogID, Engine, _lib, synth  # noqa: E402
from clonos_amd.engine import _COL_FIELDS, _columns_struct, _payloads_struct  # noqa: E402
from clonos_amd.replay import DeterminantResponseEvent, accumulate, log_id_array  # noqa: E402

REPS, WARM = 20, 5
MAX_LOG2 = int(os.environ.get("PROBE_MAX_LOG2", 19))
PARENT = os.environ.get("PROBE_PARENT_LIB", os.path.join(ROOT, "ab", "libparent.so"))
WIDE = os.environ.get("PROBE_WIDE_LIB", os.path.join(ROOT, "ab", "libwide.so"))
P = C.c_void_p


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


class RawEngine:
    """An engine of any build of the library (ABI 6), for the two calls of line (a)."""

    def __init__(self, path, small=True):
        self.lib = lib = C.CDLL(path)
        lib.clg_config_default.argtypes = [C.POINTER(_lib.Config)]
        lib.clg_engine_create.argtypes = [C.POINTER(_lib.Config), C.POINTER(P)]
        lib.clg_engine_destroy.argtypes = [P]
        lib.clg_columnize.argtypes = [P, C.POINTER(_lib.Decoded), P, C.c_uint32, C.POINTER(_lib.Columns)]
        lib.clg_gather_payloads.argtypes = [P, P, P, P, C.c_uint32, P, P, P, C.c_uint32, C.POINTER(_lib.Payloads)]
        cfg = _lib.Config()
        lib.clg_config_default(C.byref(cfg))
        cfg.segment_bytes, cfg.pool_segments = 16384, 64
        cfg.ifl_segment_bytes, cfg.ifl_pool_segments = 16384, 64
        self.h = P()
        old = os.environ.get("CLONOS_COLUMNS_SMALL")
        if not small:
            os.environ["CLONOS_COLUMNS_SMALL"] = "0"
        try:
            assert lib.clg_engine_create(C.byref(cfg), C.byref(self.h)) == 0
        finally:
            if not small:
                if old is None:
                    del os.environ["CLONOS_COLUMNS_SMALL"]
                else:
                    os.environ["CLONOS_COLUMNS_SMALL"] = old

    def close(self):
        self.lib.clg_engine_destroy(self.h)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to("cuda")


def timed_rounds(calls):
    """calls: name -> callable; alternating, WARM rounds dropped; name -> list of ms."""
    ms = {k: [] for k in calls}
    for r in range(WARM + REPS):
        for k, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                ms[k].append(dt)
    return ms


def crossover_columns(engines, rng):
    rows = []
    for lg in range(10, MAX_LOG2 + 1):
        n = 1 << lg
        tag = rng.choice(np.arange(8, dtype=np.uint8), n, p=[.3, .3, .1, .02, .02, .03, .03, .2])
        v0 = rng.integers(-100, 100, n).astype(np.int64)
        w_idx = np.nonzero((tag >= 3) & (tag <= 6))[0].astype(np.uint32)
        nw = int(w_idx.size)
        src = [dev(tag), dev(v0), dev(w_idx)] + [torch.zeros(max(nw, 1) * w, dtype=torch.uint8, device="cuda")
                                                 for w in (4, 8, 4, 4, 1)]
        d = _lib.Decoded()
        d.tag, d.v0, d.w_idx, d.w_rc, d.w_v1, d.w_var_off, d.w_var_len, d.w_sub = [t.data_ptr() for t in src]
        d.n_rec, d.n_wide, d.cap, d.wcap, d.out_kind = n, nw, n, nw, _lib.CLG_MEM_DEVICE
        outs = {}
        for name in engines:
            widths = (1, 1, 8, 4, 4, 4, 4, 8, 4, 4, 1, 8)
            bufs = [torch.zeros(max(n, 1) * w, dtype=torch.uint8, device="cuda") for w in widths]
            c = _lib.Columns()
            for f, b in zip(("tag", "order", "timestamp", "rng", "buffer_built", "w_idx", "w_rc", "w_v1", "w_var_off",
                             "w_var_len", "w_sub", "w_v0"), bufs):
                setattr(c, f, b.data_ptr())
            c.cap_tag = c.cap_order = c.cap_timestamp = c.cap_rng = c.cap_buffer_built = c.cap_wide = n
            sb = np.zeros(10, np.uint64)
            c.span_base, c.out_kind = sb.ctypes.data, _lib.CLG_MEM_DEVICE
            outs[name] = (c, bufs, sb)
        base = np.array([0, n], np.uint64)

        def call(name):
            e = engines[name]
            assert e.lib.clg_columnize(e.h, C.byref(d), base.ctypes.data, 1, C.byref(outs[name][0])) == 0

        ms = timed_rounds({name: (lambda name=name: call(name)) for name in engines})
        ref = next(iter(engines))
        for name in engines:  # the results agree
            for a, b in zip(outs[name][1], outs[ref][1]):
                assert torch.equal(a, b), (n, name)
            assert (outs[name][2] == outs[ref][2]).all()
        rows.append({"records": n, "wide": nw, **{f"{k}_ms": spread(v) for k, v in ms.items()}})
    return rows


def crossover_payloads(engines, rng):
    rows = []
    span = 1 << 17  # (at most kPaySmallBytes, so that `on` takes the small path up to kPaySmallRows)
    data = dev(rng.integers(0, 256, span, dtype=np.uint8))
    for lg in range(10, MAX_LOG2 + 1):
        n = 1 << lg
        wl = rng.integers(0, 48, n).astype(np.uint32)
        wl[rng.random(n) < 0.1] = 200
        wo = rng.integers(0, span - 200, n).astype(np.uint32)
        nv = int(wl.sum())
        d_wo, d_wl = dev(wo), dev(wl)
        so, sl, rb = np.array([0], np.uint64), np.array([span], np.uint64), np.array([0, n], np.uint64)
        outs = {}
        for name in engines:
            var = torch.zeros(nv + 1, dtype=torch.uint8, device="cuda")
            pos = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            p = _lib.Payloads()
            p.var, p.pos, p.cap_var, p.cap_pos, p.out_kind = var.data_ptr(), pos.data_ptr(), nv, n + 1, _lib.CLG_MEM_DEVICE
            outs[name] = (p, var, pos)

        def call(name):
            e = engines[name]
            assert e.lib.clg_gather_payloads(e.h, data.data_ptr(), so.ctypes.data, sl.ctypes.data, 1, d_wo.data_ptr(),
                                             d_wl.data_ptr(), rb.ctypes.data, _lib.CLG_MEM_DEVICE,
                                             C.byref(outs[name][0])) == 0

        ms = timed_rounds({name: (lambda name=name: call(name)) for name in engines})
        ref = next(iter(engines))
        for name in engines:
            assert torch.equal(outs[name][1], outs[ref][1]) and torch.equal(outs[name][2], outs[ref][2]), (n, name)
        rows.append({"rows": n, "payload_bytes": nv, "span_bytes": span, **{f"{k}_ms": spread(v) for k, v in ms.items()}})
    return rows


def bb(rng, n):
    return b"".join(b"\x07" + struct.pack(">i", int(x)) for x in rng.integers(1, 1 << 20, n))


def replay_jobs(rng, n_vertices, main_bytes, n_sub, sub_records):
    per = len(synth.config3_epoch(1000, rng)[0]) / 1000.0
    jobs = []
    for v in range(n_vertices):
        ev = DeterminantResponseEvent(True, v)
        ev.put(CausalLogID.main(v), synth.config3_epoch(int(main_bytes / per), rng)[0].tobytes())
        subs = [CausalLogID.sub(v, 7, 8, j) for j in range(n_sub)]
        for s in subs:
            ev.put(s, bb(rng, sub_records))
        jobs.append((v, accumulate(v, [ev]), log_id_array(subs)))
    return jobs


def replay_prep(name, jobs, eng_on, eng_off):
    n = len(jobs)
    vs = (_lib.ReplayVertex * n)()
    main_bytes = sub_bytes = n_sub = 0
    for i, (vid, acc, t) in enumerate(jobs):
        vs[i] = _lib.ReplayVertex(C.pointer(acc._c), C.cast(t.ctypes.data, C.POINTER(_lib.CausalLogIdC)), len(t), vid, 0)
        e = acc.entries()
        mb = int(e["len"][e["id"]["is_main"] != 0].sum())
        main_bytes += mb
        sub_bytes += int(e["len"].sum()) - mb
        n_sub += len(t)
    sizes = np.empty(max(1, sub_bytes // 5), np.int32)
    sub = [np.zeros(n_sub + 1, np.uint64), np.zeros(max(1, n_sub), np.uint64), np.zeros(max(1, n_sub), np.int32),
           np.zeros(max(1, n_sub), np.int64), np.zeros(max(1, n_sub), np.int32)]
    sub_args = [sizes.ctypes.data, sizes.size] + [a.ctypes.data for a in sub]
    # SoA outputs
    cap, wcap = main_bytes // 2 + n + 1, main_bytes // 6 + n + 1
    soa = [np.empty(cap, t) for t in (np.uint32, np.uint8, np.int64)] + \
          [np.empty(wcap, t) for t in (np.uint32, np.int32, np.int64, np.uint32, np.uint32, np.uint8)]
    d = _lib.Decoded()
    d.off, d.tag, d.v0, d.w_idx, d.w_rc, d.w_v1, d.w_var_off, d.w_var_len, d.w_sub = [a.ctypes.data for a in soa]
    d.cap, d.wcap, d.out_kind = cap, wcap, _lib.CLG_MEM_HOST
    rec_base = np.zeros(n + 1, np.uint64)
    o_soa = _lib.ReplayOut(C.pointer(d), rec_base.ctypes.data, *sub_args)
    # columns outputs
    arrs = Engine._column_bounds(main_bytes, n)
    base = np.zeros((n + 1) * 5, np.uint64)
    c = _columns_struct(arrs, base, _lib.CLG_MEM_HOST)
    var, pos = Engine._payload_bounds(main_bytes, n)
    p = _payloads_struct(var, pos)
    o_col = _lib.ReplayColumnsOut(C.pointer(c), C.pointer(p), *sub_args)

    L = _lib.lib
    calls = {
        "soa": lambda: _lib.check(L.clg_replay_prepare(eng_on.handle, vs, n, C.byref(o_soa))),
        "columns_small_on": lambda: _lib.check(L.clg_replay_prepare_columns(eng_on.handle, vs, n, C.byref(o_col))),
        "columns_small_off": lambda: _lib.check(L.clg_replay_prepare_columns(eng_off.handle, vs, n, C.byref(o_col))),
    }
    ms = timed_rounds(calls)
    nc = [int(x) for x in c.n_class]
    col_bytes = int(c.n_rec) + nc[0] + 8 * nc[1] + 4 * nc[2] + 4 * nc[3] + 33 * nc[4]
    st = eng_on.kernel_stats()
    return {"workload": f"{name}: {n} main logs, {main_bytes} bytes, {n_sub} subpartition buffers, {sub_bytes} bytes",
            "records": int(d.n_rec), "wide_rows": int(d.n_wide),
            "soa_bytes_delivered": 13 * int(d.n_rec) + 25 * int(d.n_wide),
            "columns_bytes_delivered": col_bytes + int(p.n_var) + 8 * (int(p.n_rows) + 1),
            "took_columns_small": "columns_small" in st, "took_payloads_small": "payloads_small" in st,
            **{f"{k}_ms": spread(v) for k, v in ms.items()}}


def host_outputs(eng_on, rng, n):
    """clg_columnize of n records on the small path: device outputs against host outputs."""
    tag = rng.choice(np.arange(8, dtype=np.uint8), n, p=[.3, .3, .1, .02, .02, .03, .03, .2])
    w_idx = np.nonzero((tag >= 3) & (tag <= 6))[0].astype(np.uint32)
    nw = int(w_idx.size)
    src = [dev(tag), dev(rng.integers(-100, 100, n).astype(np.int64)), dev(w_idx)] + \
          [torch.zeros(max(nw, 1) * w, dtype=torch.uint8, device="cuda") for w in (4, 8, 4, 4, 1)]
    d = _lib.Decoded()
    d.tag, d.v0, d.w_idx, d.w_rc, d.w_v1, d.w_var_off, d.w_var_len, d.w_sub = [t.data_ptr() for t in src]
    d.n_rec, d.n_wide, d.cap, d.wcap, d.out_kind = n, nw, n, nw, _lib.CLG_MEM_DEVICE
    base = np.array([0, n], np.uint64)
    arrs = {k: np.empty(n + 1, dt) for k, dt in _COL_FIELDS}
    ch = _columns_struct(arrs, np.zeros(10, np.uint64), _lib.CLG_MEM_HOST)
    widths = (1, 1, 8, 4, 4, 4, 4, 8, 4, 4, 1, 8)
    bufs = [torch.zeros(n * w, dtype=torch.uint8, device="cuda") for w in widths]
    cd = _lib.Columns()
    for f, b in zip(("tag", "order", "timestamp", "rng", "buffer_built", "w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len",
                     "w_sub", "w_v0"), bufs):
        setattr(cd, f, b.data_ptr())
    cd.cap_tag = cd.cap_order = cd.cap_timestamp = cd.cap_rng = cd.cap_buffer_built = cd.cap_wide = n
    cd.out_kind = _lib.CLG_MEM_DEVICE
    L = _lib.lib
    ms = timed_rounds({
        "device_out": lambda: _lib.check(L.clg_columnize(eng_on.handle, C.byref(d), base.ctypes.data, 1, C.byref(cd))),
        "host_out_scratch_plus_one_copy": lambda: _lib.check(L.clg_columnize(eng_on.handle, C.byref(d), base.ctypes.data, 1,
                                                                             C.byref(ch))),
    })
    return {"records": n, "registered_host_memory_written_by_the_kernel": "not built, not measured",
            **{f"{k}_ms": spread(v) for k, v in ms.items()}}


def main():
    rng = np.random.default_rng(synth.SEED_CONFIG2)
    res = {"reps": REPS, "warmup_rounds": WARM,
           "note": "host clock around synchronous calls, the compared calls alternating in one process"}
    engines = {}
    if os.path.exists(PARENT):
        engines["parent"] = RawEngine(PARENT)
    else:
        res["parent"] = f"not measured: {os.path.relpath(PARENT, ROOT)} is not there"
    engines["off"] = RawEngine(_lib.LIB_PATH, small=False)
    engines["on"] = RawEngine(_lib.LIB_PATH)
    if os.path.exists(WIDE):
        engines["wide"] = RawEngine(WIDE)
    else:
        res["wide"] = f"not measured: {os.path.relpath(WIDE, ROOT)} is not there"
    res["a_crossover_columns"] = crossover_columns(engines, rng)
    res["a_crossover_payloads"] = crossover_payloads(engines, rng)
    for e in engines.values():
        e.close()

    eng_on = Engine(segment_bytes=16384, pool_segments=256, timing=True)
    os.environ["CLONOS_COLUMNS_SMALL"] = "0"
    eng_off = Engine(segment_bytes=16384, pool_segments=256, timing=True)
    del os.environ["CLONOS_COLUMNS_SMALL"]
    res["b_replay_prep"] = [
        replay_prep("config 5", replay_jobs(rng, 16, 45_000, 4, 200), eng_on, eng_off),
        replay_prep("config 1 epoch", replay_jobs(rng, 44, 73_000 // 44, 1, 20), eng_on, eng_off),
    ]
    res["c_host_outputs"] = host_outputs(eng_on, rng, 1 << 15)
    eng_on.close()
    eng_off.close()

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "columns_small_probe.json"))
    with open(dest, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
