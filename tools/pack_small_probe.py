"""Developer probe: the one-launch pack (k_pack_small) against the multi-kernel forms, and replay
preparation as packed columns against its SoA and plain-columns forms.  One process, the compared
calls alternating, 20 repeats after 5 warm-up rounds, each figure as median (min - max) of the host
clock around a call that ends in a synchronise.

  (a) crossover   clg_pack_columns at 1 Ki .. 64 Ki values of config 2's mix and clg_pack_wide at
                  1 Ki .. 16 Ki rows of config 3's mix, device in and device out, through up to four
                  libraries:
                    parent  the parent commit's library (PROBE_PARENT_LIB, default ab/libparent.so,
                            from `tools/ab_build.sh parent`): the multi-kernel forms
                    off     this tree's library with CLONOS_PACK_SMALL=0: the same forms, to confirm
                    on      this tree's library: the one launch up to the constants in pack.h /
                            pack_wide.h, the multi-kernel forms past them
                    wide    (PROBE_WIDE_LIB, default ab/libwide.so) this tree built from a copy whose
                            kPackSmallBlocks / kWPackSmallRows are raised past every probed size: the
                            one launch at every size, which is what sets the constants
                  A library that is not there is left out and reported as not measured.
  (b) the call    clg_replay_prepare, clg_replay_prepare_columns and the packed-wide call with the
                  form on and off, into plain host arrays, on config 1's epoch and on config 5's
                  replay-prep shape (16 main logs of ~45 KB): wall time and bytes delivered.

Writes profiles/pack_small_probe.json and prints it."""
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
from clonos_amd import CausalLogID, Engine, _lib, columnize_host, synth  # noqa: E402
from clonos_amd.engine import PACK_BLOCK, _columns_struct, _packed_struct, _packed_wide_struct, _payloads_struct  # noqa: E402
from clonos_amd.replay import DeterminantResponseEvent, accumulate, log_id_array  # noqa: E402

REPS, WARM = 20, 5
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
        lib.clg_pack_columns.argtypes = [P, C.POINTER(_lib.Columns), C.POINTER(_lib.Packed)]
        lib.clg_pack_wide.argtypes = [P, C.POINTER(_lib.Columns), C.POINTER(_lib.PackedWideC)]
        cfg = _lib.Config()
        lib.clg_config_default(C.byref(cfg))
        cfg.segment_bytes, cfg.pool_segments = 16384, 64
        cfg.ifl_segment_bytes, cfg.ifl_pool_segments = 16384, 64
        self.h = P()
        old = os.environ.get("CLONOS_PACK_SMALL")
        if not small:
            os.environ["CLONOS_PACK_SMALL"] = "0"
        try:
            assert lib.clg_engine_create(C.byref(cfg), C.byref(self.h)) == 0
        finally:
            if not small:
                if old is None:
                    del os.environ["CLONOS_PACK_SMALL"]
                else:
                    os.environ["CLONOS_PACK_SMALL"] = old

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


def columns_of(data):
    """The plain columns of encoded log bytes, on the host (the CPU oracle's decode)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _columns_util import oracle_batch
    return columnize_host(oracle_batch([bytes(data)]))


NARROW = ("tag", "order", "timestamp", "rng", "buffer_built")
WIDE_ROWS = ("w_idx", "w_rc", "w_v1", "w_var_off", "w_var_len", "w_sub", "w_v0")


def crossover(engines, cols, wide, sizes):
    """clg_pack_columns (wide: clg_pack_wide) of the first n values / rows of cols, device in and out."""
    rows = []
    for n in sizes:
        c = _lib.Columns()
        keep = []
        if wide:
            names, total = ("tag",) + WIDE_ROWS, len(cols.w_idx)
            if n > total:
                break
            c.n_rec, c.n_class[4] = len(cols.tag), n
        else:
            names, total = NARROW, len(cols.tag)
            if n > total:
                break
            c.n_rec = n  # the classes' shares of the first n records
            t = np.asarray(cols.tag[:n])
            for k, cls in enumerate(((t == 0), (t == 1), (t == 2), (t == 7))):
                c.n_class[k] = int(cls.sum())
        for name in names:
            a = np.asarray(getattr(cols, name))
            a = a if name == "tag" and wide else a[:n]
            keep.append(dev(a) if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda"))
            setattr(c, name, keep[-1].data_ptr())
        c.out_kind = _lib.CLG_MEM_DEVICE
        outs = {}
        for name in engines:
            desc = torch.zeros(32 * (8 * (n // 1024) + 64), dtype=torch.uint8, device="cuda")
            bits = torch.zeros(40 * n + 4096, dtype=torch.uint8, device="cuda")
            p = (_lib.PackedWideC if wide else _lib.Packed)()
            p.desc, p.bits, p.cap_desc, p.cap_bits, p.out_kind = desc.data_ptr(), bits.data_ptr(), desc.numel() // 32, bits.numel(), 1
            outs[name] = (p, desc, bits)

        def call(name):
            e = engines[name]
            f = e.lib.clg_pack_wide if wide else e.lib.clg_pack_columns
            assert f(e.h, C.byref(c), C.byref(outs[name][0])) == 0

        ms = timed_rounds({name: (lambda name=name: call(name)) for name in engines})
        ref = next(iter(engines))
        for name in engines:  # the results agree, byte for byte
            assert torch.equal(outs[name][1], outs[ref][1]) and torch.equal(outs[name][2], outs[ref][2]), (n, name)
        p = outs[ref][0]
        rows.append({"rows" if wide else "values": n, "blocks": int(p.blk_base[len(p.n_val)]), "payload_bytes": int(p.n_bits),
                     **{f"{k}_ms": spread(v) for k, v in ms.items()}})
    return rows


def bb(rng, n):
    return b"".join(b"\x07" + struct.pack(">i", int(x)) for x in rng.integers(1, 1 << 20, n))


def config5_jobs(rng):
    per = len(synth.config3_epoch(1000, rng)[0]) / 1000.0
    jobs = []
    for v in range(16):
        ev = DeterminantResponseEvent(True, v)
        ev.put(CausalLogID.main(v), synth.config3_epoch(int(45_000 / per), rng)[0].tobytes())
        subs = [CausalLogID.sub(v, 7, 8, j) for j in range(4)]
        for s in subs:
            ev.put(s, bb(rng, 200))
        jobs.append((v, accumulate(v, [ev]), log_id_array(subs)))
    return jobs


def config1_jobs(rng):
    _, logs = synth.config1_job(rng)
    by_vertex = {}
    for lid, data in logs.items():
        by_vertex.setdefault(lid.vertex_id, []).append((lid, bytes(data)))
    jobs = []
    for v, held in sorted(by_vertex.items()):
        ev = DeterminantResponseEvent(True, v)
        for lid, data in held:
            ev.put(lid, data)
        jobs.append((v, accumulate(v, [ev]), log_id_array([lid for lid, _ in held if not lid.is_main])))
    return jobs


def the_call(name, jobs, eng_on, eng_off):
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
    cap, wcap = main_bytes // 2 + n + 1, main_bytes // 6 + n + 1
    soa = [np.empty(cap, t) for t in (np.uint32, np.uint8, np.int64)] + \
          [np.empty(wcap, t) for t in (np.uint32, np.int32, np.int64, np.uint32, np.uint32, np.uint8)]
    d = _lib.Decoded()
    d.off, d.tag, d.v0, d.w_idx, d.w_rc, d.w_v1, d.w_var_off, d.w_var_len, d.w_sub = [a.ctypes.data for a in soa]
    d.cap, d.wcap, d.out_kind = cap, wcap, _lib.CLG_MEM_HOST
    rec_base = np.zeros(n + 1, np.uint64)
    o_soa = _lib.ReplayOut(C.pointer(d), rec_base.ctypes.data, *sub_args)
    arrs = Engine._column_bounds(main_bytes, n)
    base = np.zeros((n + 1) * 5, np.uint64)
    c = _columns_struct(arrs, base, _lib.CLG_MEM_HOST)
    var, pos = Engine._payload_bounds(main_bytes, n)
    p = _payloads_struct(var, pos)
    o_col = _lib.ReplayColumnsOut(C.pointer(c), C.pointer(p), *sub_args)
    # the packed-wide outputs, sized as Engine._decode_packed sizes them
    rows = main_bytes // 6 + n + 1
    desc, wdesc = np.empty(main_bytes // 1024 + 5, PACK_BLOCK), np.empty(8 * (rows // 1024) + _lib.WPACK_STREAMS, PACK_BLOCK)
    bits, wbits = np.empty(main_bytes + 16 * desc.size, np.uint8), np.empty(35 * rows + 16 * wdesc.size, np.uint8)
    pk, wpk = _packed_struct(desc, bits), _packed_wide_struct(wdesc, wbits)
    base2 = np.zeros((n + 1) * 5, np.uint64)
    sz = _lib.Columns()
    sz.span_base, sz.out_kind = base2.ctypes.data, _lib.CLG_MEM_HOST
    var2, _ = Engine._payload_bounds(main_bytes, n)
    p2 = _payloads_struct(var2, None)
    o_pk = _lib.ReplayPackedOut(C.pointer(sz), C.pointer(p2), C.pointer(pk), C.pointer(wpk), *sub_args)

    L = _lib.lib
    calls = {
        "soa": lambda: _lib.check(L.clg_replay_prepare(eng_on.handle, vs, n, C.byref(o_soa))),
        "columns": lambda: _lib.check(L.clg_replay_prepare_columns(eng_on.handle, vs, n, C.byref(o_col))),
        "packed_wide_on": lambda: _lib.check(L.clg_replay_prepare_columns_packed(eng_on.handle, vs, n, C.byref(o_pk))),
        "packed_wide_off": lambda: _lib.check(L.clg_replay_prepare_columns_packed(eng_off.handle, vs, n, C.byref(o_pk))),
    }
    eng_on.kernel_stats_reset()
    ms = timed_rounds(calls)
    nc = [int(x) for x in c.n_class]
    st = eng_on.kernel_stats()
    return {"workload": f"{name}: {n} main logs, {main_bytes} bytes, {n_sub} subpartition buffers, {sub_bytes} bytes",
            "records": int(d.n_rec), "wide_rows": int(d.n_wide), "narrow_blocks": int(pk.blk_base[5]),
            "soa_bytes_delivered": 13 * int(d.n_rec) + 25 * int(d.n_wide),
            "columns_bytes_delivered": int(c.n_rec) + nc[0] + 8 * nc[1] + 4 * nc[2] + 4 * nc[3] + 33 * nc[4] + int(p.n_var)
            + 8 * (int(p.n_rows) + 1),
            "packed_wide_bytes_delivered": 32 * int(pk.blk_base[5]) + int(pk.n_bits) + 32 * int(wpk.blk_base[26])
            + int(wpk.n_bits) + int(p2.n_var),
            "took_pack_small": st.get("pack_small", {"launches": 0})["launches"] > 0,
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
    c2 = columns_of(synth.config2_log(1 << 16, rng)[0])
    c3 = columns_of(synth.config3_epoch(1 << 16, rng)[0])
    res["a_crossover_narrow"] = crossover(engines, c2, False, [1 << k for k in range(10, 17)])
    res["a_crossover_wide"] = crossover(engines, c3, True, [1 << k for k in range(10, 15)])
    for e in engines.values():
        e.close()

    eng_on = Engine(segment_bytes=16384, pool_segments=256, timing=True)
    os.environ["CLONOS_PACK_SMALL"] = "0"
    eng_off = Engine(segment_bytes=16384, pool_segments=256, timing=True)
    del os.environ["CLONOS_PACK_SMALL"]
    res["b_the_call"] = [the_call("config 1 epoch", config1_jobs(rng), eng_on, eng_off),
                         the_call("config 5", config5_jobs(rng), eng_on, eng_off)]
    eng_on.close()
    eng_off.close()

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "pack_small_probe.json"))
    with open(dest, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
