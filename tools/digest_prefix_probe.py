"""Developer probe: prefix digests over config 2's logs (64 logs x 1 M records in 16 KiB
segments), beside the whole-log digest of the same ranges, timed by the engine's HIP events in
one process and alternating, so no variant finds the bytes any warmer than another:

  log_digest          clg_digest_logs
  prefix_one_cut      clg_digest_prefixes, one cut per log, at its end (the same rows)
  prefix_16_cuts      clg_digest_prefixes, 16 cuts per log at arbitrary places, none on a word
                      boundary, the last at the end

Writes profiles/digest_prefix_probe.json and prints it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (the engine binds torch's HIP runtime)
from clonos_amd import CausalLogID, Engine, digest_prefixes_host, synth  # noqa: E402

REPS = 10

n_logs, n_rec = int(os.environ.get("PROBE_LOGS", 64)), int(os.environ.get("PROBE_REC", 1_000_000))
rng = np.random.default_rng(synth.SEED_CONFIG2)
bufs = [synth.config2_log(n_rec, rng)[0] for _ in range(n_logs)]
seg = 16384
pool = sum(int(b.size) // seg + 2 for b in bufs) + 64
total = sum(int(b.size) for b in bufs)
crng = np.random.default_rng(7)
one = [np.array([b.size]) for b in bufs]
many = []
for b in bufs:
    c = np.sort(crng.integers(1, int(b.size) - 4, 15))
    c = c - c % 4 + 1 + np.arange(15) % 3  # residues 1, 2, 3: no cut on a word boundary
    many.append(np.concatenate([c, [b.size]]))
with Engine(segment_bytes=seg, pool_segments=pool, timing=True) as eng:
    logs = []
    for v, b in enumerate(bufs):
        lg = eng.open_log(CausalLogID.main(v))
        lg.processUpstreamDelta(b.tobytes(), 0, 1)
        logs.append(lg)
    h = np.array([lg.handle for lg in logs], np.uint32)
    ep = np.ones(n_logs, np.int64)
    ms = {"log_digest": [], "prefix_one_cut": [], "prefix_16_cuts": []}

    def timed(name, stat, call):
        eng.sync()
        eng.kernel_stats_reset()
        got = call()
        eng.sync()
        st = eng.kernel_stats()[stat]
        assert st["launches"] == 1 and st["bytes"] == total
        ms[name].append(st["ms"])
        return got

    for k in range(3 + REPS):
        if k == 3:
            ms = {name: [] for name in ms}
        dg = timed("log_digest", "log_digest", lambda: eng.digest_logs(h, ep))
        p1 = timed("prefix_one_cut", "log_digest_prefix", lambda: eng.digest_prefixes(h, ep, one)[0])
        p16 = timed("prefix_16_cuts", "log_digest_prefix", lambda: eng.digest_prefixes(h, ep, many)[0])
    assert (p1 == dg).all() and (p16[15::16] == dg).all()
    assert (p16[:16] == digest_prefixes_host(bufs[0], many[0])).all()  # (one log against the CPU)
    res = {"workload": f"config 2: {n_logs} logs x {n_rec} records, {total} bytes in {seg}-byte segments",
           "reps": REPS}
    for name, v in ms.items():
        res[name + "_ms"] = {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        res[name + "_tb_per_s"] = round(total / float(np.median(v)) / 1e9, 3)
    res["one_cut_over_log_digest"] = round(float(np.median(ms["prefix_one_cut"]) / np.median(ms["log_digest"])), 3)
    res["16_cuts_over_log_digest"] = round(float(np.median(ms["prefix_16_cuts"]) / np.median(ms["log_digest"])), 3)
    res["note"] = ("HIP-event time of all kernels of a call under one stat (two for log_digest, three for the "
                   "prefix digests); every call reads the same bytes once.")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "digest_prefix_probe.json"))
with open(dest, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
