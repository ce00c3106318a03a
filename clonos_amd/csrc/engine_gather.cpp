// engine_gather.cpp -- reading log bytes back: slices and getDeterminants through the gather
// kernels (pieces, run plans and their staging), the staging of caller spans, and what reads
// the same runs: the log digests and the comparison of two copies of a log.
#include "engine_impl.h"
#include "diff.h"
#include "digest.h"
#include "slice_order.h"

// Pieces of [phys, phys+n) of a log, split at segment boundaries.
void clg_engine::add_pieces(const Log& l, int32_t phys, int32_t n, uint64_t dst, std::vector<clg::GatherPiece>& out) {
  while (n > 0) {
    const uint32_t si = uint32_t(phys) / C(), so = uint32_t(phys) % C();
    const uint32_t take = std::min<uint32_t>(uint32_t(n), C() - so);
    out.push_back(clg::GatherPiece{seg_addr(l.segs[si]) + so, dst, take, 0});
    phys += int32_t(take);
    dst += take;
    n -= int32_t(take);
  }
}

int clg_engine::run_gather(const std::vector<clg::GatherPiece>& pieces, uint64_t total, void* out, uint32_t out_kind,
                           const char* stat, bool wait) {
  if (pieces.empty()) return CLG_OK;
  const size_t db = pieces.size() * sizeof(clg::GatherPiece);
  CHK(h_desc.ensure(db));
  CHK(d_desc.ensure(db));
  memcpy(h_desc.p, pieces.data(), db);
  HIPCHK(hipMemcpyAsync(d_desc.p, h_desc.p, db, hipMemcpyHostToDevice, stream));
  return gather_out(out, out_kind, total, stat, wait, [&](uint8_t* dout) {
    return clg::launch_gather(d_desc.as<clg::GatherPiece>(), uint32_t(pieces.size()), dout, stream);
  });
}

// A run plan on the device.  The descriptors, staged through s.h into s.d on `on`:
// runs | segment table | `extra_bytes` of the caller's at the next 16-byte boundary; then the
// pieces, expanded on the device into s.pieces.
// (Tried and removed: pieces in source order -- every consumer's piece of one segment back
// to back on one XCD, for L2 hits -- took the isolated config-2 gather from 0.39 to 0.43 ms
// and cost 0.1 ms of host grouping per step.  Round 5: a segment-major gather, one block per
// log segment copying it for every consumer of that log (each segment read from HBM once):
// in the config-2 step the gather fell from 0.68 to 0.54 ms but the decode beside it rose
// from 0.62 to 0.75 and the step from 0.732 to 0.786 ms; isolated 0.46 against 0.39 ms.
// Kept: the same pieces with a log's consumers ordered window by window (slice_order.h),
// k_gather as it is.  At 128 segments per window the gather fetches 0.32 GB per launch
// instead of 0.84, the 0.31 GB minimum nearly, with the writes unchanged; alone it still
// takes 0.39 ms, so the re-reads are not what bounds the gather itself, which writes 1.4 GB
// in that time whatever it reads; in the step, beside the decode's traffic, they cost about
// 2 % (0.723 against 0.737 ms).  Windows of 16 segments and fewer fetch as little and are
// slower alone (0.41, 0.43 ms): DESIGN.md section 7, "A windowed order".)
int clg_engine::stage_run_plan(const RunPlan& p, DescSet s, hipStream_t on, StagedPlan* sp, const void* extra,
                               size_t extra_bytes) {
  const size_t rb = p.runs.size() * sizeof(clg::SegSpan), o_tab = al16(rb), tb = p.segtab.size() * 4;
  const size_t o_extra = extra_bytes ? al16(o_tab + tb) : o_tab + tb, hb = o_extra + extra_bytes;
  CHK(s.h.ensure(hb));
  CHK(s.d.ensure(hb));
  CHK(s.pieces.ensure(size_t(p.n_pieces) * sizeof(clg::GatherPiece)));
  uint8_t* h = s.h.as<uint8_t>();
  memcpy(h, p.runs.data(), rb);
  memcpy(h + o_tab, p.segtab.data(), tb);
  if (extra_bytes) memcpy(h + o_extra, extra, extra_bytes);
  HIPCHK(hipMemcpyAsync(s.d.p, h, hb, hipMemcpyHostToDevice, on));
  const uint8_t* d = s.d.as<uint8_t>();
  *sp = StagedPlan{s.d.as<clg::SegSpan>(), s.pieces.as<clg::GatherPiece>(), d + o_extra};
  return clg::launch_expand_pieces(sp->runs, uint32_t(p.runs.size()), p.n_pieces,
                                   reinterpret_cast<const uint32_t*>(d + o_tab), pool, C(), s.pieces.as<clg::GatherPiece>(), on);
}

// Batched gather from runs: pieces are generated on the device (k_expand_pieces).
int clg_engine::run_gather_runs(const RunPlan& p, void* out, uint32_t out_kind) {
  if (p.runs.empty() || !p.n_pieces) return CLG_OK;
  if (out_kind == CLG_MEM_DEVICE && (cfg.flags & CLG_F_ASYNC_SLICE)) return gather_runs_async(p, out);
  StagedPlan sp;
  CHK(stage_run_plan(p, DescSet{h_desc, d_desc, d_pieces}, stream, &sp));
  return gather_out(out, out_kind, p.total, "slice_gather", true,
                    [&](uint8_t* dout) { return clg::launch_gather(sp.pieces, p.n_pieces, dout, stream); });
}

// getDeterminants(start_epoch[i]) of log[i] as runs (clg_get_determinants_batch,
// clg_digest_logs, clg_diff_logs): run i's output offset is its place in the packed order,
// its pad the request index; len[i] / out_off[i] (optional) per request.
int clg_engine::plan_determinant_runs(const uint32_t* log, const int64_t* start_epoch, uint32_t n, uint32_t* len,
                                      uint64_t* out_off, RunPlan& p) {
  for (uint32_t i = 0; i < n; ++i) {
    Log* l;
    CHK(get_log(log[i], &l));
    int32_t s = 0, nb = 0;
    if (l->depth != 0) CHK(determinants_range(*l, start_epoch[i], &s, &nb));
    if (len) len[i] = uint32_t(nb);
    if (out_off) out_off[i] = p.total;
    p.add(log[i], s, nb, i);
  }
  return CLG_OK;
}

// Spans [off[i], off[i] + len[i]) of `bytes` for a kernel: span i starts at
// *base + (off[i] - *base_off).  Device memory is read in place; of host memory the range
// [lo, hi) that covers the non-empty spans is staged through h_stage into d_stage (queued on
// `stream`), with 16 guard bytes for the kernels' aligned loads.
int clg_engine::stage_spans(const uint8_t* bytes, const uint64_t* off, const uint64_t* len, uint32_t n, uint32_t in_kind,
                            const uint8_t** base, uint64_t* base_off) {
  *base = bytes;
  *base_off = 0;
  if (in_kind != CLG_MEM_HOST) return CLG_OK;
  uint64_t lo = UINT64_MAX, hi = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (len[i] == 0) continue;
    lo = std::min(lo, off[i]);
    hi = std::max(hi, off[i] + len[i]);
  }
  if (lo == UINT64_MAX) lo = hi = 0;
  CHK(d_stage.ensure(hi - lo + 16));
  CHK(h_stage.ensure(hi - lo + 16));
  if (hi > lo) {
    memcpy(h_stage.p, bytes + lo, hi - lo);
    HIPCHK(hipMemcpyAsync(d_stage.p, h_stage.p, hi - lo, hipMemcpyHostToDevice, stream));
  }
  *base = d_stage.as<uint8_t>();
  *base_off = lo;
  return CLG_OK;
}

// The digest kernels' constant table, uploaded once.
int clg_engine::ensure_dgtab() {
  if (dgtab_ready) return CLG_OK;
  uint64_t tab[clg::kDigestTabWords];
  clg::digest_table(tab);
  CHK(d_dgtab.ensure(sizeof(tab)));
  HIPCHK(hipMemcpy(d_dgtab.p, tab, sizeof(tab), hipMemcpyHostToDevice));
  dgtab_ready = true;
  return CLG_OK;
}

// Prefix digests (clg_digest_prefixes, clg_digest_epochs; digest.h): request i's cuts are
// cuts[first[i] .. first[i + 1]), first[0] = 0, already checked not to decrease; a row per cut
// into out.  Each non-empty stretch between two clamped cuts is one run (pad: its cut), so a
// request's bytes up to its largest cut are read once; empty stretches live only in the
// chain's per-cut table.  Staged behind the plan: first | cut table | lead-ins.
int clg_engine::digest_prefixes(const uint32_t* log, const int64_t* start_epoch, uint32_t n, const uint64_t* first,
                                const uint32_t* cuts, clg_digest* out) {
  const uint64_t K = first[n];
  if (!K) return CLG_OK;
  if (K >> 32) return fail(CLG_E_INVALID_ARG, "%llu cuts in one call", (unsigned long long)K);
  RunPlan p(*this, uint32_t(K));
  std::vector<clg::PrefixCut> tab(K);
  std::vector<uint32_t> lead;
  lead.reserve(K);
  uint64_t most = 0;
  for (uint32_t i = 0; i < n; ++i) {
    Log* l;
    CHK(get_log(log[i], &l));
    int32_t s = 0, nb = 0;
    if (l->depth != 0) CHK(determinants_range(*l, start_epoch[i], &s, &nb));
    most = std::max(most, first[i + 1] - first[i]);
    uint32_t prev = 0;
    for (uint64_t k = first[i]; k < first[i + 1]; ++k) {
      const uint32_t c = std::min(cuts[k], uint32_t(nb));
      tab[k] = clg::PrefixCut{clg::dg_words(c) - clg::dg_words(prev), c, clg::kPrefixNoSlot, 0};
      if (c > prev) {
        tab[k].slot = uint32_t(p.runs.size());
        lead.push_back(prev & 3u);
        p.add(log[i], s + int32_t(prev), int32_t(c - prev), uint32_t(k));
        prev = c;
      }
    }
  }
  if (p.runs.empty()) {  // every clamped cut is 0
    memset(out, 0, size_t(K) * sizeof(clg_digest));
    return CLG_OK;
  }
  CHK(flush());
  const size_t fb = size_t(n + 1) * 8, cb = size_t(K) * sizeof(clg::PrefixCut), lb = lead.size() * 4;
  std::vector<uint8_t> extra(fb + cb + lb);
  memcpy(extra.data(), first, fb);
  memcpy(extra.data() + fb, tab.data(), cb);
  memcpy(extra.data() + fb + cb, lead.data(), lb);
  StagedPlan sp;
  CHK(stage_run_plan(p, DescSet{h_desc, d_desc, d_pieces}, stream, &sp, extra.data(), extra.size()));
  CHK(ensure_dgtab());
  const uint32_t n_runs = uint32_t(p.runs.size());
  CHK(d_dgpart.ensure(size_t(p.n_pieces) * 8 + 8));
  CHK(d_dgsum.ensure(size_t(n_runs) * 8));
  CHK(d_dgout.ensure(size_t(K) * sizeof(clg_digest)));
  CHK(h_dgout.ensure(size_t(K) * sizeof(clg_digest)));
  CHK(timed("log_digest_prefix", p.total, [&] {
    return clg::launch_digest_prefixes(
        sp.pieces, p.n_pieces, sp.runs, n_runs, reinterpret_cast<const uint32_t*>(sp.extra + fb + cb),
        reinterpret_cast<const uint64_t*>(sp.extra), n, reinterpret_cast<const clg::PrefixCut*>(sp.extra + fb),
        most <= clg::kPrefixFewCuts, d_dgtab.as<uint64_t>(), d_dgpart.as<uint64_t>(), d_dgsum.as<uint64_t>(),
        d_dgout.as<clg_digest>(), stream);
  }));
  HIPCHK(hipMemcpyAsync(h_dgout.p, d_dgout.p, size_t(K) * sizeof(clg_digest), hipMemcpyDeviceToHost, stream));
  CHK(sync());
  memcpy(out, h_dgout.p, size_t(K) * sizeof(clg_digest));
  return CLG_OK;
}

// The digest of every run (digest.hip), `n` results read back into out: out[run.pad] for a
// run, {0, 0} for a request without one.  d_runs / d_pc: the runs and their pieces on the
// device, queued on `stream`.
int clg_engine::run_digest(const clg::SegSpan* d_runs, uint32_t n_runs, const clg::GatherPiece* d_pc, uint32_t n_pieces,
                           uint64_t bytes, uint32_t n, clg_digest* out) {
  CHK(ensure_dgtab());
  CHK(d_dgpart.ensure(size_t(n_pieces) * 8 + 8));
  CHK(d_dgout.ensure(size_t(n) * sizeof(clg_digest)));
  CHK(h_dgout.ensure(size_t(n) * sizeof(clg_digest)));
  HIPCHK(hipMemsetAsync(d_dgout.p, 0, size_t(n) * sizeof(clg_digest), stream));
  CHK(timed("log_digest", bytes, [&] {
    return clg::launch_digest(d_pc, n_pieces, d_runs, n_runs, d_dgtab.as<uint64_t>(), d_dgpart.as<uint64_t>(),
                              d_dgout.as<clg_digest>(), stream);
  }));
  HIPCHK(hipMemcpyAsync(h_dgout.p, d_dgout.p, size_t(n) * sizeof(clg_digest), hipMemcpyDeviceToHost, stream));
  CHK(sync());
  memcpy(out, h_dgout.p, size_t(n) * sizeof(clg_digest));
  return CLG_OK;
}

// Device-output slice gather on gstream, after everything already queued on `stream`
// (appends); returns without waiting.  Its own descriptor buffers, so the next decode
// on `stream` does not touch them; the next gather waits for this one first.
int clg_engine::gather_runs_async(const RunPlan& p, void* out) {
  const uint32_t set = gseq++ & 1u;
  if (gdone[set]) HIPCHK(hipEventSynchronize(gdone[set]));  // the gather two calls ago released this set
  else HIPCHK(hipEventCreateWithFlags(&gdone[set], hipEventDisableTiming));
  // no wait on `stream`: every pool write (flush, upstream scatter) has completed when
  // its call returned, and decodes only read the pool
  StagedPlan sp;
  CHK(stage_run_plan(p, DescSet{h_gdesc[set], d_gdesc[set], d_gpieces[set]}, gstream, &sp));
  CHK(timed("slice_gather", 2 * p.total, [&] {
    return clg::launch_gather(sp.pieces, p.n_pieces, static_cast<uint8_t*>(out), gstream);
  }, gstream));
  HIPCHK(hipEventRecord(gdone[set], gstream));
  g_pending = true;
  return CLG_OK;
}

int clg_engine::get_delta(uint32_t h, ChKey k, int64_t epoch, void* out, uint32_t cap, uint32_t kind, uint32_t* n,
                          bool host_only) {
  *n = 0;
  Log* l;
  CHK(get_log(h, &l));
  auto ci = l->consumers.find(k);
  if (ci == l->consumers.end()) return fail(CLG_E_NO_CONSUMER, "consumer not registered on log %u", h);
  {
    const int32_t p = ci->second.es->offset + ci->second.offset;
    const int32_t nb = bytes_to_send(*l, epoch, p);
    if (nb < 0 || p < 0 || int64_t(p) + nb > capacity(*l))
      return fail(CLG_E_STATE, "delta [%d, %d) outside log of capacity %d", p, p + nb, capacity(*l));
    if (uint32_t(nb) > cap) {
      *n = uint32_t(nb);  // required size (the consumer does not advance)
      return fail(CLG_E_CAPACITY, "delta needs %d bytes", nb);
    }
    if (kind == CLG_MEM_HOST && p >= l->tail_start && p + nb <= l->writer) {  // the host tail holds it
      int32_t phys, nb2;
      CHK(take_delta(h, k, epoch, &phys, &nb2));
      if (nb2) memcpy(out, l->tail.data() + (phys - l->tail_start), size_t(nb2));
      *n = uint32_t(nb2);
      return CLG_OK;
    }
  }
  if (host_only) return kNeedGpu;
  CHK(flush());
  int32_t phys, nb;
  CHK(take_delta(h, k, epoch, &phys, &nb));
  std::vector<clg::GatherPiece> pieces;
  add_pieces(*l, phys, nb, 0, pieces);
  CHK(run_gather(pieces, uint64_t(nb), out, kind));
  *n = uint32_t(nb);
  return CLG_OK;
}

int clg_engine::determinants_range(const Log& l, int64_t start_epoch, int32_t* start, int32_t* nb) {  // :285-313
  int32_t s = 0;
  auto it = l.epochs.find(start_epoch);
  if (it != l.epochs.end())
    s = it->offset;
  else if (!l.epochs.empty())
    s = l.epochs.begin()->offset;
  *start = s;
  *nb = l.writer - s;
  if (*nb < 0 || s < 0 || l.writer > capacity(l))  // makeDeltaUnsafe IndexOutOfBounds
    return fail(CLG_E_STATE, "determinant range [%d, %d) outside the log", s, l.writer);
  return CLG_OK;
}

int clg_engine::get_determinants(uint32_t h, int64_t start_epoch, void* out, uint32_t cap, uint32_t kind, uint32_t* n,
                                 bool host_only) {
  *n = 0;
  Log* l;
  CHK(get_log(h, &l));
  if (l->depth == 0) return CLG_OK;
  int32_t s, nb;
  CHK(determinants_range(*l, start_epoch, &s, &nb));
  if (uint32_t(nb) > cap) {
    *n = uint32_t(nb);  // required size
    return fail(CLG_E_CAPACITY, "getDeterminants needs %d bytes", nb);
  }
  if (kind == CLG_MEM_HOST && s >= l->tail_start) {  // the host tail holds it
    if (nb) memcpy(out, l->tail.data() + (s - l->tail_start), size_t(nb));
    *n = uint32_t(nb);
    return CLG_OK;
  }
  if (host_only) return kNeedGpu;
  CHK(flush());
  std::vector<clg::GatherPiece> pieces;
  add_pieces(*l, s, nb, 0, pieces);
  CHK(run_gather(pieces, uint64_t(nb), out, kind));
  *n = uint32_t(nb);
  return CLG_OK;
}

extern "C" {

int clg_get_delta(clg_engine* e, uint32_t log, clg_channel_id c, int64_t epoch, void* out, uint32_t cap,
                  uint32_t kind, uint32_t* n) {
  {  // the host tail holds it: no GPU, only this log's stripe
    LOG_GUARD(e, log);
    const int r = e->get_delta(log, ChKey{c.lo, c.hi}, epoch, out, cap, kind, n, true);
    if (r != clg_engine::kNeedGpu) return r;
  }
  ENGINE_GUARD(e);
  return e->get_delta(log, ChKey{c.lo, c.hi}, epoch, out, cap, kind, n);
}

int clg_get_determinants(clg_engine* e, uint32_t log, int64_t start_epoch, void* out, uint32_t cap, uint32_t kind,
                         uint32_t* n) {
  {
    LOG_GUARD(e, log);
    const int r = e->get_determinants(log, start_epoch, out, cap, kind, n, true);
    if (r != clg_engine::kNeedGpu) return r;
  }
  ENGINE_GUARD(e);
  return e->get_determinants(log, start_epoch, out, cap, kind, n);
}

}  // extern "C"

extern "C" {

int clg_log_read_phys(clg_engine* e, uint32_t h, int32_t phys, uint32_t n, uint8_t* host_out) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  if (phys < 0 || int64_t(phys) + n > e->capacity(*l)) return fail(CLG_E_STATE, "range outside log");
  CHK(e->flush());
  std::vector<clg::GatherPiece> pieces;
  e->add_pieces(*l, phys, int32_t(n), 0, pieces);
  return e->run_gather(pieces, n, host_out, CLG_MEM_HOST);
}

// getDeterminants(startEpoch) of many logs (respondToDeterminantRequest's copies for a
// replay-prep merge, JobCausalLogImpl.java:188-204): the ranges on the host, the bytes by
// one device gather, back to back in request order.
int clg_get_determinants_batch(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, void* out,
                               uint64_t cap, uint32_t out_kind, uint64_t* out_off, uint32_t* len, uint64_t* total) {
  ENGINE_GUARD(e);
  if (n && (!log || !start_epoch || !len)) return fail(CLG_E_INVALID_ARG, "null argument");
  if (!out) {  // sizes only (the merge measures every copy first): no gather plan
    uint64_t dst = 0;
    for (uint32_t i = 0; i < n; ++i) {
      Log* l;
      CHK(e->get_log(log[i], &l));
      int32_t s = 0, nb = 0;
      if (l->depth != 0) CHK(e->determinants_range(*l, start_epoch[i], &s, &nb));
      len[i] = uint32_t(nb);
      if (out_off) out_off[i] = dst;
      dst += uint64_t(nb);
    }
    if (total) *total = dst;
    return CLG_OK;
  }
  clg_engine::RunPlan p(*e, n);
  CHK(e->plan_determinant_runs(log, start_epoch, n, len, out_off, p));
  if (total) *total = p.total;
  if (p.total > cap) return fail(CLG_E_CAPACITY, "getDeterminants batch needs %llu bytes", (unsigned long long)p.total);
  CHK(e->flush());
  return e->run_gather_runs(p, out, out_kind);
}

// The digest of getDeterminants(start_epoch[i]) of log[i] (digest.h): the ranges, runs and
// segment table as clg_get_determinants_batch builds them, then a read-only pass over the
// pieces.  What LogReplayerImpl.checkFinished (LogReplayerImpl.java:126-128) asserts by length
// alone, and only under -ea, a caller can assert by content.
int clg_digest_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, clg_digest* out) {
  ENGINE_GUARD(e);
  if (n && (!log || !start_epoch || !out)) return fail(CLG_E_INVALID_ARG, "null argument");
  if (!n) return CLG_OK;
  clg_engine::RunPlan p(*e, n);
  CHK(e->plan_determinant_runs(log, start_epoch, n, nullptr, nullptr, p));
  if (p.runs.empty()) {
    memset(out, 0, size_t(n) * sizeof(clg_digest));
    return CLG_OK;
  }
  CHK(e->flush());
  clg_engine::StagedPlan sp;
  CHK(e->stage_run_plan(p, clg_engine::DescSet{e->h_desc, e->d_desc, e->d_pieces}, e->stream, &sp));
  return e->run_digest(sp.runs, uint32_t(p.runs.size()), sp.pieces, p.n_pieces, p.total, n, out);
}

// The digest of spans of host or device memory: the same pieces, one per 16 KiB of span, built
// on the host (a host input is staged as clg_decode_host stages its bytes).  What
// DeterminantResponseEvent.merge (DeterminantResponseEvent.java:137-146) decides on lengths
// alone, the receiver of a merged winner can check by content.
int clg_digest_spans(clg_engine* e, const uint8_t* bytes, const uint64_t* off, const uint64_t* len, uint32_t n,
                     uint32_t in_kind, clg_digest* out) {
  ENGINE_GUARD(e);
  if (n && (!off || !len || !out)) return fail(CLG_E_INVALID_ARG, "null argument");
  if (in_kind != CLG_MEM_HOST && in_kind != CLG_MEM_DEVICE) return fail(CLG_E_INVALID_ARG, "in_kind %u", in_kind);
  if (!n) return CLG_OK;
  constexpr uint64_t kPiece = 16384;
  uint64_t total = 0, n_pieces = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (len[i] >> 32) return fail(CLG_E_INVALID_ARG, "span %u of %llu bytes", i, (unsigned long long)len[i]);
    total += len[i];
    n_pieces += (len[i] + kPiece - 1) / kPiece;
  }
  if (!total) {
    memset(out, 0, size_t(n) * sizeof(clg_digest));
    return CLG_OK;
  }
  if (!bytes) return fail(CLG_E_INVALID_ARG, "null argument");
  if (n_pieces >> 32) return fail(CLG_E_INVALID_ARG, "spans of %llu bytes in one call", (unsigned long long)total);
  const uint8_t* base;  // span i starts at base + (off[i] - base_off)
  uint64_t base_off;
  CHK(e->stage_spans(bytes, off, len, n, in_kind, &base, &base_off));
  std::vector<clg::SegSpan> runs;
  std::vector<clg::GatherPiece> pieces;
  runs.reserve(n);
  pieces.reserve(n_pieces);
  uint64_t dst = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (len[i] == 0) continue;
    runs.push_back(clg::SegSpan{0, 0, uint32_t(len[i]), dst, uint32_t(pieces.size()), i});
    for (uint64_t a = 0; a < len[i]; a += kPiece)
      pieces.push_back(clg::GatherPiece{base + (off[i] - base_off) + a, dst + a, uint32_t(std::min(kPiece, len[i] - a)), 0});
    dst += len[i];
  }
  const size_t rb = clg_engine::al16(runs.size() * sizeof(clg::SegSpan)), pb = pieces.size() * sizeof(clg::GatherPiece);
  CHK(e->h_desc.ensure(rb + pb));
  CHK(e->d_desc.ensure(rb + pb));
  memcpy(e->h_desc.as<uint8_t>(), runs.data(), runs.size() * sizeof(clg::SegSpan));
  memcpy(e->h_desc.as<uint8_t>() + rb, pieces.data(), pb);
  HIPCHK(hipMemcpyAsync(e->d_desc.p, e->h_desc.p, rb + pb, hipMemcpyHostToDevice, e->stream));
  return e->run_digest(e->d_desc.as<clg::SegSpan>(), uint32_t(runs.size()),
                       reinterpret_cast<const clg::GatherPiece*>(e->d_desc.as<uint8_t>() + rb), uint32_t(pieces.size()),
                       total, n, out);
}

int clg_digest_host(const uint8_t* bytes, uint64_t n, clg_digest* out) {
  if (!out || (n && !bytes)) return fail(CLG_E_INVALID_ARG, "null argument");
  *out = clg_digest{clg::dg_bytes(bytes, n), n};
  return CLG_OK;
}

// The digest of getDeterminants(start_epoch[i]) of log[i] at each of the request's cuts
// (digest.h, "prefix digests"), the range read once.  DeterminantResponseEvent.merge
// (DeterminantResponseEvent.java:137-146) keeps the longest copy on its length alone and
// ThreadCausalLogImpl.processUpstreamDelta drops what lies below its own offset unread: both
// take the shorter copy for a prefix of the longer.  The holder of the longer copy can check
// that with the other side's 16 bytes: its own digest at the other side's length.
int clg_digest_prefixes(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                        const uint64_t* cut_first, const uint32_t* cuts, clg_digest* out) {
  ENGINE_GUARD(e);
  if (!cut_first || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  if (cut_first[0] != 0) return fail(CLG_E_INVALID_ARG, "cut_first[0] is %llu", (unsigned long long)cut_first[0]);
  for (uint32_t i = 0; i < n; ++i)
    if (cut_first[i + 1] < cut_first[i]) return fail(CLG_E_INVALID_ARG, "cut_first decreases at request %u", i);
  if (cut_first[n] && (!cuts || !out)) return fail(CLG_E_INVALID_ARG, "null argument");
  for (uint32_t i = 0; i < n; ++i)
    for (uint64_t k = cut_first[i] + 1; k < cut_first[i + 1]; ++k)
      if (cuts[k] < cuts[k - 1]) return fail(CLG_E_INVALID_ARG, "cuts of request %u decrease", i);
  return e->digest_prefixes(log, start_epoch, n, cut_first, cuts, out);
}

// Cuts at the range's own epoch ends: a row per epoch of the range, so two holders of a log can
// name the first epoch in which their copies part without moving a log byte -- the check behind
// the same merge by length (DeterminantResponseEvent.java:137-146) and offset dedup
// (ThreadCausalLogImpl.processUpstreamDelta), epoch by epoch.  A depth-0 log and a log without
// epochs have no rows.
int clg_digest_epochs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, uint64_t cap,
                      uint64_t* first, int64_t* epoch_id, clg_digest* out, uint64_t* total) {
  ENGINE_GUARD(e);
  if (!first || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  if (out && !epoch_id) return fail(CLG_E_INVALID_ARG, "null argument");
  std::vector<uint32_t> cuts;
  first[0] = 0;
  for (uint32_t i = 0; i < n; ++i) {
    Log* l;
    CHK(e->get_log(log[i], &l));
    uint64_t rows = 0;
    if (l->depth != 0 && !l->epochs.empty()) {
      int32_t s = 0, nb = 0;
      CHK(e->determinants_range(*l, start_epoch[i], &s, &nb));
      const auto* ep = l->epochs.find(start_epoch[i]);
      if (ep == l->epochs.end()) ep = l->epochs.begin();
      rows = uint64_t(l->epochs.end() - ep);
      if (out && first[i] + rows <= cap) {
        for (int32_t prev = s; ep != l->epochs.end(); ++ep) {
          // an epoch ends where the next one starts, the last at the writer
          const int32_t end = ep + 1 != l->epochs.end() ? (ep + 1)->offset : l->writer;
          if (end < prev) return fail(CLG_E_STATE, "epoch %lld of log %u ends before it starts", (long long)ep->id, log[i]);
          epoch_id[cuts.size()] = ep->id;
          cuts.push_back(uint32_t(end - s));
          prev = end;
        }
      }
    }
    first[i + 1] = first[i] + rows;
  }
  if (total) *total = first[n];
  if (!out) return CLG_OK;
  if (first[n] > cap) return fail(CLG_E_CAPACITY, "epoch digests need %llu rows", (unsigned long long)first[n]);
  return e->digest_prefixes(log, start_epoch, n, first, cuts.data(), out);
}

int clg_digest_prefixes_host(const uint8_t* bytes, uint64_t n, const uint32_t* cuts, uint32_t n_cuts, clg_digest* out) {
  if ((n_cuts && (!cuts || !out)) || (n && !bytes)) return fail(CLG_E_INVALID_ARG, "null argument");
  for (uint32_t j = 1; j < n_cuts; ++j)
    if (cuts[j] < cuts[j - 1]) return fail(CLG_E_INVALID_ARG, "cuts decrease at %u", j);
  std::vector<uint64_t> hash(n_cuts), len(n_cuts);
  clg::dg_prefixes(bytes, n, cuts, n_cuts, hash.data(), len.data());
  for (uint32_t j = 0; j < n_cuts; ++j) out[j] = clg_digest{hash[j], len[j]};
  return CLG_OK;
}

// The longest common prefix of getDeterminants(start_epoch[i]) of log[i] and a reference span
// (diff.h): the ranges, runs, segment table and pieces as clg_digest_logs builds them, each run
// with the device address of its reference (host input staged as clg_digest_spans stages it),
// then a read-only pass over both.  Where LogReplayerImpl.checkFinished
// (LogReplayerImpl.java:126-128) and the digests say only that two copies part, this says where.
int clg_diff_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, const uint8_t* bytes,
                  const uint64_t* off, const uint64_t* len, uint32_t in_kind, clg_diff* out) {
  ENGINE_GUARD(e);
  if (n && (!log || !start_epoch || !off || !len || !out)) return fail(CLG_E_INVALID_ARG, "null argument");
  if (in_kind != CLG_MEM_HOST && in_kind != CLG_MEM_DEVICE) return fail(CLG_E_INVALID_ARG, "in_kind %u", in_kind);
  if (!n) return CLG_OK;
  bool any = false;
  for (uint32_t i = 0; i < n; ++i) {
    if (len[i] >> 32) return fail(CLG_E_INVALID_ARG, "span %u of %llu bytes", i, (unsigned long long)len[i]);
    any |= len[i] != 0;
  }
  if (any && !bytes) return fail(CLG_E_INVALID_ARG, "null argument");
  std::vector<uint32_t> len_log(n);
  clg_engine::RunPlan p(*e, n);
  CHK(e->plan_determinant_runs(log, start_epoch, n, len_log.data(), nullptr, p));
  for (uint32_t i = 0; i < n; ++i) out[i] = clg_diff{0, len_log[i], len[i]};  // (a request without a run stays so)
  if (p.runs.empty()) return CLG_OK;
  CHK(e->flush());
  const uint8_t* base;  // span i starts at base + (off[i] - base_off)
  uint64_t base_off;
  CHK(e->stage_spans(bytes, off, len, n, in_kind, &base, &base_off));
  std::vector<clg::DiffRef> refs(p.runs.size());  // staged behind the plan: runs | segment table | references
  uint64_t compared = 0;
  for (size_t k = 0; k < p.runs.size(); ++k) {
    const uint32_t i = p.runs[k].pad;
    refs[k] = clg::DiffRef{len[i] ? base + (off[i] - base_off) : nullptr, uint32_t(len[i]), 0};
    compared += 2 * std::min<uint64_t>(p.runs[k].len, len[i]);
  }
  clg_engine::StagedPlan sp;
  CHK(e->stage_run_plan(p, clg_engine::DescSet{e->h_desc, e->d_desc, e->d_pieces}, e->stream, &sp, refs.data(),
                        refs.size() * sizeof(clg::DiffRef)));
  const uint32_t n_pieces = p.n_pieces;
  CHK(e->d_dffirst.ensure(size_t(n_pieces) * 4 + 4));
  CHK(e->d_dfout.ensure(size_t(n) * sizeof(clg_diff)));
  CHK(e->h_dfout.ensure(size_t(n) * sizeof(clg_diff)));
  memcpy(e->h_dfout.p, out, size_t(n) * sizeof(clg_diff));
  HIPCHK(hipMemcpyAsync(e->d_dfout.p, e->h_dfout.p, size_t(n) * sizeof(clg_diff), hipMemcpyHostToDevice, e->stream));
  CHK(e->timed("log_diff", compared, [&] {
    return clg::launch_diff(sp.pieces, n_pieces, sp.runs, uint32_t(p.runs.size()),
                            reinterpret_cast<const clg::DiffRef*>(sp.extra), e->d_dffirst.as<uint32_t>(),
                            e->d_dfout.as<clg_diff>(), e->stream);
  }));
  HIPCHK(hipMemcpyAsync(e->h_dfout.p, e->d_dfout.p, size_t(n) * sizeof(clg_diff), hipMemcpyDeviceToHost, e->stream));
  CHK(e->sync());
  memcpy(out, e->h_dfout.p, size_t(n) * sizeof(clg_diff));
  return CLG_OK;
}

int clg_lcp_host(const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb, uint64_t* lcp) {
  if (!lcp || (na && !a) || (nb && !b)) return fail(CLG_E_INVALID_ARG, "null argument");
  *lcp = clg::df_lcp_bytes(a, na, b, nb);
  return CLG_OK;
}

int clg_slice_batch(clg_engine* e, const clg_slice_req* reqs, uint32_t n, clg_slice_res* res, void* out, uint64_t cap,
                    uint32_t out_kind, uint64_t* total) {
  ENGINE_GUARD_KEEP(e);
  if (!(out_kind == CLG_MEM_DEVICE && (e->cfg.flags & CLG_F_ASYNC_SLICE))) e->settle();
  if (n && (!reqs || !res)) return fail(CLG_E_INVALID_ARG, "null argument");
  CHK(e->flush());
  clg_engine::RunPlan p(*e, n);
  const uint32_t C = e->C();
  for (uint32_t i = 0; i < n; ++i) {
    clg_slice_res& r = res[i];
    r = clg_slice_res{CLG_OK, 0, 0, 0, p.total};
    const ChKey k{reqs[i].consumer.lo, reqs[i].consumer.hi};
    int32_t has = 0;
    int st = e->has_delta(reqs[i].log, k, reqs[i].epoch, &has);
    if (st != CLG_OK) {
      r.status = st;
      continue;
    }
    r.has_delta = has;
    if (!has) continue;
    st = e->offset_from_epoch(reqs[i].log, k, &r.offset_from_epoch);  // Abstract...:199 before :201
    if (st != CLG_OK) {
      r.status = st;
      continue;
    }
    int32_t phys, nb;
    st = e->take_delta(reqs[i].log, k, reqs[i].epoch, &phys, &nb);
    if (st != CLG_OK) {
      r.status = st;
      continue;
    }
    if (p.total + uint64_t(nb) > cap) {
      // undo the consumer advance so the request can be retried with a bigger buffer
      e->logs[reqs[i].log].consumers[k].offset -= nb;
      r.status = CLG_E_CAPACITY;
      continue;
    }
    r.len = nb;
    p.add(reqs[i].log, phys, nb, i);
  }
  if (total) *total = p.total;
  // dispatch order only: the same pieces, n_pieces as it was
  const long long gw = e->sw.gather_window;
  clg::window_order(p.runs, C, gw < 0 ? clg::default_window(C) : uint32_t(std::min<long long>(gw, UINT32_MAX)));
  return e->run_gather_runs(p, out, out_kind);
}

}  // extern "C"
