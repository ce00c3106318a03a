// engine.cpp -- host side of the MI355X causal-log engine (implements include/clonos_engine.h).
//
// Owns: the HBM segment pool (components of determinantBufferSize bytes), the per-log
// metadata with exactly the reference's semantics, host staging of appends, and the
// batching of all byte work into gfx950 kernels (kernels.hip) on one HIP stream.
//
// R/ = flink-runtime/src/main/java/org/apache/flink/runtime/causal/ of the reference.
// The log metadata mirrors R/log/thread/ThreadCausalLogImpl.java:51-527 line for line in
// behaviour (EpochStartOffset objects shared by reference with ConsumerOffset, Netty
// component-granular discardReadComponents), but the bytes never leave HBM.
//
// This unit: the error text, the registry of clg_host_register, engine create / destroy, timing,
// the segment pool, flush, append and upstream deltas, checkpoints and truncation, consumer
// seeks, jobs and log handles, the kernel statistics, the static_asserts on the ABI structs.
// Slices and digests are in engine_gather.cpp, the decodes in engine_decode.cpp, the typed-columns
// family in engine_columns.cpp, engine_pack.cpp and engine_encode_columns.cpp (what those share is
// in engine_columns.h), replay preparation with encode, enrich and process-delta in
// engine_replay.cpp, the in-flight log in engine_inflight.cpp; what all the units share is in
// engine_impl.h.
#include "engine_impl.h"

static_assert(sizeof(clg_delta_req) == 32, "clg_delta_req layout");
static_assert(sizeof(clg_diff) == 24, "clg_diff layout");
static_assert(sizeof(clg_columns) == 232, "clg_columns layout");
static_assert(sizeof(clg_payloads) == 64, "clg_payloads layout");
static_assert(sizeof(clg_columns_in) == 176, "clg_columns_in layout");
static_assert(sizeof(clg_packed) == 136, "clg_packed layout");
static_assert(sizeof(clg_unpack_bad) == 16, "clg_unpack_bad layout");
static_assert(sizeof(clg_packed_wide) == 480, "clg_packed_wide layout");
static_assert(sizeof(clg_encoded) == 56, "clg_encoded layout");
static_assert(sizeof(clg_packed_payloads) == 96, "clg_packed_payloads layout");

namespace clg_internal {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// A launch helper's CLG_E_DEVICE carries the HIP error into the error text.
void note_launch_error(const char* what) {
  if (const char* m = clg::take_launch_error()) fail(CLG_E_DEVICE, "%s: %s", what, m);
}

}  // namespace clg_internal

// clg_host_register's ranges: host base -> device address (for CLG_MEM_MAPPED outputs)
namespace {
struct Mapped {
  uintptr_t host;
  uint64_t bytes;
  uintptr_t dev;
};
std::mutex g_map_mu;
std::vector<Mapped> g_mapped;
}  // namespace
// The device address of registered host memory [h, h + n) (0: not wholly inside one
// registered range).
uintptr_t clg_mapped_device_address(const void* h, uint64_t n) {
  std::lock_guard<std::mutex> g(g_map_mu);
  for (const Mapped& m : g_mapped)
    if (uintptr_t(h) >= m.host && uintptr_t(h) < m.host + m.bytes && n <= m.host + m.bytes - uintptr_t(h))
      return m.dev + (uintptr_t(h) - m.host);
  return 0;
}
// How many of the n bytes at h one copy may take: up to the first edge of a registered range
// inside them (the HIP runtime refuses a copy that crosses the end of registered memory).
uint64_t clg_mapped_piece(const void* h, uint64_t n) {
  std::lock_guard<std::mutex> g(g_map_mu);
  for (const Mapped& m : g_mapped)
    for (const uintptr_t edge : {m.host, m.host + uintptr_t(m.bytes)})
      if (edge > uintptr_t(h) && edge - uintptr_t(h) < n) n = edge - uintptr_t(h);
  return n;
}

namespace clg_internal {  // error text for the host-only translation units (response.cpp)
int set_error(int code, const char* msg) { return fail(code, "%s", msg); }
}  // namespace clg_internal

// ---------------------------------------------------------------- timing helpers
hipEvent_t clg_engine::get_event() {
  if (!ev_pool.empty()) {
    hipEvent_t e = ev_pool.back();
    ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

// ready_only: only the timings whose end event has completed (the rest stay pending)
void clg_engine::collect_timings(bool ready_only) {
  if (ready_only) {
    std::vector<PendingTiming> later;
    for (auto& t : timings)
      if (hipEventQuery(t.b) == hipErrorNotReady) later.push_back(t);
    if (!later.empty()) {
      std::vector<PendingTiming> done;
      for (auto& t : timings)
        if (hipEventQuery(t.b) != hipErrorNotReady) done.push_back(t);
      timings.swap(done);
      collect_timings();
      timings.swap(later);
      return;
    }
  }
  for (auto& t : timings) {
    float ms = 0;
    hipEventSynchronize(t.b);
    hipEventElapsedTime(&ms, t.a, t.b);
    Stat& s = stats[t.name];
    s.launches++;
    s.ms += ms;
    s.bytes += t.bytes;
    ev_pool.push_back(t.a);
    ev_pool.push_back(t.b);
  }
  timings.clear();
}

int clg_engine::gwait() {
  if (g_pending) {
    g_pending = false;
    HIPCHK(hipStreamSynchronize(gstream));
  }
  return CLG_OK;
}

// The arena for kernels queued next on `stream`, its bump counter reset first.
int clg_engine::jarena_reset(clg::JArena* a) {
  CHK(d_jarena.ensure(jarena_bytes + 256));
  HIPCHK(hipMemsetAsync(d_jarena.p, 0, 8, stream));
  *a = clg::JArena{d_jarena.as<uint8_t>() + 256, jarena_bytes, d_jarena.as<unsigned long long>()};
  return CLG_OK;
}

// Queues a read-back of the arena's bump counter into slot k, after the walks queued so
// far; jarena_spilled(k) (after a sync) says whether any of them found the arena full --
// then some walk returned kJsSpill and whatever the kernels derived from it is void.
int clg_engine::jarena_note(int k) {
  CHK(h_jused.ensure(64));
  HIPCHK(hipMemcpyAsync(h_jused.as<uint64_t>() + k, d_jarena.p, 8, hipMemcpyDeviceToHost, stream));
  return CLG_OK;
}

int clg_engine::jarena_clear_note(int k) {
  CHK(h_jused.ensure(64));
  h_jused.as<uint64_t>()[k] = 0;
  return CLG_OK;
}

int clg_engine::jarena_grow() {
  CHK(sync());  // kernels still using the old arena
  if (jarena_bytes >= (size_t(1) << 36))
    return fail(CLG_E_DEVICE, "Serializable walker spill arena would exceed 64 GiB");
  jarena_bytes *= 2;
  stats["jser_arena_grow"].launches++;
  return CLG_OK;
}

int clg_engine::sync() {
  CHK(gwait());
  HIPCHK(hipStreamSynchronize(stream));
  collect_timings();
  return CLG_OK;
}

// notEnoughSpaceFor / addComponent (:351-353, :438-452): all-or-nothing.
int clg_engine::ensure_space(Log& l, int32_t n) {
  if (int64_t(l.writer) + n <= capacity(l)) return CLG_OK;
  std::lock_guard<std::mutex> g(pool_mu);
  return ensure_space_locked(l, n);
}

int clg_engine::ensure_space_locked(Log& l, int32_t n) {  // pool_mu held
  int64_t need_bytes = int64_t(l.writer) + n - capacity(l);
  if (need_bytes <= 0) return CLG_OK;
  size_t need = size_t((need_bytes + C() - 1) / C());
  if (need > free_segs.size())
    return fail(CLG_E_NOSPACE, "segment pool exhausted (need %zu, free %zu)", need, free_segs.size());
  for (size_t i = 0; i < need; ++i) {
    l.segs.push_back(free_segs.back());
    ++seg_life[free_segs.back()];
    free_segs.pop_back();
  }
  return CLG_OK;
}

void clg_engine::write_pending(Log& l, const uint8_t* b, uint32_t n) {
  if (l.flushed == l.writer && n) {
    std::lock_guard<std::mutex> g(dirty_mu);
    dirty.push_back(uint32_t(&l - logs.data()));
  }
  l.tail.insert(l.tail.end(), b, b + n);
  l.writer += int32_t(n);
}

// ---------------------------------------------------------------- flush (append scatter)
// Drops flushed bytes from the front of a log's host tail beyond the configured keep.
void clg_engine::trim_tail(Log& l) {
  const size_t keep = cfg.host_tail_bytes;
  const size_t flushed_in_tail = size_t(l.flushed - l.tail_start);
  if (flushed_in_tail <= 2 * keep) return;  // amortised: trim to `keep` once it doubled
  const size_t drop = flushed_in_tail - keep;
  l.tail.erase(l.tail.begin(), l.tail.begin() + long(drop));
  l.tail_start += int32_t(drop);
}

// Staged (unflushed) bytes of one log are bounded: past this the append that crossed it
// flushes (the host holds at most ~this + host_tail_bytes per log).
bool clg_engine::over_stage_limit(uint32_t h) const {
  const uint32_t lim = std::max<uint32_t>(65536u, 2u * cfg.host_tail_bytes);
  return h < logs.size() && logs[h].open && logs[h].pending_bytes() > lim;
}

int clg_engine::flush() {
  size_t total = 0, nchunks = 0;
  for (uint32_t h : dirty) {
    const Log& l = logs[h];
    if (l.open && l.pending_bytes()) {
      total += l.pending_bytes();
      nchunks += l.pending_bytes() / C() + 2;
    }
  }
  if (total == 0) {
    dirty.clear();
    return CLG_OK;
  }
  CHK(gwait());  // an in-flight gather may still read the segments about to be written
  const size_t desc_bytes = nchunks * sizeof(clg::ScatterChunk);
  CHK(h_stage.ensure(total));
  CHK(h_desc.ensure(desc_bytes));
  CHK(d_stage.ensure(total));
  uint8_t* hs = h_stage.as<uint8_t>();
  clg::ScatterChunk *const ch0 = h_desc.as<clg::ScatterChunk>(), *ch = ch0;
  size_t off = 0;
  for (uint32_t h : dirty) {
    Log& l = logs[h];
    const uint32_t pb = l.open ? l.pending_bytes() : 0u;
    if (!pb) continue;
    memcpy(hs + off, l.pending_data(), pb);
    ch = add_chunks(ch, l, uint32_t(l.flushed), pb, off);
    off += pb;
    l.flushed = l.writer;
    trim_tail(l);
  }
  dirty.clear();
  HIPCHK(hipMemcpyAsync(d_stage.p, hs, total, hipMemcpyHostToDevice, stream));
  CHK(scatter_chunks("append_scatter", size_t(ch - ch0), total, d_stage.as<uint8_t>(), true));
  // the pinned staging buffers are reused by the next flush: wait for the copies
  HIPCHK(hipStreamSynchronize(stream));
  return CLG_OK;
}

int clg_engine::scatter_chunks(const char* name, size_t n, uint64_t total, const uint8_t* d_src, bool side) {
  const size_t db = n * sizeof(clg::ScatterChunk);
  CHK(d_desc.ensure(db));
  HIPCHK(hipMemcpyAsync(d_desc.p, h_desc.p, db, hipMemcpyHostToDevice, stream));
  return timed(name, 2 * total, [&] {
    return clg::launch_scatter(d_desc.as<clg::ScatterChunk>(), uint32_t(n), d_src, stream, side ? side_arg() : nullptr);
  });
}

// ---------------------------------------------------------------- ThreadCausalLog ops
int clg_engine::append(uint32_t h, int64_t epoch, const uint8_t* b, uint32_t n) {  // :158-177
  Log* l;
  CHK(get_log(h, &l));
  if (l->depth == 0) return CLG_OK;
  if (n && !b) return fail(CLG_E_INVALID_ARG, "null record");
  CHK(ensure_space(*l, int32_t(n)));
  compute_if_absent(*l, epoch);
  write_pending(*l, b, n);
  return CLG_OK;
}

int clg_engine::upstream(uint32_t h, int64_t epoch, int32_t off_from_epoch, const uint8_t* d, uint32_t n) {  // :117-154
  Log* l;
  CHK(get_log(h, &l));
  if (n == 0) return CLG_OK;
  if (!d) return fail(CLG_E_INVALID_ARG, "null delta");
  auto es = compute_if_absent(*l, epoch);
  const int32_t cur = l->writer - es->offset;
  const int32_t num_new = (off_from_epoch + int32_t(n)) - cur;
  if (num_new > 0) {
    // :136-137 add components before delta.readerIndex(<0) throws (:143): capacity grows
    CHK(ensure_space(*l, num_new));
    if (num_new > int32_t(n))
      return fail(CLG_E_GAP, "upstream delta leaves a gap: offsetFromEpoch %d, %u bytes, log at %d", off_from_epoch,
                  n, cur);
    write_pending(*l, d + (n - uint32_t(num_new)), uint32_t(num_new));
  }
  return CLG_OK;
}

// Batched processUpstreamDelta (:117-154) over one input buffer.  Device input (e.g.
// an RCCL receive buffer) is scattered straight into the log segments: pending host
// bytes are flushed first, so the logs' byte order is preserved.
int clg_engine::upstream_batch(clg_delta_req* r, uint32_t n, const uint8_t* bytes, uint32_t in_kind) {
  HostTimer ht(this, "host_upstream_batch");
  if (in_kind != CLG_MEM_DEVICE) {
    for (uint32_t i = 0; i < n; ++i) {
      r[i].status = upstream(r[i].log, r[i].epoch, r[i].offset_from_epoch, bytes + r[i].src_off, r[i].len);
    }
    return CLG_OK;
  }
  std::optional<HostTimer> hsub(std::in_place, this, "host_up_wait");  // (CLONOS_HOST_PROF sub-stages)
  CHK(flush());
  CHK(gwait());  // the scatter below writes segments an in-flight gather may read
  hsub.reset();
  if (n >= kParallelLogs) {
    int st = CLG_OK;
    if (upstream_parallel(r, n, bytes, &st)) return st;
  }
  // the chunks go straight into the pinned descriptor buffer (a config-4 batch has 66 k of
  // them: a fresh vector per call cost page faults, and a copy)
  size_t bound = 0;
  for (uint32_t i = 0; i < n; ++i) bound += r[i].len / C() + 2;
  CHK(h_desc.ensure(std::max<size_t>(1, bound) * sizeof(clg::ScatterChunk)));
  clg::ScatterChunk *const ch0 = h_desc.as<clg::ScatterChunk>(), *ch = ch0;
  size_t total = 0;
  std::unique_lock<std::mutex> pool_guard(pool_mu);  // once for the batch, not per log
  for (uint32_t i = 0; i < n; ++i) {
    r[i].status = CLG_OK;
    Log* l;
    if ((r[i].status = get_log(r[i].log, &l)) != CLG_OK || r[i].len == 0) continue;
    auto es = compute_if_absent(*l, r[i].epoch);
    const int32_t cur = l->writer - es->offset;
    const int32_t num_new = (r[i].offset_from_epoch + int32_t(r[i].len)) - cur;
    if (num_new <= 0) continue;
    if ((r[i].status = ensure_space_locked(*l, num_new)) != CLG_OK) continue;  // before the gap check (:136-143)
    if (num_new > int32_t(r[i].len)) {
      r[i].status = fail(CLG_E_GAP, "upstream delta leaves a gap: offsetFromEpoch %d, %u bytes, log at %d",
                         r[i].offset_from_epoch, r[i].len, cur);
      continue;
    }
    ch = add_chunks(ch, *l, uint32_t(l->writer), uint32_t(num_new), r[i].src_off + (r[i].len - uint32_t(num_new)));
    l->writer += num_new;
    l->flushed = l->writer;
    reset_tail(*l);  // these bytes go to HBM only
    total += size_t(num_new);
  }
  pool_guard.unlock();
  if (ch == ch0) return CLG_OK;
  CHK(scatter_chunks("upstream_scatter", size_t(ch - ch0), total, bytes, true));
  return sync();  // the caller's buffer and the pinned descriptors are free again
}

bool clg_engine::upstream_parallel(clg_delta_req* r, uint32_t n, const uint8_t* bytes, int* out_st) {
  std::optional<HostTimer> hsub(std::in_place, this, "host_up_seen");
  up_seen.assign(logs.size(), 0);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t h = r[i].log;
    if (h < logs.size()) {
      if (up_seen[h]) return false;  // two deltas of one log apply in order: the serial loop
      up_seen[h] = 1;
    }
  }
  WorkPool* wp = workers();
  const unsigned P = wp->size();
  const uint32_t per = (n + P - 1) / P, Cb = C();
  up_plan.resize(n);
  // per part: segments, chunks and bytes it needs, and whether a request leaves a gap
  struct UpPart {
    uint64_t need = 0, chunks = 0, bytes = 0;
    bool gap = false;
  };
  std::vector<UpPart> upart(P + 1);
  hsub.emplace(this, "host_up_pass1");
  wp->run([&](unsigned k, unsigned) {
    UpPart q;
    for (uint32_t i = k * per; i < std::min(n, (k + 1) * per); ++i) {
      UpPlan& u = up_plan[i];
      u = UpPlan{0, 0, 0, 0, 0, 0, 0};
      r[i].status = CLG_OK;
      Log* l;
      if ((r[i].status = get_log(r[i].log, &l)) != CLG_OK || r[i].len == 0) continue;
      auto es = compute_if_absent(*l, r[i].epoch);
      const int32_t cur = l->writer - es->offset;
      const int32_t num_new = (r[i].offset_from_epoch + int32_t(r[i].len)) - cur;
      if (num_new <= 0) continue;
      const int64_t need_bytes = int64_t(l->writer) + num_new - capacity(*l);
      u.num_new = num_new;
      u.writer = l->writer;
      u.cur = cur;
      u.need = need_bytes > 0 ? uint32_t((need_bytes + Cb - 1) / Cb) : 0u;
      q.need += u.need;
      if (num_new > int32_t(r[i].len)) {
        q.gap = true;
      } else {
        u.chunks = chunk_count(uint32_t(u.writer), uint32_t(num_new), Cb);
        q.chunks += u.chunks;
        q.bytes += uint64_t(num_new);
      }
    }
    upart[k + 1] = q;
  });
  hsub.emplace(this, "host_up_serial");
  std::unique_lock<std::mutex> pool_guard(pool_mu);
  const size_t top = free_segs.size();
  size_t taken = 0, nch = 0, total = 0;
  bool any_gap = false;
  for (unsigned k = 0; k < P; ++k) {
    any_gap |= upart[k + 1].gap;
    upart[k + 1].need += upart[k].need;
    upart[k + 1].chunks += upart[k].chunks;
    upart[k + 1].bytes += upart[k].bytes;
  }
  // every request served (the usual batch): each part places its own segments and chunks
  // from the parts' prefix in the second pass, as the request-order loop below would
  const bool placed_in_parts = !any_gap && upart[P].need <= top;
  if (placed_in_parts) {
    taken = upart[P].need;
    nch = upart[P].chunks;
    total = upart[P].bytes;
  } else for (uint32_t i = 0; i < n; ++i) {  // request order: the pool and the chunk list
    UpPlan& u = up_plan[i];
    if (!u.num_new) continue;
    if (u.need > top - taken) {
      r[i].status = fail(CLG_E_NOSPACE, "segment pool exhausted (need %u, free %zu)", u.need, top - taken);
      u.num_new = 0;
      u.need = 0;
      continue;
    }
    u.seg_from = taken;
    taken += u.need;
    if (u.num_new > int32_t(r[i].len)) {  // the segments stay (:136-143), nothing is written
      r[i].status = fail(CLG_E_GAP, "upstream delta leaves a gap: offsetFromEpoch %d, %u bytes, log at %d",
                         r[i].offset_from_epoch, r[i].len, u.cur);
      u.num_new = 0;
      continue;
    }
    u.ch_from = nch;  // (u.chunks from the first pass: no log record touched here)
    nch += u.chunks;
    total += size_t(u.num_new);
  }
  if (int st = h_desc.ensure(std::max<size_t>(1, nch) * sizeof(clg::ScatterChunk)); st != CLG_OK) {
    *out_st = st;
    return true;
  }
  clg::ScatterChunk* ch = h_desc.as<clg::ScatterChunk>();
  hsub.emplace(this, "host_up_pass2");
  wp->run([&](unsigned k, unsigned) {
    uint64_t sf = upart[k].need, cf = upart[k].chunks;
    for (uint32_t i = k * per; i < std::min(n, (k + 1) * per); ++i) {
      UpPlan& u = up_plan[i];
      if (placed_in_parts && u.num_new) {
        u.seg_from = sf;
        sf += u.need;
        u.ch_from = cf;
        cf += u.chunks;
      }
      if (!u.need && !u.num_new) continue;
      Log& l = logs[r[i].log];
      for (uint32_t j = 0; j < u.need; ++j) {  // pop order
        const uint32_t sg = free_segs[top - 1 - (u.seg_from + j)];
        l.segs.push_back(sg);
        ++seg_life[sg];  // (each segment is taken by one part)
      }
      if (!u.num_new) continue;
      add_chunks(ch + u.ch_from, l, uint32_t(l.writer), uint32_t(u.num_new), r[i].src_off + (r[i].len - uint32_t(u.num_new)));
      l.writer += u.num_new;
      l.flushed = l.writer;
      reset_tail(l);  // these bytes go to HBM only
    }
  });
  free_segs.resize(top - taken);
  pool_guard.unlock();
  hsub.emplace(this, "host_up_gpu");
  *out_st = CLG_OK;
  if (!nch) return true;
  if ((*out_st = scatter_chunks("upstream_scatter", nch, total, bytes, true)) != CLG_OK) return true;
  *out_st = sync();
  return true;
}

int clg_engine::has_delta(uint32_t h, ChKey k, int64_t epoch, int32_t* out) {  // :196-240
  Log* l;
  CHK(get_log(h, &l));
  *out = 0;
  if (l->depth == 0) return CLG_OK;
  auto it = l->epochs.find(epoch);
  if (it == l->epochs.end()) return CLG_OK;
  auto ci = l->consumers.find(k);
  if (ci == l->consumers.end()) ci = l->consumers.emplace(k, Consumer{EpochMap::ref(*it), 0}).first;
  Consumer& c = ci->second;
  if (c.es->id != epoch) {
    if (c.es->id > epoch)
      return fail(CLG_E_CONSUMER_BACKWARDS, "Consumer went backwards, current epoch %lld requested %lld",
                  (long long)c.es->id, (long long)epoch);
    c.es = EpochMap::ref(*it);
    c.offset = 0;
  }
  *out = bytes_to_send(*l, epoch, c.es->offset + c.offset) != 0;
  return CLG_OK;
}

int clg_engine::offset_from_epoch(uint32_t h, ChKey k, int32_t* out) {  // :243-246
  Log* l;
  CHK(get_log(h, &l));
  auto ci = l->consumers.find(k);
  if (ci == l->consumers.end()) return fail(CLG_E_NO_CONSUMER, "consumer not registered on log %u", h);
  *out = ci->second.offset;
  return CLG_OK;
}

// getDeltaForConsumer :249-277, metadata half: returns (phys, nb) and advances.
int clg_engine::take_delta(uint32_t h, ChKey k, int64_t epoch, int32_t* phys, int32_t* nb) {
  Log* l;
  CHK(get_log(h, &l));
  auto ci = l->consumers.find(k);
  if (ci == l->consumers.end()) return fail(CLG_E_NO_CONSUMER, "consumer not registered on log %u", h);
  Consumer& c = ci->second;
  const int32_t p = c.es->offset + c.offset;
  const int32_t n = bytes_to_send(*l, epoch, p);
  if (n < 0 || p < 0 || int64_t(p) + n > capacity(*l))
    return fail(CLG_E_STATE, "delta [%d, %d) outside log of capacity %d", p, p + n, capacity(*l));
  c.offset += n;
  *phys = p;
  *nb = n;
  return CLG_OK;
}

// notifyCheckpointComplete :398-435 (flushes first so no staged byte lives in a dropped
// component).
int clg_engine::checkpoint_complete(Log& l, int64_t cp) { return checkpoint_complete(l, cp, free_segs); }

// (freed: where the dropped segments go -- a host thread's own list in the parallel truncation)
int clg_engine::checkpoint_complete(Log& l, int64_t cp, std::vector<uint32_t>& freed) {
  const int32_t R = compute_if_absent(l, cp)->offset;  // (read before the erase moves entries)
  l.epochs.erase_below(cp);
  if (R < 0 || R > l.writer) return fail(CLG_E_STATE, "readerIndex %d outside [0, %d]", R, l.writer);
  int32_t move = 0;
  if (R != 0) {
    size_t drop;
    if (R == l.writer && l.writer == capacity(l)) {  // discard-all case
      drop = l.segs.size();
      move = R;
    } else {
      drop = size_t(R) / C();
      move = int32_t(drop * C());
    }
    for (size_t i = 0; i < drop; ++i) freed.push_back(l.segs[i]);
    l.segs.erase_front(drop);
  }
  l.epochs.rebase(move);
  l.writer -= move;
  l.flushed -= move;
  l.tail_start -= move;
  if (l.tail_start < 0) {  // bytes of dropped components
    l.tail.erase(l.tail.begin(), l.tail.begin() + std::min<long>(long(l.tail.size()), long(-l.tail_start)));
    l.tail_start = 0;
    if (l.tail_start + int32_t(l.tail.size()) != l.writer) reset_tail(l);
  }
  return CLG_OK;
}

// The CPUs this process may use: its affinity mask, capped by a cgroup CPU quota (a GPU box
// shares its host between GPUs: 16 CPUs per GPU on the MI355X pool).
int clg_engine::usable_cpus() {
  int n = 0;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
  if (n <= 0) n = int(std::thread::hardware_concurrency());
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    long long period = 0;
    if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
      n = std::min<long long>(n, std::max<long long>(1, atoll(q) / period));
    fclose(f);
  }
  return std::max(1, n);
}

// Host threads for the per-log loops: CLONOS_HOST_THREADS, else up to 16 of the usable CPUs.
// Config 4's step on one box (round 5): 2.49 ms with 16 against 3.1-3.4 ms with 8; round 6,
// median of four each: 2.09 / 2.20 / 2.40 ms with 16 / 14 / 12.
WorkPool* clg_engine::workers() {
  if (!host_pool) {
    const int n = std::max(1, std::min(sw.host_threads, usable_cpus()));
    host_pool = std::make_unique<WorkPool>(unsigned(n));
  }
  return host_pool.get();
}

// =======================================================================================
// C-ABI
// =======================================================================================

extern "C" {

void clg_config_default(clg_config* cfg) {
  memset(cfg, 0, sizeof *cfg);
  cfg->segment_bytes = 16384;  // NettyConfig.java:86-89
  cfg->pool_segments = 16384;  // 256 MiB
  cfg->device = 0;
  cfg->sharing_depth = CLG_FULL_SHARING;
  cfg->host_tail_bytes = 16384;    // one component of each log's tail kept on the host
  cfg->ifl_segment_bytes = 32768;  // the in-flight log's pool: Flink's 32 KiB memory segments
  cfg->ifl_pool_segments = 4096;   // 128 MiB
}

int clg_abi_version(void) { return CLG_ABI_VERSION; }

int clg_host_register(void* p, uint64_t bytes) {
  if (!p || !bytes) return fail(CLG_E_INVALID_ARG, "null or empty range");
  hipError_t er = hipHostRegister(p, size_t(bytes), hipHostRegisterMapped);
  if (er != hipSuccess) return fail(CLG_E_DEVICE, "hipHostRegister(%llu bytes): %s", (unsigned long long)bytes,
                                     hipGetErrorString(er));
  void* d = nullptr;
  er = hipHostGetDevicePointer(&d, p, 0);
  if (er != hipSuccess) {
    (void)hipHostUnregister(p);
    return fail(CLG_E_DEVICE, "hipHostGetDevicePointer: %s", hipGetErrorString(er));
  }
  std::lock_guard<std::mutex> g(g_map_mu);
  g_mapped.push_back(Mapped{uintptr_t(p), bytes, uintptr_t(d)});
  return CLG_OK;
}

int clg_host_unregister(void* p) {
  {
    std::lock_guard<std::mutex> g(g_map_mu);
    auto it = std::find_if(g_mapped.begin(), g_mapped.end(), [&](const Mapped& m) { return m.host == uintptr_t(p); });
    if (it == g_mapped.end()) return fail(CLG_E_INVALID_ARG, "range not registered");
    g_mapped.erase(it);
  }
  const hipError_t er = hipHostUnregister(p);
  return er == hipSuccess ? CLG_OK : fail(CLG_E_DEVICE, "hipHostUnregister: %s", hipGetErrorString(er));
}

const char* clg_last_error(void) { return g_err.c_str(); }

int clg_engine_create(const clg_config* cfg, clg_engine** out) {
  if (!cfg || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->segment_bytes < 16 || (cfg->segment_bytes & 15) || cfg->pool_segments == 0)
    return fail(CLG_E_INVALID_ARG, "segment_bytes must be a positive multiple of 16 and pool_segments > 0");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(CLG_E_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(CLG_E_INVALID_ARG, "device %d out of range", cfg->device);
  std::unique_ptr<clg_engine> e(new clg_engine());
  e->cfg = *cfg;
  e->fused_decode = !(cfg->flags & CLG_F_ROBUST_DECODE) && !e->sw.robust_decode;
  e->small_decode = !(cfg->flags & CLG_F_NO_SMALL_DECODE) && e->sw.small_decode;
  if (e->sw.jser_arena) e->jarena_bytes = e->sw.jser_arena;
  HIPCHK(hipSetDevice(cfg->device));
  {
    // The device-output slice gather (HBM-bound) runs beside the next decode (VALU-bound):
    // its queue gets the higher priority so its workgroups are dispatched first
    // (CLONOS_GATHER_PRIO=0: same priority as the decode stream; 2: the decode stream's
    // queue higher instead, so the decode's short set-up, scan and read-back launches do not
    // wait behind the gather's workgroups).
    const int mode = e->sw.gather_prio;
    int lo = 0, hi = 0;
    const bool prio = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo;
    if (prio && mode == 2) HIPCHK(hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, hi));
    else HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    if (prio && mode == 1) HIPCHK(hipStreamCreateWithPriority(&e->gstream, hipStreamNonBlocking, hi));
    else HIPCHK(hipStreamCreateWithFlags(&e->gstream, hipStreamNonBlocking));
  }
  HIPCHK(hipEventCreateWithFlags(&e->gready, hipEventDisableTiming));
  const size_t pool_bytes = size_t(cfg->segment_bytes) * cfg->pool_segments;
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, pool_bytes + 2 * kPoolGuard));  // guards: aligned over-reads either side
  e->pool_alloc = p;
  e->pool = static_cast<uint8_t*>(p) + kPoolGuard;
  e->free_segs.resize(cfg->pool_segments);
  for (uint32_t i = 0; i < cfg->pool_segments; ++i) e->free_segs[i] = cfg->pool_segments - 1 - i;
  e->seg_life.assign(cfg->pool_segments, 0u);
  // the sidecar: C / 64 entries per segment (256 for 16 KiB: config 3 averages ~100), its
  // positions 16 bits (segments up to 64 KiB); CLONOS_SIDECAR=0 turns it off (developer A/B)
  if (cfg->segment_bytes <= 65536u && cfg->pool_segments && e->sw.sidecar) {
    const uint32_t cap = std::min<uint32_t>(clg::kSideCapMax, std::max<uint32_t>(8u, cfg->segment_bytes / 64u));
    const size_t hb = size_t(cfg->pool_segments) * 8, eb = size_t(cfg->pool_segments) * cap * 4;
    // (no room beside a pool sized to the HBM: the engine runs without it, the decode scans)
    if (hipMalloc(&p, hb + eb) == hipSuccess) {
      e->side_alloc = p;
      HIPCHK(hipMemset(p, 0, hb));  // life 0: every segment's first chunk starts its list
      e->side = clg::SideCar{static_cast<uint64_t*>(p), reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(p) + hb),
                             e->pool, pool_bytes, cfg->segment_bytes, cap};
    } else {
      (void)hipGetLastError();  // (the failed allocation is not the engine's error)
    }
  }
  e->ifl_C = cfg->ifl_segment_bytes ? cfg->ifl_segment_bytes : 32768u;
  const uint32_t ifl_n = cfg->ifl_pool_segments ? cfg->ifl_pool_segments : 4096u;
  if (e->ifl_C % 16) return fail(CLG_E_INVALID_ARG, "ifl_segment_bytes must be a multiple of 16");
  e->cfg.ifl_segment_bytes = e->ifl_C;
  e->cfg.ifl_pool_segments = ifl_n;
  HIPCHK(hipMalloc(&p, size_t(e->ifl_C) * ifl_n + 2 * kPoolGuard));
  e->ifl_alloc = p;
  e->ifl_pool = static_cast<uint8_t*>(p) + kPoolGuard;
  e->ifl_free.resize(ifl_n);
  for (uint32_t i = 0; i < ifl_n; ++i) e->ifl_free[i] = ifl_n - 1 - i;
  e->jobs.emplace_back();  // job 0: the default job
  e->jobs[0].open = true;
  e->jobs[0].depth = cfg->sharing_depth;
  *out = e.release();
  return CLG_OK;
}

void clg_engine_destroy(clg_engine* e) {
  if (!e) return;
  hipSetDevice(e->cfg.device);
  e->settle();  // a pending asynchronous decode: its events go back to the pool
  hipStreamSynchronize(e->stream);
  e->gwait();
  for (auto& t : e->timings) {
    hipEventDestroy(t.a);
    hipEventDestroy(t.b);
  }
  for (auto ev : e->ev_pool) hipEventDestroy(ev);
  for (auto ev : e->zdone)
    if (ev) hipEventDestroy(ev);
  if (e->pool_alloc) hipFree(e->pool_alloc);
  if (e->side_alloc) hipFree(e->side_alloc);
  if (e->ifl_alloc) hipFree(e->ifl_alloc);
  hipStreamDestroy(e->stream);
  if (e->gstream) hipStreamDestroy(e->gstream);
  if (e->gready) hipEventDestroy(e->gready);
  for (auto ev : e->gdone)
    if (ev) hipEventDestroy(ev);
  delete e;
}

void* clg_engine_stream(clg_engine* e) { return e ? (void*)e->stream : nullptr; }
void* clg_gather_stream(clg_engine* e) { return e ? (void*)e->gstream : nullptr; }

int clg_sync(clg_engine* e) {
  ENGINE_GUARD(e);
  CHK(e->flush());
  return e->sync();
}

int clg_pool_stats(clg_engine* e, uint32_t* used, uint32_t* free_segments) {
  ENGINE_GUARD(e);
  *free_segments = uint32_t(e->free_segs.size());
  *used = e->cfg.pool_segments - *free_segments;
  return CLG_OK;
}

int clg_job_open(clg_engine* e, uint64_t job_lo, uint64_t job_hi, int32_t sharing_depth, uint32_t* job) {
  ENGINE_GUARD(e);
  if (!job) return fail(CLG_E_INVALID_ARG, "null argument");
  for (uint32_t j = 0; j < e->jobs.size(); ++j)
    if (e->jobs[j].open && e->jobs[j].lo == job_lo && e->jobs[j].hi == job_hi && j != 0)
      return fail(CLG_E_INVALID_ARG, "job already open");
  Job nj;
  nj.open = true;
  nj.lo = job_lo;
  nj.hi = job_hi;
  nj.depth = sharing_depth;
  for (uint32_t j = 1; j < e->jobs.size(); ++j)
    if (!e->jobs[j].open) {
      e->jobs[j] = nj;
      *job = j;
      return CLG_OK;
    }
  e->jobs.push_back(nj);
  *job = uint32_t(e->jobs.size() - 1);
  return CLG_OK;
}

int clg_job_close(clg_engine* e, uint32_t job) {
  ENGINE_GUARD(e);
  if (job >= e->jobs.size() || !e->jobs[job].open) return fail(CLG_E_NO_LOG, "unknown job %u", job);
  for (uint32_t h = 0; h < e->logs.size(); ++h)
    if (e->logs[h].open && e->logs[h].job == job) CHK(clg_log_close(e, h));
  if (job != 0) e->jobs[job] = Job();
  else e->jobs[0].latest_cp = 0;
  return CLG_OK;
}

int clg_log_open(clg_engine* e, uint32_t job, const clg_causal_log_id* id, uint32_t* handle) {
  ENGINE_GUARD(e);
  if (!id || !handle) return fail(CLG_E_INVALID_ARG, "null argument");
  if (job >= e->jobs.size() || !e->jobs[job].open) return fail(CLG_E_NO_LOG, "unknown job %u", job);
  const IdKey k = key_of(job, *id);
  if (e->by_id.count(k)) return fail(CLG_E_INVALID_ARG, "log already open");
  Log l;
  l.id = *id;
  l.job = job;
  l.depth = e->jobs[job].depth;
  l.open = true;
  if (e->free_segs.empty()) return fail(CLG_E_NOSPACE, "segment pool exhausted");
  l.segs.push_back(e->free_segs.back());  // ctor addComponent() :102
  ++e->seg_life[e->free_segs.back()];
  e->free_segs.pop_back();
  const uint32_t h = uint32_t(e->logs.size());  // handles are never reused: a stale one is CLG_E_NO_LOG
  e->logs.push_back(std::move(l));
  e->by_id[k] = h;
  *handle = h;
  return CLG_OK;
}

int clg_log_close(clg_engine* e, uint32_t h) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  CHK(e->sync());
  for (uint32_t s : l->segs) e->free_segs.push_back(s);
  e->by_id.erase(key_of(l->job, l->id));
  *l = Log();
  return CLG_OK;
}

int clg_log_find(clg_engine* e, uint32_t job, const clg_causal_log_id* id, uint32_t* handle) {
  ENGINE_GUARD(e);
  auto it = e->by_id.find(key_of(job, *id));
  if (it == e->by_id.end()) return fail(CLG_E_NO_LOG, "log not found");
  *handle = it->second;
  return CLG_OK;
}

int clg_log_get_id(clg_engine* e, uint32_t h, clg_causal_log_id* id, uint32_t* job) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  if (id) *id = l->id;
  if (job) *job = l->job;
  return CLG_OK;
}

int clg_append(clg_engine* e, uint32_t log, int64_t epoch, const uint8_t* rec, uint32_t n) {
  bool spill;
  {
    LOG_GUARD(e, log);
    CHK(e->append(log, epoch, rec, n));
    spill = e->over_stage_limit(log);
  }
  if (!spill) return CLG_OK;
  ENGINE_GUARD(e);  // bounded write-behind: this log's staged bytes go to HBM now
  return e->flush();
}

int clg_append_batch(clg_engine* e, const uint32_t* log, const int64_t* epoch, const uint64_t* off,
                     const uint32_t* len, uint32_t n, const uint8_t* bytes) {
  ENGINE_GUARD(e);
  for (uint32_t i = 0; i < n; ++i) CHK(e->append(log[i], epoch[i], bytes + off[i], len[i]));
  return CLG_OK;
}

int clg_upstream_delta(clg_engine* e, uint32_t log, int64_t epoch, int32_t off, const uint8_t* d, uint32_t n) {
  bool spill;
  {
    LOG_GUARD(e, log);
    CHK(e->upstream(log, epoch, off, d, n));
    spill = e->over_stage_limit(log);
  }
  if (!spill) return CLG_OK;
  ENGINE_GUARD(e);
  return e->flush();
}

int clg_log_length(clg_engine* e, uint32_t h, int32_t* out) {  // :180-192
  LOG_GUARD(e, h);
  Log* l;
  CHK(e->get_log(h, &l));
  *out = l->epochs.empty() ? l->writer : l->writer - l->epochs.begin()->offset;
  return CLG_OK;
}

int clg_log_length_batch(clg_engine* e, const uint32_t* log, uint32_t n, int32_t* out, uint64_t* total) {
  ENGINE_GUARD(e);
  if (n && !log) return fail(CLG_E_INVALID_ARG, "null argument");
  uint64_t t = 0;
  for (uint32_t i = 0; i < n; ++i) {
    Log* l;
    CHK(e->get_log(log[i], &l));
    const int32_t v = l->epochs.empty() ? l->writer : l->writer - l->epochs.begin()->offset;
    if (out) out[i] = v;
    t += uint64_t(v);
  }
  if (total) *total = t;
  return CLG_OK;
}

int clg_has_delta(clg_engine* e, uint32_t log, clg_channel_id c, int64_t epoch, int32_t* out) {
  LOG_GUARD(e, log);
  return e->has_delta(log, ChKey{c.lo, c.hi}, epoch, out);
}

int clg_offset_from_epoch(clg_engine* e, uint32_t log, clg_channel_id c, int32_t* out) {
  LOG_GUARD(e, log);
  return e->offset_from_epoch(log, ChKey{c.lo, c.hi}, out);
}

}  // extern "C"

extern "C" {

int clg_notify_checkpoint_complete(clg_engine* e, uint32_t h, int64_t cp) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  CHK(e->flush());
  return e->checkpoint_complete(*l, cp);
}

int clg_unregister_consumer(clg_engine* e, uint32_t h, clg_channel_id c) {
  LOG_GUARD(e, h);
  Log* l;
  CHK(e->get_log(h, &l));
  l->consumers.erase(ChKey{c.lo, c.hi});
  return CLG_OK;
}

int clg_log_get_state(clg_engine* e, uint32_t h, clg_log_state* st, int64_t* ids, int32_t* offs, int32_t cap) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  st->writer = l->writer;
  st->capacity = e->capacity(*l);
  st->n_components = int32_t(l->segs.size());
  st->n_epochs = int32_t(l->epochs.size());
  int32_t i = 0;
  for (auto& ep : l->epochs) {
    if (i < cap) {
      if (ids) ids[i] = ep.id;
      if (offs) offs[i] = ep.offset;
    }
    ++i;
  }
  return i > cap && (ids || offs) ? fail(CLG_E_CAPACITY, "%d epochs", i) : CLG_OK;
}

int clg_consumer_state(clg_engine* e, uint32_t h, clg_channel_id c, int32_t* exists, int64_t* epoch, int32_t* offset) {
  ENGINE_GUARD(e);
  Log* l;
  CHK(e->get_log(h, &l));
  auto ci = l->consumers.find(ChKey{c.lo, c.hi});
  *exists = ci != l->consumers.end();
  if (*exists) {
    *epoch = ci->second.es->id;
    *offset = ci->second.offset;
  }
  return CLG_OK;
}

}  // extern "C"

extern "C" {

int clg_consumer_seek(clg_engine* e, uint32_t h, clg_channel_id c, int64_t epoch, int32_t offset) {
  ENGINE_GUARD_KEEP(e);
  Log* l;
  CHK(e->get_log(h, &l));
  auto it = l->epochs.find(epoch);
  if (it == l->epochs.end()) return fail(CLG_E_STATE, "epoch %lld not in log", (long long)epoch);
  l->consumers[ChKey{c.lo, c.hi}] = Consumer{EpochMap::ref(*it), offset};
  return CLG_OK;
}

int clg_upstream_delta_batch(clg_engine* e, clg_delta_req* reqs, uint32_t n, const uint8_t* bytes, uint32_t in_kind) {
  ENGINE_GUARD_KEEP(e);
  clg_engine::HostTimer ht(e, "host_abi_upstream");  // (CLONOS_HOST_PROF: lock held to here; settle and the call)
  e->settle();
  if (n && (!reqs || !bytes)) return fail(CLG_E_INVALID_ARG, "null argument");
  return e->upstream_batch(reqs, n, bytes, in_kind);
}

int clg_consumer_seek_batch(clg_engine* e, const clg_slice_req* reqs, const int32_t* offsets, uint32_t n) {
  ENGINE_GUARD_KEEP(e);
  if (n && (!reqs || !offsets)) return fail(CLG_E_INVALID_ARG, "null argument");
  for (uint32_t i = 0; i < n; ++i) {
    Log* l;
    CHK(e->get_log(reqs[i].log, &l));
    auto it = l->epochs.find(reqs[i].epoch);
    if (it == l->epochs.end()) return fail(CLG_E_STATE, "epoch %lld not in log", (long long)reqs[i].epoch);
    l->consumers[ChKey{reqs[i].consumer.lo, reqs[i].consumer.hi}] = Consumer{EpochMap::ref(*it), offsets[i]};
  }
  return CLG_OK;
}

int clg_truncate_all(clg_engine* e, uint32_t job, int64_t cp, int32_t* applied) {  // JobCausalLogImpl :230-246
  // Beside queued asynchronous decodes whose ranges start at or above cp (config 4's step:
  // the host truncates while the GPU decodes the new epoch): the truncation only drops bytes
  // below cp, so the queued kernels read nothing it frees -- its segments return to the pool
  // once those decodes complete.  Otherwise (a decode from below cp, appends not yet flushed)
  // the queued decodes complete first.
  ENGINE_GUARD_KEEP(e);
  bool defer = false;
  if (e->any_active()) {
    int64_t mn = INT64_MAX;
    for (const auto& d : e->pq)
      if (d.active) mn = std::min(mn, d.min_epoch);
    const bool dirty = !e->dirty.empty();  // (appends not yet flushed: the flush below writes segments)
    if (cp > mn || dirty) CHK(e->settle());
    else defer = true;
  } else {
    e->release_later();
  }
  if (applied) *applied = 0;
  if (job >= e->jobs.size() || !e->jobs[job].open) return fail(CLG_E_NO_LOG, "unknown job %u", job);
  Job& j = e->jobs[job];
  if (j.latest_cp >= cp) return CLG_OK;  // the CAS: only a newer checkpoint fans out
  j.latest_cp = cp;
  ++e->rebase_gen;
  std::vector<uint32_t>& to = defer ? e->free_later : e->free_segs;
  CHK(e->flush());
  clg_engine::HostTimer ht(e, "host_truncate_all");
  if (e->logs.size() >= clg_engine::kParallelLogs) {
    // 66 k logs (config 4): the host threads take parts of the log table.  A log whose epochs
    // below cp hold shared EpochStart objects (a consumer refers to them) is left to this
    // thread (their blocks go back to a per-thread free list); each part collects its freed
    // segments, which join the pool after.
    WorkPool* wp = e->workers();
    const unsigned P = wp->size();
    const size_t nl = e->logs.size(), per = (nl + P - 1) / P;
    std::vector<std::vector<uint32_t>> freed(P), later(P);
    std::vector<int> st(P, CLG_OK);
    wp->run([&](unsigned k, unsigned) {
      const size_t i1 = std::min(nl, (k + 1) * per);
      for (size_t i = k * per; i < i1; ++i) {
        if (i + 8 < i1) {  // the Log objects ahead (per-log work is bound by their cache misses)
          const char* q = reinterpret_cast<const char*>(&e->logs[i + 8]);
          for (size_t b = 0; b < sizeof(Log); b += 64) __builtin_prefetch(q + b, 1);
        }
        Log& l = e->logs[i];
        if (!l.open || l.job != job) continue;
        bool shared = false;
        for (const EpochEnt& x : l.epochs) {
          if (x.id >= cp) break;
          shared |= x.shared != nullptr;
        }
        if (shared) {
          later[k].push_back(uint32_t(i));
          continue;
        }
        if ((st[k] = e->checkpoint_complete(l, cp, freed[k])) != CLG_OK) return;
      }
    });
    ht.lap("host_trunc_pool");
    for (unsigned k = 0; k < P; ++k) to.insert(to.end(), freed[k].begin(), freed[k].end());
    for (unsigned k = 0; k < P; ++k)
      if (st[k] != CLG_OK) return fail(st[k], "checkpoint completion failed on a log (state outside its bounds)");
    size_t n_later = 0;
    for (unsigned k = 0; k < P; ++k) {
      n_later += later[k].size();
      for (uint32_t i : later[k]) CHK(e->checkpoint_complete(e->logs[i], cp, to));
    }
    ht.lap(n_later ? "host_trunc_later" : "host_trunc_free");
  } else {
    for (auto& l : e->logs)
      if (l.open && l.job == job) CHK(e->checkpoint_complete(l, cp, to));
  }
  if (applied) *applied = 1;
  return CLG_OK;
}

}  // extern "C"

extern "C" {

int clg_kernel_stats(clg_engine* e, clg_kernel_stat* out, uint32_t cap, uint32_t* n) {
  ENGINE_GUARD(e);
  CHK(e->sync());
  uint32_t i = 0;
  for (auto& kv : e->stats) {
    if (i < cap) {
      memset(&out[i], 0, sizeof out[i]);
      snprintf(out[i].name, sizeof out[i].name, "%s", kv.first.c_str());
      out[i].launches = kv.second.launches;
      out[i].total_ms = kv.second.ms;
      out[i].bytes = kv.second.bytes;
    }
    ++i;
  }
  *n = i;
  return CLG_OK;
}

int clg_kernel_stats_reset(clg_engine* e) {
  ENGINE_GUARD(e);
  CHK(e->sync());
  e->stats.clear();
  return CLG_OK;
}

}  // extern "C"
