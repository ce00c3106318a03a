// engine_replay.cpp -- what recovery and the delta messages batch over the engine's other units:
// clg_replay_prep, replay preparation in its soa and columns forms (clg_replay_prepare*),
// clg_encode_batch, and the delta messages' headers written and parsed on the host
// (clg_enrich_batch, clg_process_delta).
#include "engine_columns.h"
#include "columns.h"
#include "pack_wide.h"

extern "C" {

int clg_replay_prep(clg_engine* e, const uint64_t* key, const uint8_t* bytes, const uint64_t* off, const uint64_t* len,
                    uint32_t n, uint32_t* winner, uint32_t* n_keys, clg_decoded* out, uint64_t* span_rec_base) {
  ENGINE_GUARD(e);
  if (n && (!key || !off || !len || !winner || !n_keys)) return fail(CLG_E_INVALID_ARG, "null argument");
  // DeterminantResponseEvent.merge :136-146: per CausalLogID keep the longer buffer,
  // ties -> the later one (v2).  Keys keep first-appearance order.
  std::unordered_map<uint64_t, uint32_t> best;
  std::vector<uint64_t> order;
  for (uint32_t i = 0; i < n; ++i) {
    auto it = best.find(key[i]);
    if (it == best.end()) {
      best.emplace(key[i], i);
      order.push_back(key[i]);
    } else if (!(len[it->second] > len[i])) {
      it->second = i;
    }
  }
  *n_keys = uint32_t(order.size());
  std::vector<uint64_t> so(order.size()), sl(order.size());
  for (size_t k = 0; k < order.size(); ++k) {
    winner[k] = best[order[k]];
    so[k] = off[winner[k]];
    sl[k] = len[winner[k]];
  }
  if (!out) return CLG_OK;
  return clg_decode_host(e, bytes, so.data(), sl.data(), uint32_t(order.size()), out, span_rec_base);
}

}  // extern "C"

// ReplayingState (:58-66, :108-130) + SubpartitionRecoveryThread.run (:157-188) +
// LogReplayerImpl (:51-158), batched over failed vertices.  Main logs go through the
// batched decode; subpartition recovery buffers through k_bufsizes (5-byte BufferBuilt
// records, no chain walk).  All inputs are staged to HBM in one copy.
//
// replay_prepare is both forms' lookup, staging, subpartition kernels and outputs; only the
// main-log step differs: `main(build, main_bytes, staged)` decodes the main logs (span i = vertex
// i) from the plan `build` fills over the staged bytes, whose places `staged` gives as contiguous
// PaySpans.  finish_sub: a main step that fails does not end the call before the subpartition
// outputs are delivered (the columns form: a decode error is a result there); its status is the
// call's.
namespace {
struct ReplaySubOut {  // clg_replay_out's subpartition fields
  int32_t* buffer_sizes;
  uint64_t sizes_cap;
  uint64_t* sizes_base;
  uint64_t* sub_count;
  int32_t* sub_status;
  int64_t* sub_err_off;
  int32_t* sub_err_tag;
};
using ReplayBuild = clg_engine::PlanBuild;
using ReplayMain = std::function<int(const ReplayBuild&, uint64_t, const std::vector<clg::PaySpan>&)>;
}  // namespace
static int replay_prepare(clg_engine* e, const clg_replay_vertex* v, uint32_t n, const ReplaySubOut* out, bool dev_in,
                          bool finish_sub, const ReplayMain& main);
static int replay_prepare_soa(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_out* out, bool dev_in) {
  ENGINE_GUARD(e);
  if (!out || !out->main || !out->main_rec_base || (n && !v)) return fail(CLG_E_INVALID_ARG, "null argument");
  const ReplaySubOut so{out->buffer_sizes, out->sizes_cap,   out->sizes_base, out->sub_count,
                        out->sub_status,   out->sub_err_off, out->sub_err_tag};
  return replay_prepare(e, v, n, &so, dev_in, false,
                        [&](const ReplayBuild& build, uint64_t main_bytes, const std::vector<clg::PaySpan>&) {
                          return e->decode(build, main_bytes, out->main, out->main_rec_base);
                        });
}

extern "C" {

int clg_replay_prepare(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_out* out) {
  return replay_prepare_soa(e, v, n, out, false);
}
int clg_replay_prepare_device(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_out* out) {
  return replay_prepare_soa(e, v, n, out, true);
}

}  // extern "C"

// The columns form: the main step is the decode into engine scratch, the columns of what it
// produced, and (var set) the payload column of the wide rows, gathered from the bytes where
// replay_prepare staged them.  They are not staged a second time: d_stage has two writers,
// flush() and stage_spans(), and neither runs between the staging and the payload gather -- the
// decode and its fallbacks re-plan at the same addresses, the column kernels do not touch it, and
// the spans handed to the gather are contiguous device memory already (no payload_spans_bytes).
static int replay_prepare_columns(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_columns_out* out,
                                  bool dev_in) {
  ENGINE_GUARD(e);
  if (!out || !out->main || (n && !v)) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::col_reset_result(out->main);
  if (out->var) clg::pay_reset_result(out->var);
  const ReplaySubOut so{out->buffer_sizes, out->sizes_cap,   out->sizes_base, out->sub_count,
                        out->sub_status,   out->sub_err_off, out->sub_err_tag};
  return replay_prepare(
      e, v, n, &so, dev_in, true, [&](const ReplayBuild& build, uint64_t main_bytes, const std::vector<clg::PaySpan>& staged) {
        const auto run = [&](clg_decoded* d, uint64_t* base) { return e->decode(build, main_bytes, d, base); };
        if (!out->var) return decode_columns(e, run, n, out->main);
        return decode_columns_var(e, run, n, out->main, out->var, [&](std::vector<clg::PaySpan>& spans, std::vector<uint32_t>&) {
          spans = staged;
          return CLG_OK;
        });
      });
}

extern "C" {

int clg_replay_prepare_columns(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_columns_out* out) {
  return replay_prepare_columns(e, v, n, out, false);
}
int clg_replay_prepare_columns_device(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_columns_out* out) {
  return replay_prepare_columns(e, v, n, out, true);
}

}  // extern "C"

// The packed form: the main step is the packed decodes' body (decode_columns_packed) over the
// staged bytes, with the staged spans for the payload gather as above.
static int replay_prepare_packed(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_packed_out* out, bool dev_in) {
  ENGINE_GUARD(e);
  if (!out || !out->sizes || !out->narrow || (n && !v)) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::col_reset_result(out->sizes);
  clg::pack_reset_result(out->narrow);
  if (out->wide) clg::wpack_reset_result(out->wide);
  if (out->var) clg::pay_reset_result(out->var);
  const ReplaySubOut so{out->buffer_sizes, out->sizes_cap,   out->sizes_base, out->sub_count,
                        out->sub_status,   out->sub_err_off, out->sub_err_tag};
  return replay_prepare(
      e, v, n, &so, dev_in, true, [&](const ReplayBuild& build, uint64_t main_bytes, const std::vector<clg::PaySpan>& staged) {
        const auto run = [&](clg_decoded* d, uint64_t* base) { return e->decode(build, main_bytes, d, base); };
        return decode_columns_packed(
            e, run, n, out->sizes, out->var, out->narrow,
            [&](std::vector<clg::PaySpan>& spans, std::vector<uint32_t>&) {
              spans = staged;
              return CLG_OK;
            },
            out->wide);
      });
}

extern "C" {

int clg_replay_prepare_columns_packed(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_packed_out* out) {
  return replay_prepare_packed(e, v, n, out, false);
}
int clg_replay_prepare_columns_packed_device(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_packed_out* out) {
  return replay_prepare_packed(e, v, n, out, true);
}

}  // extern "C"

// Pinned read-back of replay-prep's subpartition results: sizes, then count, err_off (8 B
// each), status, err_tag (4 B each) per subpartition, as they lie on the device.
static size_t o_rout_cnt(uint64_t n_sizes) { return (size_t(n_sizes) * 4 + 15) & ~size_t(15); }
static size_t o_rout_end(uint32_t ns, uint64_t n_sizes) { return o_rout_cnt(n_sizes) + size_t(ns) * 24 + 64; }
static int replay_prepare(clg_engine* e, const clg_replay_vertex* v, uint32_t n, const ReplaySubOut* out, bool dev_in,
                          bool finish_sub, const ReplayMain& main) {
  clg_engine::HostTimer lap(e, "host_replay_rest");  // (laps below: the sections)
  struct Piece {
    const uint8_t* p;
    uint64_t len;
  };
  std::vector<Piece> mains(n), subs;
  // the accumulated map's entries by CausalLogID (equals :128-149), per vertex: an
  // open-addressing table, O(entries + subpartitions) (a std::map took 0.16 ms for config 5's
  // 16 vertices x 129 entries)
  std::vector<IdKey> keys;
  std::vector<uint32_t> slot;  // entry index + 1 (0: empty)
  uint64_t mask = 0;
  const clg_response* indexed = nullptr;
  auto hkey = [](const IdKey& k) {  // splitmix64 finaliser over the fields (a vertex's keys differ in sub only)
    auto mix = [](uint64_t z) {
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      return z ^ (z >> 31);
    };
    return mix(mix(uint64_t(uint16_t(k.v)) | uint64_t(k.main) << 16 | (uint64_t(uint8_t(k.sub)) << 24 ^ uint64_t(k.lo))) ^
               uint64_t(k.hi));
  };
  auto same = [](const IdKey& a, const IdKey& b) {
    return a.v == b.v && a.main == b.main && a.sub == b.sub && a.lo == b.lo && a.hi == b.hi;
  };
  auto lookup = [&](const clg_response* r, const clg_causal_log_id& id) -> Piece {
    if (!r) return Piece{nullptr, 0};
    if (r != indexed) {
      uint64_t size = 16;
      while (size < 2ull * r->n) size <<= 1;
      mask = size - 1;
      slot.assign(size, 0u);
      keys.resize(r->n);
      for (uint32_t i = 0; i < r->n; ++i) {
        keys[i] = key_of(0, r->entries[i].id);
        uint64_t h = hkey(keys[i]) & mask;
        while (slot[h] && !same(keys[slot[h] - 1], keys[i])) h = (h + 1) & mask;
        if (!slot[h]) slot[h] = i + 1;  // the first of equal keys
      }
      indexed = r;
    }
    const IdKey k = key_of(0, id);
    for (uint64_t h = hkey(k) & mask; slot[h]; h = (h + 1) & mask)
      if (same(keys[slot[h] - 1], k)) return Piece{r->entries[slot[h] - 1].bytes, r->entries[slot[h] - 1].len};
    return Piece{nullptr, 0};
  };
  subs.reserve(1024);
  for (uint32_t i = 0; i < n; ++i) {
    if (v[i].n_subpartitions && !v[i].subpartitions) return fail(CLG_E_INVALID_ARG, "null subpartition table");
    clg_causal_log_id mid{};
    mid.vertex_id = v[i].vertex_id;
    mid.is_main = 1;
    mains[i] = lookup(v[i].acc, mid);
    for (uint32_t j = 0; j < v[i].n_subpartitions; ++j) {
      clg_causal_log_id sid = v[i].subpartitions[j];
      sid.vertex_id = v[i].vertex_id;  // id.replace(lower, upper, index) keeps the vertex (:114, :121)
      sid.is_main = 0;
      subs.push_back(lookup(v[i].acc, sid));
    }
  }
  lap.lap("host_replay_index");
  const uint32_t ns = uint32_t(subs.size());
  if (ns && (!out->sizes_base || !out->sub_count || !out->sub_status || !out->sub_err_off || !out->sub_err_tag))
    return fail(CLG_E_INVALID_ARG, "null subpartition output");
  // sizes capacity: one slot per whole 5-byte record
  uint64_t n_sizes = 0;
  for (uint32_t j = 0; j < ns; ++j) {
    out->sizes_base[j] = n_sizes;
    n_sizes += subs[j].len / 5;
  }
  if (ns) out->sizes_base[ns] = n_sizes;
  if (n_sizes > out->sizes_cap || (n_sizes && !out->buffer_sizes))
    return fail(CLG_E_CAPACITY, "buffer_sizes needs %llu entries", (unsigned long long)n_sizes);
  // stage main logs then subpartition buffers (16-byte aligned pieces) in one copy
  std::vector<uint64_t> at(n + ns);
  uint64_t total = 0, main_bytes = 0, sub_bytes = 0;
  for (uint32_t i = 0; i < n + ns; ++i) {
    const Piece& pc = i < n ? mains[i] : subs[i - n];
    at[i] = total;
    total += (pc.len + 15) & ~uint64_t(15);
    (i < n ? main_bytes : sub_bytes) += pc.len;
  }
  CHK(e->d_stage.ensure(total + 16));
  if (dev_in) {  // the winners already in HBM (e.g. an RCCL receive buffer): one device gather
    std::vector<clg::GatherPiece> pieces;
    for (uint32_t i = 0; i < n + ns; ++i) {
      const Piece& pc = i < n ? mains[i] : subs[i - n];
      for (uint64_t o = 0; o < pc.len; o += 1u << 30)  // a piece's length is 32-bit
        pieces.push_back(clg::GatherPiece{pc.p + o, at[i] + o, uint32_t(std::min<uint64_t>(pc.len - o, 1u << 30)), 0});
    }
    // (no wait: the kernels below read the staged bytes on the same stream)
    CHK(e->run_gather(pieces, total, e->d_stage.p, CLG_MEM_DEVICE, "replay_stage", false));
  } else {
    CHK(e->h_stage.ensure(total + 16));
    for (uint32_t i = 0; i < n + ns; ++i) {
      const Piece& pc = i < n ? mains[i] : subs[i - n];
      if (pc.len) memcpy(e->h_stage.as<uint8_t>() + at[i], pc.p, pc.len);
    }
    if (total) HIPCHK(hipMemcpyAsync(e->d_stage.p, e->h_stage.p, total, hipMemcpyHostToDevice, e->stream));
  }
  lap.lap("host_replay_stage");
  const uint8_t* dst = e->d_stage.as<uint8_t>();
  // subpartition buffers first (their kernels only read the staged bytes)
  std::function<int(clg::JArena)> classify;
  const int32_t* d_sub_status = nullptr;
  if (ns) {
    std::vector<clg::BufSpan> bs(ns);
    std::vector<clg::BufChunk> bc;
    constexpr uint64_t kRecPerChunk = 256;
    for (uint32_t j = 0; j < ns; ++j) {
      bs[j] = clg::BufSpan{dst + at[n + j], subs[j].len, out->sizes_base[j]};
      const uint64_t nk = (subs[j].len + 4) / 5;  // records incl. a partial tail
      for (uint64_t k = 0; k < nk; k += kRecPerChunk)
        bc.push_back(clg::BufChunk{j, 0, k, std::min(nk, k + kRecPerChunk)});
    }
    const size_t o_spans = 0, o_chunks = (ns * sizeof(clg::BufSpan) + 15) & ~size_t(15);
    const size_t o_res = (o_chunks + bc.size() * sizeof(clg::BufChunk) + 15) & ~size_t(15);
    const size_t res_bytes = size_t(ns) * (8 + 8 + 4 + 8 + 4);  // first_bad, count, status, err_off, err_tag
    CHK(e->h_rmeta.ensure(o_res + res_bytes + 64));
    CHK(e->d_rmeta.ensure(o_res + res_bytes + 64));
    uint8_t* hm = e->h_rmeta.as<uint8_t>();
    memcpy(hm + o_spans, bs.data(), ns * sizeof(clg::BufSpan));
    memcpy(hm + o_chunks, bc.data(), bc.size() * sizeof(clg::BufChunk));
    HIPCHK(hipMemcpyAsync(e->d_rmeta.p, hm, o_res, hipMemcpyHostToDevice, e->stream));
    uint8_t* dm = e->d_rmeta.as<uint8_t>();
    uint64_t* d_first = reinterpret_cast<uint64_t*>(dm + o_res);
    uint64_t* d_count = d_first + ns;
    int64_t* d_eoff = reinterpret_cast<int64_t*>(d_count + ns);
    int32_t* d_status = reinterpret_cast<int32_t*>(d_eoff + ns);
    int32_t* d_etag = d_status + ns;
    HIPCHK(hipMemsetAsync(d_first, 0xFF, ns * 8, e->stream));
    CHK(e->d_rsizes.ensure(std::max<uint64_t>(1, n_sizes) * 4));
    const auto* d_spans = reinterpret_cast<const clg::BufSpan*>(dm + o_spans);
    CHK(e->timed("replay_bufsizes", sub_bytes + 4 * n_sizes, [&] {
      return clg::launch_bufsizes(reinterpret_cast<const clg::BufChunk*>(dm + o_chunks), uint32_t(bc.size()), d_spans,
                                  e->d_rsizes.as<int32_t>(), d_first, e->stream);
    }));
    clg::JArena jar;
    CHK(e->jarena_reset(&jar));
    CHK(clg::launch_bufsizes_classify(d_spans, ns, d_first, d_count, d_status, d_eoff, d_etag, jar, e->stream));
    CHK(e->jarena_clear_note(1));
    CHK(e->jarena_note(1));
    classify = [=](clg::JArena a) {
      return clg::launch_bufsizes_classify(d_spans, ns, d_first, d_count, d_status, d_eoff, d_etag, a, e->stream);
    };
    d_sub_status = d_status;
    // read back into pinned memory (asynchronous; into the caller's pageable arrays each copy
    // was a staged synchronous one), copied out after the decode's sync below
    CHK(e->h_rout.ensure(o_rout_end(ns, n_sizes)));
    uint8_t* hr = e->h_rout.as<uint8_t>();
    if (n_sizes) HIPCHK(hipMemcpyAsync(hr, e->d_rsizes.p, n_sizes * 4, hipMemcpyDeviceToHost, e->stream));
    // count, err_off, status, err_tag: adjacent on the device (d_first's block): one copy
    HIPCHK(hipMemcpyAsync(hr + o_rout_cnt(n_sizes), d_count, size_t(ns) * 24, hipMemcpyDeviceToHost, e->stream));
  }
  lap.lap("host_replay_sizes");
  // main logs: the batched decode (span i = vertex i)
  const ReplayBuild build = [&](clg_engine::DecodePlan& p, uint32_t T) {
    for (uint32_t i = 0; i < n; ++i) e->plan_host_span(p, dst + at[i], mains[i].len, i, T);
  };
  std::vector<clg::PaySpan> staged(n);
  for (uint32_t i = 0; i < n; ++i) staged[i] = clg::PaySpan{mains[i].len ? dst + at[i] : nullptr, 0, mains[i].len, 0, 0};
  const int main_status = main(build, main_bytes, staged);
  if (main_status != CLG_OK && !finish_sub) return main_status;
  const std::string main_err = main_status != CLG_OK ? g_err : std::string();
  lap.lap("host_replay_decode");
  CHK(e->sync());
  // a Serializable walk in a subpartition buffer found the spill arena full: again, larger
  uint8_t* hr = e->h_rout.as<uint8_t>();
  const size_t oc = o_rout_cnt(n_sizes);
  while (ns && e->jarena_spilled(1)) {
    CHK(e->jarena_grow());
    clg::JArena jar;
    CHK(e->jarena_reset(&jar));
    CHK(classify(jar));
    CHK(e->jarena_note(1));
    HIPCHK(hipMemcpyAsync(hr + oc + size_t(ns) * 16, d_sub_status, size_t(ns) * 4, hipMemcpyDeviceToHost, e->stream));
    CHK(e->sync());
  }
  if (ns) {
    if (n_sizes) memcpy(out->buffer_sizes, hr, n_sizes * 4);
    memcpy(out->sub_count, hr + oc, size_t(ns) * 8);
    memcpy(out->sub_err_off, hr + oc + size_t(ns) * 8, size_t(ns) * 8);
    memcpy(out->sub_status, hr + oc + size_t(ns) * 16, size_t(ns) * 4);
    memcpy(out->sub_err_tag, hr + oc + size_t(ns) * 20, size_t(ns) * 4);
  }
  lap.lap("host_replay_finish");
  if (main_status != CLG_OK) g_err = main_err;
  return main_status;
}

extern "C" {

// SimpleDeterminantEncoder.encodeTo over a batch (encode.hip): sizes pass, one host read
// of the total, write pass.
int clg_encode_batch(clg_engine* e, const clg_encode_in* in, void* out, uint64_t cap, uint32_t out_kind,
                     uint64_t* n_out, uint64_t* bad_index) {
  ENGINE_GUARD(e);
  if (!in || !n_out || (in->n && (!in->tag || !in->v0)) ||
      (in->n_wide && (!in->w_idx || !in->w_rc || !in->w_v1 || !in->w_var_off || !in->w_var_len || !in->w_sub)) ||
      (in->var_len && !in->var))
    return fail(CLG_E_INVALID_ARG, "null argument");
  *n_out = 0;
  if (bad_index) *bad_index = UINT64_MAX;
  if (in->n == 0) return CLG_OK;
  const uint64_t n = in->n, nw = in->n_wide;
  clg::EncodeIn d{in->tag,       in->v0,    in->w_idx, in->w_rc, in->w_v1, in->w_var_off,
                  in->w_var_len, in->w_sub, in->var,   n,        nw,       in->var_len};
  if (in->in_kind != CLG_MEM_DEVICE) {  // stage the host arrays in one device buffer
    const size_t sz[9] = {n, 8 * n, 4 * nw, 4 * nw, 8 * nw, 4 * nw, 4 * nw, nw, size_t(in->var_len)};
    const void* src[9] = {in->tag, in->v0, in->w_idx, in->w_rc, in->w_v1, in->w_var_off, in->w_var_len, in->w_sub, in->var};
    size_t off[9], tot = 0;
    for (int i = 0; i < 9; ++i) {
      off[i] = tot;
      tot += (sz[i] + 15) & ~size_t(15);
    }
    CHK(e->d_encin.ensure(tot + 16));
    uint8_t* b = e->d_encin.as<uint8_t>();
    for (int i = 0; i < 9; ++i)
      if (sz[i]) HIPCHK(hipMemcpyAsync(b + off[i], src[i], sz[i], hipMemcpyHostToDevice, e->stream));
    d = clg::EncodeIn{b + off[0], reinterpret_cast<const int64_t*>(b + off[1]), reinterpret_cast<const uint32_t*>(b + off[2]),
                      reinterpret_cast<const int32_t*>(b + off[3]), reinterpret_cast<const int64_t*>(b + off[4]),
                      reinterpret_cast<const uint32_t*>(b + off[5]), reinterpret_cast<const uint32_t*>(b + off[6]),
                      b + off[7], b + off[8], n, nw, in->var_len};
  }
  const uint64_t nb = (n + 1023) / 1024;
  const size_t o_wsum = 0, o_wbase = (nb * 4 + 15) & ~size_t(15), o_bsum = o_wbase + (((nb + 1) * 8 + 15) & ~size_t(15)),
               o_bbase = o_bsum + ((nb * 8 + 15) & ~size_t(15)), o_bad = o_bbase + (((nb + 1) * 8 + 15) & ~size_t(15));
  CHK(e->d_encw.ensure(o_bad + 16));
  uint8_t* w = e->d_encw.as<uint8_t>();
  auto* wsum = reinterpret_cast<uint32_t*>(w + o_wsum);
  auto* wbase = reinterpret_cast<uint64_t*>(w + o_wbase);
  auto* bsum = reinterpret_cast<uint64_t*>(w + o_bsum);
  auto* bbase = reinterpret_cast<uint64_t*>(w + o_bbase);
  auto* bad = reinterpret_cast<uint32_t*>(w + o_bad);
  HIPCHK(hipMemsetAsync(bad, 0xFF, 4, e->stream));
  CHK(clg::launch_encode(d, wsum, wbase, bsum, bbase, bad, nullptr, 0, e->stream));
  uint64_t hres[2] = {0, 0};  // total bytes, wide rows used
  uint32_t hbad = 0;
  HIPCHK(hipMemcpyAsync(&hres[0], bbase + nb, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(&hres[1], wbase + nb, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(&hbad, bad, 4, hipMemcpyDeviceToHost, e->stream));
  CHK(e->sync());
  if (hbad != 0xFFFFFFFFu || hres[1] != nw) {
    if (bad_index) *bad_index = hbad != 0xFFFFFFFFu ? hbad : n;
    return fail(CLG_E_INVALID_ARG,
                "record %llu: invalid tag, side-table row or payload range (%llu wide rows given, %llu used)",
                (unsigned long long)(hbad != 0xFFFFFFFFu ? hbad : n), (unsigned long long)nw,
                (unsigned long long)hres[1]);
  }
  *n_out = hres[0];
  if (hres[0] > cap || !out) return fail(CLG_E_CAPACITY, "encode needs %llu bytes", (unsigned long long)hres[0]);
  uint8_t* dst = static_cast<uint8_t*>(out);
  if (out_kind != CLG_MEM_DEVICE) {
    CHK(e->d_encout.ensure(hres[0] + 16));
    dst = e->d_encout.as<uint8_t>();
  }
  CHK(e->timed("encode_write", hres[0] + 9 * n + 25 * nw + in->var_len,
               [&] { return clg::launch_encode(d, wsum, wbase, bsum, bbase, bad, dst, 1, e->stream); }));
  if (out_kind != CLG_MEM_DEVICE) HIPCHK(hipMemcpyAsync(out, dst, hres[0], hipMemcpyDeviceToHost, e->stream));
  return e->sync();
}

}  // extern "C"

namespace {
void wr16(std::vector<uint8_t>& b, uint16_t v) { b.push_back(uint8_t(v >> 8)); b.push_back(uint8_t(v)); }
void wr32(std::vector<uint8_t>& b, uint32_t v) { wr16(b, uint16_t(v >> 16)); wr16(b, uint16_t(v)); }
void wr64(std::vector<uint8_t>& b, uint64_t v) { wr32(b, uint32_t(v >> 32)); wr32(b, uint32_t(v)); }
uint32_t rd32(const uint8_t* p) { return uint32_t(p[0]) << 24 | uint32_t(p[1]) << 16 | uint32_t(p[2]) << 8 | p[3]; }
uint64_t rd64(const uint8_t* p) { return uint64_t(rd32(p)) << 32 | rd32(p + 4); }
}  // namespace

extern "C" {

// enrichWithCausalLogDelta (AbstractDeltaSerializerDeserializer.java:89-115) for a batch of
// channels: host metadata (hasDelta / offset / take) and header bytes, then one gather
// kernel writes headers and deltas into the output.
int clg_enrich_batch(clg_engine* e, uint32_t strategy, clg_enrich_req* reqs, uint32_t n, const uint32_t* log,
                     const uint8_t* flags, void* out, uint64_t cap, uint32_t out_kind, uint64_t* total) {
  ENGINE_GUARD(e);
  if ((n && (!reqs || !log)) || !total || strategy > CLG_DELTA_HIERARCHICAL)
    return fail(CLG_E_INVALID_ARG, "null argument or unknown strategy");
  CHK(e->flush());
  struct Adv {
    uint32_t log;
    ChKey k;
    int32_t nb;
  };
  struct Sent {
    uint32_t log;
    int32_t phys, nb;
    uint64_t dst;
  };
  std::vector<Adv> advs;
  std::vector<Sent> sent;
  std::vector<uint8_t> hdr;          // all headers back to back
  std::vector<uint64_t> hdr_at(n);   // request -> its header offset in hdr
  uint64_t dst = 0;
  for (uint32_t i = 0; i < n; ++i) {
    clg_enrich_req& r = reqs[i];
    r.status = CLG_OK;
    r.out_off = dst;
    const ChKey k{r.consumer.lo, r.consumer.hi};
    const size_t h0 = hdr.size();
    hdr_at[i] = h0;
    wr32(hdr, 0);  // header size, patched below (:98, :103)
    wr64(hdr, uint64_t(r.epoch));
    uint64_t dlen = 0;
    auto one = [&](uint32_t j, bool* has_out, int32_t* ofe, int32_t* nb) -> int {  // hasDelta, then take if sent
      int32_t has = 0;
      *has_out = false;
      CHK(e->has_delta(log[j], k, r.epoch, &has));
      if (!has || !(flags ? (flags[j] & CLG_DE_SEND) : 1)) return CLG_OK;
      CHK(e->offset_from_epoch(log[j], k, ofe));
      int32_t phys;
      CHK(e->take_delta(log[j], k, r.epoch, &phys, nb));
      advs.push_back(Adv{log[j], k, *nb});
      sent.push_back(Sent{log[j], phys, *nb, dlen});  // dst relative to the request's deltas, fixed below
      dlen += uint64_t(*nb);
      *has_out = true;
      return CLG_OK;
    };
    const size_t sent0 = sent.size();
    int st = CLG_OK;
    if (strategy == CLG_DELTA_FLAT) {  // [CausalLogID][offsetFromEpoch i32][len i32] per sent log (:80-84, :91-99)
      for (uint32_t j = r.first; j < r.first + r.count && st == CLG_OK; ++j) {
        bool has;
        int32_t ofe = 0, nb = 0;
        st = one(j, &has, &ofe, &nb);
        if (st != CLG_OK || !has) continue;
        const clg_causal_log_id& id = e->logs[log[j]].id;
        wr16(hdr, uint16_t(id.vertex_id));
        hdr.push_back(id.is_main ? 1 : 0);
        if (!id.is_main) {
          wr64(hdr, uint64_t(id.irp_lower));
          wr64(hdr, uint64_t(id.irp_upper));
          hdr.push_back(uint8_t(id.subpartition));
        }
        wr32(hdr, uint32_t(ofe));
        wr32(hdr, uint32_t(nb));
      }
    } else {  // Grouping: per vertex [vertex i16][hasMain]{main}[numPartitions u8]{[lo][hi][numSub u8]{[sub][ofe][len]}}
      uint32_t j = r.first;
      const uint32_t end = r.first + r.count;
      while (j < end && st == CLG_OK) {
        const int16_t v = e->logs[log[j]].id.vertex_id;
        const size_t vstart = hdr.size();
        int updates = 0;
        wr16(hdr, uint16_t(v));  // :113-115
        bool has = false;
        int32_t ofe = 0, nb = 0;
        if (e->logs[log[j]].id.is_main) {  // :116-121
          st = one(j, &has, &ofe, &nb);
          ++j;
        }
        if (st != CLG_OK) break;
        hdr.push_back(has ? 1 : 0);
        if (has) {
          wr32(hdr, uint32_t(ofe));
          wr32(hdr, uint32_t(nb));
          ++updates;
        }
        const size_t np_at = hdr.size();
        hdr.push_back(0);  // numPartitionDeltas (:134-141)
        int parts = 0;
        while (j < end && st == CLG_OK && e->logs[log[j]].id.vertex_id == v && !e->logs[log[j]].id.is_main) {
          const int64_t lo = e->logs[log[j]].id.irp_lower, hi = e->logs[log[j]].id.irp_upper;
          const size_t pstart = hdr.size();
          wr64(hdr, uint64_t(lo));  // :146-148
          wr64(hdr, uint64_t(hi));
          const size_t ns_at = hdr.size();
          hdr.push_back(0);
          int subs = 0;
          while (j < end && e->logs[log[j]].id.vertex_id == v && !e->logs[log[j]].id.is_main &&
                 e->logs[log[j]].id.irp_lower == lo && e->logs[log[j]].id.irp_upper == hi) {
            bool hs;
            int32_t o2 = 0, n2 = 0;
            st = one(j, &hs, &o2, &n2);
            if (st != CLG_OK) break;
            if (hs) {  // :150-154
              hdr.push_back(uint8_t(e->logs[log[j]].id.subpartition));
              wr32(hdr, uint32_t(o2));
              wr32(hdr, uint32_t(n2));
              ++subs;
            }
            ++j;
          }
          if (subs == 0) {
            hdr.resize(pstart);  // :156-158
          } else {
            hdr[ns_at] = uint8_t(subs);
            ++parts;
          }
        }
        hdr[np_at] = uint8_t(parts);
        updates += parts;
        if (updates == 0) hdr.resize(vstart);  // :125-126
        if (j < end && st == CLG_OK && e->logs[log[j]].id.vertex_id != v) continue;
        if (j < end && st == CLG_OK && e->logs[log[j]].id.vertex_id == v && e->logs[log[j]].id.is_main) {
          st = fail(CLG_E_INVALID_ARG, "hierarchical entries: vertex %d repeats", int(v));
        }
      }
    }
    if (st != CLG_OK) {  // undo this request's takes; the request reports the error
      for (size_t q = sent0; q < sent.size(); ++q) e->logs[sent[q].log].consumers[k].offset -= sent[q].nb;
      advs.resize(advs.size() - (sent.size() - sent0));
      sent.resize(sent0);
      hdr.resize(h0);
      r.status = st;
      r.header_bytes = 0;
      r.out_len = 0;
      continue;
    }
    const uint32_t hb = uint32_t(hdr.size() - h0);
    hdr[h0] = uint8_t(hb >> 24), hdr[h0 + 1] = uint8_t(hb >> 16), hdr[h0 + 2] = uint8_t(hb >> 8), hdr[h0 + 3] = uint8_t(hb);
    for (size_t q = sent0; q < sent.size(); ++q) sent[q].dst += dst + hb;
    r.header_bytes = hb;
    r.out_len = hb + dlen;
    dst += r.out_len;
  }
  *total = dst;
  if (dst > cap || (dst && !out)) {  // nothing moves: undo every take
    for (auto& a : advs) e->logs[a.log].consumers[a.k].offset -= a.nb;
    return fail(CLG_E_CAPACITY, "enrich needs %llu bytes", (unsigned long long)dst);
  }
  if (dst == 0) return CLG_OK;
  // headers staged in HBM (guard bytes either side for the gather's aligned reads)
  constexpr size_t kG = 32;
  CHK(e->d_hdr.ensure(hdr.size() + 2 * kG));
  CHK(e->h_stage.ensure(hdr.size() + 16));
  memcpy(e->h_stage.p, hdr.data(), hdr.size());
  uint8_t* dh = e->d_hdr.as<uint8_t>() + kG;
  HIPCHK(hipMemcpyAsync(dh, e->h_stage.p, hdr.size(), hipMemcpyHostToDevice, e->stream));
  std::vector<clg::GatherPiece> pieces;
  for (uint32_t i = 0; i < n; ++i)
    if (reqs[i].status == CLG_OK && reqs[i].header_bytes)
      pieces.push_back(clg::GatherPiece{dh + hdr_at[i], reqs[i].out_off, reqs[i].header_bytes, 0});
  for (auto& q : sent)
    if (q.nb > 0) e->add_pieces(e->logs[q.log], q.phys, q.nb, q.dst, pieces);
  return e->run_gather(pieces, dst, out, out_kind);
}

// processCausalLogDelta (:117-163): header parsed on the host, deltas applied by the
// batched upstream scatter straight from the message buffer.
int clg_process_delta(clg_engine* e, uint32_t job, uint32_t strategy, const uint8_t* msg, uint64_t n,
                      uint32_t in_kind, int64_t* epoch, uint32_t* handles, uint32_t cap, uint32_t* n_logs,
                      uint64_t* consumed) {
  ENGINE_GUARD(e);
  if (job >= e->jobs.size() || !e->jobs[job].open) return fail(CLG_E_NO_LOG, "unknown job %u", job);
  if (!msg || !epoch || !n_logs || strategy > CLG_DELTA_HIERARCHICAL) return fail(CLG_E_INVALID_ARG, "null argument");
  *n_logs = 0;
  if (n < 12) return fail(CLG_E_TRUNCATED, "delta header truncated");
  std::vector<uint8_t> hb(12);
  if (in_kind == CLG_MEM_DEVICE) HIPCHK(hipMemcpy(hb.data(), msg, 12, hipMemcpyDeviceToHost));
  else memcpy(hb.data(), msg, 12);
  const int32_t hsize = int32_t(rd32(hb.data()));
  if (hsize < 12 || uint64_t(hsize) > n) return fail(CLG_E_TRUNCATED, "delta header size %d", hsize);
  hb.resize(size_t(hsize));
  if (in_kind == CLG_MEM_DEVICE) HIPCHK(hipMemcpy(hb.data(), msg, size_t(hsize), hipMemcpyDeviceToHost));
  else memcpy(hb.data(), msg, size_t(hsize));
  *epoch = int64_t(rd64(hb.data() + 4));
  size_t p = 12;
  uint64_t delta_at = uint64_t(hsize);
  std::vector<clg_delta_req> reqs;
  auto need = [&](size_t k) { return p + k <= size_t(hsize); };
  auto apply = [&](const clg_causal_log_id& id) -> int {  // processThreadDelta :129-163
    if (!need(8)) return fail(CLG_E_TRUNCATED, "delta record truncated");
    const int32_t ofe = int32_t(rd32(&hb[p])), len = int32_t(rd32(&hb[p + 4]));
    p += 8;
    if (len < 0 || delta_at + uint64_t(len) > n) return fail(CLG_E_TRUNCATED, "delta past the message");
    uint32_t h;
    const IdKey key = key_of(job, id);
    auto it = e->by_id.find(key);
    if (it == e->by_id.end()) {
      CHK(clg_log_open(e, job, &id, &h));  // insertNewUpstreamLog
    } else {
      h = it->second;
    }
    reqs.push_back(clg_delta_req{h, ofe, *epoch, delta_at, uint32_t(len), 0});
    delta_at += uint64_t(len);
    if (*n_logs < cap && handles) handles[*n_logs] = h;
    ++*n_logs;
    return CLG_OK;
  };
  while (p < size_t(hsize)) {
    clg_causal_log_id id{};
    if (!need(3)) return fail(CLG_E_TRUNCATED, "CausalLogID truncated");
    id.vertex_id = int16_t(uint16_t(hb[p]) << 8 | hb[p + 1]);
    const bool main = hb[p + 2] != 0;
    p += 3;
    if (strategy == CLG_DELTA_FLAT) {  // deserializeCausalLogID (Flat :107-119)
      id.is_main = main ? 1 : 0;
      if (!main) {
        if (!need(17)) return fail(CLG_E_TRUNCATED, "CausalLogID truncated");
        id.irp_lower = int64_t(rd64(&hb[p]));
        id.irp_upper = int64_t(rd64(&hb[p + 8]));
        id.subpartition = int8_t(hb[p + 16]);
        p += 17;
      }
      CHK(apply(id));
    } else {  // Grouping deserializeStrategyStep :66-88
      if (main) {
        id.is_main = 1;
        CHK(apply(id));
      }
      if (!need(1)) return fail(CLG_E_TRUNCATED, "partition count truncated");
      const int np = int(int8_t(hb[p++]));
      for (int q = 0; q < np; ++q) {
        if (!need(17)) return fail(CLG_E_TRUNCATED, "partition truncated");
        clg_causal_log_id sid{};
        sid.vertex_id = id.vertex_id;
        sid.irp_lower = int64_t(rd64(&hb[p]));
        sid.irp_upper = int64_t(rd64(&hb[p + 8]));
        const int ns = int(int8_t(hb[p + 16]));
        p += 17;
        for (int t = 0; t < ns; ++t) {
          if (!need(1)) return fail(CLG_E_TRUNCATED, "subpartition truncated");
          sid.subpartition = int8_t(hb[p++]);
          CHK(apply(sid));
        }
      }
    }
  }
  if (consumed) *consumed = delta_at;
  if (reqs.empty()) return CLG_OK;
  CHK(e->upstream_batch(reqs.data(), uint32_t(reqs.size()), msg, in_kind));
  for (auto& r : reqs)
    if (r.status != CLG_OK) return fail(r.status, "processUpstreamDelta failed on log %u", r.log);
  return CLG_OK;
}

}  // extern "C"
