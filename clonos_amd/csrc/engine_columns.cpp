// engine_columns.cpp -- the typed-columns family, decode -> columns: the placement of the family's
// arrays (placement.h; its helpers are defined here and declared in engine_columns.h for the pack and
// encode units), the columns of a decoded batch and the decodes into columns, the payload column;
// clg_columnize*, clg_decode_{logs,host}_columns, ..._columns_var and clg_gather_payloads*.
// decode_columns and decode_columns_var also serve replay preparation (engine_replay.cpp), and
// engine_pack.cpp's packed decodes run the decode, the columns and the payload gather from here.
#include "engine_columns.h"
#include "columns.h"

// ---- placement (placement.h): where the kernels of this family read and write ------------------
static_assert(clg::kPlaceHost == CLG_MEM_HOST && clg::kPlaceDevice == CLG_MEM_DEVICE && clg::kPlaceMapped == CLG_MEM_MAPPED,
              "placement.h numbers the memory kinds as the ABI does");

// The placement of n arrays of one memory kind; a misaligned or (reject_unresolved) unregistered
// array fails the call, naming `what` the arrays are.
int place_arrays(const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, const char* what, clg::Placement* pl) {
  *pl = clg::place(s, n, kind, policy, clg_mapped_device_address);
  if (pl->verdict != clg::PlaceVerdict::misaligned && pl->verdict != clg::PlaceVerdict::not_registered) return CLG_OK;
  return fail(CLG_E_INVALID_ARG, "%s array %d is not %s", what, pl->bad,
              pl->verdict == clg::PlaceVerdict::misaligned ? "aligned to its element"
                                                           : "inside memory registered with clg_host_register");
}
// A copy to or from a caller's array (the source of a host-to-device copy, else the destination),
// in pieces that cross no edge of a registered range: an array need not lie wholly inside one.
int copy_caller(clg_engine* e, void* dst, const void* src, uint64_t bytes, hipMemcpyKind kind, uint32_t mem_kind) {
  const char* caller = static_cast<const char*>(kind == hipMemcpyHostToDevice ? src : dst);
  for (uint64_t at = 0, k; at < bytes; at += k) {
    k = mem_kind == CLG_MEM_DEVICE ? bytes : clg_mapped_piece(caller + at, bytes - at);  // (device memory: one copy)
    HIPCHK(hipMemcpyAsync(static_cast<char*>(dst) + at, static_cast<const char*>(src) + at, k, kind, e->stream));
  }
  return CLG_OK;
}
// The placement of outputs; staged: `buf` grown to the slots, `extra` bytes behind them and 16
// spare, and the arrays bound to their slots.
int place_out(DevBuf& buf, const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, const char* what, clg::Placement* pl,
              size_t extra) {
  CHK(place_arrays(s, n, kind, policy, what, pl));
  if (!pl->staged()) return CLG_OK;
  CHK(buf.ensure(pl->total + extra + 16));
  pl->bind(s, n, buf.p);
  return CLG_OK;
}
// The placement of inputs: the same, and a staged array's copy in queued (not an absent or empty one's).
int place_in(clg_engine* e, DevBuf& buf, const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, const char* what,
             clg::Placement* pl, size_t extra) {
  CHK(place_out(buf, s, n, kind, policy, what, pl, extra));
  for (int i = 0; i < n && pl->staged(); ++i)
    if (s[i].p && s[i].bytes) CHK(copy_caller(e, pl->at<void>(i), s[i].p, s[i].bytes, hipMemcpyHostToDevice));
  return CLG_OK;
}
// A staged output's copies out, queued behind the kernels that filled the slots (no-op in place).
int stage_out(clg_engine* e, const PlaceSpec* s, int n, const clg::Placement& pl) {
  for (int i = 0; i < n && pl.staged(); ++i)
    if (s[i].p && s[i].bytes) CHK(copy_caller(e, const_cast<void*>(s[i].p), pl.at<void>(i), s[i].bytes, hipMemcpyDeviceToHost));
  return CLG_OK;
}

// ---- typed replay columns (columns.h) -------------------------------------------------------
// The stable partition of a decoded batch by determinant class, from the decode's output where
// it lies: count and scan, the host's capacity check on the scan's totals, then the write, the
// span bases and the wide rows' v0.  LogReplayerImpl (LogReplayerImpl.java:61-119) asks for one
// typed value at a time and never for a record's offset: the columns are what it consumes.
namespace {

// The input's array that column array i passes through unchanged (null: the kernels compute it).
const void* col_through(const clg_decoded& in, int i) {
  const void* const src[clg::kColArrays] = {in.tag,  nullptr,      nullptr,      nullptr,  nullptr, in.w_idx, in.w_rc,
                                            in.w_v1, in.w_var_off, in.w_var_len, in.w_sub, nullptr};
  return src[i];
}
// The two failures columnize_small and columnize_device share.
int col_bad_tag(clg_columns* out, const uint64_t* span_rec_base, uint32_t n_spans, uint64_t index, uint64_t tag) {
  out->err_status = CLG_E_INVALID_ARG;
  out->err_span = clg::col_span_of(span_rec_base, n_spans, index);
  out->err_off = int64_t(index);
  out->err_tag = int32_t(tag);
  return fail(CLG_E_INVALID_ARG, "record %llu has tag %llu", (unsigned long long)index, (unsigned long long)tag);
}
int col_too_small(const char* name, uint64_t n, const uint64_t tot[clg::kColClasses]) {
  return fail(CLG_E_CAPACITY, "column %s is too small (records %llu; totals %llu %llu %llu %llu %llu)", name,
              (unsigned long long)n, (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)tot[2],
              (unsigned long long)tot[3], (unsigned long long)tot[4]);
}
int col_wide_count(uint64_t n_wide, uint64_t held) {
  return fail(CLG_E_INVALID_ARG, "n_wide is %llu, the tags hold %llu wide records", (unsigned long long)n_wide,
              (unsigned long long)held);
}

// A batch of at most kColSmallRecords records and kColSmallSpans spans, in one launch
// (k_col_small): the kernel does the check below itself and reports it in pinned memory, so the
// call has one host sync (two for CLG_MEM_HOST outputs, whose packed size is known only then).
// columnize_device has checked the arguments.
int columnize_small(clg_engine* e, const clg_decoded& in, const uint64_t* span_rec_base, uint32_t n_spans,
                    clg_columns* out) {
  const uint64_t n = in.n_rec, nw = in.n_wide;
  const bool sizes_only = clg::col_sizes_only(*out);
  const bool want_sb = out->span_base && n_spans;
  // pinned: result block | span bases | span boundaries
  const size_t o_sb = clg_engine::al16(sizeof(clg::ColSmallRes)), sbn = size_t(n_spans) + 1;
  const size_t o_srb = o_sb + sbn * clg::kColClasses * 8;
  CHK(e->h_colsmall.ensure(o_srb + sbn * 8));
  uint8_t* hp = e->h_colsmall.as<uint8_t>();
  clg::ColSmallRes* res = reinterpret_cast<clg::ColSmallRes*>(hp);
  uint64_t* h_sb = reinterpret_cast<uint64_t*>(hp + o_sb);
  uint64_t* h_srb = reinterpret_cast<uint64_t*>(hp + o_srb);
  if (want_sb) memcpy(h_srb, span_rec_base, sbn * 8);

  // where the kernel writes: the caller's device arrays, the device side of registered host
  // arrays, or (plain host memory, and registered memory that is not wholly inside one registered
  // range) one packed engine buffer that is read back in one copy.  The registry is asked for
  // each array's capacity, not its length: the lengths are known only after the one launch.
  PlaceSpec spec[clg::kColArrays];
  for (int i = 0; i < clg::kColArrays; ++i)
    spec[i] = {clg::col_ptr(*out, i), clg::col_array_cap(*out, i) * clg::kColArray[i].width, clg::kColArray[i].width};
  clg::Placement pl;
  CHK(place_arrays(spec, clg::kColArrays, out->out_kind, PlacePolicy::stage_if_unresolved, "column", &pl));
  const bool packed = pl.staged();
  void* dev[clg::kColArrays];
  for (int i = 0; i < clg::kColArrays; ++i) dev[i] = pl.at<void>(i);
  clg::ColSmallOut so{};
  if (packed && !sizes_only) {
    CHK(e->d_colout.ensure(clg::col_pack_bound(n, nw) + 16));
    so.pack = e->d_colout.as<uint8_t>();
  } else if (!sizes_only) {
    for (int i = 0; i < clg::kColArrays; ++i)  // (an array that is the input's own stays as it is)
      if (dev[i] == col_through(in, i)) dev[i] = nullptr;
    so.tag = static_cast<uint8_t*>(dev[0]), so.order = static_cast<int8_t*>(dev[1]);
    so.timestamp = static_cast<int64_t*>(dev[2]), so.rng = static_cast<int32_t*>(dev[3]);
    so.buffer_built = static_cast<int32_t*>(dev[4]), so.w_idx = static_cast<uint32_t*>(dev[5]);
    so.w_rc = static_cast<int32_t*>(dev[6]), so.w_v1 = static_cast<int64_t*>(dev[7]);
    so.w_var_off = static_cast<uint32_t*>(dev[8]), so.w_var_len = static_cast<uint32_t*>(dev[9]);
    so.w_sub = static_cast<uint8_t*>(dev[10]), so.w_v0 = static_cast<int64_t*>(dev[11]);
  }
  for (int i = 0; i < clg::kColNarrowArrays; ++i) so.cap[i] = clg::col_array_cap(*out, i);
  so.cap[5] = out->cap_wide;  // (the wide arrays share one capacity: none when one of them is absent)
  for (int i = clg::kColNarrowArrays; i < clg::kColArrays; ++i) so.cap[5] = std::min(so.cap[5], clg::col_array_cap(*out, i));
  const clg::ColSmallIn si{in.tag,       in.v0,       in.w_idx, in.w_rc, in.w_v1, in.w_var_off,
                           in.w_var_len, in.w_sub,    want_sb ? h_srb : nullptr,  n,       nw,
                           want_sb ? n_spans : 0u, sizes_only ? 1u : 0u};
  e->stats["columns_small"].launches++;
  // (bytes: the tags twice and v0 once, the columns, the side rows in and out; as the multi-kernel form counts them)
  const uint64_t moved = (want_sb ? sbn * 48 : 0) + (sizes_only ? n : 2 * n + 8 * n + 8 * (n - std::min(n, nw)) + 58 * nw);
  CHK(e->timed("decode_columns", moved, [&] { return clg::launch_col_small(si, so, res, want_sb ? h_sb : nullptr, e->stream); }));
  CHK(e->sync());
  out->n_rec = n;
  if (res->verdict == clg::kColSmallBadTag) return col_bad_tag(out, span_rec_base, n_spans, res->bad_index, res->bad_tag);
  uint64_t tot[clg::kColClasses];
  for (uint32_t c = 0; c < clg::kColClasses; ++c) out->n_class[c] = tot[c] = res->total[c];
  if (res->verdict == clg::kColSmallWideCount)
    return col_wide_count(nw, tot[clg::kColWide]);
  if (res->verdict == clg::kColSmallWritten && packed && res->pack_off[12]) {
    const uint64_t end = res->pack_off[12];
    if (end > clg::col_pack_bound(n, nw)) return fail(CLG_E_DEVICE, "the packed columns end at %llu", (unsigned long long)end);
    CHK(e->h_colpack.ensure(end));
    HIPCHK(hipMemcpyAsync(e->h_colpack.p, so.pack, end, hipMemcpyDeviceToHost, e->stream));
    CHK(e->sync());
    for (int i = 0; i < clg::kColArrays; ++i)
      if (const uint64_t cnt = clg::col_array_len(i, n, tot))
        memcpy(clg::col_ptr(*out, i), e->h_colpack.as<uint8_t>() + res->pack_off[i], cnt * clg::kColArray[i].width);
  }
  if (out->span_base) {
    if (n_spans) memcpy(out->span_base, h_sb, sbn * 8 * clg::kColClasses);
    else memcpy(out->span_base, tot, sizeof tot);
  }
  // (short_cap: the narrow array's index, 5 for the wide arrays)
  if (res->verdict == clg::kColSmallCapacity) return col_too_small(clg::kColArray[std::min(res->short_cap, 5u)].name, n, tot);
  return CLG_OK;
}

// ---- the payload column (payload.h) ---------------------------------------------------------
// The wide rows' payload bytes packed in row order: size and scan, the host's check of the
// scan's totals, then pos and the copy.  Host work is O(spans + segments covered): a PaySpan per
// span and the segment table; the rows stay on the device.
//
// At most kPaySmallRows rows over spans of at most kPaySmallBytes bytes, in one launch
// (k_pay_small): the kernel does the check itself and reports it in pinned memory.  One host sync
// (two for outputs that are not device memory: pos | var come back packed in one copy).
// gather_payloads_device has checked the arguments and uploaded the descriptors behind `in`.
int gather_payloads_small(clg_engine* e, const clg::PayIn& in, clg_payloads* out, bool sizes_only, uint64_t span_bytes,
                          uint64_t desc_bytes) {
  const uint64_t n = in.n_rows;
  CHK(e->h_payres.ensure(sizeof(clg::PaySmallRes)));
  clg::PaySmallRes* res = e->h_payres.as<clg::PaySmallRes>();
  const uint64_t cap_pos = out->pos ? out->cap_pos : 0, cap_var = out->var ? out->cap_var : 0;
  // where the kernel writes: the caller's device arrays, or (host and registered memory alike:
  // the short rows' byte stores stay off the link) engine staging, pos | var; sizes only: nowhere.
  // Staging holds what the spans hold.  Rows of a caller may overlap, so n_var can be more: then
  // the kernel reports the staging as short, and runs once more with staging of n_var bytes.
  PlaceSpec dst[2] = {{out->pos, (n + 1) * 8, 8}, {out->var, std::min(cap_var, span_bytes), 1}};
  clg::Placement pl;
  e->stats["payloads_small"].launches++;
  for (int round = 0;; ++round) {
    if (!sizes_only) CHK(place_out(e->d_payout, dst, 2, out->out_kind, PlacePolicy::stage_unless_device, "payload", &pl));
    CHK(e->timed("decode_payloads", n * 20 + (n + 1) * 8 + desc_bytes, [&] {
      return clg::launch_pay_small(in, pl.at<uint64_t>(0), pl.at<uint8_t>(1), cap_pos, pl.staged() ? dst[1].bytes : cap_var,
                                   sizes_only, res, e->stream);
    }));
    CHK(e->sync());
    if (round || !pl.staged() || res->verdict != clg::kPaySmallCapacity || !res->short_cap || res->n_var > cap_var) break;
    dst[1].bytes = res->n_var;
  }
  out->n_var = res->n_var;
  if (res->verdict == clg::kPaySmallBadRow) {
    out->bad_row = res->bad_row;
    return fail(CLG_E_INVALID_ARG, "row %llu passes its span's end", (unsigned long long)res->bad_row);
  }
  if (res->verdict == clg::kPaySmallCapacity)
    return pay_too_small(res->short_cap ? "var" : "pos", n, res->n_var);
  if (res->verdict == clg::kPaySmallWritten && pl.staged()) {  // pos | var come back in one copy
    const uint64_t nv = res->n_var, pb = pl.off[1];
    CHK(e->h_paypack.ensure(pb + nv));
    HIPCHK(hipMemcpyAsync(e->h_paypack.p, pl.at<void>(0), pb + nv, hipMemcpyDeviceToHost, e->stream));
    CHK(e->sync());
    memcpy(out->pos, e->h_paypack.p, (n + 1) * 8);
    if (nv) memcpy(out->var, e->h_paypack.as<uint8_t>() + pb, nv);
  }
  return CLG_OK;
}

// The rows of a caller: device arrays as they are, host arrays staged.
int stage_payload_rows(clg_engine* e, const uint32_t* off, const uint32_t* len, uint64_t n, uint32_t in_kind,
                       const uint32_t** d_off, const uint32_t** d_len) {
  *d_off = off;
  *d_len = len;
  if (in_kind != CLG_MEM_HOST || !n) return CLG_OK;
  if (!off || !len) return fail(CLG_E_INVALID_ARG, "null row array");
  const PlaceSpec rows[2] = {{off, n * 4, 4}, {len, n * 4, 4}};
  clg::Placement pl;
  CHK(place_in(e, e->d_payrows, rows, 2, in_kind, PlacePolicy::stage_unless_device, "row", &pl));
  *d_off = pl.at<const uint32_t>(0);
  *d_len = pl.at<const uint32_t>(1);
  return CLG_OK;
}

// Spans of one buffer (host input staged as clg_decode_host stages it) as contiguous PaySpans.
int payload_spans_bytes(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                        uint32_t n, uint32_t in_kind, std::vector<clg::PaySpan>& spans) {
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; ++i) total += span_len[i];
  if (total && !bytes) return fail(CLG_E_INVALID_ARG, "null argument");
  const uint8_t* base = bytes;
  uint64_t base_off = 0;
  if (total) CHK(e->stage_spans(bytes, span_off, span_len, n, in_kind, &base, &base_off));
  spans.resize(n);
  for (uint32_t i = 0; i < n; ++i)
    spans[i] = clg::PaySpan{span_len[i] ? base + (span_off[i] - base_off) : nullptr, 0, span_len[i], 0, 0};
  return CLG_OK;
}

// getDeterminants(start_epoch[i]) of log[i], in place: plan_log_span's run and table entries.
int payload_spans_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                       std::vector<clg::PaySpan>& spans, std::vector<uint32_t>& segtab) {
  CHK(e->flush());
  spans.resize(n);
  const uint32_t C = e->C();
  for (uint32_t i = 0; i < n; ++i) {
    Log* l;
    CHK(e->get_log(log[i], &l));
    int32_t s = 0, nb = 0;
    if (l->depth != 0) CHK(e->determinants_range(*l, start_epoch[i], &s, &nb));
    spans[i] = clg::PaySpan{nullptr, segtab.size(), uint64_t(nb), 0, 0};
    if (nb > 0) {  // only the segments the span covers go into the table (phys rebased on them)
      const uint32_t s0 = uint32_t(s) / C, s1 = uint32_t(s + nb - 1) / C + 1;
      spans[i].phys = uint32_t(s) - s0 * C;
      segtab.insert(segtab.end(), l->segs.begin() + s0, l->segs.begin() + s1);
    }
  }
  return CLG_OK;
}

DecodeRun run_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n) {
  return [=](clg_decoded* d, uint64_t* base) { return clg_decode_logs(e, log, start_epoch, n, d, base); };
}
DecodeRun run_host(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len, uint32_t n) {
  return [=](clg_decoded* d, uint64_t* base) { return clg_decode_host(e, bytes, span_off, span_len, n, d, base); };
}

}  // namespace

int pay_too_small(const char* name, uint64_t rows, uint64_t bytes) {
  return fail(CLG_E_CAPACITY, "%s is too small (rows %llu, payload bytes %llu)", name, (unsigned long long)rows,
              (unsigned long long)bytes);
}

// `in`: device addresses (the caller's device arrays, engine scratch, or the device side of
// registered host memory).
int columnize_device(clg_engine* e, const clg_decoded& in, const uint64_t* span_rec_base, uint32_t n_spans,
                     clg_columns* out) {
  clg::col_reset_result(out);
  const uint64_t n = in.n_rec, nw = in.n_wide;
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  if ((n && (!in.tag || !in.v0)) || (nw && (!in.w_idx || !in.w_rc || !in.w_v1 || !in.w_var_off || !in.w_var_len || !in.w_sub)))
    return fail(CLG_E_INVALID_ARG, "null input array");
  if (!clg::col_spans_ok(span_rec_base, n_spans, n))
    return fail(CLG_E_INVALID_ARG, "span_rec_base decreases or passes n_rec");
  if ((n + clg::kColTile - 1) / clg::kColTile >> 31) return fail(CLG_E_INVALID_ARG, "%llu records in one call", (unsigned long long)n);
  for (int i = 0; i < clg::kColArrays && out->out_kind != CLG_MEM_HOST; ++i)  // (an empty array's too: no length is known yet)
    if (uintptr_t(clg::col_ptr(*out, i)) % clg::kColArray[i].width)
      return fail(CLG_E_INVALID_ARG, "column %d is not aligned to its element", i);
  if (e->sw.columns_small && n <= clg::kColSmallRecords && n_spans <= clg::kColSmallSpans)
    return columnize_small(e, in, span_rec_base, n_spans, out);
  const uint32_t n_tiles = uint32_t((n + clg::kColTile - 1) / clg::kColTile);
  const clg::ColIn cin{in.tag, in.v0, in.w_idx, n, nw};

  // count and scan; the totals come back before anything is written to the caller
  CHK(e->d_colcnt.ensure(size_t(n_tiles) * clg::kColCountWords * 4 + 64));
  CHK(e->d_colbase.ensure(size_t(n_tiles) * clg::kColClasses * 8 + 64));
  CHK(e->h_colres.ensure(sizeof(clg::ColRes)));
  clg::ColRes* res = e->h_colres.as<clg::ColRes>();
  CHK(e->timed("decode_columns", n, [&] {
    return clg::launch_col_count_scan(cin, n_tiles, e->d_colcnt.as<uint32_t>(), e->d_colbase.as<uint64_t>(), res, e->stream);
  }));
  CHK(e->sync());
  out->n_rec = n;
  if (res->bad_tile != clg::kColNoTile) {  // a tag above 7: one wave finds the record
    CHK(clg::launch_col_find_bad(cin, res->bad_tile, res, e->stream));
    CHK(e->sync());
    return col_bad_tag(out, span_rec_base, n_spans, res->bad_index, res->bad_tag);
  }
  uint64_t tot[clg::kColClasses];
  for (uint32_t c = 0; c < clg::kColClasses; ++c) out->n_class[c] = tot[c] = res->total[c];
  if (tot[clg::kColWide] != nw)
    return col_wide_count(nw, tot[clg::kColWide]);
  const bool sizes_only = clg::col_sizes_only(*out);
  const char* short_col = sizes_only ? nullptr : clg::col_short_column(*out, n, tot);
  const bool write = !sizes_only && !short_col;

  // where the kernels write: the caller's device arrays, the device side of registered host
  // arrays, or engine staging (plain host memory, and registered memory that is not wholly
  // inside one registered range).  Only the arrays the kernels write, each with its length (known
  // here, unlike in columnize_small); those passed through are copied below and absent here.
  PlaceSpec wr[clg::kColArrays];
  for (int i = 0; i < clg::kColArrays; ++i)
    wr[i] = {col_through(in, i) ? nullptr : clg::col_ptr(*out, i), clg::col_array_len(i, n, tot) * clg::kColArray[i].width,
             clg::kColArray[i].width};
  clg::Placement pl;
  if (write) CHK(place_out(e->d_colout, wr, clg::kColArrays, out->out_kind, PlacePolicy::stage_if_unresolved, "column", &pl));
  const clg::ColOut cout_{pl.at<int8_t>(1), pl.at<int64_t>(2), pl.at<int32_t>(3), pl.at<int32_t>(4), pl.at<int64_t>(11)};
  const bool want_sb = out->span_base && n_spans;
  if (want_sb) {
    const size_t sb = size_t(n_spans + 1) * 8;
    CHK(e->h_colsb.ensure(sb * clg::kColClasses));
    CHK(e->d_colsrb.ensure(sb));
    CHK(e->d_colsb.ensure(sb * clg::kColClasses));
    memcpy(e->h_colsb.p, span_rec_base, sb);
    HIPCHK(hipMemcpyAsync(e->d_colsrb.p, e->h_colsb.p, sb, hipMemcpyHostToDevice, e->stream));
  }
  uint64_t moved = n_tiles * uint64_t(clg::kColClasses) * 8 + (want_sb ? uint64_t(n_spans + 1) * 48 : 0);
  if (write) moved += n + 8 * (n - nw) + tot[0] + 8 * tot[1] + 4 * tot[2] + 4 * tot[3] + 20 * nw;
  CHK(e->timed("decode_columns", moved, [&] {
    return clg::launch_col_write(cin, n_tiles, e->d_colbase.as<uint64_t>(), res, write, cout_,
                                 want_sb ? e->d_colsrb.as<uint64_t>() : nullptr, n_spans, e->d_colsb.as<uint64_t>(), e->stream);
  }));
  if (want_sb)  // (h_colsb's copy of span_rec_base was uploaded by the copy queued before the kernels)
    HIPCHK(hipMemcpyAsync(e->h_colsb.p, e->d_colsb.p, size_t(n_spans + 1) * 8 * clg::kColClasses, hipMemcpyDeviceToHost, e->stream));
  if (write) {
    // the arrays that stay as they are: the tags and the side rows
    for (int i = 0; i < clg::kColArrays; ++i) {
      const void* src = col_through(in, i);
      void* dst = clg::col_ptr(*out, i);
      if (src && wr[i].bytes && dst != src) CHK(copy_caller(e, dst, src, wr[i].bytes, hipMemcpyDefault, out->out_kind));
    }
    CHK(stage_out(e, wr, clg::kColArrays, pl));
  }
  CHK(e->sync());
  if (out->span_base) {
    if (n_spans) memcpy(out->span_base, e->h_colsb.p, size_t(n_spans + 1) * 8 * clg::kColClasses);
    else memcpy(out->span_base, tot, sizeof tot);
  }
  if (short_col) return col_too_small(short_col, n, tot);
  return CLG_OK;
}

// The decode into engine scratch (the host-output staging arrays, kept between calls), grown
// and run again on the decode's own CLG_E_CAPACITY, then the columns of what it produced.
// keep (optional): the decoded batch in engine scratch and columnize_device's own status, for
// the payload column of the same rows (decode_columns_var).
int decode_columns(clg_engine* e, const DecodeRun& run, uint32_t n_spans, clg_columns* out, ColKeep* keep) {
  clg::col_reset_result(out);
  std::vector<uint64_t> base(size_t(n_spans) + 1, 0);
  clg_decoded d{};
  uint64_t need = 1u << 16, wneed = 1u << 12;
  int st = CLG_OK;
  for (int round = 0;; ++round) {
    clg::DecodeOut o;
    CHK(e->scratch_out(need, wneed, &o));
    d = clg_decoded{};
    d.off = o.off, d.tag = o.tag, d.v0 = o.v0, d.w_idx = o.w_idx, d.w_rc = o.w_rc, d.w_v1 = o.w_v1;
    d.w_var_off = o.w_var_off, d.w_var_len = o.w_var_len, d.w_sub = o.w_sub;
    d.cap = std::min({uint64_t(e->d_o_off.cap / 4), uint64_t(e->d_o_tag.cap), uint64_t(e->d_o_v0.cap / 8)});
    d.wcap = std::min({uint64_t(e->d_o_widx.cap / 4), uint64_t(e->d_o_wrc.cap / 4), uint64_t(e->d_o_wv1.cap / 8),
                       uint64_t(e->d_o_wvo.cap / 4), uint64_t(e->d_o_wvl.cap / 4), uint64_t(e->d_o_wsub.cap)});
    d.out_kind = CLG_MEM_DEVICE;
    st = run(&d, base.data());
    if (st != CLG_E_CAPACITY || round == 2) break;
    need = std::max<uint64_t>(d.n_rec, d.cap);  // (the decode reported what it produced)
    wneed = std::max<uint64_t>(d.n_wide, d.wcap);
  }
  if (st == CLG_E_CAPACITY) return st;
  if (st != CLG_OK && d.err_status == CLG_OK) return st;  // an engine failure, not a decode result
  const std::string decode_err = st != CLG_OK ? g_err : std::string();
  const int col_status = columnize_device(e, d, base.data(), n_spans, out);
  if (keep) keep->d = d, keep->valid = true, keep->col_status = col_status;
  CHK(col_status);
  out->err_status = d.err_status;
  out->err_span = d.err_span;
  out->err_off = d.err_off;
  out->err_tag = d.err_tag;
  if (st != CLG_OK) g_err = decode_err;
  return st;
}

// d_off / d_len: device addresses of the rows.  sizes_forced: fill the results, write nothing.
int gather_payloads_device(clg_engine* e, const std::vector<clg::PaySpan>& spans, const std::vector<uint32_t>& segtab,
                           const uint32_t* d_off, const uint32_t* d_len, const uint64_t* row_base, clg_payloads* out,
                           bool sizes_forced, bool no_pos) {
  // (no_pos, the packed-wide decodes only: var is delivered without pos, which the caller rebuilds
  // from the lengths; the kernels then write no pos and the one-launch form, which does, is not taken)
  const uint32_t ns = uint32_t(spans.size());
  clg::pay_reset_result(out);
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  if (!clg::pay_row_base_ok(row_base, ns)) return fail(CLG_E_INVALID_ARG, "row_base does not start at 0 or decreases");
  const uint64_t n = ns ? row_base[ns] : 0;
  if (n > 0xFFFFFFFFull) return fail(CLG_E_INVALID_ARG, "%llu rows in one call", (unsigned long long)n);
  out->n_rows = n;
  const bool sizes_only = sizes_forced || clg::pay_sizes_only(*out);
  const bool direct = out->out_kind == CLG_MEM_DEVICE;
  if (!sizes_only && direct && uintptr_t(out->pos) % 8) return fail(CLG_E_INVALID_ARG, "pos is not aligned to its element");
  if (!n) {  // no rows: only pos[0]
    if (sizes_only || no_pos) return CLG_OK;
    if (const char* name = clg::pay_short(*out, 0, 0)) return fail(CLG_E_CAPACITY, "%s is too small (rows 0)", name);
    const uint64_t zero = 0;
    if (direct) HIPCHK(hipMemcpy(out->pos, &zero, 8, hipMemcpyHostToDevice));
    else out->pos[0] = 0;
    return CLG_OK;
  }
  if (!d_off || !d_len) return fail(CLG_E_INVALID_ARG, "null row array");
  const uint32_t n_tiles = uint32_t((n + clg::kPayTile - 1) / clg::kPayTile);

  // span table | row_base | segment table, in one upload
  const size_t sb = size_t(ns) * sizeof(clg::PaySpan), rb = size_t(ns + 1) * 8, tb = segtab.size() * 4;
  CHK(e->h_paydesc.ensure(sb + rb + tb + 16));
  CHK(e->d_paydesc.ensure(sb + rb + tb + 16));
  uint8_t* h = e->h_paydesc.as<uint8_t>();
  memcpy(h, spans.data(), sb);
  memcpy(h + sb, row_base, rb);
  if (tb) memcpy(h + sb + rb, segtab.data(), tb);
  HIPCHK(hipMemcpyAsync(e->d_paydesc.p, h, sb + rb + tb, hipMemcpyHostToDevice, e->stream));
  const uint8_t* dd = e->d_paydesc.as<uint8_t>();
  const clg::PayIn in{d_off, d_len, reinterpret_cast<const uint64_t*>(dd + sb), reinterpret_cast<const clg::PaySpan*>(dd),
                      reinterpret_cast<const uint32_t*>(dd + sb + rb), e->pool, n, ns, e->C()};
  uint64_t span_bytes = 0;  // (an upper bound of n_var)
  for (const clg::PaySpan& sp : spans) span_bytes += sp.len;
  if (!no_pos && e->sw.columns_small && n <= clg::kPaySmallRows && span_bytes <= clg::kPaySmallBytes)
    return gather_payloads_small(e, in, out, sizes_only, span_bytes, sb + rb);
  CHK(e->d_paytile.ensure(size_t(n_tiles) * 24 + 64));
  uint64_t* d_sum = e->d_paytile.as<uint64_t>();
  uint64_t* d_bad = d_sum + n_tiles;
  uint64_t* d_base = d_bad + n_tiles;
  CHK(e->h_payres.ensure(sizeof(clg::PayRes)));
  clg::PayRes* res = e->h_payres.as<clg::PayRes>();

  // size and scan; the totals come back before anything is written to the caller
  CHK(e->timed("decode_payloads", n * 8 + uint64_t(n_tiles) * 40 + sb + rb, [&] {
    return clg::launch_pay_size_scan(in, n_tiles, d_sum, d_bad, d_base, res, e->stream);
  }));
  CHK(e->sync());
  out->n_var = res->n_var;
  if (res->bad_row != clg::kPayNoRow) {
    out->bad_row = res->bad_row;
    return fail(CLG_E_INVALID_ARG, "row %llu passes its span's end", (unsigned long long)res->bad_row);
  }
  if (sizes_only) return CLG_OK;
  const uint64_t nv = res->n_var;
  const char* short_name = !no_pos ? clg::pay_short(*out, n, nv) : (out->var ? out->cap_var : 0) < nv ? "var" : nullptr;
  if (short_name) return pay_too_small(short_name, n, nv);

  // where the kernels write: the caller's device arrays, or engine staging and one copy each
  // (host and registered memory alike: the short rows' byte stores stay off the link)
  const PlaceSpec dst[2] = {{no_pos ? nullptr : out->pos, (n + 1) * 8, 8}, {out->var, nv, 1}};
  clg::Placement pl;
  CHK(place_out(e->d_payout, dst, 2, out->out_kind, PlacePolicy::stage_unless_device, "payload", &pl));
  CHK(e->timed("decode_payloads", n * 12 + (no_pos ? 0 : (n + 1) * 8) + uint64_t(n_tiles) * 8 + 2 * nv, [&] {
    return clg::launch_pay_write(in, n_tiles, d_base, nv, pl.at<uint64_t>(0), pl.at<uint8_t>(1), e->stream);
  }));
  CHK(stage_out(e, dst, 2, pl));
  return e->sync();
}

// The wide rows' base per span (and their total), out of the span bases of all classes.
std::vector<uint64_t> wide_row_base(const uint64_t* span_base, uint32_t n) {
  std::vector<uint64_t> row_base(size_t(n) + 1);
  for (uint32_t s = 0; s <= n; ++s) row_base[s] = span_base[size_t(s) * clg::kColClasses + clg::kColWide];
  return row_base;
}

// decode_columns, then the payloads of the wide rows it produced (row_base: the columns' wide
// span bases).  The columns' status wins when it is not CLG_OK.
int decode_columns_var(clg_engine* e, const DecodeRun& run, uint32_t n, clg_columns* out, clg_payloads* var,
                       const PaySpansOf& spans_of) {
  clg::pay_reset_result(var);
  std::vector<uint64_t> own_sb;
  uint64_t* const caller_sb = out->span_base;
  if (!caller_sb) {  // (the wide bases are needed whether or not the caller asked for them)
    own_sb.assign(size_t(n + 1) * clg::kColClasses, 0);
    out->span_base = own_sb.data();
  }
  ColKeep keep;
  const int cs = decode_columns(e, run, n, out, &keep);
  const std::string col_err = g_err;
  const std::vector<uint64_t> row_base = wide_row_base(out->span_base, n);
  out->span_base = caller_sb;
  if (!keep.valid || (keep.col_status != CLG_OK && keep.col_status != CLG_E_CAPACITY)) return cs;
  std::vector<clg::PaySpan> spans;
  std::vector<uint32_t> segtab;
  int ps = spans_of(spans, segtab);
  if (ps == CLG_OK)
    ps = gather_payloads_device(e, spans, segtab, keep.d.w_var_off, keep.d.w_var_len, row_base.data(), var,
                                keep.col_status == CLG_E_CAPACITY);
  if (cs != CLG_OK) {
    g_err = col_err;
    return cs;
  }
  return ps;
}

DecodeSource source_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n) {
  return {run_logs(e, log, start_epoch, n), [=](std::vector<clg::PaySpan>& spans, std::vector<uint32_t>& segtab) {
            return payload_spans_logs(e, log, start_epoch, n, spans, segtab);
          }};
}
DecodeSource source_host(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                         uint32_t n) {
  return {run_host(e, bytes, span_off, span_len, n), [=](std::vector<clg::PaySpan>& spans, std::vector<uint32_t>&) {
            return payload_spans_bytes(e, bytes, span_off, span_len, n, CLG_MEM_HOST, spans);
          }};
}

extern "C" {

int clg_gather_payloads(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                        uint32_t n_spans, const uint32_t* w_var_off, const uint32_t* w_var_len,
                        const uint64_t* row_base, uint32_t in_kind, clg_payloads* out) {
  ENGINE_GUARD(e);
  if (!out || (n_spans && (!span_off || !span_len || !row_base))) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::pay_reset_result(out);
  if (in_kind != CLG_MEM_HOST && in_kind != CLG_MEM_DEVICE) return fail(CLG_E_INVALID_ARG, "in_kind %u", in_kind);
  if (!clg::pay_row_base_ok(row_base, n_spans)) return fail(CLG_E_INVALID_ARG, "row_base does not start at 0 or decreases");
  std::vector<clg::PaySpan> spans;
  CHK(payload_spans_bytes(e, bytes, span_off, span_len, n_spans, in_kind, spans));
  const uint32_t *d_off, *d_len;
  CHK(stage_payload_rows(e, w_var_off, w_var_len, n_spans ? row_base[n_spans] : 0, in_kind, &d_off, &d_len));
  return gather_payloads_device(e, spans, {}, d_off, d_len, row_base, out);
}

int clg_gather_payloads_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                             const uint32_t* w_var_off, const uint32_t* w_var_len, const uint64_t* row_base,
                             uint32_t in_kind, clg_payloads* out) {
  ENGINE_GUARD(e);
  if (!out || (n && (!log || !start_epoch || !row_base))) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::pay_reset_result(out);
  if (in_kind != CLG_MEM_HOST && in_kind != CLG_MEM_DEVICE) return fail(CLG_E_INVALID_ARG, "in_kind %u", in_kind);
  if (!clg::pay_row_base_ok(row_base, n)) return fail(CLG_E_INVALID_ARG, "row_base does not start at 0 or decreases");
  std::vector<clg::PaySpan> spans;
  std::vector<uint32_t> segtab;
  CHK(payload_spans_logs(e, log, start_epoch, n, spans, segtab));
  const uint32_t *d_off, *d_len;
  CHK(stage_payload_rows(e, w_var_off, w_var_len, n ? row_base[n] : 0, in_kind, &d_off, &d_len));
  return gather_payloads_device(e, spans, segtab, d_off, d_len, row_base, out);
}

int clg_decode_logs_columns_var(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                                clg_columns* out, clg_payloads* var) {
  ENGINE_GUARD(e);
  if (!out || !var || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  const DecodeSource src = source_logs(e, log, start_epoch, n);
  return decode_columns_var(e, src.run, n, out, var, src.spans_of);
}

int clg_decode_host_columns_var(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off,
                                const uint64_t* span_len, uint32_t n, clg_columns* out, clg_payloads* var) {
  ENGINE_GUARD(e);
  if (!out || !var || (n && (!span_off || !span_len))) return fail(CLG_E_INVALID_ARG, "null argument");
  // The bytes are staged again: the decode's staged copy shares d_stage with its fallbacks'
  // re-plans, so whether it is intact when the decode returns depends on the path the decode took.
  const DecodeSource src = source_host(e, bytes, span_off, span_len, n);
  return decode_columns_var(e, src.run, n, out, var, src.spans_of);
}

int clg_gather_payloads_host(const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                             uint32_t n_spans, const uint32_t* w_var_off, const uint32_t* w_var_len,
                             const uint64_t* row_base, clg_payloads* out) {
  const char* what = "";
  const int st = clg::pay_build_host(bytes, span_off, span_len, n_spans, w_var_off, w_var_len, row_base, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "payloads: %s", what);
}

int clg_columnize(clg_engine* e, const clg_decoded* in, const uint64_t* span_rec_base, uint32_t n_spans,
                  clg_columns* out) {
  ENGINE_GUARD(e);
  if (!in || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  if (in->out_kind != CLG_MEM_DEVICE && in->out_kind != CLG_MEM_MAPPED)  // (host input is not staged here)
    return fail(CLG_E_INVALID_ARG, "the decoded batch must be device or registered memory (out_kind %u)", in->out_kind);
  clg_decoded d = *in;
  // registered host memory: its device side.  (Element size 1: the input's alignment is not checked.)
  const uint64_t n = in->n_rec, w = in->n_wide;
  const PlaceSpec ins[8] = {{d.tag, n, 1},       {d.v0, n * 8, 1},        {d.w_idx, w * 4, 1},     {d.w_rc, w * 4, 1},
                            {d.w_v1, w * 8, 1},  {d.w_var_off, w * 4, 1}, {d.w_var_len, w * 4, 1}, {d.w_sub, w, 1}};
  clg::Placement pl;
  CHK(place_arrays(ins, 8, in->out_kind, PlacePolicy::reject_unresolved, "input", &pl));
  d.tag = pl.at<uint8_t>(0), d.v0 = pl.at<int64_t>(1), d.w_idx = pl.at<uint32_t>(2), d.w_rc = pl.at<int32_t>(3);
  d.w_v1 = pl.at<int64_t>(4), d.w_var_off = pl.at<uint32_t>(5), d.w_var_len = pl.at<uint32_t>(6), d.w_sub = pl.at<uint8_t>(7);
  return columnize_device(e, d, span_rec_base, n_spans, out);
}

int clg_decode_logs_columns(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                            clg_columns* out) {
  ENGINE_GUARD(e);
  if (!out || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  return decode_columns(e, run_logs(e, log, start_epoch, n), n, out);
}

int clg_decode_host_columns(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                            uint32_t n, clg_columns* out) {
  ENGINE_GUARD(e);
  if (!out || (n && (!span_off || !span_len))) return fail(CLG_E_INVALID_ARG, "null argument");
  return decode_columns(e, run_host(e, bytes, span_off, span_len, n), n, out);
}

int clg_columnize_host(const clg_decoded* in, const uint64_t* span_rec_base, uint32_t n_spans, clg_columns* out) {
  const char* what = "";
  const int st = clg::col_build_host(in, span_rec_base, n_spans, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "columns: %s", what);
}

}  // extern "C"
