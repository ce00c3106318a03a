// engine_columns.cpp -- the typed-columns family: the placement of its arrays (placement.h), the
// columns of a decoded batch and the decodes into columns, the payload column, packed columns out
// and in, packed wide rows, the encode of typed columns and their append to logs; clg_pack_columns to
// clg_columnize_host, clg_pack_wide*, clg_unpack_wide_host, clg_decode_*_columns_packed_wide,
// clg_encode_columns*, clg_append_columns*, clg_unpack_columns*, clg_unpack_wide and the calls that
// take both packed forms (clg_*_columns_packed_wide*).  The placement
// helpers are file-local; decode_columns and decode_columns_var are declared in engine_impl.h for
// replay preparation (engine_replay.cpp).
#include "engine_impl.h"
#include "columns.h"
#include "encode_columns.h"
#include "pack.h"
#include "pack_wide.h"
#include "payload.h"
#include "placement.h"

// ---- typed replay columns (columns.h) -------------------------------------------------------
// The stable partition of a decoded batch by determinant class, from the decode's output where
// it lies: count and scan, the host's capacity check on the scan's totals, then the write, the
// span bases and the wide rows' v0.  LogReplayerImpl (LogReplayerImpl.java:61-119) asks for one
// typed value at a time and never for a record's offset: the columns are what it consumes.
namespace {

// ---- placement (placement.h): where the kernels of this family read and write ------------------
static_assert(clg::kPlaceHost == CLG_MEM_HOST && clg::kPlaceDevice == CLG_MEM_DEVICE && clg::kPlaceMapped == CLG_MEM_MAPPED,
              "placement.h numbers the memory kinds as the ABI does");
using clg::mem_kind_ok;
using clg::PlacePolicy;
using clg::PlaceSpec;

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
int copy_caller(clg_engine* e, void* dst, const void* src, uint64_t bytes, hipMemcpyKind kind,
                uint32_t mem_kind = CLG_MEM_HOST) {
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
              size_t extra = 0) {
  CHK(place_arrays(s, n, kind, policy, what, pl));
  if (!pl->staged()) return CLG_OK;
  CHK(buf.ensure(pl->total + extra + 16));
  pl->bind(s, n, buf.p);
  return CLG_OK;
}
// The placement of inputs: the same, and a staged array's copy in queued (not an absent or empty one's).
int place_in(clg_engine* e, DevBuf& buf, const PlaceSpec* s, int n, uint32_t kind, PlacePolicy policy, const char* what,
             clg::Placement* pl, size_t extra = 0) {
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
int pay_too_small(const char* name, uint64_t rows, uint64_t bytes) {
  return fail(CLG_E_CAPACITY, "%s is too small (rows %llu, payload bytes %llu)", name, (unsigned long long)rows,
              (unsigned long long)bytes);
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

}  // namespace

// The decode into engine scratch (the host-output staging arrays, kept between calls), grown
// and run again on the decode's own CLG_E_CAPACITY, then the columns of what it produced.
// keep (optional): the decoded batch in engine scratch and columnize_device's own status, for
// the payload column of the same rows (decode_columns_var).
struct ColKeep {
  clg_decoded d{};
  bool valid = false;        // the decode produced a batch and columnize_device ran
  int col_status = CLG_OK;   // columnize_device's
};
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

namespace {

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

// d_off / d_len: device addresses of the rows.  sizes_forced: fill the results, write nothing.
int gather_payloads_device(clg_engine* e, const std::vector<clg::PaySpan>& spans, const std::vector<uint32_t>& segtab,
                           const uint32_t* d_off, const uint32_t* d_len, const uint64_t* row_base, clg_payloads* out,
                           bool sizes_forced = false, bool no_pos = false) {
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

// The wide rows' base per span (and their total), out of the span bases of all classes.
std::vector<uint64_t> wide_row_base(const uint64_t* span_base, uint32_t n) {
  std::vector<uint64_t> row_base(size_t(n) + 1);
  for (uint32_t s = 0; s <= n; ++s) row_base[s] = span_base[size_t(s) * clg::kColClasses + clg::kColWide];
  return row_base;
}

}  // namespace

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

namespace {

// ---- packed typed columns (pack.h) ----------------------------------------------------------
// The five narrow columns bit-packed where they lie: measure and the offset scan, the host's
// capacity check on the scan's total, then the write.  A LogReplayerImpl cursor
// (LogReplayerImpl.java:61-119) pops one typed value at a time from the blocks.

// Measure and scan over device-side streams: out's results are filled, the descriptors (with
// their offsets) are left in d_packdesc.
int pack_sizes(clg_engine* e, const clg::PackSrc& src, clg_packed* out, clg::PackIn* pin) {
  clg::pack_reset_result(out);
  clg::pack_layout(src.n, out);
  const uint64_t nb = out->blk_base[clg::kPackStreams];
  if (nb >> 31) return fail(CLG_E_INVALID_ARG, "%llu blocks in one call", (unsigned long long)nb);
  uint64_t in_bytes = 0;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) {
    if (src.n[c] && !src.col[c]) return fail(CLG_E_INVALID_ARG, "null input array (stream %u)", c);
    if (uintptr_t(src.col[c]) % clg::pack_stream_bytes(c))
      return fail(CLG_E_INVALID_ARG, "stream %u is not aligned to its element", c);
    pin->col[c] = src.col[c], pin->n[c] = src.n[c];
    in_bytes += src.n[c] * clg::pack_stream_bytes(c);
  }
  for (uint32_t c = 0; c <= clg::kPackStreams; ++c) pin->blk_base[c] = out->blk_base[c];
  const uint64_t ng = (nb + clg::kPackScanGroup - 1) / clg::kPackScanGroup;
  CHK(e->d_packdesc.ensure(size_t(nb) * sizeof(clg_pack_block) + 64));
  CHK(e->d_packsum.ensure(size_t(ng) * 8 + 64));
  CHK(e->h_packres.ensure(sizeof(clg::PackRes)));
  clg::PackRes* res = e->h_packres.as<clg::PackRes>();
  // (bytes: the columns once, a descriptor written, read and written again, the groups' sums)
  CHK(e->timed("pack_columns", in_bytes + nb * 72 + ng * 24, [&] {
    return clg::launch_pack_measure_scan(*pin, uint32_t(nb), e->d_packdesc.as<clg_pack_block>(), e->d_packsum.as<uint64_t>(),
                                         res, e->stream);
  }));
  CHK(e->sync());
  out->n_bits = res->n_bits;
  return CLG_OK;
}

// ---- what the two packed families share, over a PackView of either's struct ---------------------

int pack_out_check(const clg::PackView& out, const char* what = "") {  // (a packed input's, too)
  if (!mem_kind_ok(out.out_kind)) return fail(CLG_E_INVALID_ARG, "%sout_kind %u", what, out.out_kind);
  if (out.out_kind != CLG_MEM_HOST && (uintptr_t(out.desc) % 8 || uintptr_t(out.bits) % 16))
    return fail(CLG_E_INVALID_ARG, "desc must be aligned to 8 bytes and bits to 16");
  return CLG_OK;
}

// The write pass, after the sizes and the capacity check: device and registered outputs are
// written by the kernel, host ones through engine staging and one copy each.  launch(desc, bits):
// the family's write kernel over the placed outputs; in_bytes: what it reads of the values.
template <class Launch>
int pack_write(clg_engine* e, const clg::PackView& out, DevBuf& staging, const char* stat, uint64_t in_bytes,
               const Launch& launch) {
  const uint64_t nb = out.blocks(), nbits = *out.n_bits;
  if (!nb) return CLG_OK;
  const PlaceSpec dst[2] = {{out.desc, nb * sizeof(clg_pack_block), 8}, {out.bits, nbits, 16}};
  clg::Placement pl;
  CHK(place_out(staging, dst, 2, out.out_kind, PlacePolicy::stage_if_unresolved, "packed", &pl));
  CHK(e->timed(stat, in_bytes + nb * 64 + nbits, [&] { return launch(pl.at<clg_pack_block>(0), pl.at<uint8_t>(1)); }));
  CHK(stage_out(e, dst, 2, pl));
  return e->sync();
}

// prefix: "packed columns" or "packed wide rows".
int pack_capacity_error(const clg::PackView& out, const char* prefix, const char* name) {
  return fail(CLG_E_CAPACITY, "%s: %s is too small (blocks %llu, payload bytes %llu)", prefix, name,
              (unsigned long long)out.blocks(), (unsigned long long)*out.n_bits);
}

// Past the sizes: nothing more for the sizes-only call, the capacity error for a short output,
// else the write.
template <class Write>
int pack_finish(const clg::PackView& out, const char* prefix, const Write& write) {
  if (clg::pack_sizes_only(out)) return CLG_OK;
  if (const char* name = clg::pack_short(out)) return pack_capacity_error(out, prefix, name);
  return write();
}

int pack_write(clg_engine* e, const clg::PackIn& pin, const clg_packed* out) {
  uint64_t in_bytes = 0;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) in_bytes += pin.n[c] * clg::pack_stream_bytes(c);
  const uint64_t nb = out->blk_base[clg::kPackStreams];
  const auto launch = [&](clg_pack_block* desc, uint8_t* bits) {
    return clg::launch_pack_write(pin, uint32_t(nb), e->d_packdesc.as<clg_pack_block>(), desc, bits, nb, out->n_bits, e->stream);
  };
  return pack_write(e, clg::pack_view(*out), e->d_packout, "pack_columns", in_bytes, launch);
}

// ---- packed wide rows (pack_wide.h) ---------------------------------------------------------
// Kind and count and the scan of the tile counts, the host's check of the bad-row word and its
// layout of the 26 streams from the four totals, the split into per-kind arrays in engine scratch,
// measure and the offset scan, the host's capacity check, then the write.

// Everything up to the sizes, over device-side rows: out's results are filled, the stream table is
// left in d_wpacktab and the descriptors (with their offsets) in d_wpackdesc.
int wpack_sizes(clg_engine* e, const clg::WPackSrc& src, clg_packed_wide* out) {
  clg::wpack_reset_result(out);
  const uint64_t nw = src.n_wide;
  if (nw >> 32) return fail(CLG_E_INVALID_ARG, "%llu wide rows in one call", (unsigned long long)nw);
  if (!nw) return CLG_OK;  // no rows: 26 empty streams, nothing to launch (a log without wide records pays nothing)
  const uint32_t nt = uint32_t((nw + clg::kWPackTile - 1) / clg::kWPackTile);
  const uint64_t kb[4] = {nw, uint64_t(nt) * clg::kWPackKinds * 4, uint64_t(nt) * clg::kWPackKinds * 8, 8};
  size_t ka[5];
  CHK(e->d_wpackkind.ensure(clg::place_layout(kb, 4, ka) + 16));
  uint8_t* ks = e->d_wpackkind.as<uint8_t>();
  uint8_t* d_kind = ks + ka[0];
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(ks + ka[1]);
  uint64_t* d_base = reinterpret_cast<uint64_t*>(ks + ka[2]);
  unsigned long long* d_bad = reinterpret_cast<unsigned long long*>(ks + ka[3]);
  CHK(e->h_wpackres.ensure(sizeof(clg::WPackRes) + sizeof(clg::PackRes)));
  clg::WPackRes* res = e->h_wpackres.as<clg::WPackRes>();
  clg::PackRes* pres = reinterpret_cast<clg::PackRes*>(res + 1);
  // (bytes: w_idx, a tag and the kind byte a row; the tile counts written, read and their bases written)
  CHK(e->timed("pack_wide", nw * 6 + uint64_t(nt) * 64,
               [&] { return clg::launch_wpack_count_scan(src, nt, d_kind, d_cnt, d_base, d_bad, res, e->stream); }));
  CHK(e->sync());
  if (res->bad_row != ~0ull) {
    out->bad_row = res->bad_row;
    return fail(CLG_E_INVALID_ARG, "packed wide rows: row %llu's w_idx or tag is not a wide record's", (unsigned long long)res->bad_row);
  }
  if (res->tot[0] + res->tot[1] + res->tot[2] + res->tot[3] != nw) return fail(CLG_E_DEVICE, "packed wide rows: the kinds' totals do not sum to the rows");
  clg::wpack_layout(nw, res->tot, out);
  const uint64_t nb = out->blk_base[clg::kWPackStreams];

  // the per-kind arrays and the stream table
  constexpr int kArrays = int(clg::kWPackKinds * clg::kWPackFields);
  uint64_t cb[kArrays];
  size_t so[kArrays + 1];
  for (uint32_t t = 0; t < clg::kWPackKinds; ++t)
    for (uint32_t f = 0; f < clg::kWPackFields; ++f)
      cb[t * clg::kWPackFields + f] = res->tot[t] * clg::pack_elem_bytes(clg::kWPackField[f].elem);
  CHK(e->d_wpacksoa.ensure(clg::place_layout(cb, kArrays, so) + 16));
  CHK(e->h_wpacktab.ensure(sizeof(clg::WPackTab)));
  CHK(e->d_wpacktab.ensure(sizeof(clg::WPackTab)));
  clg::WPackTab* tab = e->h_wpacktab.as<clg::WPackTab>();
  tab->col[CLG_WPACK_KIND] = d_kind, tab->col[CLG_WPACK_IDX] = src.w_idx;
  for (int i = 0; i < kArrays; ++i) tab->col[2 + i] = e->d_wpacksoa.as<uint8_t>() + so[i];
  for (uint32_t c = 0; c < clg::kWPackStreams; ++c) tab->n[c] = out->n_val[c];
  for (uint32_t c = 0; c <= clg::kWPackStreams; ++c) tab->blk_base[c] = out->blk_base[c];
  HIPCHK(hipMemcpyAsync(e->d_wpacktab.p, tab, sizeof(clg::WPackTab), hipMemcpyHostToDevice, e->stream));
  const uint64_t ng = (nb + clg::kPackScanGroup - 1) / clg::kPackScanGroup;
  CHK(e->d_wpackdesc.ensure(size_t(nb) * sizeof(clg_pack_block) + 64));
  CHK(e->d_wpacksum.ensure(size_t(ng) * 8 + 64));
  // (bytes: the split reads a kind byte and 29 B a row and writes them; the measure reads the 26
  // streams, 34 B a row; a descriptor written, read and written again, the groups' sums)
  CHK(e->timed("pack_wide", nw * (1 + 29 + 29 + 34) + nb * 72 + ng * 24, [&] {
    const int st = clg::launch_wpack_split_measure(src, nt, d_kind, d_base, e->d_wpacktab.as<clg::WPackTab>(), uint32_t(nb),
                                                   e->d_wpackdesc.as<clg_pack_block>(), e->stream);
    if (st != CLG_OK) return st;
    return clg::launch_pack_scan(uint32_t(nb), e->d_wpackdesc.as<clg_pack_block>(), e->d_wpacksum.as<uint64_t>(), pres, e->stream);
  }));
  CHK(e->sync());
  out->n_bits = pres->n_bits;
  return CLG_OK;
}

int wpack_write(clg_engine* e, const clg_packed_wide* out) {
  const uint64_t nb = out->blk_base[clg::kWPackStreams];
  const auto launch = [&](clg_pack_block* desc, uint8_t* bits) {
    return clg::launch_wpack_write(e->d_wpacktab.as<clg::WPackTab>(), uint32_t(nb), e->d_wpackdesc.as<clg_pack_block>(), desc, bits,
                                   nb, out->n_bits, e->stream);
  };
  return pack_write(e, clg::pack_view(*out), e->d_wpackout, "pack_wide", out->n_val[CLG_WPACK_KIND] * 34, launch);
}

// The decode into engine scratch and the columns of what it produced, also in engine scratch;
// then the pack, the wide rows as they are and (var) the payload column of the same rows.
// Every size is known before anything is written to the caller.  wpk (the packed-wide decodes):
// the wide rows are delivered packed as well and no plain row is copied to the caller; `wide` then
// carries only sizes, and var may come without pos, which is the prefix sum of w_var_len.
int decode_columns_packed(clg_engine* e, const DecodeRun& run, uint32_t n, clg_columns* wide, clg_payloads* var,
                          clg_packed* out, const PaySpansOf& spans_of, clg_packed_wide* wpk = nullptr) {
  if (wide->tag || wide->order || wide->timestamp || wide->rng || wide->buffer_built)
    return fail(CLG_E_INVALID_ARG, "the narrow column pointers of `wide` must be NULL: those columns are delivered packed");
  if (wpk)
    for (int i = clg::kColNarrowArrays; i < clg::kColArrays; ++i)
      if (clg::col_ptr(*wide, i)) return fail(CLG_E_INVALID_ARG, "every column pointer of `sizes` must be NULL: the wide rows are delivered packed");
  if (!mem_kind_ok(wide->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", wide->out_kind);
  CHK(pack_out_check(clg::pack_view(*out)));
  if (wpk) CHK(pack_out_check(clg::pack_view(*wpk)));
  clg::col_reset_result(wide);
  clg::pack_reset_result(out);
  if (wpk) clg::wpack_reset_result(wpk);
  if (var) clg::pay_reset_result(var);
  const bool no_pos = wpk && var && var->var && !var->pos;

  // the decode, and the columns' sizes and span bases
  std::vector<uint64_t> sb(size_t(n + 1) * clg::kColClasses, 0);
  clg_columns sizes{};
  sizes.span_base = sb.data();
  sizes.out_kind = CLG_MEM_DEVICE;
  ColKeep keep;
  const int cs = decode_columns(e, run, n, &sizes, &keep);
  const std::string col_err = g_err;
  wide->n_rec = sizes.n_rec;
  for (uint32_t c = 0; c < clg::kColClasses; ++c) wide->n_class[c] = sizes.n_class[c];
  wide->err_status = sizes.err_status, wide->err_span = sizes.err_span;
  wide->err_off = sizes.err_off, wide->err_tag = sizes.err_tag;
  if (!keep.valid || keep.col_status != CLG_OK) return cs;
  if (wide->span_base) memcpy(wide->span_base, sb.data(), sb.size() * 8);
  const uint64_t nr = sizes.n_rec, nw = sizes.n_class[clg::kColWide];
  const uint64_t* tot = sizes.n_class;

  // the narrow columns and w_v0 into engine scratch (the tags and the side rows stay where the
  // decode left them)
  const uint64_t cb[5] = {tot[0], tot[1] * 8, tot[2] * 4, tot[3] * 4, nw * 8};
  size_t at[6];
  CHK(e->d_packcol.ensure(clg::place_layout(cb, 5, at) + 16));
  uint8_t* sc = e->d_packcol.as<uint8_t>();
  clg_columns full{};
  full.tag = keep.d.tag, full.order = reinterpret_cast<int8_t*>(sc + at[0]);
  full.timestamp = reinterpret_cast<int64_t*>(sc + at[1]), full.rng = reinterpret_cast<int32_t*>(sc + at[2]);
  full.buffer_built = reinterpret_cast<int32_t*>(sc + at[3]), full.w_v0 = reinterpret_cast<int64_t*>(sc + at[4]);
  full.w_idx = keep.d.w_idx, full.w_rc = keep.d.w_rc, full.w_v1 = keep.d.w_v1, full.w_var_off = keep.d.w_var_off;
  full.w_var_len = keep.d.w_var_len, full.w_sub = keep.d.w_sub;
  full.cap_tag = nr, full.cap_order = tot[0], full.cap_timestamp = tot[1], full.cap_rng = tot[2];
  full.cap_buffer_built = tot[3], full.cap_wide = nw;
  full.out_kind = CLG_MEM_DEVICE;
  CHK(columnize_device(e, keep.d, nullptr, 0, &full));

  // every size, before anything is written to the caller
  const clg::PackSrc src{{full.tag, full.order, full.timestamp, full.rng, full.buffer_built}, {nr, tot[0], tot[1], tot[2], tot[3]}};
  clg::PackIn pin{};
  CHK(pack_sizes(e, src, out, &pin));
  if (wpk)
    CHK(wpack_sizes(e, clg::WPackSrc{full.tag, full.w_idx, full.w_rc, full.w_v1, full.w_var_off, full.w_var_len, full.w_sub, full.w_v0, nr, nw},
                    wpk));
  int ps = CLG_OK;
  std::vector<clg::PaySpan> spans;
  std::vector<uint32_t> segtab;
  const std::vector<uint64_t> row_base = wide_row_base(sb.data(), n);
  if (var) {
    ps = spans_of(spans, segtab);
    if (ps == CLG_OK) ps = gather_payloads_device(e, spans, segtab, keep.d.w_var_off, keep.d.w_var_len, row_base.data(), var, true);
  }
  const std::string pay_err = g_err;
  const int w0 = clg::kColNarrowArrays, w1 = clg::kColArrays;  // (the wide arrays: the table's last seven)
  bool wide_any = false, wide_short = false;
  for (int i = w0; i < w1; ++i) wide_any = wide_any || clg::col_ptr(*wide, i);
  for (int i = w0; i < w1; ++i) wide_short = wide_short || (wide_any && clg::col_array_cap(*wide, i) < nw);
  const clg::PackView pv = clg::pack_view(*out), wpv = wpk ? clg::pack_view(*wpk) : clg::PackView{};
  const char* pk_short = clg::pack_sizes_only(pv) ? nullptr : clg::pack_short(pv);
  const char* wpk_short = wpk && !clg::pack_sizes_only(wpv) ? clg::pack_short(wpv) : nullptr;
  const char* pay_short = !var || ps != CLG_OK || clg::pay_sizes_only(*var) ? nullptr
                          : !no_pos                                         ? clg::pay_short(*var, var->n_rows, var->n_var)
                          : var->cap_var < var->n_var                       ? "var"
                                                                            : nullptr;
  if (wide_short) return fail(CLG_E_CAPACITY, "the wide rows' arrays are too small (rows %llu)", (unsigned long long)nw);
  if (pk_short) return pack_capacity_error(pv, "packed columns", pk_short);
  if (wpk_short) return pack_capacity_error(wpv, "packed wide rows", wpk_short);
  if (pay_short) return pay_too_small(pay_short, var->n_rows, var->n_var);

  // the writes
  if (!clg::pack_sizes_only(pv)) CHK(pack_write(e, pin, out));
  if (wpk && !clg::pack_sizes_only(wpv)) CHK(wpack_write(e, wpk));
  if (wide_any && nw) {
    for (int i = w0; i < w1; ++i)
      CHK(copy_caller(e, clg::col_ptr(*wide, i), clg::col_ptr(full, i), nw * clg::kColArray[i].width, hipMemcpyDefault,
                      wide->out_kind));
    CHK(e->sync());
  }
  if (var && ps == CLG_OK && !clg::pay_sizes_only(*var))
    ps = gather_payloads_device(e, spans, segtab, keep.d.w_var_off, keep.d.w_var_len, row_base.data(), var, false, no_pos);
  else if (ps != CLG_OK)
    g_err = pay_err;
  if (cs != CLG_OK) {
    g_err = col_err;
    return cs;
  }
  return ps;
}

// What the decode-to-columns entry points decode, per source kind: `run` decodes it into the
// arrays it is given, `spans_of` gives its spans to the payload gather.
struct DecodeSource {
  DecodeRun run;
  PaySpansOf spans_of;
};
DecodeRun run_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n) {
  return [=](clg_decoded* d, uint64_t* base) { return clg_decode_logs(e, log, start_epoch, n, d, base); };
}
DecodeRun run_host(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len, uint32_t n) {
  return [=](clg_decoded* d, uint64_t* base) { return clg_decode_host(e, bytes, span_off, span_len, n, d, base); };
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

}  // namespace

extern "C" {

int clg_pack_columns(clg_engine* e, const clg_columns* in, clg_packed* out) {
  ENGINE_GUARD(e);
  if (!in || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::pack_reset_result(out);
  CHK(pack_out_check(clg::pack_view(*out)));
  clg::PackSrc src = clg::pack_src(*in);
  for (uint32_t c = 0; c < clg::kPackStreams; ++c)
    if (src.n[c] && !src.col[c]) return fail(CLG_E_INVALID_ARG, "null input array (stream %u)", c);
  if (!mem_kind_ok(in->out_kind)) return fail(CLG_E_INVALID_ARG, "the columns' out_kind %u", in->out_kind);
  PlaceSpec ins[clg::kPackStreams];
  for (uint32_t c = 0; c < clg::kPackStreams; ++c)
    ins[c] = {src.col[c], src.n[c] * clg::pack_stream_bytes(c), clg::pack_stream_bytes(c)};
  clg::Placement pl;
  const int st = place_in(e, e->d_packin, ins, clg::kPackStreams, in->out_kind, PlacePolicy::stage_if_unresolved, "stream", &pl);
  if (st != CLG_OK) return clg::pack_layout(src.n, out), st;  // (a misaligned stream: the layout is filled, as pack_sizes fills it)
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) src.col[c] = pl.at<const void>(c);
  clg::PackIn pin{};
  CHK(pack_sizes(e, src, out, &pin));
  return pack_finish(clg::pack_view(*out), "packed columns", [&] { return pack_write(e, pin, out); });
}

int clg_pack_wide(clg_engine* e, const clg_columns* in, clg_packed_wide* out) {
  ENGINE_GUARD(e);
  if (!in || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::wpack_reset_result(out);
  CHK(pack_out_check(clg::pack_view(*out)));
  if (!mem_kind_ok(in->out_kind)) return fail(CLG_E_INVALID_ARG, "the columns' out_kind %u", in->out_kind);
  const uint64_t nr = in->n_rec, nw = in->n_class[clg::kColWide];
  const PlaceSpec ins[8] = {{in->tag, nw ? nr : 0, 1},         {in->w_idx, nw * 4, 4},     {in->w_rc, nw * 4, 4}, {in->w_v1, nw * 8, 8},
                            {in->w_var_off, nw * 4, 4}, {in->w_var_len, nw * 4, 4}, {in->w_sub, nw, 1},    {in->w_v0, nw * 8, 8}};
  for (int i = 1; i < 8; ++i)
    if (nw && !ins[i].p) return fail(CLG_E_INVALID_ARG, "null input array (%d)", i);
  if (nw && !in->tag) return fail(CLG_E_INVALID_ARG, "null input array (tag)");
  clg::Placement pl;
  CHK(place_in(e, e->d_wpackin, ins, 8, in->out_kind, PlacePolicy::stage_if_unresolved, "wide", &pl));
  const clg::WPackSrc src{pl.at<const uint8_t>(0),  pl.at<const uint32_t>(1), pl.at<const int32_t>(2), pl.at<const int64_t>(3),
                          pl.at<const uint32_t>(4), pl.at<const uint32_t>(5), pl.at<const uint8_t>(6), pl.at<const int64_t>(7),
                          nr,                       nw};
  CHK(wpack_sizes(e, src, out));
  return pack_finish(clg::pack_view(*out), "packed wide rows", [&] { return wpack_write(e, out); });
}

int clg_pack_wide_host(const clg_columns* in, clg_packed_wide* out) {
  const char* what = "";
  const int st = clg::wpack_build_host(in, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "packed wide rows: %s", what);
}

int clg_unpack_wide_host(const clg_packed_wide* in, clg_columns* out, clg_unpack_bad* bad) {
  const char* what = "";
  const int st = clg::wpack_unpack_host(in, out, bad, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "unpack wide rows: %s", what);
}

int clg_decode_logs_columns_packed(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                                   clg_columns* wide, clg_payloads* var, clg_packed* out) {
  ENGINE_GUARD(e);
  if (!wide || !out || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  const DecodeSource src = source_logs(e, log, start_epoch, n);
  return decode_columns_packed(e, src.run, n, wide, var, out, src.spans_of);
}

int clg_decode_host_columns_packed(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off,
                                   const uint64_t* span_len, uint32_t n, clg_columns* wide, clg_payloads* var,
                                   clg_packed* out) {
  ENGINE_GUARD(e);
  if (!wide || !out || (n && (!span_off || !span_len))) return fail(CLG_E_INVALID_ARG, "null argument");
  const DecodeSource src = source_host(e, bytes, span_off, span_len, n);
  return decode_columns_packed(e, src.run, n, wide, var, out, src.spans_of);
}

int clg_decode_logs_columns_packed_wide(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                                        clg_columns* sizes, clg_payloads* var, clg_packed* narrow, clg_packed_wide* wide) {
  ENGINE_GUARD(e);
  if (!sizes || !narrow || !wide || (n && (!log || !start_epoch))) return fail(CLG_E_INVALID_ARG, "null argument");
  const DecodeSource src = source_logs(e, log, start_epoch, n);
  return decode_columns_packed(e, src.run, n, sizes, var, narrow, src.spans_of, wide);
}

int clg_decode_host_columns_packed_wide(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off,
                                        const uint64_t* span_len, uint32_t n, clg_columns* sizes, clg_payloads* var,
                                        clg_packed* narrow, clg_packed_wide* wide) {
  ENGINE_GUARD(e);
  if (!sizes || !narrow || !wide || (n && (!span_off || !span_len))) return fail(CLG_E_INVALID_ARG, "null argument");
  const DecodeSource src = source_host(e, bytes, span_off, span_len, n);
  return decode_columns_packed(e, src.run, n, sizes, var, narrow, src.spans_of, wide);
}

int clg_pack_columns_host(const clg_columns* in, clg_packed* out) {
  const char* what = "";
  const int st = clg::pack_build_host(in, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "packed columns: %s", what);
}

int clg_unpack_columns_host(const clg_packed* in, uint32_t stream, uint64_t first, uint64_t count, void* out) {
  const char* what = "";
  const int st = clg::pack_unpack_host(in, stream, first, count, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "unpack columns: %s", what);
}

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

// ---- encode typed columns (encode_columns.h) ------------------------------------------------
namespace {

// A checked, sized encode: what the write pass needs.
struct EcolPlan {
  clg::EcolIn d{};
  uint32_t n_tiles = 0;
  const uint64_t* d_base = nullptr;
  const uint64_t* d_bbase = nullptr;
  uint64_t n_bytes = 0;
  uint64_t in_bytes = 0;  // bytes of the input arrays (for the stats)
};

// The packed calls: device addresses of the leading n arrays in EcolIn's order (5: the narrow
// columns; 12: the wide rows, w_idx and pos as well), used as they are whatever in_kind says of
// the other arrays.  cross (the packed-wide calls): the cross rule's word in pinned memory, filled
// by a copy queued before the sizes; it is read after their sync and before the encode's own checks.
struct EcolDev {
  const void* col[12] = {};
  int n = 0;
  const unsigned long long* cross = nullptr;
  clg_unpack_bad* bad = nullptr;
};

int ecol_invalid(clg_encoded* out, uint32_t what, uint64_t index) {
  static const char* const kind[] = {"", "tag", "totals", "span", "row"};
  out->n_bytes = 0;
  out->bad_what = what;
  out->bad_index = index;
  return fail(CLG_E_INVALID_ARG, "encode columns: bad %s, index %llu", kind[what], (unsigned long long)index);
}

// Count, scan, bytes, scan64 and span bases, then the host's check of their results (pinned) --
// before any byte is written anywhere.  Fills out's results and, when given, sbb[ns + 1].
// dev (the packed calls): see EcolDev.
int ecol_sizes(clg_engine* e, const clg_columns_in* in, clg_encoded* out, EcolPlan* p, uint64_t* sbb,
               const EcolDev* dev = nullptr) {
  clg::ecol_reset_result(out);
  if (!clg::ecol_args_ok(*in)) return fail(CLG_E_INVALID_ARG, "encode columns: null input array or unknown in_kind");
  const uint64_t n = in->n_rec, *nc = in->n_class, nw = nc[clg::kColWide];
  const uint32_t ns = clg::ecol_spans(*in);
  const uint64_t rows_bad = clg::ecol_span_rows_bad(*in);
  // the arrays, in EcolIn's order: bytes, and element sizes for the alignment check
  PlaceSpec ins[13] = {{in->tag, n, 1},        {in->order, nc[0], 1},  {in->timestamp, nc[1] * 8, 8}, {in->rng, nc[2] * 4, 4},
                       {in->buffer_built, nc[3] * 4, 4},                {in->w_rc, nw * 4, 4},         {in->w_v1, nw * 8, 8},
                       {in->w_var_len, nw * 4, 4},                      {in->w_sub, nw, 1},            {in->w_v0, nw * 8, 8},
                       {in->w_idx, nw * 4, 4}, {in->pos, (nw + 1) * 8, 8},                             {in->var, in->n_var, 1}};
  for (const PlaceSpec& a : ins) p->in_bytes += a.p ? a.bytes : 0;
  // registered arrays must be registered whole; host arrays are staged, an empty one too (a valid
  // address, never read).  With dev its arrays take no part (no slot, no lookup, no copy): they
  // are absent from the placement, and their addresses are set behind it.
  for (int i = 0; dev && i < dev->n; ++i) ins[i].p = nullptr;
  const size_t sb_bytes = in->n_spans ? size_t(ns + 1) * clg::kColClasses * 8 : 0;
  clg::Placement pl;
  CHK(place_in(e, e->d_ecolin, ins, 13, in->in_kind, PlacePolicy::reject_unresolved, "encode columns: input", &pl, sb_bytes));
  for (int i = 0; dev && i < dev->n; ++i) pl.dev[i] = uintptr_t(dev->col[i]);
  const size_t o_sb = pl.staged() ? pl.total : 0;  // the span bases lie behind the staged arrays
  if (!pl.staged()) CHK(e->d_ecolin.ensure(sb_bytes + 16));
  uint8_t* din = e->d_ecolin.as<uint8_t>();
  clg::EcolIn& d = p->d;
  d = clg::EcolIn{pl.at<const uint8_t>(0),  pl.at<const int8_t>(1),   pl.at<const int64_t>(2),  pl.at<const int32_t>(3),
                  pl.at<const int32_t>(4),  pl.at<const int32_t>(5),  pl.at<const int64_t>(6),  pl.at<const uint32_t>(7),
                  pl.at<const uint8_t>(8),  pl.at<const int64_t>(9),  pl.at<const uint32_t>(10), pl.at<const uint64_t>(11),
                  pl.at<const uint8_t>(12), n, {nc[0], nc[1], nc[2], nc[3], nc[4]}, in->n_var};
  const uint64_t* d_sb = nullptr;
  if (sb_bytes && rows_bad == clg::kEcolNone) {
    HIPCHK(hipMemcpyAsync(din + o_sb, in->span_base, sb_bytes, hipMemcpyHostToDevice, e->stream));
    d_sb = reinterpret_cast<const uint64_t*>(din + o_sb);
  }

  // work: counts | class bases | byte sums | bad rows | byte bases
  const uint64_t n_tiles64 = (n + clg::kEcolTile - 1) / clg::kEcolTile;
  if (n_tiles64 > 0x7FFFFFFFull) return fail(CLG_E_INVALID_ARG, "%llu records in one call", (unsigned long long)n);
  const uint32_t nt = uint32_t(n_tiles64);
  const uint64_t wb[5] = {uint64_t(nt) * clg::kColCountWords * 4, uint64_t(nt) * clg::kColClasses * 8, uint64_t(nt) * 8,
                          uint64_t(nt) * 8, uint64_t(nt) * 8};
  size_t wo[6];
  CHK(e->d_ecolw.ensure(clg::place_layout(wb, 5, wo) + 16));
  uint8_t* wk = e->d_ecolw.as<uint8_t>();
  uint32_t* d_counts = reinterpret_cast<uint32_t*>(wk + wo[0]);
  uint64_t* d_base = reinterpret_cast<uint64_t*>(wk + wo[1]);
  uint64_t* d_sum = reinterpret_cast<uint64_t*>(wk + wo[2]);
  uint64_t* d_bad = reinterpret_cast<uint64_t*>(wk + wo[3]);
  uint64_t* d_bbase = reinterpret_cast<uint64_t*>(wk + wo[4]);
  const size_t o_eres = clg_engine::al16(sizeof(clg::ColRes)), o_so = o_eres + clg_engine::al16(sizeof(clg::EcolRes));
  CHK(e->h_ecolres.ensure(o_so + size_t(ns + 1) * 16));
  clg::ColRes* cres = e->h_ecolres.as<clg::ColRes>();
  clg::EcolRes* eres = reinterpret_cast<clg::EcolRes*>(e->h_ecolres.as<uint8_t>() + o_eres);
  uint64_t* span_out = reinterpret_cast<uint64_t*>(e->h_ecolres.as<uint8_t>() + o_so);
  p->n_tiles = nt, p->d_base = d_base, p->d_bbase = d_bbase;

  const clg::ColIn cin{d.tag, nullptr, nullptr, n, nw};
  CHK(e->timed("encode_columns", n + 13 * nw + uint64_t(nt) * 120 + sb_bytes, [&] {
    CHK(clg::launch_col_count_scan(cin, nt, d_counts, d_base, cres, e->stream));
    return clg::launch_ecol_sizes(d, nt, d_base, d_sum, d_bad, d_bbase, cres, eres, d_sb, in->n_spans, span_out, e->stream);
  }));
  CHK(e->sync());
  if (dev && dev->cross && *dev->cross != ~0ull) {
    clg::wpack_bad_cross(dev->bad, *dev->cross);
    return fail(CLG_E_INVALID_ARG, "unpack wide rows: row %llu's w_idx names no wide record of its kind",
                (unsigned long long)*dev->cross);
  }
  if (cres->bad_tile != clg::kColNoTile) {
    CHK(clg::launch_col_find_bad(cin, cres->bad_tile, cres, e->stream));
    CHK(e->sync());
    return ecol_invalid(out, CLG_ENC_BAD_TAG, cres->bad_index);
  }
  for (uint32_t c = 0; c < clg::kColClasses; ++c)
    if (cres->total[c] != nc[c]) return ecol_invalid(out, CLG_ENC_BAD_TOTALS, c);
  if (rows_bad != clg::kEcolNone) return ecol_invalid(out, CLG_ENC_BAD_SPAN, rows_bad);
  if (d_sb)
    for (uint32_t s = 0; s <= ns; ++s)
      if (span_out[size_t(s) * 2 + 1]) return ecol_invalid(out, CLG_ENC_BAD_SPAN, s);
  if (eres->bad_row != clg::kEcolNone) return ecol_invalid(out, CLG_ENC_BAD_ROW, eres->bad_row);
  p->n_bytes = out->n_bytes = eres->n_bytes;
  for (uint32_t s = 0; s <= ns; ++s) {
    const uint64_t b = d_sb ? span_out[size_t(s) * 2] : s ? eres->n_bytes : 0;
    if (sbb) sbb[s] = b;
    if (out->span_byte_base) out->span_byte_base[s] = b;
  }
  return CLG_OK;
}

int ecol_write(clg_engine* e, const EcolPlan& p, uint8_t* d_dst) {
  return e->timed("encode_columns", p.in_bytes + uint64_t(p.n_tiles) * 48 + p.n_bytes, [&] {
    return clg::launch_ecol_write(p.d, p.n_tiles, p.d_base, p.d_bbase, p.n_bytes, d_dst, e->stream);
  });
}

// clg_encode_columns after its argument checks (the engine guard held); dev as ecol_sizes'.
int encode_columns_checked(clg_engine* e, const clg_columns_in* in, clg_encoded* out, const EcolDev* dev) {
  EcolPlan p;
  CHK(ecol_sizes(e, in, out, &p, nullptr, dev));
  if (!out->bytes) return CLG_OK;  // sizes only
  if (out->cap < p.n_bytes) return fail(CLG_E_CAPACITY, "encode columns needs %llu bytes", (unsigned long long)p.n_bytes);
  if (!p.n_bytes) return CLG_OK;
  // host and registered memory alike go through staging: the edge byte stores stay off the link
  const PlaceSpec dst[1] = {{out->bytes, p.n_bytes, 1}};
  clg::Placement pl;
  CHK(place_out(e->d_ecolout, dst, 1, out->out_kind, PlacePolicy::stage_unless_device, "output", &pl));
  CHK(ecol_write(e, p, pl.at<uint8_t>(0)));
  CHK(stage_out(e, dst, 1, pl));
  return e->sync();
}

int append_columns_checked(clg_engine* e, const uint32_t* log, const int64_t* epoch, const clg_columns_in* in,
                           uint64_t* span_bytes, int32_t* status, const EcolDev* dev);

}  // namespace

extern "C" {

int clg_encode_columns(clg_engine* e, const clg_columns_in* in, clg_encoded* out) {
  ENGINE_GUARD(e);
  if (!in || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  return encode_columns_checked(e, in, out, nullptr);
}

int clg_encode_columns_host(const clg_columns_in* in, clg_encoded* out) {
  const char* what = "";
  const int st = clg::ecol_build_host(in, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "encode columns: %s", what);
}

int clg_append_columns(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans,
                       const clg_columns_in* in, uint64_t* span_bytes, int32_t* status) {
  ENGINE_GUARD(e);
  if (!in || !log || !epoch || !status) return fail(CLG_E_INVALID_ARG, "null argument");
  const uint32_t ns = clg::ecol_spans(*in);
  if (n_spans != ns) return fail(CLG_E_INVALID_ARG, "%u logs for %u spans", n_spans, ns);
  for (uint32_t s = 0; s < ns; ++s) status[s] = CLG_OK;
  return append_columns_checked(e, log, epoch, in, span_bytes, status, nullptr);
}

}  // extern "C"

namespace {
// clg_append_columns after its argument checks (the engine guard held, every status CLG_OK);
// dev as ecol_sizes'.
int append_columns_checked(clg_engine* e, const uint32_t* log, const int64_t* epoch, const clg_columns_in* in,
                           uint64_t* span_bytes, int32_t* status, const EcolDev* dev) {
  const uint32_t ns = clg::ecol_spans(*in);
  CHK(e->flush());  // pending host bytes first: the logs keep their byte order
  clg_encoded enc{};
  enc.out_kind = CLG_MEM_DEVICE;
  EcolPlan p;
  std::vector<uint64_t> sbb(size_t(ns) + 1);
  CHK(ecol_sizes(e, in, &enc, &p, sbb.data(), dev));
  for (uint32_t s = 0; s < ns && span_bytes; ++s) span_bytes[s] = sbb[s + 1] - sbb[s];
  CHK(e->d_ecolout.ensure(p.n_bytes + 16));
  CHK(ecol_write(e, p, e->d_ecolout.as<uint8_t>()));
  CHK(e->gwait());  // the scatter below writes segments an in-flight gather may read

  size_t bound = 0;
  for (uint32_t s = 0; s < ns; ++s) bound += size_t((sbb[s + 1] - sbb[s]) / e->C()) + 2;
  CHK(e->h_desc.ensure(bound * sizeof(clg::ScatterChunk)));
  clg::ScatterChunk *const ch0 = e->h_desc.as<clg::ScatterChunk>(), *ch = ch0;
  size_t total = 0;
  {
    std::lock_guard<std::mutex> pool_guard(e->pool_mu);
    for (uint32_t s = 0; s < ns; ++s) {  // clg_engine::append's steps, a span at a time
      const uint64_t len = sbb[s + 1] - sbb[s];
      Log* l;
      if ((status[s] = e->get_log(log[s], &l)) != CLG_OK) continue;
      if (l->depth == 0) continue;
      if (len >> 31) {
        status[s] = fail(CLG_E_INVALID_ARG, "span %u holds %llu bytes", s, (unsigned long long)len);
        continue;
      }
      if ((status[s] = e->ensure_space_locked(*l, int32_t(len))) != CLG_OK) continue;
      clg_engine::compute_if_absent(*l, epoch[s]);
      ch = e->add_chunks(ch, *l, uint32_t(l->writer), uint32_t(len), sbb[s]);
      l->writer += int32_t(len);
      l->flushed = l->writer;
      clg_engine::reset_tail(*l);  // these bytes are in HBM only
      total += size_t(len);
    }
  }
  if (ch == ch0) return e->sync();
  CHK(e->scatter_chunks("append_columns_scatter", size_t(ch - ch0), total, e->d_ecolout.as<uint8_t>(), true));
  return e->sync();  // the pinned descriptors are free again
}
}  // namespace

// ---- packed typed columns as input (pack.h, unpack.hip) --------------------------------------
// The way back in: a clg_packed is checked and unpacked on the device.  The check's verdict is
// read by the host after a sync, before the write pass is queued, so invalid input writes nothing.
namespace {

// Device addresses of a packed input that passed the host's layout check: device and registered
// memory in place, host memory (and registered memory not wholly inside one range) staged.
int unpack_input(clg_engine* e, const clg_packed* in, clg::UnpackIn* uin) {
  const uint64_t nb = in->blk_base[clg::kPackStreams], nbits = in->n_bits;
  if (nb >> 31) return fail(CLG_E_INVALID_ARG, "%llu blocks in one call", (unsigned long long)nb);
  CHK(pack_out_check(clg::pack_view(*in), "the packed input's "));
  const PlaceSpec ins[2] = {{in->desc, nb * sizeof(clg_pack_block), 8}, {in->bits, nbits, 16}};
  clg::Placement pl;
  CHK(place_in(e, e->d_unpackin, ins, 2, in->out_kind, PlacePolicy::stage_if_unresolved, "packed input", &pl));
  uin->desc = pl.at<const clg_pack_block>(0), uin->bits = pl.at<const uint8_t>(1), uin->n_bits = nbits;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) uin->n[c] = in->n_val[c];
  for (uint32_t c = 0; c <= clg::kPackStreams; ++c) uin->blk_base[c] = in->blk_base[c];
  return CLG_OK;
}

// The check pass and the host's reading of its verdict: CLG_E_INVALID_ARG with `bad` filled, or
// CLG_OK with the stream idle and nothing written anywhere yet.
// In two halves, so that a combined call reads the narrow and the wide verdicts after one sync:
// the check queued with the verdict's copy to pinned memory, then (after a sync) its reading.
int unpack_check_queue(clg_engine* e, const clg::UnpackIn& uin) {
  const uint64_t nb = uin.blk_base[clg::kPackStreams];
  if (!nb) return CLG_OK;
  CHK(e->d_unpackres.ensure(sizeof(clg::UnpackVerdict)));
  CHK(e->h_unpackres.ensure(sizeof(clg::UnpackVerdict)));
  // (bytes: a descriptor a block; payloads are read only where the type does not hold the range)
  CHK(e->timed("unpack_columns", nb * sizeof(clg_pack_block),
               [&] { return clg::launch_unpack_check(uin, uint32_t(nb), e->d_unpackres.as<clg::UnpackVerdict>(), e->stream); }));
  HIPCHK(hipMemcpyAsync(e->h_unpackres.p, e->d_unpackres.p, sizeof(clg::UnpackVerdict), hipMemcpyDeviceToHost, e->stream));
  return CLG_OK;
}
int unpack_check_read(clg_engine* e, const clg::UnpackIn& uin, clg_unpack_bad* bad) {
  if (!uin.blk_base[clg::kPackStreams]) return CLG_OK;
  const clg::UnpackVerdict* res = e->h_unpackres.as<clg::UnpackVerdict>();
  const bool block = res->bad_block != 0;
  if (!block && !res->bad_value) return CLG_OK;
  const uint64_t blk = ~uint64_t(block ? res->bad_block : res->bad_value);
  uint32_t c = 0;
  while (c + 1 < clg::kPackStreams && blk >= uin.blk_base[c + 1]) ++c;
  clg::pack_bad_set(bad, block ? CLG_UNPACK_BAD_BLOCK : CLG_UNPACK_BAD_VALUE, c, blk - uin.blk_base[c]);
  return fail(CLG_E_INVALID_ARG, "unpack columns: %s (stream %u, block %llu)",
              block ? "malformed block descriptor" : "a value outside the stream's type", c,
              (unsigned long long)(blk - uin.blk_base[c]));
}
int unpack_check(clg_engine* e, const clg::UnpackIn& uin, clg_unpack_bad* bad) {
  if (!uin.blk_base[clg::kPackStreams]) return CLG_OK;
  CHK(unpack_check_queue(e, uin));
  CHK(e->sync());
  return unpack_check_read(e, uin, bad);
}

int unpack_write(clg_engine* e, const clg::UnpackIn& uin, const clg::UnpackOut& uout) {
  const uint64_t nb = uin.blk_base[clg::kPackStreams];
  uint64_t out_bytes = 0;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) out_bytes += uin.n[c] * clg::pack_stream_bytes(c);
  // (bytes: the descriptors again, the payloads, the plain columns once)
  return e->timed("unpack_columns", nb * sizeof(clg_pack_block) + uin.n_bits + out_bytes,
                  [&] { return clg::launch_unpack_write(uin, uout, uint32_t(nb), e->stream); });
}

// `narrow` unpacked into engine scratch for the encode: the layout and `rest`'s totals on the
// host, the check, then the write queued on the engine's stream (the encode's kernels follow it
// there).  col[5]: the plain columns' device addresses.
// unpack_for_encode up to the check: the host's checks, the input placed and the scratch columns
// laid out.  The packed-wide calls queue the wide rows' check behind the narrow one themselves.
int unpack_for_encode_begin(clg_engine* e, const clg_packed* narrow, const clg_columns_in* rest, clg_unpack_bad* bad,
                            const void* col[clg::kPackStreams], clg::UnpackIn* uin_out, clg::UnpackOut* uout_out) {
  clg::pack_bad_reset(bad);
  if (rest->tag || rest->order || rest->timestamp || rest->rng || rest->buffer_built)
    return fail(CLG_E_INVALID_ARG, "the narrow column pointers of `rest` must be NULL: those columns are given packed");
  uint32_t stream;
  if (!clg::pack_layout_in_ok(clg::pack_view(*narrow), &stream)) {
    clg::pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, stream, 0);
    return fail(CLG_E_INVALID_ARG, "unpack columns: blk_base, n_val, the capacities and the pointers disagree (stream %u)", stream);
  }
  const uint64_t want[clg::kPackStreams] = {rest->n_rec, rest->n_class[0], rest->n_class[1], rest->n_class[2], rest->n_class[3]};
  for (uint32_t c = 0; c < clg::kPackStreams; ++c)
    if (want[c] != narrow->n_val[c]) {
      clg::pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, c, 0);
      return fail(CLG_E_INVALID_ARG, "stream %u holds %llu values, `rest` says %llu", c, (unsigned long long)narrow->n_val[c],
                  (unsigned long long)want[c]);
    }
  clg::UnpackIn& uin = *uin_out;
  uin = clg::UnpackIn{};
  CHK(unpack_input(e, narrow, &uin));
  uint64_t cb[clg::kPackStreams];
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) cb[c] = narrow->n_val[c] * clg::pack_stream_bytes(c);
  size_t at[clg::kPackStreams + 1];
  CHK(e->d_unpackcol.ensure(clg::place_layout(cb, clg::kPackStreams, at) + 16));
  *uout_out = clg::UnpackOut{};
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) col[c] = uout_out->col[c] = e->d_unpackcol.as<uint8_t>() + at[c];
  return CLG_OK;
}
int unpack_for_encode(clg_engine* e, const clg_packed* narrow, const clg_columns_in* rest, clg_unpack_bad* bad,
                      const void* col[clg::kPackStreams]) {
  clg::UnpackIn uin;
  clg::UnpackOut uout;
  CHK(unpack_for_encode_begin(e, narrow, rest, bad, col, &uin, &uout));
  CHK(unpack_check(e, uin, bad));
  return unpack_write(e, uin, uout);
}

// `rest` with the scratch columns in place of its null narrow pointers (ecol_args_ok wants them).
clg_columns_in with_narrow(const clg_columns_in& rest, const void* const col[clg::kPackStreams]) {
  clg_columns_in full = rest;
  full.tag = static_cast<const uint8_t*>(col[0]), full.order = static_cast<const int8_t*>(col[1]);
  full.timestamp = static_cast<const int64_t*>(col[2]), full.rng = static_cast<const int32_t*>(col[3]);
  full.buffer_built = static_cast<const int32_t*>(col[4]);
  return full;
}

EcolDev ecol_dev_narrow(const void* const col[clg::kPackStreams]) {
  EcolDev dev;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) dev.col[c] = col[c];
  dev.n = int(clg::kPackStreams);
  return dev;
}

}  // namespace

extern "C" {

int clg_unpack_columns(clg_engine* e, const clg_packed* in, clg_columns* out, clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  bool done;
  const char* what = "";
  const int st = clg::pack_unpack_begin(in, out, bad, &done, &what);
  if (st != CLG_OK) return fail(st, "unpack columns: %s", what);
  if (done) return CLG_OK;
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  const clg::UnpackDst dst = clg::unpack_dst(*out);
  PlaceSpec outs[clg::kPackStreams];
  for (uint32_t c = 0; c < clg::kPackStreams; ++c)
    outs[c] = {dst.col[c], in->n_val[c] * clg::pack_stream_bytes(c), clg::pack_stream_bytes(c)};
  clg::Placement pl;
  CHK(place_out(e->d_unpackout, outs, clg::kPackStreams, out->out_kind, PlacePolicy::stage_if_unresolved, "column", &pl));
  clg::UnpackIn uin{};
  CHK(unpack_input(e, in, &uin));
  clg::UnpackOut uout{};
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) uout.col[c] = pl.at<void>(c);
  CHK(unpack_check(e, uin, bad));
  CHK(unpack_write(e, uin, uout));
  CHK(stage_out(e, outs, clg::kPackStreams, pl));
  return e->sync();
}

int clg_unpack_columns_all_host(const clg_packed* in, clg_columns* out, clg_unpack_bad* bad) {
  const char* what = "";
  const int st = clg::pack_unpack_all_host(in, out, bad, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "unpack columns: %s", what);
}

int clg_encode_columns_packed(clg_engine* e, const clg_packed* narrow, const clg_columns_in* rest, clg_encoded* out,
                              clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  if (!narrow || !rest || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  clg::ecol_reset_result(out);
  const void* col[clg::kPackStreams];
  CHK(unpack_for_encode(e, narrow, rest, bad, col));
  const clg_columns_in full = with_narrow(*rest, col);
  const EcolDev dev = ecol_dev_narrow(col);
  return encode_columns_checked(e, &full, out, &dev);
}

int clg_append_columns_packed(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans,
                              const clg_packed* narrow, const clg_columns_in* rest, uint64_t* span_bytes, int32_t* status,
                              clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  if (!narrow || !rest || !log || !epoch || !status) return fail(CLG_E_INVALID_ARG, "null argument");
  const uint32_t ns = clg::ecol_spans(*rest);
  if (n_spans != ns) return fail(CLG_E_INVALID_ARG, "%u logs for %u spans", n_spans, ns);
  for (uint32_t s = 0; s < ns; ++s) status[s] = CLG_OK;
  const void* col[clg::kPackStreams];
  CHK(unpack_for_encode(e, narrow, rest, bad, col));
  const clg_columns_in full = with_narrow(*rest, col);
  const EcolDev dev = ecol_dev_narrow(col);
  return append_columns_checked(e, log, epoch, &full, span_bytes, status, &dev);
}

}  // extern "C"

// ---- packed wide rows as input (pack_wide.h, unpack_wide.hip) ---------------------------------
// The way back in for the wide rows: check, kind and scan, the host's reading of the verdict and
// the histogram after one sync, then write, merge and (where wanted) pos.  Invalid input writes
// nothing outside engine scratch.
namespace {

// What a checked clg_packed_wide's unpack works with between its two halves.
struct WUnpackPlan {
  uint64_t nw = 0, nb = 0;
  uint32_t nt = 0;
  uint32_t* d_cnt = nullptr;
  uint64_t *d_base = nullptr, *d_tsum = nullptr;
  clg::WUnpackVerdict* d_verdict = nullptr;
  clg::WUnpackTab* tab = nullptr;  // pinned: the host's copy
};

// A packed input that passed the host's layout check, with rows: the input placed (device and
// registered memory in place, host memory staged), the scratch laid out and the stream table
// uploaded.  d_idx: where w_idx goes.
int wunpack_begin(clg_engine* e, const clg_packed_wide* in, void* d_idx, WUnpackPlan* p) {
  const uint64_t nw = in->n_val[CLG_WPACK_KIND], nb = in->blk_base[clg::kWPackStreams];
  if (nw >> 32) return fail(CLG_E_INVALID_ARG, "%llu wide rows in one call", (unsigned long long)nw);
  if (nb >> 31) return fail(CLG_E_INVALID_ARG, "%llu blocks in one call", (unsigned long long)nb);
  CHK(pack_out_check(clg::pack_view(*in), "the packed input's "));
  const PlaceSpec ins[2] = {{in->desc, nb * sizeof(clg_pack_block), 8}, {in->bits, in->n_bits, 16}};
  clg::Placement pl;
  CHK(place_in(e, e->d_wunpackin, ins, 2, in->out_kind, PlacePolicy::stage_if_unresolved, "packed input", &pl));
  p->nw = nw, p->nb = nb, p->nt = uint32_t(clg::pack_blocks_of(nw));
  const uint64_t nt = p->nt;
  const uint64_t wb[5] = {nw, nt * clg::kWPackKinds * 4, nt * clg::kWPackKinds * 8, nt * 8, sizeof(clg::WUnpackVerdict)};
  size_t wo[6];
  CHK(e->d_wunpackwork.ensure(clg::place_layout(wb, 5, wo) + 16));
  uint8_t* wk = e->d_wunpackwork.as<uint8_t>();
  p->d_cnt = reinterpret_cast<uint32_t*>(wk + wo[1]);
  p->d_base = reinterpret_cast<uint64_t*>(wk + wo[2]);
  p->d_tsum = reinterpret_cast<uint64_t*>(wk + wo[3]);
  p->d_verdict = reinterpret_cast<clg::WUnpackVerdict*>(wk + wo[4]);
  constexpr int kArrays = int(clg::kWPackKinds * clg::kWPackFields);
  uint64_t cb[kArrays];
  size_t so[kArrays + 1];
  for (uint32_t t = 0; t < clg::kWPackKinds; ++t)
    for (uint32_t f = 0; f < clg::kWPackFields; ++f)
      cb[t * clg::kWPackFields + f] = in->n_val[clg::wpack_stream(t, f)] * clg::pack_elem_bytes(clg::kWPackField[f].elem);
  CHK(e->d_wunpacksoa.ensure(clg::place_layout(cb, kArrays, so) + 16));
  CHK(e->h_wunpacktab.ensure(sizeof(clg::WUnpackTab)));
  CHK(e->d_wunpacktab.ensure(sizeof(clg::WUnpackTab)));
  CHK(e->h_wunpackres.ensure(sizeof(clg::WUnpackRes) + sizeof(clg::WUnpackVerdict)));
  clg::WUnpackTab* tab = p->tab = e->h_wunpacktab.as<clg::WUnpackTab>();
  tab->desc = pl.at<const clg_pack_block>(0), tab->bits = pl.at<const uint8_t>(1), tab->n_bits = in->n_bits;
  for (uint32_t c = 0; c < clg::kWPackStreams; ++c) tab->n[c] = in->n_val[c];
  for (uint32_t c = 0; c <= clg::kWPackStreams; ++c) tab->blk_base[c] = in->blk_base[c];
  tab->col[CLG_WPACK_KIND] = wk + wo[0], tab->col[CLG_WPACK_IDX] = d_idx;
  for (int i = 0; i < kArrays; ++i) tab->col[2 + i] = e->d_wunpacksoa.as<uint8_t>() + so[i];
  HIPCHK(hipMemcpyAsync(e->d_wunpacktab.p, tab, sizeof(clg::WUnpackTab), hipMemcpyHostToDevice, e->stream));
  return CLG_OK;
}

// The check passes queued, with the verdict's copy to pinned memory (the totals are written there
// by the scan).
int wunpack_check_queue(clg_engine* e, const WUnpackPlan& p) {
  clg::WUnpackRes* res = e->h_wunpackres.as<clg::WUnpackRes>();
  // (bytes: a descriptor a block, twice for KIND's; KIND's payload is below a byte a row, its
  // plain byte written; the tile counts written, read and their bases written)
  CHK(e->timed("unpack_wide", p.nb * sizeof(clg_pack_block) + p.nw * 2 + uint64_t(p.nt) * 96, [&] {
    return clg::launch_wunpack_check(e->d_wunpacktab.as<clg::WUnpackTab>(), uint32_t(p.nb), p.nt, p.d_cnt, p.d_base, p.d_verdict,
                                     res, e->stream);
  }));
  HIPCHK(hipMemcpyAsync(res + 1, p.d_verdict, sizeof(clg::WUnpackVerdict), hipMemcpyDeviceToHost, e->stream));
  return CLG_OK;
}

// After the sync: BLOCK, then VALUE, then the histogram, in clg_unpack_wide_host's order.
// offset: added to the stream reported (the combined calls: kWPackBadStream).
int wunpack_check_read(clg_engine* e, const WUnpackPlan& p, clg_unpack_bad* bad, uint32_t offset) {
  const clg::WUnpackRes* res = e->h_wunpackres.as<clg::WUnpackRes>();
  const clg::WUnpackVerdict* v = reinterpret_cast<const clg::WUnpackVerdict*>(res + 1);
  const auto found = [&](uint32_t what, uint64_t blk, const char* text) {
    uint32_t c = 0;
    while (c + 1 < clg::kWPackStreams && blk >= p.tab->blk_base[c + 1]) ++c;
    clg::pack_bad_set(bad, what, offset + c, blk - p.tab->blk_base[c]);
    return fail(CLG_E_INVALID_ARG, "unpack wide rows: %s (stream %u, block %llu)", text, c,
                (unsigned long long)(blk - p.tab->blk_base[c]));
  };
  if (v->bad_block) return found(CLG_UNPACK_BAD_BLOCK, ~uint64_t(v->bad_block), "malformed block descriptor");
  const uint64_t vblk = ~uint64_t(v->bad_value);
  if (v->bad_value && vblk < p.tab->blk_base[1]) return found(CLG_UNPACK_BAD_VALUE, vblk, "a KIND above 3");
  for (uint32_t t = 0; t < clg::kWPackKinds; ++t)
    if (res->tot[t] != p.tab->n[clg::wpack_stream(t, 0)]) {
      clg::pack_bad_set(bad, CLG_UNPACK_BAD_VALUE, offset, 0);
      return fail(CLG_E_INVALID_ARG, "unpack wide rows: the kinds' counts differ from the streams' lengths");
    }
  if (v->bad_value) return found(CLG_UNPACK_BAD_VALUE, vblk, "a value outside the stream's type");
  return CLG_OK;
}

// Write, merge and pos queued.  dst: the rows' device addresses; pos: null when not wanted.
int wunpack_write_queue(clg_engine* e, const WUnpackPlan& p, const clg::WUnpackDst& dst, uint64_t* pos, uint64_t n_bits) {
  // (bytes: the descriptors and payloads of streams 1 .. 25, their 37 B a row written and read
  // again with the kind byte, 37 B a row written in row order; pos: the lengths read, 8 B written)
  return e->timed("unpack_wide", p.nb * sizeof(clg_pack_block) + n_bits + p.nw * (37 + 38 + 37 + (pos ? 12 : 0)), [&] {
    return clg::launch_wunpack_write(e->d_wunpacktab.as<clg::WUnpackTab>(), uint32_t(p.nb), p.nt, p.nt, p.d_base, dst, p.nw,
                                     p.d_tsum, pos, p.d_verdict, e->stream);
  });
}

// Both packed forms unpacked into engine scratch for the encode.  full: `rest` with the scratch
// arrays in place of its null pointers; dev: their addresses for ecol_sizes, with the cross rule's
// word.  The checks' order is wpack_unpack_both_host's.
int unpack_both_for_encode(clg_engine* e, const clg_packed* narrow, const clg_packed_wide* wide, const clg_columns_in* rest,
                           clg_unpack_bad* bad, clg_columns_in* full, EcolDev* dev) {
  clg::pack_bad_reset(bad);
  if (!clg::wpack_rest_ok(*rest))
    return fail(CLG_E_INVALID_ARG, "the column pointers of `rest` that the packed forms give must be NULL");
  const char* what = "";
  if (const int st = clg::wpack_both_layout(*narrow, *wide, *rest, bad, &what)) return fail(st, "unpack columns: %s", what);
  const void* col[clg::kPackStreams];
  clg::UnpackIn uin;
  clg::UnpackOut uout;
  CHK(unpack_for_encode_begin(e, narrow, rest, bad, col, &uin, &uout));
  *full = with_narrow(*rest, col);
  *dev = ecol_dev_narrow(col);
  const uint64_t nw = rest->n_class[4];
  if (!nw) {  // no rows: nothing of the wide form is launched or waited for
    CHK(unpack_check(e, uin, bad));
    return unpack_write(e, uin, uout);
  }
  // the rows in EcolIn's order behind the narrow columns: w_rc, w_v1, w_var_len, w_sub, w_v0, w_idx, pos
  const uint64_t rb[7] = {nw * 4, nw * 8, nw * 4, nw, nw * 8, nw * 4, (nw + 1) * 8};
  size_t ro[8];
  CHK(e->d_wunpackrow.ensure(clg::place_layout(rb, 7, ro) + 16));
  uint8_t* rw = e->d_wunpackrow.as<uint8_t>();
  for (int i = 0; i < 7; ++i) dev->col[5 + i] = rw + ro[i];
  dev->n = 12;
  WUnpackPlan p;
  CHK(wunpack_begin(e, wide, rw + ro[5], &p));
  CHK(unpack_check_queue(e, uin));
  CHK(wunpack_check_queue(e, p));
  CHK(e->sync());
  CHK(unpack_check_read(e, uin, bad));
  CHK(wunpack_check_read(e, p, bad, clg::kWPackBadStream));
  CHK(unpack_write(e, uin, uout));
  // (w_var_off is checked like every stream but not put back in row order: the encode does not read it)
  const clg::WUnpackDst dst{{rw + ro[0], rw + ro[1], nullptr, rw + ro[2], rw + ro[3], rw + ro[4]},
                            static_cast<const uint8_t*>(col[0]), rest->n_rec};
  CHK(wunpack_write_queue(e, p, dst, reinterpret_cast<uint64_t*>(rw + ro[6]), wide->n_bits));
  unsigned long long* cross = &reinterpret_cast<clg::WUnpackVerdict*>(e->h_wunpackres.as<clg::WUnpackRes>() + 1)->cross_row;
  HIPCHK(hipMemcpyAsync(cross, &p.d_verdict->cross_row, sizeof *cross, hipMemcpyDeviceToHost, e->stream));
  dev->cross = cross, dev->bad = bad;
  full->w_rc = reinterpret_cast<const int32_t*>(dev->col[5]), full->w_v1 = reinterpret_cast<const int64_t*>(dev->col[6]);
  full->w_var_len = reinterpret_cast<const uint32_t*>(dev->col[7]), full->w_sub = reinterpret_cast<const uint8_t*>(dev->col[8]);
  full->w_v0 = reinterpret_cast<const int64_t*>(dev->col[9]), full->w_idx = reinterpret_cast<const uint32_t*>(dev->col[10]);
  full->pos = reinterpret_cast<const uint64_t*>(dev->col[11]);
  return CLG_OK;
}

}  // namespace

extern "C" {

int clg_unpack_wide(clg_engine* e, const clg_packed_wide* in, clg_columns* out, uint64_t* pos, clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  clg::pack_bad_reset(bad);
  if (!in || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  uint32_t stream;
  if (!clg::wpack_layout_in_ok(*in, &stream)) {
    clg::pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, stream, 0);
    return fail(CLG_E_INVALID_ARG, "unpack wide rows: blk_base, n_val, the capacities and the pointers disagree (stream %u)", stream);
  }
  const uint64_t nw = in->n_val[CLG_WPACK_KIND];
  out->n_class[4] = nw;
  const clg::WPackCols cols = clg::wpack_cols(*out);
  bool any = out->w_idx != nullptr || pos != nullptr, all = out->w_idx != nullptr;
  for (uint32_t f = 0; f < clg::kWPackFields; ++f) any = any || cols.col[f], all = all && cols.col[f];
  if (!any) return CLG_OK;  // sizes only
  if ((!all && nw) || out->cap_wide < nw) return fail(CLG_E_CAPACITY, "unpack wide rows: the wide rows' arrays are too small");
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  if (!nw) {  // no rows: nothing is launched, and only a device pos is waited for
    if (!pos) return CLG_OK;
    if (out->out_kind != CLG_MEM_DEVICE) return pos[0] = 0, CLG_OK;
    HIPCHK(hipMemsetAsync(pos, 0, 8, e->stream));
    return e->sync();
  }
  // the outputs: w_idx, the six fields in kWPackField's order, pos
  PlaceSpec outs[8] = {{out->w_idx, nw * 4, 4}};
  for (uint32_t f = 0; f < clg::kWPackFields; ++f) {
    const uint32_t eb = clg::pack_elem_bytes(clg::kWPackField[f].elem);
    outs[1 + f] = {cols.col[f], nw * eb, eb};
  }
  outs[7] = {pos, (nw + 1) * 8, 8};
  clg::Placement pl;
  CHK(place_out(e->d_wunpackout, outs, 8, out->out_kind, PlacePolicy::stage_if_unresolved, "wide", &pl));
  WUnpackPlan p;
  CHK(wunpack_begin(e, in, pl.at<void>(0), &p));
  CHK(wunpack_check_queue(e, p));
  CHK(e->sync());
  CHK(wunpack_check_read(e, p, bad, 0));
  clg::WUnpackDst dst{};
  for (uint32_t f = 0; f < clg::kWPackFields; ++f) dst.col[f] = pl.at<void>(1 + int(f));
  CHK(wunpack_write_queue(e, p, dst, pl.at<uint64_t>(7), in->n_bits));
  CHK(stage_out(e, outs, 8, pl));
  return e->sync();
}

int clg_encode_columns_packed_wide(clg_engine* e, const clg_packed* narrow, const clg_packed_wide* wide,
                                   const clg_columns_in* rest, clg_encoded* out, clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  if (!narrow || !wide || !rest || !out) return fail(CLG_E_INVALID_ARG, "null argument");
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  clg::ecol_reset_result(out);
  clg_columns_in full;
  EcolDev dev;
  CHK(unpack_both_for_encode(e, narrow, wide, rest, bad, &full, &dev));
  return encode_columns_checked(e, &full, out, &dev);
}

int clg_append_columns_packed_wide(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans,
                                   const clg_packed* narrow, const clg_packed_wide* wide, const clg_columns_in* rest,
                                   uint64_t* span_bytes, int32_t* status, clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  if (!narrow || !wide || !rest || !log || !epoch || !status) return fail(CLG_E_INVALID_ARG, "null argument");
  const uint32_t ns = clg::ecol_spans(*rest);
  if (n_spans != ns) return fail(CLG_E_INVALID_ARG, "%u logs for %u spans", n_spans, ns);
  for (uint32_t s = 0; s < ns; ++s) status[s] = CLG_OK;
  clg_columns_in full;
  EcolDev dev;
  CHK(unpack_both_for_encode(e, narrow, wide, rest, bad, &full, &dev));
  return append_columns_checked(e, log, epoch, &full, span_bytes, status, &dev);
}

int clg_encode_columns_packed_wide_host(const clg_packed* narrow, const clg_packed_wide* wide, const clg_columns_in* rest,
                                        clg_encoded* out, clg_unpack_bad* bad) {
  if (!out) return fail(CLG_E_INVALID_ARG, "null argument");
  clg::ecol_reset_result(out);
  clg::WPackBothHost h;
  clg_columns_in full;
  const char* what = "";
  int st = clg::wpack_unpack_both_host(narrow, wide, rest, bad, &h, &full, &what);
  if (st != CLG_OK) return fail(st, "unpack columns: %s", what);
  st = clg::ecol_build_host(&full, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "encode columns: %s", what);
}

}  // extern "C"
