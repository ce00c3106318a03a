// engine_encode_columns.cpp -- the typed-columns family, columns -> log bytes: the encode of typed
// columns and their append to logs (encode_columns.h), and the way back in of the two packed forms,
// which the packed encodes and appends unpack into engine scratch first; clg_encode_columns*,
// clg_append_columns*, clg_unpack_columns* and clg_unpack_wide*.  The unpacks sit with the encode
// because the packed encodes queue the unpack's kernels and the encode's on one stream and read the
// verdicts of both after one sync.
#include "engine_columns.h"
#include "columns.h"
#include "encode_columns.h"
#include "pack_wide.h"

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

// The packed calls: device addresses of the leading n arrays of kEcolArray (kEcolNarrowArrays: the
// narrow columns; kEcolPackedArrays: the wide rows, w_idx and pos as well), used as they are whatever
// in_kind says of the other arrays.  cross (the packed-wide calls): the cross rule's word in pinned memory, filled
// by a copy queued before the sizes; it is read after their sync and before the encode's own checks.
struct EcolDev {
  const void* col[clg::kEcolPackedArrays] = {};
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
  // the arrays (kEcolArray): bytes, and element sizes for the alignment check
  constexpr int kArrays = clg::kEcolArrays;
  PlaceSpec ins[kArrays];
  for (int i = 0; i < kArrays; ++i) ins[i] = {clg::ecol_in_ptr(*in, i), clg::ecol_array_bytes(*in, i), clg::kEcolArray[i].width};
  for (const PlaceSpec& a : ins) p->in_bytes += a.p ? a.bytes : 0;
  // registered arrays must be registered whole; host arrays are staged, an empty one too (a valid
  // address, never read).  With dev its arrays take no part (no slot, no lookup, no copy): they
  // are absent from the placement, and their addresses are set behind it.
  for (int i = 0; dev && i < dev->n; ++i) ins[i].p = nullptr;
  const size_t sb_bytes = in->n_spans ? size_t(ns + 1) * clg::kColClasses * 8 : 0;
  clg::Placement pl;
  CHK(place_in(e, e->d_ecolin, ins, kArrays, in->in_kind, PlacePolicy::reject_unresolved, "encode columns: input", &pl, sb_bytes));
  for (int i = 0; dev && i < dev->n; ++i) pl.dev[i] = uintptr_t(dev->col[i]);
  const size_t o_sb = pl.staged() ? pl.total : 0;  // the span bases lie behind the staged arrays
  if (!pl.staged()) CHK(e->d_ecolin.ensure(sb_bytes + 16));
  uint8_t* din = e->d_ecolin.as<uint8_t>();
  clg::EcolIn& d = p->d;  // (typed, so written out: the members in kEcolArray's order, which is EcolIn's)
#define CLG_SAME(m) offsetof(clg::EcolIn, m) == offsetof(clg_columns_in, m)
  static_assert(kArrays == 13 && offsetof(clg::EcolIn, n) == 13 * sizeof(void*) && CLG_SAME(tag) && CLG_SAME(order) && CLG_SAME(timestamp) &&
                    CLG_SAME(rng) && CLG_SAME(buffer_built) && CLG_SAME(w_rc) && CLG_SAME(w_v1) && CLG_SAME(w_var_len) && CLG_SAME(w_sub) &&
                    CLG_SAME(w_v0) && CLG_SAME(w_idx) && CLG_SAME(pos) && CLG_SAME(var),
                "EcolIn's arrays are clg_columns_in's, in its order: kEcolArray's");
#undef CLG_SAME
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
  clg::Carve<5> wk;
  CHK(carve(e->d_ecolw, wb, &wk));
  uint32_t* d_counts = wk.at<uint32_t>(0);
  uint64_t *d_base = wk.at<uint64_t>(1), *d_sum = wk.at<uint64_t>(2), *d_bad = wk.at<uint64_t>(3), *d_bbase = wk.at<uint64_t>(4);
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

// The argument checks of the clg_append_columns* calls.  given: no pointer the call needs is null.
int append_args_check(bool given, const clg_columns_in* in, uint32_t n_spans, int32_t* status) {
  if (!given) return fail(CLG_E_INVALID_ARG, "null argument");
  const uint32_t ns = clg::ecol_spans(*in);
  if (n_spans != ns) return fail(CLG_E_INVALID_ARG, "%u logs for %u spans", n_spans, ns);
  for (uint32_t s = 0; s < ns; ++s) status[s] = CLG_OK;
  return CLG_OK;
}
// Those of the packed encodes, and out's results reset.
int encode_packed_args_check(bool given, clg_encoded* out) {
  if (!given) return fail(CLG_E_INVALID_ARG, "null argument");
  if (!mem_kind_ok(out->out_kind)) return fail(CLG_E_INVALID_ARG, "out_kind %u", out->out_kind);
  clg::ecol_reset_result(out);
  return CLG_OK;
}

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

// ---- packed typed columns as input (pack.h, unpack.hip) --------------------------------------
// The way back in: a clg_packed is checked and unpacked on the device.  The check's verdict is
// read by the host after a sync, before the write pass is queued, so invalid input writes nothing.

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
  const uint32_t c = clg::pack_stream_of_block(uin.blk_base, clg::kPackStreams, blk);
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
  clg::Carve<int(clg::kPackStreams)> at;
  CHK(carve(e->d_unpackcol, cb, &at));
  *uout_out = clg::UnpackOut{};
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) col[c] = uout_out->col[c] = at.at<uint8_t>(int(c));
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
  static_assert(clg::kEcolNarrowArrays == int(clg::kPackStreams), "a clg_packed's streams are kEcolArray's leading arrays");
  clg_columns_in full = rest;
  for (int i = 0; i < clg::kEcolNarrowArrays; ++i) clg::ecol_in_set(&full, i, col[i]);
  return full;
}

EcolDev ecol_dev_narrow(const void* const col[clg::kPackStreams]) {
  EcolDev dev;
  for (uint32_t c = 0; c < clg::kPackStreams; ++c) dev.col[c] = col[c];
  dev.n = int(clg::kPackStreams);
  return dev;
}

// ---- packed wide rows as input (pack_wide.h, unpack_wide.hip) ---------------------------------
// The way back in for the wide rows: check, kind and scan, the host's reading of the verdict and
// the histogram after one sync, then write, merge and (where wanted) pos.  Invalid input writes
// nothing outside engine scratch.

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
  clg::Carve<5> wk;  // the kind bytes | tile counts | tile bases | tile sums | the verdict
  CHK(carve(e->d_wunpackwork, wb, &wk));
  p->d_cnt = wk.at<uint32_t>(1), p->d_base = wk.at<uint64_t>(2), p->d_tsum = wk.at<uint64_t>(3);
  p->d_verdict = wk.at<clg::WUnpackVerdict>(4);
  constexpr int kArrays = int(clg::kWPackKinds * clg::kWPackFields);
  uint64_t cb[kArrays];
  clg::Carve<kArrays> so;
  for (uint32_t t = 0; t < clg::kWPackKinds; ++t)
    for (uint32_t f = 0; f < clg::kWPackFields; ++f)
      cb[t * clg::kWPackFields + f] = in->n_val[clg::wpack_stream(t, f)] * clg::pack_elem_bytes(clg::kWPackField[f].elem);
  CHK(carve(e->d_wunpacksoa, cb, &so));
  CHK(e->h_wunpacktab.ensure(sizeof(clg::WUnpackTab)));
  CHK(e->d_wunpacktab.ensure(sizeof(clg::WUnpackTab)));
  CHK(e->h_wunpackres.ensure(sizeof(clg::WUnpackRes) + sizeof(clg::WUnpackVerdict)));
  clg::WUnpackTab* tab = p->tab = e->h_wunpacktab.as<clg::WUnpackTab>();
  tab->desc = pl.at<const clg_pack_block>(0), tab->bits = pl.at<const uint8_t>(1), tab->n_bits = in->n_bits;
  for (uint32_t c = 0; c < clg::kWPackStreams; ++c) tab->n[c] = in->n_val[c];
  for (uint32_t c = 0; c <= clg::kWPackStreams; ++c) tab->blk_base[c] = in->blk_base[c];
  tab->col[CLG_WPACK_KIND] = wk.at<uint8_t>(0), tab->col[CLG_WPACK_IDX] = d_idx;
  for (int i = 0; i < kArrays; ++i) tab->col[2 + i] = so.at<uint8_t>(i);
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
    const uint32_t c = clg::pack_stream_of_block(p.tab->blk_base, clg::kWPackStreams, blk);
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
  // the rows behind the narrow columns, as kEcolArray has them: w_rc, w_v1, w_var_len, w_sub, w_v0, w_idx, pos
  constexpr int k0 = clg::kEcolNarrowArrays, kRows = clg::kEcolPackedArrays - k0;
  uint64_t rb[kRows];
  for (int i = 0; i < kRows; ++i) rb[i] = clg::ecol_array_bytes(*rest, k0 + i);
  clg::Carve<kRows> rw;
  CHK(carve(e->d_wunpackrow, rb, &rw));
  for (int i = 0; i < kRows; ++i) clg::ecol_in_set(full, k0 + i, dev->col[k0 + i] = rw.at<uint8_t>(i));
  dev->n = clg::kEcolPackedArrays;
  const auto row = [](const void* p) { return const_cast<void*>(p); };  // (scratch, which clg_columns_in types const)
  WUnpackPlan p;
  CHK(wunpack_begin(e, wide, row(full->w_idx), &p));
  CHK(unpack_check_queue(e, uin));
  CHK(wunpack_check_queue(e, p));
  CHK(e->sync());
  CHK(unpack_check_read(e, uin, bad));
  CHK(wunpack_check_read(e, p, bad, clg::kWPackBadStream));
  CHK(unpack_write(e, uin, uout));
  // (w_var_off is checked like every stream but not put back in row order: the encode does not read it)
  const clg::WUnpackDst dst{{row(full->w_rc), row(full->w_v1), nullptr, row(full->w_var_len), row(full->w_sub), row(full->w_v0)},
                            full->tag, rest->n_rec};
  CHK(wunpack_write_queue(e, p, dst, const_cast<uint64_t*>(full->pos), wide->n_bits));
  unsigned long long* cross = &reinterpret_cast<clg::WUnpackVerdict*>(e->h_wunpackres.as<clg::WUnpackRes>() + 1)->cross_row;
  HIPCHK(hipMemcpyAsync(cross, &p.d_verdict->cross_row, sizeof *cross, hipMemcpyDeviceToHost, e->stream));
  dev->cross = cross, dev->bad = bad;
  return CLG_OK;
}

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
  CHK(append_args_check(in && log && epoch && status, in, n_spans, status));
  return append_columns_checked(e, log, epoch, in, span_bytes, status, nullptr);
}

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

int clg_unpack_columns_host(const clg_packed* in, uint32_t stream, uint64_t first, uint64_t count, void* out) {
  const char* what = "";
  const int st = clg::pack_unpack_host(in, stream, first, count, out, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "unpack columns: %s", what);
}

int clg_encode_columns_packed(clg_engine* e, const clg_packed* narrow, const clg_columns_in* rest, clg_encoded* out,
                              clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  CHK(encode_packed_args_check(narrow && rest && out, out));
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
  CHK(append_args_check(narrow && rest && log && epoch && status, rest, n_spans, status));
  const void* col[clg::kPackStreams];
  CHK(unpack_for_encode(e, narrow, rest, bad, col));
  const clg_columns_in full = with_narrow(*rest, col);
  const EcolDev dev = ecol_dev_narrow(col);
  return append_columns_checked(e, log, epoch, &full, span_bytes, status, &dev);
}

int clg_unpack_wide_host(const clg_packed_wide* in, clg_columns* out, clg_unpack_bad* bad) {
  const char* what = "";
  const int st = clg::wpack_unpack_host(in, out, bad, &what);
  return st == CLG_OK ? CLG_OK : fail(st, "unpack wide rows: %s", what);
}

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
  CHK(encode_packed_args_check(narrow && wide && rest && out, out));
  clg_columns_in full;
  EcolDev dev;
  CHK(unpack_both_for_encode(e, narrow, wide, rest, bad, &full, &dev));
  return encode_columns_checked(e, &full, out, &dev);
}

int clg_append_columns_packed_wide(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans,
                                   const clg_packed* narrow, const clg_packed_wide* wide, const clg_columns_in* rest,
                                   uint64_t* span_bytes, int32_t* status, clg_unpack_bad* bad) {
  ENGINE_GUARD(e);
  CHK(append_args_check(narrow && wide && rest && log && epoch && status, rest, n_spans, status));
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
