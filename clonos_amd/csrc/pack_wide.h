// pack_wide.h -- packed wide rows: the format's one definition, for the kernels (pack_wide.hip),
// the engine and the CPU version.
//
// A wide row (w_idx, w_rc, w_v1, w_var_off, w_var_len, w_sub, w_v0) belongs to one of four record
// kinds, kind = tag[w_idx] - 3, and one w_* array mixes what the four kinds keep in it: stream
// lengths beside millisecond clocks beside checkpoint ids.  So the rows are partitioned by kind
// first (stable: rank r of kind t is the r-th row of that kind) and every field of every kind is a
// stream of its own; two more streams, the kinds and the w_idx of all rows in row order, let a
// reader put the rows back.  26 streams (kWPackStreams), each cut into blocks of kPackBlock values
// that are packed by pack.h's block codec: residuals, ref, width, payload, padding.
//
//   stream 0 KIND, 1 IDX, then 2 + 6 * kind + field with the fields in kWPackField's order
//
// The element and the scheme of a stream (pack.h's words) are kWPackField's and part of the
// format.  A field a kind never uses is all zeros and costs a width-0 descriptor per block; nothing
// about the values is assumed, so any w_* content round-trips.
//
// Plain C++: compiles under hipcc (host and device) and under g++ without HIP
// (tests/wpack_host.cpp).
#pragma once
#include "pack.h"

namespace clg {

constexpr uint32_t kWPackKinds = CLG_WPACK_KINDS;
constexpr uint32_t kWPackFields = CLG_WPACK_FIELDS;
constexpr uint32_t kWPackStreams = CLG_WPACK_STREAMS;
constexpr uint32_t kWPackFirstTag = 3;  // kind = tag - kWPackFirstTag
static_assert(kWPackStreams == 2 + kWPackKinds * kWPackFields, "KIND, IDX and a stream per (kind, field)");

// The scheme table.  V0 of kind 0 is a stream length (FOR); of kinds 1 - 3 a clock or a checkpoint
// id (DELTA).
struct WPackField {
  uint8_t elem, scheme_kind0, scheme_rest;
};
constexpr WPackField kWPackField[kWPackFields] = {
    {kElemI32, kPackFor, kPackFor},      // RC       w_rc
    {kElemI64, kPackDelta, kPackDelta},  // V1       w_v1
    {kElemU32, kPackDelta, kPackDelta},  // VAR_OFF  w_var_off
    {kElemU32, kPackFor, kPackFor},      // VAR_LEN  w_var_len
    {kElemU8, kPackFor, kPackFor},       // SUB      w_sub
    {kElemI64, kPackFor, kPackDelta},    // V0       w_v0
};
constexpr uint32_t kWPackKindElem = kElemU8, kWPackKindScheme = kPackFor;
constexpr uint32_t kWPackIdxElem = kElemU32, kWPackIdxScheme = kPackDelta;

// The table folded into two words (two bits of element and one of scheme a stream), so that device
// code indexes a constant and not an array.
constexpr uint64_t wpack_fold_elem() {
  uint64_t w = uint64_t(kWPackKindElem) | uint64_t(kWPackIdxElem) << 2;
  for (uint32_t t = 0; t < kWPackKinds; ++t)
    for (uint32_t f = 0; f < kWPackFields; ++f) w |= uint64_t(kWPackField[f].elem) << (2 * (2 + t * kWPackFields + f));
  return w;
}
constexpr uint32_t wpack_fold_scheme() {
  uint32_t w = kWPackKindScheme | kWPackIdxScheme << 1;
  for (uint32_t t = 0; t < kWPackKinds; ++t)
    for (uint32_t f = 0; f < kWPackFields; ++f)
      w |= uint32_t(t ? kWPackField[f].scheme_rest : kWPackField[f].scheme_kind0) << (2 + t * kWPackFields + f);
  return w;
}
constexpr uint64_t kWPackElemBits = wpack_fold_elem();
constexpr uint32_t kWPackSchemeBits = wpack_fold_scheme();

CLG_PACK_HD uint32_t wpack_stream(uint32_t kind, uint32_t field) { return 2 + kind * kWPackFields + field; }
CLG_PACK_HD uint32_t wpack_stream_elem(uint32_t stream) { return uint32_t(kWPackElemBits >> (2 * stream)) & 3u; }
CLG_PACK_HD bool wpack_is_delta(uint32_t stream) { return (kWPackSchemeBits >> stream & 1u) != 0; }

// The row's kind, or kWPackKinds for a row that has none (w_idx past the tags, a narrow tag).
CLG_PACK_HD uint32_t wpack_kind_of(const uint8_t* tag, uint64_t n_rec, uint32_t idx) {
  if (idx >= n_rec) return kWPackKinds;
  const uint32_t kind = uint32_t(tag[idx]) - kWPackFirstTag;
  return kind < kWPackKinds ? kind : kWPackKinds;
}

// The six field arrays of a clg_columns, in kWPackField's order.
struct WPackCols {
  void* col[kWPackFields];
};
inline WPackCols wpack_cols(const clg_columns& c) {
  return WPackCols{{c.w_rc, c.w_v1, c.w_var_off, c.w_var_len, c.w_sub, c.w_v0}};
}

inline void wpack_reset_result(clg_packed_wide* out) {
  for (uint32_t c = 0; c < kWPackStreams; ++c) out->n_val[c] = 0;
  for (uint32_t c = 0; c <= kWPackStreams; ++c) out->blk_base[c] = 0;
  out->n_bits = 0;
  out->bad_row = ~0ull;
}
// The 26 streams' lengths and block bases from the rows and the kinds' totals: n_val[26],
// blk_base[27].  Stated once for the host and for the one-launch form, which lays its table out in LDS.
CLG_PACK_HD void wpack_layout_streams(uint64_t n_wide, const uint64_t tot[kWPackKinds], uint64_t* n_val, uint64_t* blk_base) {
  n_val[CLG_WPACK_KIND] = n_val[CLG_WPACK_IDX] = n_wide;
  for (uint32_t t = 0; t < kWPackKinds; ++t)
    for (uint32_t f = 0; f < kWPackFields; ++f) n_val[wpack_stream(t, f)] = tot[t];
  blk_base[0] = 0;
  for (uint32_t c = 0; c < kWPackStreams; ++c) blk_base[c + 1] = blk_base[c] + pack_blocks(n_val[c]);
}
// n_val and blk_base of `out` from the rows and the kinds' totals.
inline void wpack_layout(uint64_t n_wide, const uint64_t tot[kWPackKinds], clg_packed_wide* out) {
  wpack_layout_streams(n_wide, tot, out->n_val, out->blk_base);
}

// ---- the one-launch form (pack_small.hip) ------------------------------------------------------
// At most kWPackSmallRows rows are packed by one launch of one workgroup (k_pack_small).  The
// floor is the one-launch payload form's largest batch (payload.h kPaySmallRows); the engine
// asserts it.
constexpr uint32_t kWPackSmallRows = 8193;
// The blocks n_wide rows can make, however the kinds share them: KIND and IDX hold
// pack_blocks(n_wide) each, and the four kinds' blocks of one field sum to at most
// (n_wide + 4 * (kPackBlock - 1)) / kPackBlock.
constexpr uint64_t wpack_kind_blocks_bound(uint64_t n_wide) { return (n_wide + kWPackKinds * (kPackBlock - 1)) / kPackBlock; }
constexpr uint64_t wpack_blocks_bound(uint64_t n_wide) {
  return n_wide ? 2 * ((n_wide + kPackBlock - 1) / kPackBlock) + kWPackFields * wpack_kind_blocks_bound(n_wide) : 0;
}
constexpr uint32_t kWPackSmallBlocks = uint32_t(wpack_blocks_bound(kWPackSmallRows));
// The payload bytes n_wide rows can make, however the kinds share them (pack.h's bound per stream;
// a field's bits once for all rows and a block's padding, below 16 bytes, for every block it can have).
inline uint64_t wpack_bits_bound(uint64_t n_wide) {
  if (!n_wide) return 0;
  uint64_t b = pack_bits_bound(kWPackKindElem, kWPackKindScheme != kPackFor, n_wide) +
               pack_bits_bound(kWPackIdxElem, kWPackIdxScheme != kPackFor, n_wide);
  for (uint32_t f = 0; f < kWPackFields; ++f) {
    const bool delta = kWPackField[f].scheme_kind0 != kPackFor || kWPackField[f].scheme_rest != kPackFor;
    b += (n_wide * pack_width_bound(kWPackField[f].elem, delta) + 7) / 8 + 16 * wpack_kind_blocks_bound(n_wide);
  }
  return b;
}
// The one-launch form's per-kind field arrays in engine scratch: a field's four kinds one behind
// the other in one array of n_wide elements, the fields at 16-byte-aligned offsets in kWPackField's
// order.  wpack_soa_field(f, n_wide): the field's offset ([kWPackFields]: the end).
CLG_PACK_HD uint64_t wpack_soa_field(uint32_t field, uint64_t n_wide) {
  uint64_t at = 0;
  for (uint32_t f = 0; f < field; ++f) at += (n_wide * pack_elem_bytes(wpack_stream_elem(wpack_stream(0, f))) + 15) & ~uint64_t(15);
  return at;
}
inline PackView pack_view(const clg_packed_wide& p) {
  return PackView{p.desc, p.bits, p.cap_desc, p.cap_bits, p.out_kind, kWPackStreams, p.n_val, p.blk_base, &p.n_bits};
}

// The packed wide rows of host columns (clg_pack_wide_host): the split by kind, then pack.h's
// measure and write over the 26 streams.
inline int wpack_build_host(const clg_columns* in, clg_packed_wide* out, const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  *what = "";
  if (!in || !out) return *what = "null argument", CLG_E_INVALID_ARG;
  wpack_reset_result(out);
  const uint64_t nw = in->n_class[4], nr = in->n_rec;
  const WPackCols cols = wpack_cols(*in);
  if (nw) {
    if (!in->w_idx || !in->tag) return *what = "null input array", CLG_E_INVALID_ARG;
    for (uint32_t f = 0; f < kWPackFields; ++f)
      if (!cols.col[f]) return *what = "null input array", CLG_E_INVALID_ARG;
  }
  // the split: every stream's values, extended
  std::vector<int64_t> val[kWPackStreams];
  val[CLG_WPACK_KIND].reserve(size_t(nw)), val[CLG_WPACK_IDX].reserve(size_t(nw));
  uint64_t tot[kWPackKinds] = {};
  for (uint64_t k = 0; k < nw; ++k) {
    const uint32_t kind = wpack_kind_of(in->tag, nr, in->w_idx[k]);
    if (kind >= kWPackKinds) return out->bad_row = k, *what = "a row's w_idx or tag is not a wide record's", CLG_E_INVALID_ARG;
    val[CLG_WPACK_KIND].push_back(int64_t(kind));
    val[CLG_WPACK_IDX].push_back(int64_t(in->w_idx[k]));
    for (uint32_t f = 0; f < kWPackFields; ++f)
      val[wpack_stream(kind, f)].push_back(pack_load(kWPackField[f].elem, cols.col[f], k));
    ++tot[kind];
  }
  wpack_layout(nw, tot, out);
  const auto extend = [&](uint32_t c, uint64_t i0, uint32_t m, int64_t* x) { memcpy(x, val[c].data() + i0, m * sizeof(int64_t)); };
  return pack_build_blocks(pack_view(*out), kWPackSchemeBits, extend, out->desc, out->bits, &out->n_bits, what);
}

// ---- a clg_packed_wide read as input (clg_unpack_wide_host) ----------------------------------
// Nothing is trusted.  The checks and their order are pack_unpack_all_host's: the layout, then the
// sizes and the capacity, then every block, then every value; each kind of finding is reported
// with its lowest (stream, block).  The layout has three rules of its own, and the values two:
//   layout  n_val[KIND] == n_val[IDX] (stream 1 otherwise); the six streams of one kind have equal
//           n_val (the lowest stream that differs from its kind's RC); the kinds' n_val sum to
//           n_val[KIND] (stream 0)
//   value   a KIND above 3 (stream 0, its block); KIND's histogram equal to the kinds' n_val
//           (stream 0, block 0; tested once every KIND is a kind, before the other streams' values)

inline bool wpack_layout_in_ok(const clg_packed_wide& p, uint32_t* stream) {
  if (!pack_layout_in_ok(pack_view(p), stream)) return false;
  if (p.n_val[CLG_WPACK_KIND] != p.n_val[CLG_WPACK_IDX]) return *stream = CLG_WPACK_IDX, false;
  uint64_t sum = 0;
  for (uint32_t t = 0; t < kWPackKinds; ++t) {
    const uint64_t n = p.n_val[wpack_stream(t, 0)];
    for (uint32_t f = 1; f < kWPackFields; ++f)
      if (p.n_val[wpack_stream(t, f)] != n) return *stream = wpack_stream(t, f), false;
    if (n > p.n_val[CLG_WPACK_KIND] - sum) return false;  // (the sum passes the rows: no wrap)
    sum += n;
  }
  return sum == p.n_val[CLG_WPACK_KIND];
}

// kinds (optional): every row's kind, for the cross rule below.
inline int wpack_unpack_host(const clg_packed_wide* in, clg_columns* out, clg_unpack_bad* bad, const char** what = nullptr,
                             std::vector<uint8_t>* kinds = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  *what = "";
  pack_bad_reset(bad);
  if (!in || !out) return *what = "null argument", CLG_E_INVALID_ARG;
  uint32_t stream;
  if (!wpack_layout_in_ok(*in, &stream))
    return *what = "blk_base, n_val, the capacities and the pointers disagree", pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, stream, 0);
  const uint64_t nw = in->n_val[CLG_WPACK_KIND];
  out->n_class[4] = nw;
  const WPackCols cols = wpack_cols(*out);
  bool any = out->w_idx != nullptr, all = out->w_idx != nullptr;
  for (uint32_t f = 0; f < kWPackFields; ++f) any = any || cols.col[f], all = all && cols.col[f];
  if (!any) return CLG_OK;  // sizes only
  if ((!all && nw) || out->cap_wide < nw) return *what = "the wide rows' arrays are too small", CLG_E_CAPACITY;
  // every block, then every value
  for (uint32_t c = 0; c < kWPackStreams; ++c)
    for (uint64_t b = 0; b < pack_blocks_of(in->n_val[c]); ++b)
      if (!pack_block_in_ok(in->desc[in->blk_base[c] + b], wpack_is_delta(c), b, in->n_val[c], in->n_bits))
        return *what = "malformed block descriptor", pack_bad_set(bad, CLG_UNPACK_BAD_BLOCK, c, b);
  std::vector<int64_t> val[kWPackStreams];
  for (uint32_t c = 0; c < kWPackStreams; ++c) {
    val[c].resize(size_t(in->n_val[c]));
    const uint32_t elem = wpack_stream_elem(c);
    for (uint64_t b = 0; b < pack_blocks_of(in->n_val[c]); ++b) {
      const clg_pack_block& d = in->desc[in->blk_base[c] + b];
      int64_t* x = val[c].data() + b * kPackBlock;
      pack_decode_block(d, wpack_is_delta(c), in->bits + d.pos, x);
      for (uint32_t i = 0; i < d.count; ++i)
        if (!pack_elem_value_ok(elem, x[i]) ||(c == CLG_WPACK_KIND && x[i] >= int64_t(kWPackKinds)))
          return *what = "a value outside the stream's type", pack_bad_set(bad, CLG_UNPACK_BAD_VALUE, c, b);
    }
    if (c == CLG_WPACK_KIND) {
      uint64_t hist[kWPackKinds] = {};
      for (uint64_t k = 0; k < nw; ++k) ++hist[val[c][size_t(k)]];
      for (uint32_t t = 0; t < kWPackKinds; ++t)
        if (hist[t] != in->n_val[wpack_stream(t, 0)])
          return *what = "the kinds' counts differ from the streams' lengths", pack_bad_set(bad, CLG_UNPACK_BAD_VALUE, 0, 0);
    }
  }
  // the writes: row k takes the next rank of its kind
  uint64_t rank[kWPackKinds] = {};
  for (uint64_t k = 0; k < nw; ++k) {
    const uint32_t kind = uint32_t(val[CLG_WPACK_KIND][size_t(k)]);
    const uint64_t r = rank[kind]++;
    out->w_idx[k] = uint32_t(val[CLG_WPACK_IDX][size_t(k)]);
    for (uint32_t f = 0; f < kWPackFields; ++f) pack_store(kWPackField[f].elem, cols.col[f], k, val[wpack_stream(kind, f)][size_t(r)]);
    if (kinds) kinds->push_back(uint8_t(kind));
  }
  return CLG_OK;
}

// ---- both packed forms read together (clg_encode_columns_packed_wide and its kin) --------------
// A finding in the wide rows reports stream kWPackBadStream + its stream.  One more rule, which
// only a call that holds the tags can test (clg_pack_wide enforces it with bad_row): row k names
// a wide record of its own kind.  The lowest offending row is reported as VALUE,
// kWPackBadStream + IDX, block k / kPackBlock.
constexpr uint32_t kWPackBadStream = CLG_UNPACK_WIDE_STREAM;
CLG_PACK_HD bool wpack_cross_ok(const uint8_t* tag, uint64_t n_rec, uint32_t idx, uint32_t kind) {
  return wpack_kind_of(tag, n_rec, idx) == kind;
}
inline int wpack_bad_wide(clg_unpack_bad* bad, uint32_t what, uint32_t stream, uint64_t block) {
  return pack_bad_set(bad, what, kWPackBadStream + stream, block);
}
inline int wpack_bad_cross(clg_unpack_bad* bad, uint64_t row) {
  return wpack_bad_wide(bad, CLG_UNPACK_BAD_VALUE, CLG_WPACK_IDX, row / kPackBlock);
}
// What `rest` may carry in the combined calls: none of the arrays that the packed forms give.
inline bool wpack_rest_ok(const clg_columns_in& r) {
  return !r.tag && !r.order && !r.timestamp && !r.rng && !r.buffer_built && !r.w_rc && !r.w_v1 && !r.w_var_len && !r.w_sub &&
         !r.w_v0 && !r.w_idx && !r.pos;
}
// The checks a combined call makes on the host before it reads a descriptor, in their order: the
// narrow layout and its totals against `rest`, the wide layout, the wide rows against n_class[4].
inline int wpack_both_layout(const clg_packed& narrow, const clg_packed_wide& wide, const clg_columns_in& rest,
                             clg_unpack_bad* bad, const char** what) {
  uint32_t stream;
  if (!pack_layout_in_ok(pack_view(narrow), &stream))
    return *what = "narrow: blk_base, n_val, the capacities and the pointers disagree", pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, stream, 0);
  const uint64_t want[kPackStreams] = {rest.n_rec, rest.n_class[0], rest.n_class[1], rest.n_class[2], rest.n_class[3]};
  for (uint32_t c = 0; c < kPackStreams; ++c)
    if (want[c] != narrow.n_val[c])
      return *what = "a narrow stream's length differs from `rest`", pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, c, 0);
  if (!wpack_layout_in_ok(wide, &stream))
    return *what = "wide: blk_base, n_val, the capacities and the pointers disagree", wpack_bad_wide(bad, CLG_UNPACK_BAD_LAYOUT, stream, 0);
  if (wide.n_val[CLG_WPACK_KIND] != rest.n_class[4])
    return *what = "the packed wide rows differ from `rest`'s n_class[4]", wpack_bad_wide(bad, CLG_UNPACK_BAD_LAYOUT, 0, 0);
  return CLG_OK;
}

// The exclusive prefix sum of n lengths: pos[0 .. n], pos[n] the total.
inline void wpack_pos_host(const uint32_t* len, uint64_t n, uint64_t* pos) {
  uint64_t at = 0;
  for (uint64_t k = 0; k < n; ++k) pos[k] = at, at += len[k];
  pos[n] = at;
}

// Host arrays for both unpacks and `rest` completed with them (clg_encode_columns_packed_wide_host):
// the reference the device's combined calls are held to.
struct WPackBothHost {
  std::vector<uint8_t> tag, w_sub;
  std::vector<int8_t> order;
  std::vector<int64_t> timestamp, w_v1, w_v0;
  std::vector<int32_t> rng, buffer_built, w_rc;
  std::vector<uint32_t> w_idx, w_var_off, w_var_len;
  std::vector<uint64_t> pos;
};
inline int wpack_unpack_both_host(const clg_packed* narrow, const clg_packed_wide* wide, const clg_columns_in* rest,
                                  clg_unpack_bad* bad, WPackBothHost* h, clg_columns_in* full, const char** what) {
  *what = "";
  pack_bad_reset(bad);
  if (!narrow || !wide || !rest) return *what = "null argument", CLG_E_INVALID_ARG;
  if (!wpack_rest_ok(*rest)) return *what = "the column pointers of `rest` that the packed forms give must be NULL", CLG_E_INVALID_ARG;
  if (const int st = wpack_both_layout(*narrow, *wide, *rest, bad, what)) return st;
  const uint64_t nw = rest->n_class[4];
  h->tag.resize(size_t(rest->n_rec) + 1), h->order.resize(size_t(rest->n_class[0]) + 1);
  h->timestamp.resize(size_t(rest->n_class[1]) + 1), h->rng.resize(size_t(rest->n_class[2]) + 1);
  h->buffer_built.resize(size_t(rest->n_class[3]) + 1);
  h->w_sub.resize(size_t(nw) + 1), h->w_v1.resize(size_t(nw) + 1), h->w_v0.resize(size_t(nw) + 1), h->w_rc.resize(size_t(nw) + 1);
  h->w_idx.resize(size_t(nw) + 1), h->w_var_off.resize(size_t(nw) + 1), h->w_var_len.resize(size_t(nw) + 1);
  h->pos.resize(size_t(nw) + 1);
  clg_columns c{};
  c.tag = h->tag.data(), c.order = h->order.data(), c.timestamp = h->timestamp.data(), c.rng = h->rng.data();
  c.buffer_built = h->buffer_built.data();
  c.cap_tag = rest->n_rec, c.cap_order = rest->n_class[0], c.cap_timestamp = rest->n_class[1], c.cap_rng = rest->n_class[2];
  c.cap_buffer_built = rest->n_class[3];
  c.w_idx = h->w_idx.data(), c.w_rc = h->w_rc.data(), c.w_v1 = h->w_v1.data(), c.w_var_off = h->w_var_off.data();
  c.w_var_len = h->w_var_len.data(), c.w_sub = h->w_sub.data(), c.w_v0 = h->w_v0.data();
  c.cap_wide = nw;
  if (const int st = pack_unpack_all_host(narrow, &c, bad, what)) return st;
  std::vector<uint8_t> kinds;
  kinds.reserve(size_t(nw));
  if (const int st = wpack_unpack_host(wide, &c, bad, what, &kinds)) {
    if (bad && bad->what != CLG_UNPACK_BAD_NONE) bad->stream += kWPackBadStream;
    return st;
  }
  for (uint64_t k = 0; k < nw; ++k)
    if (!wpack_cross_ok(c.tag, rest->n_rec, c.w_idx[k], kinds[size_t(k)]))
      return *what = "a row's w_idx names no wide record of its kind", wpack_bad_cross(bad, k);
  wpack_pos_host(c.w_var_len, nw, h->pos.data());
  *full = *rest;
  full->tag = c.tag, full->order = c.order, full->timestamp = c.timestamp, full->rng = c.rng, full->buffer_built = c.buffer_built;
  full->w_rc = c.w_rc, full->w_v1 = c.w_v1, full->w_var_len = c.w_var_len, full->w_sub = c.w_sub, full->w_v0 = c.w_v0;
  full->w_idx = c.w_idx, full->pos = h->pos.data();
  return CLG_OK;
}

}  // namespace clg
