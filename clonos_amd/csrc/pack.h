// pack.h -- packed typed columns: the format's one definition, for the pack kernels (pack.hip),
// the unpack kernels (unpack.hip: a packed input's rules are at the end), the engine and the CPU
// version; and the block codec of both packed families (pack_wide.h packs its 26 streams' blocks
// with it): what an element and a scheme are, and a block's measure, write, decode and check on
// the host.  The device's measure and write are pack_dev.h's.
//
// The five narrow columns of clg_columns (tag, order, timestamp, rng, buffer_built) carry far
// more bits than their values hold: a tag is one of eight values in a byte, an Order channel a
// small number in a byte, a BufferBuilt size a few bits of an i32, a Timestamp a clock that
// advances by a few units a record in an i64.  Each column is a stream, cut into blocks of
// kPackBlock values that are packed on their own (block-wise frame of reference):
//
//   residuals  FOR: r_i = x_i (k = m of them).  DELTA (timestamps): first = x_0 and
//              r_i = x_i - x_{i-1} for i >= 1 (k = m - 1), modulo 2^64
//   ref        the minimum residual as int64 (0 when k = 0)
//   width      0 when max == min, else 64 - clz(uint64(max) - uint64(ref))
//   payload    p_i = uint64(r_i) - uint64(ref) at bits [i * width, (i + 1) * width) of a
//              little-endian bit string (bit j = bit j % 64 of u64 word j / 64), zero-padded to
//              a multiple of 16 bytes
//
// All arithmetic is on the values extended to 64 bits (pack_load) and wraps, so any int64 sequence
// round-trips.  The consumers pop one typed value at a time (LogReplayerImpl.java:61-119): a cursor
// over the blocks serves them with no full unpack.
//
// Plain C++: compiles under hipcc (host and device) and under g++ without HIP
// (tests/pack_host.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/clonos_engine.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLG_PACK_HD __host__ __device__ __forceinline__
#else
#define CLG_PACK_HD inline
#endif

namespace clg {

constexpr uint32_t kPackStreams = CLG_PACK_STREAMS;
constexpr uint32_t kPackBlock = CLG_PACK_BLOCK;
// The offset scan's group: this many blocks get their offsets from one workgroup, a block a
// thread; the groups' sums are scanned by one workgroup between the two group passes.
constexpr uint32_t kPackScanGroup = 256;

static_assert(sizeof(clg_pack_block) == 32, "clg_pack_block layout");

// A stream is an element (what its values are extended to 64 bits from: unsigned ones zero-extended,
// signed ones sign-extended) and a scheme.  Both families name their streams in these words.
enum : uint32_t { kElemU8 = 0, kElemU32 = 1, kElemI32 = 2, kElemI64 = 3, kElemI8 = 4 };
enum : uint32_t { kPackFor = 0, kPackDelta = 1 };

CLG_PACK_HD uint32_t pack_elem_bytes(uint32_t elem) {
  return elem == kElemU8 || elem == kElemI8 ? 1u : elem == kElemI64 ? 8u : 4u;
}
// Value i of an array of `elem`, extended to 64 bits.
CLG_PACK_HD int64_t pack_load(uint32_t elem, const void* col, uint64_t i) {
  switch (elem) {
    case kElemU8: return int64_t(static_cast<const uint8_t*>(col)[i]);
    case kElemI8: return int64_t(static_cast<const int8_t*>(col)[i]);
    case kElemU32: return int64_t(static_cast<const uint32_t*>(col)[i]);
    case kElemI32: return int64_t(static_cast<const int32_t*>(col)[i]);
    default: return static_cast<const int64_t*>(col)[i];
  }
}
// The inverse, for a v that pack_elem_value_ok passed.
CLG_PACK_HD void pack_store(uint32_t elem, void* col, uint64_t i, int64_t v) {
  switch (elem) {
    case kElemU8: static_cast<uint8_t*>(col)[i] = uint8_t(v); break;
    case kElemI8: static_cast<int8_t*>(col)[i] = int8_t(v); break;
    case kElemU32: static_cast<uint32_t*>(col)[i] = uint32_t(v); break;
    case kElemI32: static_cast<int32_t*>(col)[i] = int32_t(v); break;
    default: static_cast<int64_t*>(col)[i] = v; break;
  }
}
// The bounds of an element narrower than 64 bits, and whether v lies inside the element's type.
CLG_PACK_HD int64_t pack_elem_lo(uint32_t elem) {
  return elem == kElemI8 ? -128 : elem == kElemI32 ? int64_t(INT32_MIN) : 0;
}
CLG_PACK_HD int64_t pack_elem_hi(uint32_t elem) {
  return elem == kElemU8 ? 255 : elem == kElemI8 ? 127 : elem == kElemI32 ? int64_t(INT32_MAX) : int64_t(UINT32_MAX);
}
CLG_PACK_HD bool pack_elem_value_ok(uint32_t elem, int64_t v) {
  return elem == kElemI64 || (v >= pack_elem_lo(elem) && v <= pack_elem_hi(elem));
}
// Does [ref, ref + 2^width - 1] lie inside the element's type?  Then no payload bit of a FOR block
// can give a value outside it and the payload need not be read for the value check.  No overflow:
// the span is compared with hi - ref only once ref is known to lie inside the (narrow) type.
CLG_PACK_HD bool pack_elem_range_inside(uint32_t elem, int64_t ref, uint32_t width) {
  if (elem == kElemI64) return true;
  if (width > 32 || ref < pack_elem_lo(elem) || ref > pack_elem_hi(elem)) return false;
  return (uint64_t(1) << width) - 1 <= uint64_t(pack_elem_hi(elem) - ref);
}

// The narrow format: the five columns' streams.  Folded into two words (three bits of element and
// one of scheme a stream), so that device code indexes a constant and not an array.
struct PackStream {
  uint8_t elem, scheme;
};
constexpr PackStream kPackStream[kPackStreams] = {
    {kElemU8, kPackFor},     // TAG           tag
    {kElemI8, kPackFor},     // ORDER         order
    {kElemI64, kPackDelta},  // TIMESTAMP     timestamp
    {kElemI32, kPackFor},    // RNG           rng
    {kElemI32, kPackFor},    // BUFFER_BUILT  buffer_built
};
static_assert(CLG_PACK_TAG == 0 && CLG_PACK_ORDER == 1 && CLG_PACK_TIMESTAMP == 2 && CLG_PACK_RNG == 3 &&
                  CLG_PACK_BUFFER_BUILT == 4 && kPackStreams == 5,
              "kPackStream's rows are the CLG_PACK_* enumerators");
constexpr uint32_t pack_fold(bool scheme) {
  uint32_t w = 0;
  for (uint32_t c = 0; c < kPackStreams; ++c)
    w |= scheme ? uint32_t(kPackStream[c].scheme) << c : uint32_t(kPackStream[c].elem) << (3 * c);
  return w;
}
constexpr uint32_t kPackElemBits = pack_fold(false), kPackSchemeBits = pack_fold(true);

// Keyed by a narrow stream: one-line wrappers over the table.
CLG_PACK_HD constexpr uint32_t pack_stream_elem(uint32_t stream) { return kPackElemBits >> (3 * stream) & 7u; }
CLG_PACK_HD constexpr bool pack_is_delta(uint32_t stream) { return (kPackSchemeBits >> stream & 1u) != 0; }
CLG_PACK_HD uint32_t pack_stream_bytes(uint32_t stream) { return pack_elem_bytes(pack_stream_elem(stream)); }
CLG_PACK_HD bool pack_value_ok(uint32_t stream, int64_t v) { return pack_elem_value_ok(pack_stream_elem(stream), v); }
CLG_PACK_HD bool pack_range_inside(uint32_t stream, int64_t ref, uint32_t width) {
  return pack_elem_range_inside(pack_stream_elem(stream), ref, width);
}

CLG_PACK_HD uint32_t pack_width(uint64_t range) {
  return range ? 64u - uint32_t(__builtin_clzll(range)) : 0u;
}
// Residuals of a block of m values (of a narrow stream: pack_resid), and its payload's bytes.
CLG_PACK_HD uint32_t pack_residuals(bool delta, uint32_t m) { return delta && m ? m - 1 : m; }
CLG_PACK_HD uint32_t pack_resid(uint32_t stream, uint32_t m) { return pack_residuals(pack_is_delta(stream), m); }
CLG_PACK_HD uint32_t pack_payload_bytes(uint32_t k, uint32_t width) {
  return 16u * uint32_t((uint64_t(k) * width + 127) / 128);
}
CLG_PACK_HD uint64_t pack_blocks(uint64_t n) { return (n + kPackBlock - 1) / kPackBlock; }

// ---- the one-launch form (pack_small.hip) ------------------------------------------------------
// A narrow input of at most kPackSmallBlocks blocks is packed by one launch of one workgroup
// (k_pack_small).  The floor is what five streams of the one-launch columns form's largest batch
// (columns.h kColSmallRecords = 32 769 records) can hold: 33 tag blocks and 32 + 4 of the other
// four; the engine asserts it.
constexpr uint32_t kPackSmallBlocks = 69;

// The widest residual a block of (elem, scheme) can hold, in bits.  FOR: the element's.  DELTA: a
// difference of two values of a narrow element needs one bit more than the element (a zero-extended
// u32 gives residuals from -(2^32 - 1) to 2^32 - 1: 33 bits); of i64 it wraps inside 64.
CLG_PACK_HD uint32_t pack_width_bound(uint32_t elem, bool delta) {
  const uint32_t bits = 8u * pack_elem_bytes(elem);
  return delta && bits < 64 ? bits + 1 : bits;
}
// The payload bytes of a stream of n values of (elem, scheme), at most: what the one-launch form
// sizes its staging by before anything is measured.
CLG_PACK_HD uint64_t pack_bits_bound(uint32_t elem, bool delta, uint64_t n) {
  const uint32_t w = pack_width_bound(elem, delta);
  const uint64_t whole = n / kPackBlock;
  const uint32_t rest = uint32_t(n % kPackBlock);
  return whole * pack_payload_bytes(pack_residuals(delta, kPackBlock), w) + pack_payload_bytes(pack_residuals(delta, rest), w);
}
// ... of the five narrow streams of lengths n.
CLG_PACK_HD uint64_t pack_bits_bound_narrow(const uint64_t n[kPackStreams]) {
  uint64_t b = 0;
  for (uint32_t c = 0; c < kPackStreams; ++c) b += pack_bits_bound(pack_stream_elem(c), pack_is_delta(c), n[c]);
  return b;
}

// The five input arrays and their lengths, from a clg_columns.
struct PackSrc {
  const void* col[kPackStreams];
  uint64_t n[kPackStreams];
};
inline PackSrc pack_src(const clg_columns& c) {
  return PackSrc{{c.tag, c.order, c.timestamp, c.rng, c.buffer_built},
                 {c.n_rec, c.n_class[0], c.n_class[1], c.n_class[2], c.n_class[3]}};
}

// What clg_packed and clg_packed_wide have in common, read through one view: the two outputs with
// their capacities and kind, and the results of `streams` streams.
struct PackView {
  const clg_pack_block* desc;
  const uint8_t* bits;
  uint64_t cap_desc, cap_bits;
  uint32_t out_kind, streams;
  const uint64_t *n_val, *blk_base, *n_bits;
  uint64_t blocks() const { return blk_base[streams]; }
};
inline PackView pack_view(const clg_packed& p) {
  return PackView{p.desc, p.bits, p.cap_desc, p.cap_bits, p.out_kind, kPackStreams, p.n_val, p.blk_base, &p.n_bits};
}
inline bool pack_sizes_only(const PackView& p) { return !p.desc && !p.bits; }
// The first output that is too small (its name), or null.
inline const char* pack_short(const PackView& p) {
  if ((p.desc ? p.cap_desc : 0) < p.blocks()) return "desc";
  if ((p.bits ? p.cap_bits : 0) < *p.n_bits) return "bits";
  return nullptr;
}

inline void pack_reset_result(clg_packed* out) {
  for (uint32_t c = 0; c < kPackStreams; ++c) out->n_val[c] = 0;
  for (uint32_t c = 0; c <= kPackStreams; ++c) out->blk_base[c] = 0;
  out->n_bits = 0;
}
// n_val and blk_base from the lengths.
inline void pack_layout(const uint64_t n[kPackStreams], clg_packed* out) {
  out->blk_base[0] = 0;
  for (uint32_t c = 0; c < kPackStreams; ++c) {
    out->n_val[c] = n[c];
    out->blk_base[c + 1] = out->blk_base[c] + pack_blocks(n[c]);
  }
}
// The stream that holds block blk of a packed form of n_streams streams (either family's blk_base).
inline uint32_t pack_stream_of_block(const uint64_t* blk_base, uint32_t n_streams, uint64_t blk) {
  uint32_t c = 0;
  while (c + 1 < n_streams && blk >= blk_base[c + 1]) ++c;
  return c;
}

// ---- the block codec on the host, over a block's values extended to int64 ----------------------

// One block's measure over its m values: the descriptor but for pos.
inline clg_pack_block pack_measure_block(const int64_t* x, uint32_t m, bool delta) {
  clg_pack_block b{};
  b.count = m;
  const uint32_t k = pack_residuals(delta, m);
  if (delta && m) b.first = x[0];
  if (!k) return b;
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  for (uint32_t i = delta ? 1 : 0; i < m; ++i) {
    const int64_t r = delta ? int64_t(uint64_t(x[i]) - uint64_t(x[i - 1])) : x[i];
    lo = r < lo ? r : lo;
    hi = r > hi ? r : hi;
  }
  b.ref = lo;
  b.width = pack_width(uint64_t(hi) - uint64_t(lo));
  return b;
}

// One block's payload into dst (pack_payload_bytes(k, width) bytes, written whole: the padding
// is zero).
inline void pack_write_block(const int64_t* x, const clg_pack_block& b, bool delta, uint8_t* dst) {
  const uint32_t k = pack_residuals(delta, b.count), w = b.width;
  const uint32_t bytes = pack_payload_bytes(k, w);
  if (!bytes) return;
  memset(dst, 0, bytes);
  uint64_t bit = 0;
  for (uint32_t i = delta ? 1 : 0; i < b.count; ++i, bit += w) {
    const uint64_t r = delta ? uint64_t(x[i]) - uint64_t(x[i - 1]) : uint64_t(x[i]);
    const uint64_t p = r - uint64_t(b.ref);
    const uint32_t sh = uint32_t(bit & 63);
    uint8_t* at = dst + (bit >> 6) * 8;
    uint64_t word;
    memcpy(&word, at, 8);
    word |= p << sh;
    memcpy(at, &word, 8);
    if (sh + w > 64) {  // (sh > 0 here: no shift by 64)
      memcpy(&word, at + 8, 8);
      word |= p >> (64 - sh);
      memcpy(at + 8, &word, 8);
    }
  }
}

// Residual i's p of a block's payload.
inline uint64_t pack_get(const uint8_t* payload, uint32_t w, uint64_t i) {
  if (!w) return 0;
  const uint64_t bit = i * w;
  const uint32_t sh = uint32_t(bit & 63);
  const uint8_t* at = payload + (bit >> 6) * 8;
  uint64_t lo, hi;
  memcpy(&lo, at, 8);
  uint64_t v = lo >> sh;
  if (sh + w > 64) {  // (sh > 0 here)
    memcpy(&hi, at + 8, 8);
    v |= hi << (64 - sh);
  }
  return w == 64 ? v : v & ((1ull << w) - 1);
}

// A well-formed block's values, extended, into x[0 .. count): FOR adds ref, DELTA is the running
// sum from the block's first value.
inline void pack_decode_block(const clg_pack_block& d, bool delta, const uint8_t* payload, int64_t* x) {
  uint64_t v = uint64_t(d.first);
  for (uint32_t i = 0; i < d.count; ++i) {
    if (!delta) v = pack_get(payload, d.width, i) + uint64_t(d.ref);
    else if (i) v += pack_get(payload, d.width, i - 1) + uint64_t(d.ref);
    x[i] = int64_t(v);
  }
}

// pack_blocks without the wrap for n near 2^64.
CLG_PACK_HD uint64_t pack_blocks_of(uint64_t n) { return n / kPackBlock + (n % kPackBlock ? 1u : 0u); }

// The block check, what an unpack reads before it trusts a descriptor: d of block b of a stream of
// n values, its payload inside [0, n_bits).  aligned: pos % 16 == 0 is required as well (the
// format's own rule; the kernels then fetch payloads with aligned 16-byte loads only).
CLG_PACK_HD bool pack_block_in_ok(const clg_pack_block& d, bool delta, uint64_t b, uint64_t n, uint64_t n_bits,
                                  bool aligned = true) {
  const uint64_t nb = pack_blocks_of(n);
  if (b >= nb) return false;
  const uint32_t want = b + 1 < nb ? kPackBlock : uint32_t(n - b * kPackBlock);
  if (d.width > 64 || d.count < 1 || d.count > kPackBlock || d.count != want) return false;
  if (aligned && d.pos % 16) return false;
  const uint64_t bytes = pack_payload_bytes(pack_residuals(delta, d.count), d.width);
  return d.pos <= n_bits && bytes <= n_bits - d.pos;
}

// What pack_build_host and wpack_build_host do once n_val and blk_base are laid out: the measure
// of every block, then (once the sizes are known to fit) the write.  scheme_bits: bit c is set for
// a DELTA stream; extend(c, i0, m, x): values [i0, i0 + m) of stream c, extended, into x.  The
// rules are clg_pack_columns': desc and bits both null is the sizes-only call; a capacity below
// its total is CLG_E_CAPACITY (*what: the output's name) with *n_bits filled and nothing written.
template <class Extend>
inline int pack_build_blocks(const PackView& p, uint32_t scheme_bits, const Extend& extend, clg_pack_block* out_desc,
                             uint8_t* out_bits, uint64_t* n_bits, const char** what) {
  const bool sizes_only = pack_sizes_only(p);
  std::vector<clg_pack_block> desc;
  if (!sizes_only) desc.reserve(size_t(p.blocks()));
  int64_t x[kPackBlock];
  uint64_t pos = 0;
  for (uint32_t c = 0; c < p.streams; ++c)
    for (uint64_t b = 0; b < pack_blocks(p.n_val[c]); ++b) {
      const bool delta = (scheme_bits >> c & 1u) != 0;
      const uint64_t i0 = b * kPackBlock;
      const uint32_t m = uint32_t(p.n_val[c] - i0 < kPackBlock ? p.n_val[c] - i0 : kPackBlock);
      extend(c, i0, m, x);
      clg_pack_block d = pack_measure_block(x, m, delta);
      d.pos = pos;
      pos += pack_payload_bytes(pack_residuals(delta, m), d.width);
      if (!sizes_only) desc.push_back(d);
    }
  *n_bits = pos;
  if (sizes_only) return CLG_OK;
  if (const char* name = pack_short(p)) return *what = name, CLG_E_CAPACITY;
  for (uint32_t c = 0; c < p.streams; ++c)
    for (uint64_t b = 0; b < pack_blocks(p.n_val[c]); ++b) {
      const clg_pack_block& d = desc[size_t(p.blk_base[c] + b)];
      extend(c, b * kPackBlock, d.count, x);
      out_desc[p.blk_base[c] + b] = d;
      pack_write_block(x, d, (scheme_bits >> c & 1u) != 0, out_bits + d.pos);
    }
  return CLG_OK;
}

// The packed form of host columns (clg_pack_columns_host).  *what (optional): a static text for
// the error.
inline int pack_build_host(const clg_columns* in, clg_packed* out, const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  *what = "";
  if (!in || !out) return *what = "null argument", CLG_E_INVALID_ARG;
  pack_reset_result(out);
  const PackSrc src = pack_src(*in);
  for (uint32_t c = 0; c < kPackStreams; ++c)
    if (src.n[c] && !src.col[c]) return *what = "null input array", CLG_E_INVALID_ARG;
  pack_layout(src.n, out);
  const auto extend = [&](uint32_t c, uint64_t i0, uint32_t m, int64_t* x) {
    for (uint32_t i = 0; i < m; ++i) x[i] = pack_load(pack_stream_elem(c), src.col[c], i0 + i);
  };
  return pack_build_blocks(pack_view(*out), kPackSchemeBits, extend, out->desc, out->bits, &out->n_bits, what);
}

// `count` values of `stream` from value index `first` into out (the stream's element type);
// only the blocks the range covers are read.  Everything read is validated, but for pos % 16:
// this call does NOT test the alignment and keeps accepting what it always accepted.
inline int pack_unpack_host(const clg_packed* in, uint32_t stream, uint64_t first, uint64_t count, void* out,
                            const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  *what = "";
  if (!in || stream >= kPackStreams) return *what = "null argument or unknown stream", CLG_E_INVALID_ARG;
  const uint64_t n = in->n_val[stream];
  if (first > n || count > n - first) return *what = "the range passes the stream's end", CLG_E_INVALID_ARG;
  if (!count) return CLG_OK;
  if (!out || !in->desc) return *what = "null array", CLG_E_INVALID_ARG;
  if (in->blk_base[stream] > in->blk_base[stream + 1] ||
      in->blk_base[stream + 1] - in->blk_base[stream] != pack_blocks(n) || in->blk_base[stream + 1] > in->cap_desc ||
      in->n_bits > in->cap_bits || (in->n_bits && !in->bits))
    return *what = "blk_base, n_val and the capacities disagree", CLG_E_INVALID_ARG;
  const uint32_t elem = pack_stream_elem(stream);
  const bool delta = pack_is_delta(stream);
  int64_t x[kPackBlock];
  uint64_t done = 0;
  for (uint64_t b = first / kPackBlock; done < count; ++b) {
    const clg_pack_block& d = in->desc[in->blk_base[stream] + b];
    if (!pack_block_in_ok(d, delta, b, n, in->n_bits, false)) return *what = "malformed block descriptor", CLG_E_INVALID_ARG;
    pack_decode_block(d, delta, in->bits + d.pos, x);
    const uint64_t i0 = b * kPackBlock;
    const uint32_t lo = uint32_t(first + done > i0 ? first + done - i0 : 0);
    const uint32_t hi = uint32_t(first + count - i0 < d.count ? first + count - i0 : d.count);
    for (uint32_t i = lo; i < hi; ++i) {
      if (!pack_elem_value_ok(elem, x[i])) return *what = "a value outside the stream's type", CLG_E_INVALID_ARG;
      pack_store(elem, out, done++, x[i]);
    }
  }
  return CLG_OK;
}

// ---- a clg_packed read as input: the whole-call unpack (clg_unpack_columns) -------------------
// The descriptors may come from another process, so nothing is trusted.  Three checks, reported
// in this order (clg_unpack_bad.what), each with the lowest (stream, block) of its kind:
//   layout  blk_base[0] == 0, blk_base does not decrease, every stream has
//           blk_base[c + 1] - blk_base[c] == pack_blocks(n_val[c]); cap_desc >= blk_base[5],
//           cap_bits >= n_bits, desc and bits non-null where something is read
//   block   pack_block_in_ok, pos % 16 == 0 included (pack_unpack_host above is the one caller
//           that leaves the alignment out).  Blocks need not lie in payload order and may share
//           or overlap payload bytes: they are only read
//   value   every unpacked value inside its stream's element (pack_elem_value_ok; timestamps pass)

inline void pack_bad_reset(clg_unpack_bad* bad) {
  if (bad) bad->what = CLG_UNPACK_BAD_NONE, bad->stream = 0, bad->block = ~0ull;
}
inline int pack_bad_set(clg_unpack_bad* bad, uint32_t what, uint32_t stream, uint64_t block) {
  if (bad) bad->what = what, bad->stream = stream, bad->block = block;
  return CLG_E_INVALID_ARG;
}

// The layout check.  False: *stream is the lowest stream whose blk_base or n_val disagree, or 0
// for the capacities and the pointers.
inline bool pack_layout_in_ok(const PackView& p, uint32_t* stream) {
  *stream = 0;
  if (p.blk_base[0] != 0) return false;
  for (uint32_t c = 0; c < p.streams; ++c)
    if (p.blk_base[c + 1] < p.blk_base[c] || p.blk_base[c + 1] - p.blk_base[c] != pack_blocks_of(p.n_val[c]))
      return *stream = c, false;
  if (p.cap_desc < p.blocks() || p.cap_bits < *p.n_bits) return false;
  if ((p.blocks() && !p.desc) || (*p.n_bits && !p.bits)) return false;
  return true;
}

// The five output arrays and their capacities, from a clg_columns (a null column holds nothing).
struct UnpackDst {
  void* col[kPackStreams];
  uint64_t cap[kPackStreams];
};
inline UnpackDst unpack_dst(const clg_columns& c) {
  return UnpackDst{{c.tag, c.order, c.timestamp, c.rng, c.buffer_built},
                   {c.tag ? c.cap_tag : 0, c.order ? c.cap_order : 0, c.timestamp ? c.cap_timestamp : 0,
                    c.rng ? c.cap_rng : 0, c.buffer_built ? c.cap_buffer_built : 0}};
}

// What every whole-call unpack does before it reads a descriptor, in this order: the layout check
// (CLG_E_INVALID_ARG, bad filled), the sizes into out (n_rec, n_class[0..3]; nothing else of out
// is touched), the sizes-only call (all five pointers null: CLG_OK, *done), the capacities
// (CLG_E_CAPACITY).  CLG_OK without *done: go on to the block and value checks.
inline int pack_unpack_begin(const clg_packed* in, clg_columns* out, clg_unpack_bad* bad, bool* done, const char** what) {
  *done = true;
  *what = "";
  pack_bad_reset(bad);
  if (!in || !out) return *what = "null argument", CLG_E_INVALID_ARG;
  uint32_t stream;
  if (!pack_layout_in_ok(pack_view(*in), &stream))
    return *what = "blk_base, n_val, the capacities and the pointers disagree", pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, stream, 0);
  out->n_rec = in->n_val[0];
  for (uint32_t c = 1; c < kPackStreams; ++c) out->n_class[c - 1] = in->n_val[c];
  const UnpackDst dst = unpack_dst(*out);
  bool any = false;
  for (uint32_t c = 0; c < kPackStreams; ++c) any = any || dst.col[c];
  if (!any) return CLG_OK;  // sizes only
  for (uint32_t c = 0; c < kPackStreams; ++c)
    if (dst.cap[c] < in->n_val[c]) return *what = "an output column is too small", CLG_E_CAPACITY;
  *done = false;
  return CLG_OK;
}

// Every value of a well-formed block inside its element's type?
inline bool pack_block_values_ok(uint32_t elem, bool delta, const clg_pack_block& d, const uint8_t* bits) {
  if (elem == kElemI64 || (!delta && pack_elem_range_inside(elem, d.ref, d.width))) return true;
  int64_t x[kPackBlock];
  pack_decode_block(d, delta, bits + d.pos, x);
  for (uint32_t i = 0; i < d.count; ++i)
    if (!pack_elem_value_ok(elem, x[i])) return false;
  return true;
}

// The whole call on the CPU (clg_unpack_columns_all_host): the reference the device unpack is held
// to.  A checking pass over every block, then the writes: invalid input writes nothing.
inline int pack_unpack_all_host(const clg_packed* in, clg_columns* out, clg_unpack_bad* bad, const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  bool done;
  const int st = pack_unpack_begin(in, out, bad, &done, what);
  if (st != CLG_OK || done) return st;
  bool bad_value = false;
  uint32_t v_stream = 0;
  uint64_t v_block = 0;
  for (uint32_t c = 0; c < kPackStreams; ++c)
    for (uint64_t b = 0; b < pack_blocks_of(in->n_val[c]); ++b) {
      const clg_pack_block& d = in->desc[in->blk_base[c] + b];
      if (!pack_block_in_ok(d, pack_is_delta(c), b, in->n_val[c], in->n_bits))
        return *what = "malformed block descriptor", pack_bad_set(bad, CLG_UNPACK_BAD_BLOCK, c, b);
      if (!bad_value && !pack_block_values_ok(pack_stream_elem(c), pack_is_delta(c), d, in->bits))
        bad_value = true, v_stream = c, v_block = b;
    }
  if (bad_value) return *what = "a value outside the stream's type", pack_bad_set(bad, CLG_UNPACK_BAD_VALUE, v_stream, v_block);
  const UnpackDst dst = unpack_dst(*out);
  int64_t x[kPackBlock];
  for (uint32_t c = 0; c < kPackStreams; ++c)
    for (uint64_t b = 0; b < pack_blocks_of(in->n_val[c]); ++b) {
      const clg_pack_block& d = in->desc[in->blk_base[c] + b];
      pack_decode_block(d, pack_is_delta(c), in->bits + d.pos, x);
      for (uint32_t i = 0; i < d.count; ++i) pack_store(pack_stream_elem(c), dst.col[c], b * kPackBlock + i, x[i]);
    }
  return CLG_OK;
}

}  // namespace clg
