// pack.h -- packed typed columns: the format's one definition, for the pack kernels (pack.hip),
// the unpack kernels (unpack.hip: a packed input's rules are at the end), the engine and the CPU
// version.
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
// All arithmetic is on the values sign-extended to 64 bits (tags zero-extended) and wraps, so
// any int64 sequence round-trips.  The consumers pop one typed value at a time
// (LogReplayerImpl.java:61-119): a cursor over the blocks serves them with no full unpack.
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

// A stream's element size in bytes, and whether it is packed from its deltas.
CLG_PACK_HD uint32_t pack_elem(uint32_t stream) {
  return stream == CLG_PACK_TIMESTAMP ? 8u : stream >= CLG_PACK_RNG ? 4u : 1u;
}
CLG_PACK_HD bool pack_is_delta(uint32_t stream) { return stream == CLG_PACK_TIMESTAMP; }

// Value i of a stream's array, extended to 64 bits (tags zero-extended, the rest sign-extended).
CLG_PACK_HD int64_t pack_load(uint32_t stream, const void* col, uint64_t i) {
  switch (stream) {
    case CLG_PACK_TAG: return int64_t(static_cast<const uint8_t*>(col)[i]);
    case CLG_PACK_ORDER: return int64_t(static_cast<const int8_t*>(col)[i]);
    case CLG_PACK_TIMESTAMP: return static_cast<const int64_t*>(col)[i];
    default: return int64_t(static_cast<const int32_t*>(col)[i]);
  }
}
// The inverse: false when v is outside the stream's type.
CLG_PACK_HD bool pack_store(uint32_t stream, void* col, uint64_t i, int64_t v) {
  switch (stream) {
    case CLG_PACK_TAG:
      if (v < 0 || v > 255) return false;
      static_cast<uint8_t*>(col)[i] = uint8_t(v);
      return true;
    case CLG_PACK_ORDER:
      if (v < -128 || v > 127) return false;
      static_cast<int8_t*>(col)[i] = int8_t(v);
      return true;
    case CLG_PACK_TIMESTAMP: static_cast<int64_t*>(col)[i] = v; return true;
    default:
      if (v < INT32_MIN || v > INT32_MAX) return false;
      static_cast<int32_t*>(col)[i] = int32_t(v);
      return true;
  }
}

CLG_PACK_HD uint32_t pack_width(uint64_t range) {
  return range ? 64u - uint32_t(__builtin_clzll(range)) : 0u;
}
// Residuals of a block of m values, and its payload's bytes.
CLG_PACK_HD uint32_t pack_resid(uint32_t stream, uint32_t m) { return pack_is_delta(stream) && m ? m - 1 : m; }
CLG_PACK_HD uint32_t pack_payload_bytes(uint32_t k, uint32_t width) {
  return 16u * uint32_t((uint64_t(k) * width + 127) / 128);
}
CLG_PACK_HD uint64_t pack_blocks(uint64_t n) { return (n + kPackBlock - 1) / kPackBlock; }

// The five input arrays and their lengths, from a clg_columns.
struct PackSrc {
  const void* col[kPackStreams];
  uint64_t n[kPackStreams];
};
inline PackSrc pack_src(const clg_columns& c) {
  return PackSrc{{c.tag, c.order, c.timestamp, c.rng, c.buffer_built},
                 {c.n_rec, c.n_class[0], c.n_class[1], c.n_class[2], c.n_class[3]}};
}

inline void pack_reset_result(clg_packed* out) {
  for (uint32_t c = 0; c < kPackStreams; ++c) out->n_val[c] = 0;
  for (uint32_t c = 0; c <= kPackStreams; ++c) out->blk_base[c] = 0;
  out->n_bits = 0;
}
inline bool pack_sizes_only(const clg_packed& p) { return !p.desc && !p.bits; }
// n_val and blk_base from the lengths.
inline void pack_layout(const uint64_t n[kPackStreams], clg_packed* out) {
  out->blk_base[0] = 0;
  for (uint32_t c = 0; c < kPackStreams; ++c) {
    out->n_val[c] = n[c];
    out->blk_base[c + 1] = out->blk_base[c] + pack_blocks(n[c]);
  }
}
// The first output that is too small (its name), or null.
inline const char* pack_short(const clg_packed& p) {
  if ((p.desc ? p.cap_desc : 0) < p.blk_base[kPackStreams]) return "desc";
  if ((p.bits ? p.cap_bits : 0) < p.n_bits) return "bits";
  return nullptr;
}

// One block's measure: the descriptor but for pos.
inline clg_pack_block pack_measure_block(uint32_t stream, const void* col, uint64_t i0, uint32_t m) {
  clg_pack_block b{};
  b.count = m;
  const bool delta = pack_is_delta(stream);
  const uint32_t k = pack_resid(stream, m);
  if (delta && m) b.first = pack_load(stream, col, i0);
  if (!k) return b;
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  int64_t prev = delta ? b.first : 0;
  for (uint32_t i = delta ? 1 : 0; i < m; ++i) {
    const int64_t x = pack_load(stream, col, i0 + i);
    const int64_t r = delta ? int64_t(uint64_t(x) - uint64_t(prev)) : x;
    prev = x;
    lo = r < lo ? r : lo;
    hi = r > hi ? r : hi;
  }
  b.ref = lo;
  b.width = pack_width(uint64_t(hi) - uint64_t(lo));
  return b;
}

// One block's payload into dst (pack_payload_bytes(k, width) bytes, written whole: the padding
// is zero).
inline void pack_write_block(uint32_t stream, const void* col, uint64_t i0, const clg_pack_block& b, uint8_t* dst) {
  const bool delta = pack_is_delta(stream);
  const uint32_t k = pack_resid(stream, b.count), w = b.width;
  const uint32_t bytes = pack_payload_bytes(k, w);
  if (!bytes) return;
  memset(dst, 0, bytes);
  int64_t prev = delta ? b.first : 0;
  uint64_t bit = 0;
  for (uint32_t i = delta ? 1 : 0; i < b.count; ++i, bit += w) {
    const int64_t x = pack_load(stream, col, i0 + i);
    const uint64_t r = delta ? uint64_t(x) - uint64_t(prev) : uint64_t(x);
    prev = x;
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

// The packed form of host columns: a measure pass over each stream, then the write pass once the
// sizes are known to fit.  The rules are clg_pack_columns':
// desc and bits both null is the sizes-only call; a capacity below its total is CLG_E_CAPACITY
// with the results filled and nothing written.  *what (optional): a static text for the error.
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
  // the measure of every block, then (once the sizes are known to fit) the write
  const bool sizes_only = pack_sizes_only(*out);
  std::vector<clg_pack_block> desc;
  if (!sizes_only) desc.reserve(size_t(out->blk_base[kPackStreams]));
  uint64_t pos = 0;
  for (uint32_t c = 0; c < kPackStreams; ++c)
    for (uint64_t b = 0; b < pack_blocks(src.n[c]); ++b) {
      const uint64_t i0 = b * kPackBlock;
      const uint32_t m = uint32_t(src.n[c] - i0 < kPackBlock ? src.n[c] - i0 : kPackBlock);
      clg_pack_block d = pack_measure_block(c, src.col[c], i0, m);
      d.pos = pos;
      pos += pack_payload_bytes(pack_resid(c, m), d.width);
      if (!sizes_only) desc.push_back(d);
    }
  out->n_bits = pos;
  if (sizes_only) return CLG_OK;
  if (const char* name = pack_short(*out)) return *what = name, CLG_E_CAPACITY;
  for (uint32_t c = 0; c < kPackStreams; ++c)
    for (uint64_t b = 0; b < pack_blocks(src.n[c]); ++b) {
      const clg_pack_block& d = desc[size_t(out->blk_base[c] + b)];
      out->desc[out->blk_base[c] + b] = d;
      pack_write_block(c, src.col[c], b * kPackBlock, d, out->bits + d.pos);
    }
  return CLG_OK;
}

// Is block b of stream c (of nb blocks, n values) well formed?  What the unpack reads before it
// trusts a descriptor.
inline bool pack_block_ok(const clg_packed& p, uint32_t c, uint64_t b) {
  const uint64_t n = p.n_val[c], nb = pack_blocks(n);
  const clg_pack_block& d = p.desc[p.blk_base[c] + b];
  const uint32_t want = b + 1 < nb ? kPackBlock : uint32_t(n - b * kPackBlock);
  if (d.width > 64 || d.count < 1 || d.count > kPackBlock || d.count != want) return false;
  const uint64_t bytes = pack_payload_bytes(pack_resid(c, d.count), d.width);
  return d.pos <= p.n_bits && bytes <= p.n_bits - d.pos;
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

// `count` values of `stream` from value index `first` into out (the stream's element type);
// only the blocks the range covers are read.  Everything read is validated.
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
  const bool delta = pack_is_delta(stream);
  uint64_t done = 0;
  for (uint64_t b = first / kPackBlock; done < count; ++b) {
    if (!pack_block_ok(*in, stream, b)) return *what = "malformed block descriptor", CLG_E_INVALID_ARG;
    const clg_pack_block& d = in->desc[in->blk_base[stream] + b];
    const uint8_t* payload = in->bits + d.pos;
    const uint64_t i0 = b * kPackBlock;
    const uint32_t lo = uint32_t(first + done > i0 ? first + done - i0 : 0);
    const uint32_t hi = uint32_t(first + count - i0 < d.count ? first + count - i0 : d.count);
    if (delta) {  // the running sum from the block's first value
      uint64_t x = uint64_t(d.first);
      for (uint32_t i = 0; i < hi; ++i) {
        if (i) x += pack_get(payload, d.width, i - 1) + uint64_t(d.ref);
        if (i >= lo && !pack_store(stream, out, done++, int64_t(x))) return *what = "a value outside the stream's type", CLG_E_INVALID_ARG;
      }
    } else {
      for (uint32_t i = lo; i < hi; ++i)
        if (!pack_store(stream, out, done++, int64_t(pack_get(payload, d.width, i) + uint64_t(d.ref))))
          return *what = "a value outside the stream's type", CLG_E_INVALID_ARG;
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
//   block   pack_block_ok's conditions plus pos % 16 == 0 (the format's own rule: the kernel then
//           fetches payloads with aligned 16-byte loads only).  pack_unpack_host above does NOT
//           test the alignment and keeps accepting what it always accepted.  Blocks need not lie
//           in payload order and may share or overlap payload bytes: they are only read
//   value   every unpacked value inside its stream's type (pack_store's rule; timestamps pass)

// pack_blocks without the wrap for n near 2^64.
CLG_PACK_HD uint64_t pack_blocks_of(uint64_t n) { return n / kPackBlock + (n % kPackBlock ? 1u : 0u); }

// The type's bounds of a stream narrower than 64 bits.
CLG_PACK_HD int64_t pack_type_lo(uint32_t stream) {
  return stream == CLG_PACK_TAG ? 0 : stream == CLG_PACK_ORDER ? -128 : int64_t(INT32_MIN);
}
CLG_PACK_HD int64_t pack_type_hi(uint32_t stream) {
  return stream == CLG_PACK_TAG ? 255 : stream == CLG_PACK_ORDER ? 127 : int64_t(INT32_MAX);
}
CLG_PACK_HD bool pack_value_ok(uint32_t stream, int64_t v) {
  return stream == CLG_PACK_TIMESTAMP || (v >= pack_type_lo(stream) && v <= pack_type_hi(stream));
}
// Does [ref, ref + 2^width - 1] lie inside the stream's type?  Then no payload bit can give a
// value outside it and the payload need not be read for the value check.  No overflow: the span
// is compared with hi - ref only once ref is known to lie inside the (narrow) type.
CLG_PACK_HD bool pack_range_inside(uint32_t stream, int64_t ref, uint32_t width) {
  if (stream == CLG_PACK_TIMESTAMP) return true;
  if (width > 32 || ref < pack_type_lo(stream) || ref > pack_type_hi(stream)) return false;
  return (uint64_t(1) << width) - 1 <= uint64_t(pack_type_hi(stream) - ref);
}

// The block check: descriptor d of block b of `stream` (n values), payloads inside [0, n_bits).
CLG_PACK_HD bool pack_block_in_ok(const clg_pack_block& d, uint32_t stream, uint64_t b, uint64_t n, uint64_t n_bits) {
  const uint64_t nb = pack_blocks_of(n);
  if (b >= nb) return false;
  const uint32_t want = b + 1 < nb ? kPackBlock : uint32_t(n - b * kPackBlock);
  if (d.width > 64 || d.count < 1 || d.count > kPackBlock || d.count != want) return false;
  if (d.pos % 16) return false;
  const uint64_t bytes = pack_payload_bytes(pack_resid(stream, d.count), d.width);
  return d.pos <= n_bits && bytes <= n_bits - d.pos;
}

inline void pack_bad_reset(clg_unpack_bad* bad) {
  if (bad) bad->what = CLG_UNPACK_BAD_NONE, bad->stream = 0, bad->block = ~0ull;
}
inline int pack_bad_set(clg_unpack_bad* bad, uint32_t what, uint32_t stream, uint64_t block) {
  if (bad) bad->what = what, bad->stream = stream, bad->block = block;
  return CLG_E_INVALID_ARG;
}

// The layout check.  False: *stream is the lowest stream whose blk_base or n_val disagree, or 0
// for the capacities and the pointers.
inline bool pack_layout_in_ok(const clg_packed& p, uint32_t* stream) {
  *stream = 0;
  if (p.blk_base[0] != 0) return false;
  for (uint32_t c = 0; c < kPackStreams; ++c)
    if (p.blk_base[c + 1] < p.blk_base[c] || p.blk_base[c + 1] - p.blk_base[c] != pack_blocks_of(p.n_val[c]))
      return *stream = c, false;
  if (p.cap_desc < p.blk_base[kPackStreams] || p.cap_bits < p.n_bits) return false;
  if ((p.blk_base[kPackStreams] && !p.desc) || (p.n_bits && !p.bits)) return false;
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
  if (!pack_layout_in_ok(*in, &stream))
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

// Every value of a well-formed block inside its stream's type?
inline bool pack_block_values_ok(uint32_t stream, const clg_pack_block& d, const uint8_t* bits) {
  if (pack_range_inside(stream, d.ref, d.width)) return true;
  for (uint32_t i = 0; i < d.count; ++i)
    if (!pack_value_ok(stream, int64_t(pack_get(bits + d.pos, d.width, i) + uint64_t(d.ref)))) return false;
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
      if (!pack_block_in_ok(d, c, b, in->n_val[c], in->n_bits))
        return *what = "malformed block descriptor", pack_bad_set(bad, CLG_UNPACK_BAD_BLOCK, c, b);
      if (!bad_value && !pack_block_values_ok(c, d, in->bits)) bad_value = true, v_stream = c, v_block = b;
    }
  if (bad_value) return *what = "a value outside the stream's type", pack_bad_set(bad, CLG_UNPACK_BAD_VALUE, v_stream, v_block);
  const UnpackDst dst = unpack_dst(*out);
  for (uint32_t c = 0; c < kPackStreams; ++c)
    for (uint64_t b = 0; b < pack_blocks_of(in->n_val[c]); ++b) {
      const clg_pack_block& d = in->desc[in->blk_base[c] + b];
      const uint8_t* payload = in->bits + d.pos;
      const uint64_t i0 = b * kPackBlock;
      if (pack_is_delta(c)) {
        uint64_t x = uint64_t(d.first);
        for (uint32_t i = 0; i < d.count; ++i) {
          if (i) x += pack_get(payload, d.width, i - 1) + uint64_t(d.ref);
          pack_store(c, dst.col[c], i0 + i, int64_t(x));
        }
      } else {
        for (uint32_t i = 0; i < d.count; ++i)
          pack_store(c, dst.col[c], i0 + i, int64_t(pack_get(payload, d.width, i) + uint64_t(d.ref)));
      }
    }
  return CLG_OK;
}

}  // namespace clg
