// pack.h -- packed typed columns: the format's one definition, for the pack kernels (pack.hip),
// the engine and the CPU version.
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

}  // namespace clg
