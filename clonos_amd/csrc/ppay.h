// ppay.h -- the packed payload column: the format's one definition, for the CPU version, the
// kernels (ppay.hip) and the engine.
//
// The payload column (payload.h) holds the wide rows' timer names, storage references and Java
// streams back to back.  They are the most repetitive bytes the engine moves: a thread's timers
// carry the same few names, and its Serializable determinants are streams of one or two classes
// that differ in their last bytes.  Rows are front-coded against an anchor row of the same length
// in the same tile, so that every row is packed and unpacked on its own.
//
// The packed form is a pure function of a payload column (var, pos) of n_rows rows:
//   len_k      pos[k + 1] - pos[k]; a row of 2^32 bytes or more is rejected
//   tile t     rows [1024 t, min(1024 (t + 1), n_rows)): one block of the LCP stream
//   anchor(k)  the lowest row j of k's tile with len_j == len_k (j <= k).  It depends on the
//              lengths alone: the unpack recomputes it and nothing about it is stored
//   lcp_k      0 when anchor(k) == k, else the count of leading bytes in which row k and row
//              anchor(k) agree, 0 .. len_k
//   tail_k     bytes [lcp_k, len_k) of row k (an anchor's tail is its whole row)
// What is stored:
//   desc, bits the stream lcp u32[n_rows], FOR, in pack.h's block format exactly (clg_pack_block,
//              the little-endian bit string, 16-byte padding, payloads in block order)
//   tail       the tails back to back in row order; n_tail is the sum of len_k - lcp_k
// Decoding: row k is tail_anchor(k)[0 : lcp_k] followed by tail_k.  The prefix comes from the
// packed bytes, never from another output row.  The lengths are not stored: the wide rows carry
// them (w_var_len), so the unpack takes pos as an input.  The pack emits the maximal lcp; the
// unpack accepts any lcp_k <= len_k for a row that is not its own anchor and requires 0 for one
// that is.
//
// Plain C++: compiles under hipcc (host and device) and under g++ without HIP
// (tests/ppay_host.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/clonos_engine.h"
#include "diff.h"
#include "pack.h"

namespace clg {

constexpr uint32_t kPpayTile = kPackBlock;  // a tile is one block of the LCP stream
constexpr uint64_t kPpayNoRow = ~0ull;
constexpr uint64_t kPpayRowLimit = 1ull << 32;  // a row's bytes, below this

// The anchor table of a tile on the device: open addressing over the lengths, twice the tile's
// rows, so that a probe always ends at a free slot.  The hash is the top bits of a Fibonacci
// product; tests build colliding lengths from it.
constexpr uint32_t kPpaySlots = 2 * kPpayTile;
constexpr uint32_t kPpayHashShift = 21;
static_assert((1u << (32 - kPpayHashShift)) == kPpaySlots, "the hash gives a slot");
CLG_PACK_HD uint32_t ppay_hash(uint32_t len) { return (len * 0x9E3779B1u) >> kPpayHashShift; }

// ---- sizes, for staging before anything is measured --------------------------------------------
CLG_PACK_HD uint64_t ppay_blocks(uint64_t n_rows) { return pack_blocks_of(n_rows); }
// n_tail <= n_var: a tail is a part of its row.
CLG_PACK_HD uint64_t ppay_tail_bound(uint64_t n_var) { return n_var; }
// n_bits <= the payload bytes of a FOR stream of n_rows u32 values.  With the descriptors, that is
// all an incompressible column grows by.
CLG_PACK_HD uint64_t ppay_bits_bound(uint64_t n_rows) { return pack_bits_bound(kElemU32, false, n_rows); }

// ---- the pos rules, of the pack and the unpack alike -------------------------------------------
// Is row k of pos a bad row?  pos[0] != 0 (row 0), pos decreasing over the row, or a row of 2^32
// bytes or more.
CLG_PACK_HD bool ppay_row_bad(uint64_t k, uint64_t p0, uint64_t p1) {
  return (k == 0 && p0 != 0) || p1 < p0 || p1 - p0 >= kPpayRowLimit;
}

inline void ppay_reset_result(clg_packed_payloads* out) {
  out->n_rows = out->n_var = out->n_bits = out->n_tail = 0;
  out->bad_row = kPpayNoRow;
}
inline bool ppay_sizes_only(const clg_packed_payloads& p) { return !p.desc && !p.bits && !p.tail; }
// The first output that is too small (its name), or null.  A null pointer holds nothing.
inline const char* ppay_short(const clg_packed_payloads& p) {
  if ((p.desc ? p.cap_desc : 0) < ppay_blocks(p.n_rows)) return "desc";
  if ((p.bits ? p.cap_bits : 0) < p.n_bits) return "bits";
  if ((p.tail ? p.cap_tail : 0) < p.n_tail) return "tail";
  return nullptr;
}

// The anchors of one tile of m rows from their lengths, on the host: anchor[i] is the lowest row
// (tile-relative) of row i's length.
inline void ppay_anchors_host(const uint64_t* pos, uint32_t m, uint32_t* anchor) {
  std::vector<uint32_t> order(m);
  for (uint32_t i = 0; i < m; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return pos[a + 1] - pos[a] < pos[b + 1] - pos[b]; });
  for (uint32_t i = 0, first = 0; i < m; ++i) {
    if (i && pos[order[i] + 1] - pos[order[i]] != pos[first + 1] - pos[first]) first = order[i];
    else if (!i) first = order[0];
    anchor[order[i]] = first;
  }
}

// The packed form of a host payload column (clg_pack_payloads_host).  The rules are
// clg_pack_columns': all three outputs null is the sizes-only call; a capacity below its total is
// CLG_E_CAPACITY with every result filled and nothing written; a bad row is CLG_E_INVALID_ARG with
// the lowest one in bad_row, found before any byte of var is read.  *what (optional): a static text.
inline int ppay_build_host(const uint8_t* var, const uint64_t* pos, uint64_t n_rows, clg_packed_payloads* out,
                           const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  *what = "";
  if (!out) return *what = "null argument", CLG_E_INVALID_ARG;
  ppay_reset_result(out);
  out->n_rows = n_rows;
  if (!n_rows) return CLG_OK;
  if (!pos) return *what = "null pos", CLG_E_INVALID_ARG;
  for (uint64_t k = 0; k < n_rows; ++k)
    if (ppay_row_bad(k, pos[k], pos[k + 1])) return out->bad_row = k, *what = "pos does not start at 0, decreases or holds a row of 2^32 bytes", CLG_E_INVALID_ARG;
  out->n_var = pos[n_rows];
  if (out->n_var && !var) return *what = "null var", CLG_E_INVALID_ARG;

  // the measure: every row's lcp, the blocks' descriptors, the totals
  std::vector<uint32_t> lcp(size_t(n_rows), 0);
  std::vector<clg_pack_block> desc(size_t(ppay_blocks(n_rows)));
  uint32_t anchor[kPpayTile];
  int64_t x[kPpayTile];
  uint64_t n_tail = 0, n_bits = 0;
  for (uint64_t t = 0; t < desc.size(); ++t) {
    const uint64_t k0 = t * kPpayTile;
    const uint32_t m = uint32_t(n_rows - k0 < kPpayTile ? n_rows - k0 : kPpayTile);
    ppay_anchors_host(pos + k0, m, anchor);
    for (uint32_t i = 0; i < m; ++i) {
      const uint64_t k = k0 + i, a = k0 + anchor[i], len = pos[k + 1] - pos[k];
      if (a != k) lcp[size_t(k)] = uint32_t(df_lcp_bytes(var + pos[k], len, var + pos[a], len));
      n_tail += len - lcp[size_t(k)];
      x[i] = int64_t(lcp[size_t(k)]);
    }
    clg_pack_block d = pack_measure_block(x, m, false);
    d.pos = n_bits;
    n_bits += pack_payload_bytes(m, d.width);
    desc[size_t(t)] = d;
  }
  out->n_bits = n_bits;
  out->n_tail = n_tail;
  if (ppay_sizes_only(*out)) return CLG_OK;
  if (const char* name = ppay_short(*out)) return *what = name, CLG_E_CAPACITY;

  // the write
  uint64_t at = 0;
  for (uint64_t t = 0; t < desc.size(); ++t) {
    const clg_pack_block& d = desc[size_t(t)];
    const uint64_t k0 = t * kPpayTile;
    for (uint32_t i = 0; i < d.count; ++i) x[i] = int64_t(lcp[size_t(k0 + i)]);
    out->desc[t] = d;
    pack_write_block(x, d, false, out->bits + d.pos);
    for (uint32_t i = 0; i < d.count; ++i) {
      const uint64_t k = k0 + i, n = pos[k + 1] - pos[k] - lcp[size_t(k)];
      if (n) memcpy(out->tail + at, var + pos[k] + lcp[size_t(k)], size_t(n));
      at += n;
    }
  }
  return CLG_OK;
}

// ---- a clg_packed_payloads read as input (clg_unpack_payloads) ---------------------------------
// Nothing is trusted.  The findings, in the order they are reported (clg_unpack_bad.what, with
// stream = CLG_PPAY_STREAM), each with its lowest block (a tile):
//   layout  cap_desc below ceil(n_rows / 1024), cap_bits < n_bits, cap_tail < n_tail, a null array
//           that would be read (desc, bits, tail, pos); block 0; checked on the host
//   block   pack_block_in_ok, pos % 16 == 0 included
//   value   an lcp above its row's length, a non-zero lcp on a row that is its own anchor,
//           pos[0] != 0, a decreasing pos, a row of 2^32 bytes or more
//   total   the sum of len_k - lcp_k differs from n_tail, or pos[n_rows] from n_var; block 0
// Past them every tail lies inside [0, n_tail), every row inside [0, n_var) and every prefix inside
// its anchor's tail, whose length is the row's own.

inline bool ppay_layout_in_ok(const clg_packed_payloads& p, const uint64_t* pos) {
  const uint64_t nb = ppay_blocks(p.n_rows);
  if (p.cap_desc < nb || p.cap_bits < p.n_bits || p.cap_tail < p.n_tail) return false;
  if ((nb && !p.desc) || (p.n_bits && !p.bits) || (p.n_tail && !p.tail) || (p.n_rows && !pos)) return false;
  return true;
}

// What every unpack does before it reads a descriptor, in this order: the layout check
// (CLG_E_INVALID_ARG, bad filled), the sizes into out (n_rows and n_var; pos is not touched), the
// sizes-only call (var null: CLG_OK, *done), the capacity (CLG_E_CAPACITY).  CLG_OK without *done:
// go on to the block, value and total checks.
inline int ppay_unpack_begin(const clg_packed_payloads* in, const uint64_t* pos, clg_payloads* out, clg_unpack_bad* bad,
                             bool* done, const char** what) {
  *done = true;
  *what = "";
  pack_bad_reset(bad);
  if (!in || !out) return *what = "null argument", CLG_E_INVALID_ARG;
  if (!ppay_layout_in_ok(*in, pos))
    return *what = "n_rows, the capacities and the pointers disagree", pack_bad_set(bad, CLG_UNPACK_BAD_LAYOUT, CLG_PPAY_STREAM, 0);
  out->n_rows = in->n_rows;
  out->n_var = in->n_var;
  if (!out->var) return CLG_OK;  // sizes only
  if (out->cap_var < in->n_var) return *what = "var is too small", CLG_E_CAPACITY;
  *done = false;
  return CLG_OK;
}

// The whole call on the CPU (clg_unpack_payloads_host): the reference the device unpack is held to.
// A checking pass over every tile, then the writes: invalid input writes nothing.
inline int ppay_unpack_host(const clg_packed_payloads* in, const uint64_t* pos, clg_payloads* out, clg_unpack_bad* bad,
                            const char** what = nullptr) {
  const char* dummy;
  if (!what) what = &dummy;
  bool done;
  const int st = ppay_unpack_begin(in, pos, out, bad, &done, what);
  if (st != CLG_OK || done) return st;
  const uint64_t n = in->n_rows, nb = ppay_blocks(n);
  for (uint64_t t = 0; t < nb; ++t)
    if (!pack_block_in_ok(in->desc[t], false, t, n, in->n_bits))
      return *what = "malformed block descriptor", pack_bad_set(bad, CLG_UNPACK_BAD_BLOCK, CLG_PPAY_STREAM, t);
  std::vector<uint32_t> lcp(size_t(n), 0), anchor(size_t(n), 0);
  int64_t x[kPpayTile];
  uint64_t sum = 0;
  for (uint64_t t = 0; t < nb; ++t) {
    const clg_pack_block& d = in->desc[t];
    const uint64_t k0 = t * kPpayTile;
    bool ok = true;
    for (uint32_t i = 0; i < d.count && ok; ++i) ok = !ppay_row_bad(k0 + i, pos[k0 + i], pos[k0 + i + 1]);
    if (ok) {
      pack_decode_block(d, false, in->bits + d.pos, x);
      ppay_anchors_host(pos + k0, d.count, anchor.data() + k0);
      for (uint32_t i = 0; i < d.count && ok; ++i) {
        const uint64_t k = k0 + i, len = pos[k + 1] - pos[k];
        ok = uint64_t(x[i]) <= len && (anchor[size_t(k)] != i || x[i] == 0);
        lcp[size_t(k)] = uint32_t(x[i]);
        sum += len - uint64_t(x[i]);
      }
    }
    if (!ok) return *what = "an lcp or a length breaks the format's rules", pack_bad_set(bad, CLG_UNPACK_BAD_VALUE, CLG_PPAY_STREAM, t);
  }
  if (sum != in->n_tail || (n ? pos[n] : 0) != in->n_var)
    return *what = "the tails do not sum to n_tail, or pos does not end at n_var", pack_bad_set(bad, CLG_UNPACK_BAD_TOTAL, CLG_PPAY_STREAM, 0);

  // the write: the tails' offsets are the running sum, in row order
  std::vector<uint64_t> toff(static_cast<size_t>(n));
  uint64_t at = 0;
  for (uint64_t k = 0; k < n; ++k) toff[size_t(k)] = at, at += pos[k + 1] - pos[k] - lcp[size_t(k)];
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t a = k / kPpayTile * kPpayTile + anchor[size_t(k)], len = pos[k + 1] - pos[k], c = lcp[size_t(k)];
    if (c) memcpy(out->var + pos[k], in->tail + toff[size_t(a)], size_t(c));
    if (len - c) memcpy(out->var + pos[k] + c, in->tail + toff[size_t(k)], size_t(len - c));
  }
  return CLG_OK;
}

}  // namespace clg
