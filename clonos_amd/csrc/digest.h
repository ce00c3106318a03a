// digest.h -- the position-sensitive log digest, written once for host and device.
//
// The digest of a span of n bytes b[0..n) is the pair {hash, len = n}:
//   p = 2^61 - 1, R = 2654435761 (a primitive root mod p, so no two positions share a weight),
//   m = ceil(n / 4), w_k = the little-endian u32 of bytes 4k .. 4k+3, zero-padded past n,
//   hash = ( sum_{k<m} w_k * R^(m-1-k) ) mod p
// i.e. h = 0, then h = (h * R + w_k) mod p for each word in order.  hash is always reduced to
// [0, p).  Two spans are taken as equal only when BOTH fields are equal.
//
// The byte-linear form sum_i b_i * 2^(8 (i mod 4)) * R^(m-1-floor(i/4)) mod p gives the same
// value; it is what lets a kernel split a span at any byte: a word straddling two segments is
// two masked words whose contributions add.
//
// For differing spans of equal length the hash is a nonzero polynomial of degree below m in the
// base, so a collision takes a root of it: probability at most m / p for a base that does not
// depend on the data.  This protects against accidents, not adversaries.
//
// Plain C++: compiles under hipcc (host and device) and under g++ without HIP
// (tests/digest_host.cpp, where the power ladder's high bits are checked, and
// tests/digest_prefix_host.cpp for the prefix digests at the end of this file).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLG_DG_HD __host__ __device__ __forceinline__
#else
#define CLG_DG_HD inline
#endif

namespace clg {

constexpr uint64_t kDigestP = (uint64_t(1) << 61) - 1;
constexpr uint32_t kDigestR = 2654435761u;
constexpr int kDigestLadder = 32;  // R^(2^j), j < 32: exponents below 2^32 words

// x < 2^63 + 2^61 -> x mod p in [0, p)
CLG_DG_HD uint64_t dg_reduce(uint64_t x) {
  x = (x & kDigestP) + (x >> 61);  // < 2^61 + 8
  return x >= kDigestP ? x - kDigestP : x;
}
// a, b in [0, p) -> (a + b) mod p
CLG_DG_HD uint64_t dg_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s >= kDigestP ? s - kDigestP : s;
}
// x < 2^62 -> x * 2^32 mod p, partly reduced (< 2^61 + 2^33)
CLG_DG_HD uint64_t dg_shl32(uint64_t x) { return (x >> 29) + ((x & ((uint64_t(1) << 29) - 1)) << 32); }

// (h * R + w) mod p for h in [0, p): R < 2^32, so two 32x32->64 multiply-adds on the halves of
// h plus a fold; no 128-bit multiply.
CLG_DG_HD uint64_t dg_step(uint64_t h, uint32_t w) {
  const uint64_t lo = uint64_t(uint32_t(h)) * kDigestR + w;  // < 2^64
  const uint64_t hi = (h >> 32) * kDigestR;                  // < 2^61
  return dg_reduce((lo & kDigestP) + (lo >> 61) + dg_shl32(hi));
}

// The same step without the last reduction, for a chain of steps: h < 2^63 in, a value
// congruent to h * R + w and again below 2^63 out (2^61 + 8 + 2^34 + 2^61).  dg_reduce ends the
// chain.
CLG_DG_HD uint64_t dg_step_lazy(uint64_t h, uint32_t w) {
  const uint64_t lo = uint64_t(uint32_t(h)) * kDigestR + w;  // < 2^64
  const uint64_t hi = (h >> 32) * kDigestR;                  // < 2^63
  return (lo & kDigestP) + (lo >> 61) + (hi >> 29) + ((hi & ((uint64_t(1) << 29) - 1)) << 32);
}

// (a * b) mod p for a, b in [0, p), by 32-bit halves (2^64 = 8 mod p)
CLG_DG_HD uint64_t dg_mul(uint64_t a, uint64_t b) {
  const uint64_t a0 = uint32_t(a), a1 = a >> 32, b0 = uint32_t(b), b1 = b >> 32;  // a1, b1 < 2^29
  const uint64_t ll = a0 * b0;            // < 2^64
  const uint64_t mid = a1 * b0 + a0 * b1; // < 2^62
  const uint64_t hh = (a1 * b1) << 3;     // < 2^61
  return dg_reduce((ll & kDigestP) + (ll >> 61) + dg_shl32(mid) + hh);
}

// lad[j] = R^(2^j) mod p, j < kDigestLadder (the square ladder)
CLG_DG_HD void dg_ladder(uint64_t* lad) {
  lad[0] = kDigestR;
  for (int j = 1; j < kDigestLadder; ++j) lad[j] = dg_mul(lad[j - 1], lad[j - 1]);
}
// R^e mod p from the ladder
CLG_DG_HD uint64_t dg_pow_lad(const uint64_t* lad, uint32_t e) {
  uint64_t r = 1;
  for (int j = 0; e; ++j, e >>= 1)
    if (e & 1u) r = dg_mul(r, lad[j]);
  return r;
}
// R^e mod p (squares as it goes)
CLG_DG_HD uint64_t dg_pow(uint32_t e) {
  uint64_t r = 1, s = kDigestR;
  for (; e; e >>= 1) {
    if (e & 1u) r = dg_mul(r, s);
    s = dg_mul(s, s);
  }
  return r;
}

// The digest of n host (or device-visible) bytes, one word at a time.
CLG_DG_HD uint64_t dg_bytes(const uint8_t* b, uint64_t n) {
  uint64_t h = 0, i = 0;
  for (; i + 4 <= n; i += 4)
    h = dg_step(h, uint32_t(b[i]) | uint32_t(b[i + 1]) << 8 | uint32_t(b[i + 2]) << 16 | uint32_t(b[i + 3]) << 24);
  if (i < n) {
    uint32_t w = 0;
    for (uint32_t k = 0; i + k < n; ++k) w |= uint32_t(b[i + k]) << (8 * k);
    h = dg_step(h, w);
  }
  return h;
}

// ---- prefix digests: the digest of b[0..c) at many cuts c_1 <= ... <= c_K in one pass ----------
// With m(c) = ceil(c / 4), c_0 = 0 and D_0 = 0:
//   D_j = D_{j-1} * R^(m(c_j) - m(c_{j-1})) + S_j  (mod p),
//   S_j = sum_{c_{j-1} <= i < c_j} b_i * 2^(8 (i mod 4)) * R^(m(c_j) - 1 - floor(i / 4)),
// the digest of the stretch [c_{j-1}, c_j) with c_{j-1} mod 4 zero bytes in front of it: the
// stretch in the span's own word frame.  A word that a cut splits gives its low bytes to one
// stretch and its high bytes to the next, with the same weight (the byte-linear form above).
CLG_DG_HD uint32_t dg_words(uint64_t c) { return uint32_t((c + 3) >> 2); }

// S of the stretch [c0, c1) of b (c0 <= c1; b is the span, not the stretch): word by word, the
// bytes of a word outside the stretch taken as zero.
CLG_DG_HD uint64_t dg_stretch(const uint8_t* b, uint64_t c0, uint64_t c1) {
  uint64_t h = 0;
  for (uint64_t k = c0 >> 2; 4 * k < c1; ++k) {
    const uint64_t lo = 4 * k < c0 ? c0 : 4 * k, hi = 4 * k + 4 < c1 ? 4 * k + 4 : c1;
    uint32_t w = 0;
    for (uint64_t i = lo; i < hi; ++i) w |= uint32_t(b[i]) << (8 * (i & 3));
    h = dg_step(h, w);
  }
  return h;
}

// The map x -> x * mul + add (mod p) that one cut applies to the digest before it; the maps of
// consecutive cuts compose associatively, which is what lets a wave scan them.
struct DgMap {
  uint64_t mul, add;  // in [0, p)
};
CLG_DG_HD uint64_t dg_apply(DgMap f, uint64_t x) { return dg_add(dg_mul(x, f.mul), f.add); }
// f first, then g
CLG_DG_HD DgMap dg_then(DgMap f, DgMap g) { return DgMap{dg_mul(f.mul, g.mul), dg_add(dg_mul(f.add, g.mul), g.add)}; }

// hash[j] / len[j] = the digest of the first min(cuts[j], n) bytes of b, cuts non-decreasing:
// the recurrence, one pass over b.  (Cuts are 32 bits, so exponents stay inside the ladder.)
CLG_DG_HD void dg_prefixes(const uint8_t* b, uint64_t n, const uint32_t* cuts, uint32_t n_cuts, uint64_t* hash,
                           uint64_t* len) {
  uint64_t d = 0, prev = 0;
  for (uint32_t j = 0; j < n_cuts; ++j) {
    const uint64_t c = cuts[j] < n ? cuts[j] : n;
    if (c > prev) d = dg_apply(DgMap{dg_pow(dg_words(c) - dg_words(prev)), dg_stretch(b, prev, c)}, d);
    hash[j] = d;
    len[j] = c;
    if (c > prev) prev = c;
  }
}

}  // namespace clg
