// pack_small.hip -- both packs of the typed-columns family (pack.h, pack_wide.h) for a small batch,
// in ONE launch of ONE workgroup: what pack.hip does in five launches and pack_wide.hip in eight,
// with the host's checks between them done by the kernel itself.
//
//  * k_pack_small  a narrow input of at most kPackSmallBlocks blocks, at most kWPackSmallRows
//                  wide rows, either or both.  The passes, a __syncthreads between them:
//                    wide rows   kinds and per-tile kind counts (wpack_row_kinds, wpack_kind_counts),
//                                the lowest bad row (a minimum per thread, through the waves), the
//                                per-kind tile bases and the four totals, the 26-stream table in
//                                LDS (wpack_layout_streams), the split into per-kind arrays in
//                                engine scratch (wpack_tile_rank, wpack_split_rows)
//                    measure     every block of every stream, one after another
//                                (pack_block_measure), the descriptors kept in LDS
//                    scan        the payload sizes into offsets, narrow and wide on their own
//                                (wave_dev.h's tile_scan, 64 bits)
//                    check       a bad row, a sizes-only call, a capacity below its total: the
//                                verdict and every size go to pinned memory, and with any verdict
//                                but kPackSmallWritten the kernel ends having written nothing to
//                                either output
//                    write       every block (pack_block_write), then the descriptors from LDS
//
// The bodies are pack_dev.h's and pack_wide_dev.h's, the ones the multi-kernel forms run: the
// result is theirs byte for byte.  The streams of both halves stand in one table in LDS (the five
// narrow ones first), indexed by a uniform stream number; nothing is indexed in the kernel
// argument but by constants.  __syncthreads only: no global atomics, no flags, no waits, no second
// workgroup; the split's scratch is written and read by this workgroup either side of a barrier.
// No private scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "pack.h"
#include "pack_wide.h"
#include "pack_wide_dev.h"
#include "kernels.h"

namespace clg {

namespace {

constexpr uint32_t kSmallStreams = kPackStreams + kWPackStreams;  // the narrow streams, then the wide ones
constexpr uint32_t kSmallBlocks = kPackSmallBlocks + kWPackSmallBlocks;
constexpr uint32_t kSmallTiles = (kWPackSmallRows + kWPackTile - 1) / kWPackTile;
constexpr uint32_t kPackSmallTooLarge = 5;  // (a verdict the host never asks for: launch_pack_small refuses first)

// The (element, scheme) pairs the two formats use: the block codec is instantiated for these.
constexpr uint32_t small_key(uint32_t elem, uint32_t scheme) { return elem * 2 + (scheme != kPackFor ? 1u : 0u); }
constexpr uint32_t kSmallKeys = 1u << small_key(kElemU8, kPackFor) | 1u << small_key(kElemI8, kPackFor) |
                                1u << small_key(kElemU32, kPackFor) | 1u << small_key(kElemU32, kPackDelta) |
                                1u << small_key(kElemI32, kPackFor) | 1u << small_key(kElemI64, kPackFor) |
                                1u << small_key(kElemI64, kPackDelta);
constexpr bool small_has(uint32_t elem, uint32_t scheme) { return (kSmallKeys >> small_key(elem, scheme) & 1u) != 0; }
constexpr bool small_keys_cover() {
  bool ok = small_has(kWPackKindElem, kWPackKindScheme);
  ok = ok && small_has(kWPackIdxElem, kWPackIdxScheme);
  for (uint32_t c = 0; c < kPackStreams; ++c) ok = ok && small_has(kPackStream[c].elem, kPackStream[c].scheme);
  for (uint32_t f = 0; f < kWPackFields; ++f)
    ok = ok && small_has(kWPackField[f].elem, kWPackField[f].scheme_kind0) && small_has(kWPackField[f].elem, kWPackField[f].scheme_rest);
  return ok;
}
static_assert(small_keys_cover(), "CLG_SMALL_DISPATCH names every (element, scheme) of kPackStream and kWPackField");
#define CLG_SMALL_DISPATCH(key, body, ...)           \
  switch (key) {                                     \
    CLG_WPACK_CASE(body, kElemU8, 0, __VA_ARGS__)    \
    CLG_WPACK_CASE(body, kElemI8, 0, __VA_ARGS__)    \
    CLG_WPACK_CASE(body, kElemU32, 0, __VA_ARGS__)   \
    CLG_WPACK_CASE(body, kElemU32, 1, __VA_ARGS__)   \
    CLG_WPACK_CASE(body, kElemI32, 0, __VA_ARGS__)   \
    CLG_WPACK_CASE(body, kElemI64, 0, __VA_ARGS__)   \
    CLG_WPACK_CASE(body, kElemI64, 1, __VA_ARGS__)   \
  }
// Stream s of the joint table: its element and scheme as the dispatch's key.
__device__ __forceinline__ uint32_t small_stream_key(uint32_t s) {
  return s < kPackStreams ? pack_stream_elem(s) * 2 + uint32_t(pack_is_delta(s))
                          : wpack_stream_elem(s - kPackStreams) * 2 + uint32_t(wpack_is_delta(s - kPackStreams));
}

// A value every thread holds alike, moved to scalar registers.
__device__ __forceinline__ uint32_t uni(uint32_t x) { return uint32_t(__builtin_amdgcn_readfirstlane(int(x))); }
__device__ __forceinline__ uint64_t uni(uint64_t x) { return uint64_t(uni(uint32_t(x))) | uint64_t(uni(uint32_t(x >> 32))) << 32; }

// The payload sizes in desc[0 .. n).pos -> their exclusive prefix; the total is returned.
__device__ __forceinline__ uint64_t small_scan(clg_pack_block* desc, uint32_t n) {
  return tile_scan<kPackThreads, 1, uint64_t>(
             n, [&](uint32_t b, uint64_t c[1]) { c[0] = desc[b].pos; },
             [&](uint32_t b, const uint64_t before[1]) { desc[b].pos = before[0]; })
      .v[0];
}

}  // namespace

__global__ __launch_bounds__(kPackThreads) void k_pack_small(const PackSmallArgs a, PackSmallRes* __restrict__ res) {
  // the block's values (the DELTA predecessors) in the measure, the payload's words in the write
  __shared__ __attribute__((aligned(16))) unsigned long long s_w[kPackBlock];
  __shared__ int64_t s_lo[kPackWaves], s_hi[kPackWaves];
  __shared__ clg_pack_block s_desc[kSmallBlocks];
  __shared__ WPackTab s_wtab;  // the wide streams, as the multi-kernel form's table
  __shared__ const void* s_col[kSmallStreams];  // both halves' streams: array, length, first descriptor slot
  __shared__ uint64_t s_n[kSmallStreams];
  __shared__ uint32_t s_slot[kSmallStreams + 1];
  __shared__ uint32_t s_cnt[kSmallTiles * kWPackKinds];
  __shared__ uint64_t s_tbase[kSmallTiles * kWPackKinds];
  __shared__ uint64_t s_tot[kWPackKinds];
  __shared__ uint64_t s_bad;
  __shared__ WPackTileLds s_l;
  const uint32_t tid = threadIdx.x;
  const uint64_t nw = a.wide.n_wide;

  uint64_t nb_narrow = 0;
#pragma unroll
  for (uint32_t c = 0; c < kPackStreams; ++c) nb_narrow += pack_blocks_of(a.narrow.n[c]);
  if (nb_narrow > kPackSmallBlocks || nw > kWPackSmallRows) {  // (uniform; never: the launch refuses it)
    if (tid == 0) res->verdict = kPackSmallTooLarge;
    return;
  }
  const uint32_t n_tiles = uint32_t((nw + kWPackTile - 1) / kWPackTile);

  // ---- the wide rows: kinds, counts, the bad row, bases and totals ---------------------------
  uint64_t bad = ~0ull;
  for (uint32_t tile = 0; tile < n_tiles; ++tile) {
    uint32_t kind[kPackPerThread];
    const uint64_t b = wpack_row_kinds(a.wide, tile, a.d_kind, kind);
    bad = b < bad ? b : bad;
    wpack_kind_counts(kind, s_cnt, tile);
    __syncthreads();
  }
  bad = block_min<kPackThreads>(bad);
  if (tid == 0) s_bad = bad;
  __syncthreads();
  const bool wide_on = nw != 0 && s_bad == ~0ull;  // (uniform)
  if (tid < kWPackKinds) {
    uint64_t run = 0;
    for (uint32_t tile = 0; tile < n_tiles && wide_on; ++tile) {
      s_tbase[tile * kWPackKinds + tid] = run;
      run += s_cnt[tile * kWPackKinds + tid];
    }
    s_tot[tid] = run;
  }
  __syncthreads();

  // ---- the joint stream table ----------------------------------------------------------------
  if (tid == 0) {
    uint32_t slot = 0;
#pragma unroll
    for (uint32_t c = 0; c < kPackStreams; ++c) {
      s_col[c] = a.narrow.col[c], s_n[c] = a.narrow.n[c], s_slot[c] = slot;
      slot += uint32_t(pack_blocks_of(a.narrow.n[c]));
    }
    wpack_layout_streams(wide_on ? nw : 0, s_tot, s_wtab.n, s_wtab.blk_base);
    s_wtab.col[CLG_WPACK_KIND] = a.d_kind, s_wtab.col[CLG_WPACK_IDX] = a.wide.w_idx;
    uint64_t before = 0;  // the rows of the kinds below t
    for (uint32_t t = 0; t < kWPackKinds; ++t) {
      for (uint32_t f = 0; f < kWPackFields; ++f)
        s_wtab.col[wpack_stream(t, f)] =
            a.d_soa + wpack_soa_field(f, nw) + before * pack_elem_bytes(wpack_stream_elem(wpack_stream(t, f)));
      before += s_tot[t];
    }
    for (uint32_t c = 0; c < kWPackStreams; ++c) {
      s_col[kPackStreams + c] = s_wtab.col[c], s_n[kPackStreams + c] = s_wtab.n[c];
      s_slot[kPackStreams + c] = slot + uint32_t(s_wtab.blk_base[c]);
    }
    s_slot[kSmallStreams] = slot + uint32_t(s_wtab.blk_base[kWPackStreams]);
  }
  __syncthreads();

  // ---- the split into per-kind arrays --------------------------------------------------------
  if (wide_on) {
    for (uint32_t tile = 0; tile < n_tiles; ++tile) {
      uint32_t kind[kPackPerThread];
      uint64_t r[kPackPerThread];
#pragma unroll
      for (uint32_t q = 0; q < kPackPerThread; ++q) {
        const uint64_t k = uint64_t(tile) * kWPackTile + q * kPackThreads + tid;
        kind[q] = k < nw ? uint32_t(a.d_kind[k]) : kWPackKinds;
      }
      wpack_tile_rank(&s_wtab, s_tbase, tile, kind, s_l, r);
      wpack_split_rows(a.wide, tile, kind, r, s_l);
      __syncthreads();
    }
  }

  // ---- measure: every block of every stream, the descriptors in LDS -----------------------------
  for (uint32_t s = 0; s < kSmallStreams; ++s) {
    const uint32_t slot0 = uni(s_slot[s]), nblk = uni(s_slot[s + 1]) - slot0;
    if (!nblk) continue;
    const void* col = reinterpret_cast<const void*>(uintptr_t(uni(uint64_t(reinterpret_cast<uintptr_t>(s_col[s])))));
    const uint64_t n = uni(s_n[s]);
    const uint32_t key = small_stream_key(s);
    for (uint32_t j = 0; j < nblk; ++j) {
      const PackAt at = pack_at(col, n, 0, j);
      CLG_SMALL_DISPATCH(key, pack_block_measure, at, &s_desc[slot0 + j], reinterpret_cast<int64_t*>(s_w), s_lo, s_hi)
      __syncthreads();
    }
  }

  // ---- scan and check ------------------------------------------------------------------------
  const uint32_t nbn = uni(s_slot[kPackStreams]), nbw = uni(s_slot[kSmallStreams]) - nbn;
  const uint64_t bits_n = small_scan(s_desc, nbn);
  const uint64_t bits_w = small_scan(s_desc + nbn, nbw);
  const bool write_n = a.out_narrow.write != 0, write_w = a.out_wide.write != 0;
  uint32_t short_cap = kPackSmallShortNone;
  if (write_w && a.out_wide.cap_bits < bits_w) short_cap = 3;
  if (write_w && a.out_wide.cap_desc < nbw) short_cap = 2;
  if (write_n && a.out_narrow.cap_bits < bits_n) short_cap = 1;
  if (write_n && a.out_narrow.cap_desc < nbn) short_cap = 0;
  const uint64_t bad_row = s_bad;
  const uint32_t verdict = bad_row != ~0ull                             ? kPackSmallBadRow
                           : a.sizes_only || (!write_n && !write_w)     ? kPackSmallSizes
                           : short_cap != kPackSmallShortNone           ? kPackSmallCapacity
                                                                        : kPackSmallWritten;
  if (tid == 0) {
    res->n_bits[0] = bits_n, res->n_bits[1] = bits_w;
#pragma unroll
    for (uint32_t t = 0; t < kWPackKinds; ++t) res->tot[t] = s_tot[t];
    res->bad_row = bad_row;
    res->verdict = verdict;
    res->short_cap = short_cap;
  }
  if (verdict != kPackSmallWritten) return;  // (uniform) nothing has been written to either output

  // ---- write: the payloads, then the descriptors ------------------------------------------------
  clg_pack_block* const desc_n = a.out_narrow.desc;
  clg_pack_block* const desc_w = a.out_wide.desc;
  uint8_t* const out_n = a.out_narrow.packed ? reinterpret_cast<uint8_t*>(desc_n + nbn) : a.out_narrow.bits;
  uint8_t* const out_w = a.out_wide.packed ? reinterpret_cast<uint8_t*>(desc_w + nbw) : a.out_wide.bits;
  for (uint32_t s = 0; s < kSmallStreams; ++s) {
    const bool narrow = s < kPackStreams;
    if (!(narrow ? write_n : write_w)) continue;
    const uint32_t slot0 = uni(s_slot[s]), nblk = uni(s_slot[s + 1]) - slot0;
    if (!nblk) continue;
    const void* col = reinterpret_cast<const void*>(uintptr_t(uni(uint64_t(reinterpret_cast<uintptr_t>(s_col[s])))));
    const uint64_t n = uni(s_n[s]);
    const uint32_t key = small_stream_key(s);
    uint8_t* const bits = narrow ? out_n : out_w;
    const uint64_t lim = narrow ? bits_n : bits_w;
    for (uint32_t j = 0; j < nblk; ++j) {
      const PackAt at = pack_at(col, n, 0, j);
      clg_pack_block d;
      d.ref = int64_t(uni(uint64_t(s_desc[slot0 + j].ref))), d.first = 0;
      d.pos = uni(s_desc[slot0 + j].pos);
      d.width = uni(s_desc[slot0 + j].width), d.count = uni(s_desc[slot0 + j].count);
      CLG_SMALL_DISPATCH(key, pack_block_write, at, d, s_w, bits, lim)
      __syncthreads();
    }
  }
  const unsigned long long* words = reinterpret_cast<const unsigned long long*>(s_desc);
  if (write_n)
    for (uint32_t i = tid; i < nbn * 4; i += kPackThreads) reinterpret_cast<unsigned long long*>(desc_n)[i] = words[i];
  if (write_w)
    for (uint32_t i = tid; i < nbw * 4; i += kPackThreads) reinterpret_cast<unsigned long long*>(desc_w)[i] = words[nbn * 4 + i];
}

int launch_pack_small(const PackSmallArgs& a, PackSmallRes* res, void* stream) {
  uint64_t nb = 0;
  for (uint32_t c = 0; c < kPackStreams; ++c) nb += pack_blocks_of(a.narrow.n[c]);
  if (nb > kPackSmallBlocks || a.wide.n_wide > kWPackSmallRows) return CLG_E_INVALID_ARG;
  hipLaunchKernelGGL(k_pack_small, dim3(1), dim3(kPackThreads), 0, (hipStream_t)stream, a, res);
  return launch_status(hipGetLastError());
}

}  // namespace clg
