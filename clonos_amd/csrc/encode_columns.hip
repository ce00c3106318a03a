// encode_columns.hip -- typed columns back to log bytes on gfx950 (encode_columns.h): the
// inverse of columns.hip and payload.hip.
//
//  (count, scan)   passes 1 and 2 are the columns' own k_col_count and k_col_scan over the tags
//                  (the tile is the columns' tile): per-tile class counts, their exclusive bases,
//                  the totals and the first tile with a tag above 7 in pinned memory
//  * k_ecol_bytes  pass 3: a workgroup per tile ranks its records within their classes (chunk
//                  ballots and mbcnt, as k_col_write), reads the wide rows' w_sub / w_var_len (and
//                  pos, w_idx where they are checked) and writes the tile's byte sum (u64) and
//                  its lowest bad row
//  * k_ecol_scan64 pass 4: ONE workgroup loops over the tiles' sums (a carry between rounds, no
//                  look-back): every tile's byte base; n_bytes and the lowest bad row go to
//                  pinned memory
//  * k_ecol_span   a wave per span boundary: the byte base of the tile that holds the span's first
//                  record plus the lengths before it inside the tile, and whether the class counts
//                  before it are the span_base row
//  * k_ecol_write  pass 5, after the host has checked everything above: a workgroup per tile ranks
//                  its records again, scans their lengths, assembles them big-endian in an LDS
//                  buffer laid out with the destination's 16-byte phase and writes the buffer out
//                  with aligned 16-byte stores, byte stores only in the tile's two edge chunks.
//                  Payloads of kEcolWaveRow bytes or more skip LDS: one wave copies the aligned
//                  interior from var to the output through copy_range<64>, the up to 15 bytes
//                  either side go through LDS, and the interior's chunks are flagged so that the
//                  buffer's write-out leaves them alone.  A tile whose bytes do not fit the buffer
//                  stores directly (records by their own lanes, long payloads by waves).
//
// Kernel boundaries order the passes: no spin waits, no atomics between workgroups and no word
// taken from another running workgroup; the bytes are deterministic.
//
// Bounds: a column is indexed only below its stated length (n_class), var only inside a row's
// range after ecol_row_ok (copy_range loads whole aligned 16-byte words that hold a byte of the
// range, as for the payload column), and no store lands at or past n_bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "copy_range.h"
#include "encode_columns.h"
#include "kernels.h"
#include "wave_dev.h"

namespace clg {

namespace {

constexpr uint32_t kEcolWaves = kEcolTileThreads / 64;
constexpr uint32_t kEcolChunks = kEcolPer * kEcolWaves;  // a tile's (round, wave) chunks, in record order
constexpr uint32_t kEcolScanThreads = 1024;
static_assert(kEcolChunks == 64, "the chunk counts are scanned by one wave");
static_assert(kEcolLds / 16 % kEcolTileThreads == 0, "the threads clear the chunk flags evenly");

// A tile's tags (record k * kEcolTileThreads + tid of the tile for k < kEcolPer; 0xFF at and
// past n) and, in cnt, the exclusive per-class count of every (round, wave) chunk in record
// order.  All kEcolTileThreads threads call it; two __syncthreads inside.
__device__ __forceinline__ void ecol_tile_tags(const uint8_t* __restrict__ tag, uint64_t n, uint64_t i0, uint32_t tid,
                                               uint8_t tg[kEcolPer], uint32_t (*cnt)[kColClasses]) {
  const uint32_t lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (uint32_t k = 0; k < kEcolPer; ++k) {
    const uint64_t i = i0 + k * kEcolTileThreads + tid;
    tg[k] = i < n ? tag[i] : uint8_t(0xFF);
  }
#pragma unroll
  for (uint32_t k = 0; k < kEcolPer; ++k) {
    const uint32_t cls = col_class(tg[k]);
#pragma unroll
    for (uint32_t c = 0; c < kColClasses; ++c) {
      const uint64_t m = __ballot(cls == c);
      if (lane == 0) cnt[k * kEcolWaves + w][c] = (uint32_t)__popcll(m);
    }
  }
  __syncthreads();
  if (tid < kEcolChunks) {
#pragma unroll
    for (uint32_t c = 0; c < kColClasses; ++c) {
      const uint32_t x = cnt[tid][c];
      cnt[tid][c] = wave_incl(x, lane) - x;
    }
  }
  __syncthreads();
}

// This record's rank within its class inside its chunk (wave-uniform call; 0 for a bad tag).
__device__ __forceinline__ uint32_t ecol_chunk_rank(uint32_t cls) {
  uint32_t rank = 0;
#pragma unroll
  for (uint32_t c = 0; c < kColClasses; ++c) {
    const uint64_t m = __ballot(cls == c);
    if (cls == c) rank = lane_rank(m);
  }
  return rank;
}

// v[cls] for cls < 5 without indexing a register array (0 for a bad class).
__device__ __forceinline__ uint64_t ecol_pick(const uint64_t v[kColClasses], uint32_t cls) {
  uint64_t x = 0;
#pragma unroll
  for (uint32_t c = 0; c < kColClasses; ++c) x = cls == c ? v[c] : x;
  return x;
}

// A wide row as the length rules need it: sub, and var_len where the format carries a payload
// (0 elsewhere, and for a row at or past the stated number of rows).
struct EcolRow {
  uint32_t sub, vl;
  bool pay;
};
__device__ __forceinline__ EcolRow ecol_row(const EcolIn& in, uint32_t tag, uint64_t row) {
  EcolRow r{0, 0, false};
  if (row >= in.n_class[kColWide]) return r;
  r.sub = in.w_sub[row];
  r.pay = ecol_has_payload(tag, r.sub);
  if (r.pay) r.vl = in.w_var_len[row];
  return r;
}

}  // namespace

// sum[tile]: the tile's encoded bytes; bad[tile]: its lowest bad row (kEcolNone: none).
// base[tile * 5 + c]: the class-c records before the tile (k_col_scan's).
__global__ __launch_bounds__(kEcolTileThreads) void k_ecol_bytes(const EcolIn in, const uint64_t* __restrict__ base,
                                                            uint64_t* __restrict__ sum, uint64_t* __restrict__ bad) {
  __shared__ uint32_t cnt[kEcolChunks][kColClasses];
  __shared__ uint64_t ws[kEcolWaves], wb[kEcolWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t i0 = uint64_t(blockIdx.x) * kEcolTile;
  const uint64_t tb4 = base[size_t(blockIdx.x) * kColClasses + kColWide];
  uint8_t tg[kEcolPer];
  ecol_tile_tags(in.tag, in.n, i0, tid, tg, cnt);
  uint64_t acc = 0, b = kEcolNone;
#pragma unroll
  for (uint32_t k = 0; k < kEcolPer; ++k) {
    const uint32_t t = tg[k], cls = col_class(t);
    const uint32_t rank = ecol_chunk_rank(cls);
    if (cls == kColWide) {
      const uint64_t row = tb4 + cnt[k * kEcolWaves + w][kColWide] + rank;
      const EcolRow r = ecol_row(in, t, row);
      if (row < in.n_class[kColWide]) {
        const bool idx_bad = in.w_idx && in.w_idx[row] != uint32_t(i0 + k * kEcolTileThreads + tid);
        const bool pay_bad = r.pay && (!in.pos || !ecol_row_ok(in.pos[row], r.vl, in.n_var));
        if ((idx_bad || pay_bad) && row < b) b = row;
      }
      acc += ecol_len(t, r.sub, r.vl);
    } else {
      acc += ecol_head_len(t, 0);  // (0 for a tag above 7 and past n)
    }
  }
  acc = wave_sum(acc);
  b = wave_min(b);
  if (lane == 0) ws[w] = acc, wb[w] = b;
  __syncthreads();
  if (tid == 0) {
    for (uint32_t k = 1; k < kEcolWaves; ++k) acc += ws[k], b = wb[k] < b ? wb[k] : b;
    sum[blockIdx.x] = acc;
    bad[blockIdx.x] = b;
  }
}

// bbase[tile]: the bytes before the tile; *res (pinned): n_bytes and the lowest bad row.
__global__ __launch_bounds__(kEcolScanThreads) void k_ecol_scan64(const uint64_t* __restrict__ sum,
                                                                 const uint64_t* __restrict__ bad, uint32_t n_tiles,
                                                                 uint64_t* __restrict__ bbase, EcolRes* __restrict__ res) {
  uint64_t b = kEcolNone;  // this thread's lowest bad row
  const auto tot = tile_scan<kEcolScanThreads, 1, uint64_t>(
      n_tiles,
      [&](uint32_t t, uint64_t c[1]) {
        c[0] = sum[t];
        const uint64_t x = bad[t];
        b = x < b ? x : b;
      },
      [&](uint32_t t, const uint64_t before[1]) { bbase[t] = before[0]; });
  b = block_min<kEcolScanThreads>(b);
  if (threadIdx.x == 0) {
    res->n_bytes = tot.v[0];
    res->bad_row = b;
  }
}

// span_out[s * 2]: the byte offset of span s's first record (s <= n_spans; n_bytes at the end);
// span_out[s * 2 + 1]: 1 when the class counts before that record are not span_base's row s.
__global__ __launch_bounds__(256) void k_ecol_span(const EcolIn in, const uint64_t* __restrict__ base,
                                                  const uint64_t* __restrict__ bbase, const ColRes* __restrict__ cres,
                                                  const EcolRes* __restrict__ eres, const uint64_t* __restrict__ span_base,
                                                  uint32_t n_spans, uint64_t* __restrict__ span_out) {
  const uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (s > n_spans) return;  // (wave-uniform)
  uint64_t want[kColClasses], r = 0;
#pragma unroll
  for (uint32_t k = 0; k < kColClasses; ++k) r += want[k] = span_base[uint64_t(s) * kColClasses + k];
  uint64_t b[kColClasses], bytes = 0, at = 0;
  uint32_t c[kColClasses] = {0, 0, 0, 0, 0};
  if (r >= in.n) {  // the end of the batch: the totals
#pragma unroll
    for (uint32_t k = 0; k < kColClasses; ++k) b[k] = cres->total[k];
    at = eres->n_bytes;
  } else {
    const uint64_t tile = r / kEcolTile, t0 = tile * kEcolTile;
#pragma unroll
    for (uint32_t k = 0; k < kColClasses; ++k) b[k] = base[tile * kColClasses + k];
    at = bbase[tile];
    uint64_t run4 = b[kColWide];
    for (uint64_t i0 = t0; i0 < r; i0 += 64) {  // (wave-uniform bounds)
      const uint64_t i = i0 + lane;
      const uint32_t t = i < r ? in.tag[i] : 0xFFu, cls = col_class(t);
#pragma unroll
      for (uint32_t q = 0; q < kColClasses; ++q) c[q] += cls == q;
      const uint64_t m = __ballot(cls == kColWide);
      if (cls == kColWide) {
        const EcolRow row = ecol_row(in, t, run4 + lane_rank(m));
        bytes += ecol_len(t, row.sub, row.vl);
      } else {
        bytes += ecol_head_len(t, 0);
      }
      run4 += (uint32_t)__popcll(m);
    }
  }
  bytes = wave_sum(bytes);
  bool ok = true;
#pragma unroll
  for (uint32_t k = 0; k < kColClasses; ++k) ok = ok && b[k] + wave_sum(c[k]) == want[k];
  if (lane == 0) {
    span_out[uint64_t(s) * 2] = at + bytes;
    span_out[uint64_t(s) * 2 + 1] = ok ? 0 : 1;
  }
}

// The tile's LDS.  out holds the tile's bytes at the destination's 16-byte phase: tile byte b at
// out[a + b], a = the destination address of the tile's first byte modulo 16.
struct EcolLds {
  uint8_t out[kEcolLds] __attribute__((aligned(16)));
  uint8_t skip[kEcolLds / 16] __attribute__((aligned(16)));  // chunk j is written by a long payload's wave
  uint64_t clen[kEcolChunks];                                // the chunks' bytes, then the bytes before them
  uint64_t total;
  uint32_t cnt[kEcolChunks][kColClasses];
};

__global__ __launch_bounds__(kEcolTileThreads) void k_ecol_write(const EcolIn in, const uint64_t* __restrict__ base,
                                                            const uint64_t* __restrict__ bbase, uint64_t n_bytes,
                                                            uint8_t* __restrict__ out) {
  __shared__ EcolLds l;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t i0 = uint64_t(blockIdx.x) * kEcolTile;
  uint64_t tb[kColClasses];
#pragma unroll
  for (uint32_t c = 0; c < kColClasses; ++c) tb[c] = base[size_t(blockIdx.x) * kColClasses + c];
  const uint64_t gbase = bbase[blockIdx.x];
  for (uint32_t j = tid; j < kEcolLds / 64; j += kEcolTileThreads) reinterpret_cast<uint32_t*>(l.skip)[j] = 0;
  uint8_t tg[kEcolPer];
  ecol_tile_tags(in.tag, in.n, i0, tid, tg, l.cnt);

  // the records' lengths: the bytes before each record inside its chunk, the chunks' sums
  uint64_t excl[kEcolPer];
#pragma unroll
  for (uint32_t k = 0; k < kEcolPer; ++k) {
    const uint32_t t = tg[k], cls = col_class(t);
    const uint32_t rank = ecol_chunk_rank(cls);
    uint64_t len = ecol_head_len(t, 0);
    if (cls == kColWide) {
      const EcolRow r = ecol_row(in, t, tb[kColWide] + l.cnt[k * kEcolWaves + w][kColWide] + rank);
      len = ecol_len(t, r.sub, r.vl);
    }
    const uint64_t inc = wave_incl(len, lane);
    excl[k] = inc - len;
    if (lane == 63) l.clen[k * kEcolWaves + w] = inc;
  }
  __syncthreads();
  if (tid < kEcolChunks) {
    const uint64_t x = l.clen[tid], s = wave_incl(x, lane);
    l.clen[tid] = s - x;
    if (tid == kEcolChunks - 1) l.total = s;
  }
  __syncthreads();
  const uint64_t total = l.total;
  if (gbase > n_bytes || total > n_bytes - gbase) return;  // (not what the host checked: nothing is stored)
  uint8_t* const gdst = out + gbase;
  const uint32_t a = uint32_t(uintptr_t(gdst) & 15);
  const bool staged = total + a <= kEcolLds;  // (block-uniform)

  // the records
#pragma unroll
  for (uint32_t k = 0; k < kEcolPer; ++k) {
    const uint32_t t = tg[k], cls = col_class(t);
    const uint32_t rank = ecol_chunk_rank(cls);
    const uint64_t at = l.clen[k * kEcolWaves + w] + excl[k];  // tile-relative
    const uint64_t idx = ecol_pick(tb, cls) + l.cnt[k * kEcolWaves + w][cls < kColClasses ? cls : 0] + rank;
    bool lng = false;
    uint64_t p_at = 0, p_src = 0;  // a long payload: its tile-relative offset and its offset in var
    uint32_t p_len = 0;
    if (cls < kColClasses && idx < ecol_pick(in.n_class, cls)) {
      int64_t v0 = 0, v1 = 0;
      int32_t rc = 0;
      EcolRow r{0, 0, false};
      if (cls == kColOrder) v0 = in.order[idx];
      else if (cls == kColTimestamp) v0 = in.timestamp[idx];
      else if (cls == kColRng) v0 = in.rng[idx];
      else if (cls == kColBufferBuilt) v0 = in.buffer_built[idx];
      else {
        r = ecol_row(in, t, idx);
        v0 = in.w_v0[idx];
        if (t != CLG_TAG_SERIALIZABLE) rc = in.w_rc[idx];
        if (t == CLG_TAG_SOURCE_CHECKPOINT) v1 = in.w_v1[idx];
      }
      const uint32_t head = ecol_head_len(t, r.sub);
      if (staged) ecol_put_head(l.out, a + at, t, v0, rc, v1, r.sub, r.vl);
      else ecol_put_head(gdst, at, t, v0, rc, v1, r.sub, r.vl);
      if (r.pay && r.vl) {
        const uint64_t src = in.pos[idx];
        if (ecol_row_ok(src, r.vl, in.n_var)) {
          if (r.vl >= kEcolWaveRow) {
            lng = true, p_at = at + head, p_src = src, p_len = r.vl;
          } else if (staged) {
            for (uint32_t j = 0; j < r.vl; ++j) l.out[a + at + head + j] = in.var[src + j];
          } else {
            for (uint32_t j = 0; j < r.vl; ++j) gdst[at + head + j] = in.var[src + j];
          }
        }
      }
    }
    // the chunk's long payloads, one at a time by the whole wave
    uint64_t m = __ballot(lng);
    while (m) {  // (wave-uniform)
      const int src_lane = __builtin_ctzll(m);
      m &= m - 1;
      const uint64_t q_at = (uint64_t)__shfl((unsigned long long)p_at, src_lane, 64);
      const uint64_t q_src = (uint64_t)__shfl((unsigned long long)p_src, src_lane, 64);
      const uint32_t q_len = (uint32_t)__shfl((int)p_len, src_lane, 64);
      uint8_t* const d0 = gdst + q_at;
      const uint8_t* const s0 = in.var + q_src;
      if (!staged) {
        copy_range<64>(s0, d0, q_len, lane);
        continue;
      }
      // staged: the aligned interior directly (its chunks flagged), the edges through LDS
      const uint32_t pre = uint32_t(-uintptr_t(d0) & 15);          // bytes before the first aligned chunk
      const uint32_t mid = (q_len - pre) & ~15u;                    // (q_len >= 64: at least 48)
      const uint32_t post = q_len - pre - mid;
      copy_range<64>(s0 + pre, d0 + pre, mid, lane);
      const uint32_t lo = uint32_t(a + q_at);                       // the payload's place in l.out
      if (lane < pre) l.out[lo + lane] = s0[lane];
      if (lane >= 16 && lane - 16 < post) l.out[lo + pre + mid + (lane - 16)] = s0[pre + mid + (lane - 16)];
      for (uint32_t j = (lo + pre) / 16 + lane; j < (lo + pre + mid) / 16; j += 64) l.skip[j] = 1;
    }
  }
  if (!staged) return;
  __syncthreads();

  // the buffer out: destination-aligned 16-byte stores, byte stores in the tile's two edge chunks
  const uint32_t end = a + uint32_t(total), nch = (end + 15) / 16;
  uint8_t* const abase = gdst - a;  // 16-byte aligned
  for (uint32_t j = tid; j < nch; j += kEcolTileThreads) {
    const uint4 v = *reinterpret_cast<const uint4*>(l.out + 16 * j);
    if (16 * j >= a && 16 * j + 16 <= end) {
      if (!l.skip[j]) {
        const u32x4 nv = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(nv, reinterpret_cast<u32x4*>(abase + 16 * j));
      }
    } else {
      const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t x = 0; x < 16; ++x)
        if (16 * j + x >= a && 16 * j + x < end) abase[16 * j + x] = uint8_t(q[x >> 2] >> (8 * (x & 3)));
    }
  }
}

int launch_ecol_sizes(const EcolIn& in, uint32_t n_tiles, const uint64_t* d_base, uint64_t* d_sum, uint64_t* d_bad,
                      uint64_t* d_bbase, const ColRes* cres, EcolRes* eres, const uint64_t* d_span_base, uint32_t n_spans,
                      uint64_t* span_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n_tiles) hipLaunchKernelGGL(k_ecol_bytes, dim3(n_tiles), dim3(kEcolTileThreads), 0, st, in, d_base, d_sum, d_bad);
  hipLaunchKernelGGL(k_ecol_scan64, dim3(1), dim3(kEcolScanThreads), 0, st, d_sum, d_bad, n_tiles, d_bbase, eres);
  if (d_span_base && span_out)
    hipLaunchKernelGGL(k_ecol_span, dim3((n_spans + 1 + 3) / 4), dim3(256), 0, st, in, d_base, d_bbase, cres, eres,
                       d_span_base, n_spans, span_out);
  return launch_status(hipGetLastError());
}

int launch_ecol_write(const EcolIn& in, uint32_t n_tiles, const uint64_t* d_base, const uint64_t* d_bbase,
                      uint64_t n_bytes, uint8_t* d_out, void* stream) {
  if (!n_tiles || !n_bytes) return CLG_OK;
  hipLaunchKernelGGL(k_ecol_write, dim3(n_tiles), dim3(kEcolTileThreads), 0, (hipStream_t)stream, in, d_base, d_bbase, n_bytes,
                     d_out);
  return launch_status(hipGetLastError());
}

}  // namespace clg
