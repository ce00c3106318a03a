// slice_order.h -- the dispatch order of a batched slice's runs (clg_slice_batch), host only.
//
// A run is one request's suffix of a log; k_expand_pieces cuts the runs into pieces in run
// order and k_gather hands each XCD a contiguous range of those pieces.  In request order an
// XCD copies consumer 0's whole suffix (MBs) before consumer 1's, so the bytes the consumers
// of one log share have left its 4 MiB L2 when the next consumer reads them.  window_order
// cuts every run where the log's physical offset passes a multiple of W segments and emits
// the sub-runs by log, then window, then consumer: the consumers of one window follow one
// another while its lines are still in L2, yet W segments apart in time, not all on the same
// lines at once (strict source order, W -> 0 pieces, measured slower: DESIGN.md section 7).
//
// A sub-run is an ordinary SegSpan -- the run's segtab_off and pad, its own phys and len, dst
// moved by the bytes before it -- and a cut lies on a segment boundary, so the pieces are the
// same pieces (source, dst, len) in another order and the packed output does not change.
// No HIP here: tests/slice_order_host.cpp compiles it for tests/test_slice_order.py.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace clg {

// A run of a log's physical bytes (kernels.h, "device-side planning": its gather pieces or
// decode tiles are generated on the device).
struct SegSpan {
  uint64_t segtab_off;  // first entry of the log's segment indices in the call's table
  uint32_t phys;        // first physical byte of the run
  uint32_t len;
  uint64_t dst;         // gather: output offset of the run; decode: span index
  uint32_t first;       // first piece / tile generated for the run
  uint32_t pad;
};

// The default window: 2 MiB of the log, half of an XCD's L2, whatever the segment size (128
// segments of 16 KiB: the best plain step of the sweep in DESIGN.md section 7, where 64 to
// 256 segments all beat request order and 16 and below lose to it).  CLONOS_GATHER_WINDOW
// gives W in segments instead; 0: request order.
constexpr uint32_t kGatherWindowBytes = 2u << 20;
constexpr uint32_t default_window(uint32_t C) { return C && C < kGatherWindowBytes ? kGatherWindowBytes / C : 1u; }

// Pieces a run expands to: one per segment of C bytes it touches (len > 0).
inline uint32_t span_pieces(const SegSpan& r, uint32_t C) { return (r.phys + r.len - 1) / C - r.phys / C + 1; }

// Reorders `runs` (len > 0 each, first = the exclusive prefix of span_pieces) as above; W in
// segments of C bytes, 0: request order.  A log is known by its segtab_off, which the planner
// hands out once per log handle, rising as logs first appear in the batch: a run whose
// segtab_off is not above every earlier one shares its log.  That test is the whole cost of a
// batch in which no log has two runs (config 4's exchange: tens of thousands of requests, no
// sort, nothing allocated), which is left as it is; returns whether `runs` changed.
inline bool window_order(std::vector<SegSpan>& runs, uint32_t C, uint32_t W) {
  const size_t n = runs.size();
  if (!W || !C || n < 2) return false;
  size_t i = 1;
  for (uint64_t top = runs[0].segtab_off; i < n && runs[i].segtab_off > top; ++i) top = runs[i].segtab_off;
  if (i == n) return false;
  // group of each run: its log's rank in order of first appearance (the keys of first
  // appearances rise, so the rank is a binary search), then a counting sort by group --
  // stable, so a log's runs stay in request order
  std::vector<uint64_t> keys;
  std::vector<uint32_t> grp(n), at;
  for (size_t k = 0; k < n; ++k) {
    const uint64_t key = runs[k].segtab_off;
    if (keys.empty() || key > keys.back()) keys.push_back(key);
    grp[k] = uint32_t(std::lower_bound(keys.begin(), keys.end(), key) - keys.begin());
  }
  at.assign(keys.size() + 1, 0);
  for (size_t k = 0; k < n; ++k) ++at[grp[k] + 1];
  for (size_t g = 0; g < keys.size(); ++g) at[g + 1] += at[g];
  std::vector<uint32_t> by_log(n);
  {
    std::vector<uint32_t> fill(at.begin(), at.end() - 1);
    for (size_t k = 0; k < n; ++k) by_log[fill[grp[k]]++] = uint32_t(k);
  }
  const uint64_t win = uint64_t(W) * C;  // window bytes (64 bits: W may exceed any log)
  std::vector<SegSpan> out;
  out.reserve(n * 2);
  uint32_t first = 0;
  for (size_t g = 0; g < keys.size(); ++g) {
    uint64_t w0 = UINT64_MAX, w1 = 0;  // the windows the log's runs touch
    for (uint32_t j = at[g]; j < at[g + 1]; ++j) {
      const SegSpan& r = runs[by_log[j]];
      w0 = std::min(w0, r.phys / win);
      w1 = std::max(w1, (uint64_t(r.phys) + r.len - 1) / win);
    }
    for (uint64_t w = w0; w <= w1; ++w) {
      for (uint32_t j = at[g]; j < at[g + 1]; ++j) {
        const SegSpan& r = runs[by_log[j]];
        const uint64_t s = std::max<uint64_t>(r.phys, w * win), e = std::min(uint64_t(r.phys) + r.len, (w + 1) * win);
        if (s >= e) continue;
        SegSpan sub{r.segtab_off, uint32_t(s), uint32_t(e - s), r.dst + (s - r.phys), first, r.pad};
        first += span_pieces(sub, C);
        out.push_back(sub);
      }
    }
  }
  runs.swap(out);
  return true;
}

}  // namespace clg
