// Host build of clonos_amd/csrc/slice_order.h for tests/test_slice_order.py (no HIP): the
// windowed dispatch order of a batched slice's runs, behind a C ABI.
#include "../clonos_amd/csrc/slice_order.h"

#include <string.h>

extern "C" {
// runs: n SegSpan (32 bytes each, the layout of kernels.h); the reordered runs are written to
// out (room for cap) and their number returned, or -1 when cap is short; *changed: whether
// window_order reordered.
int64_t so_window_order(const clg::SegSpan* runs, uint64_t n, uint32_t C, uint32_t W, clg::SegSpan* out, uint64_t cap,
                        int32_t* changed) {
  std::vector<clg::SegSpan> v(runs, runs + n);
  *changed = clg::window_order(v, C, W) ? 1 : 0;
  if (v.size() > cap) return -1;
  if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(clg::SegSpan));
  return int64_t(v.size());
}
uint32_t so_span_bytes() { return uint32_t(sizeof(clg::SegSpan)); }
uint32_t so_default_window(uint32_t C) { return clg::default_window(C); }
}
