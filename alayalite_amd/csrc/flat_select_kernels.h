// Exact k-NN above the register-list limit: selection by histogram on the MFMA scan (flat_select_kernels.hip).
// A scan in flat_range_mfma_kernel's work split counts, per query, the approximate distances d~ of the eligible
// rows into the bins of a window [lo, hi); a pick kernel finds the bin that holds rank k and makes it the next
// window, until the edge e above rank k admits few rows more than k.  The smallest radius whose proven-inside
// threshold (flat_range_bound.h) reaches e then goes to the exact range scan, whose sorted lists are cut at k.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "flat_range_mfma_kernels.h"

namespace alaya_amd {

constexpr uint32_t kSelectBins = 256;               // bins per query and pass
constexpr uint32_t kSelectPitch = kSelectBins + 1;  // counters per query: the bins, then `below`
constexpr uint32_t kSelectMaxK = kFlatRangeMaxCap / 2;  // 2048: the threshold bin and ties keep room under the cap
constexpr uint32_t kSelectMaxPasses = 4;            // full histogram passes of one call, at most
// LDS of one histogram workgroup beside the 18 KB of tile buffers: 128 histograms and the 128 windows
constexpr size_t kSelectHistLds = size_t(kMfmaScanQueries) * kSelectPitch * 4 + size_t(kMfmaScanQueries) * 3 * 4;

// Query states (FlatSelectParams::done)
constexpr uint32_t kSelectRunning = 0, kSelectDone = 1, kSelectFallback = 2;

// the narrowing stops at an edge that admits at most this many rows: a quarter more than k (at least 64 more)
// keeps the range scan's verified pairs near k per query, and one pass of 256 bins over a proposed window
// nearly always reaches it ("Round 27")
inline uint32_t flat_select_target(uint32_t k) {
  const uint32_t t = k + (k / 4 > 64 ? k / 4 : 64);
  return t < kFlatRangeMaxCap ? t : kFlatRangeMaxCap;
}

// super-tiles between two sampled ones, for a sample of about max(32 k, 65536) rows of n
inline uint32_t flat_select_sample_step(uint64_t n, uint32_t k) {
  const uint64_t want = 32ull * k > 65536 ? 32ull * k : 65536;
  const uint64_t step = n / want;
  return step < 1 ? 1u : (step > 0xffffu ? 0xffffu : static_cast<uint32_t>(step));
}

struct FlatSelectParams {
  const float *base;      // n x stride f32 rows
  const float *norms;     // L2: |b|^2 per row; IP: unused
  uint64_t n;
  uint32_t dim, stride;
  int ip;
  float max_norm;
  const uint32_t *valid;  // the validity words, or null: every row below n is eligible
  uint64_t chunk_rows, chunks;  // flat_range_mfma_plan's
  uint32_t sup_step;      // 1: every super-tile of a chunk; s: every s-th (a row sample)
  int span;               // 1: the span mode
  uint64_t nq;
  const float *qpad;      // flat_range_mfma_prepare_kernel's padded queries and |q|^2
  uint32_t qwidth;
  const float *qmeta;
  // per query, (nq rounded up to 128) entries each
  float *win;             // 3 x: lo, hi, inverse bin width
  uint32_t *hist;         // x kSelectPitch
  uint32_t *span_keys;    // 2 x: min and max of d~ as ordered keys
  uint32_t *eligible;     // one counter: eligible rows the span scan met
  float *edge;            // the smallest edge found with at least k rows below it
  uint32_t *cum;          // rows below `edge`
  uint32_t *done;         // kSelectRunning / Done / Fallback
  float *radii;           // nq: the range scan's radii
};

hipError_t launch_flat_select_init(const FlatSelectParams &p, hipStream_t s);    // span keys, eligible, done, windows
hipError_t launch_flat_select_scan(const FlatSelectParams &p, hipStream_t s);    // span or histogram, by p.span
hipError_t launch_flat_select_window(const FlatSelectParams &p, hipStream_t s);  // the first window, from the span
hipError_t launch_flat_select_clear(const FlatSelectParams &p, hipStream_t s);   // zero histograms
// sample != 0: the counts are a row sample's; they propose the window [lo, edge) and decide nothing
hipError_t launch_flat_select_pick(const FlatSelectParams &p, uint32_t k, uint32_t target, int sample, hipStream_t s);
hipError_t launch_flat_select_radius(const FlatSelectParams &p, int all_inf, hipStream_t s);
// the first k of each sorted list of `cap` slots; past min(counts, k): (0xffffffff, FLT_MAX)
hipError_t launch_flat_select_cut(const uint32_t *counts, const uint32_t *ids, const float *dists, uint32_t cap, uint64_t nq,
                                  uint32_t k, uint32_t *out_ids, float *out_dists, hipStream_t s);

}  // namespace alaya_amd
