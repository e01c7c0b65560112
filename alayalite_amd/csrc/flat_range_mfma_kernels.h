// Exact range search on the MFMA scan (flat_range_mfma_kernels.hip): the rows of one mask are scanned as whole
// 32-row tiles -- a tile is one word of (mask AND validity AND below n) -- with the bf16 hi/lo split
// contraction; two per-query thresholds (flat_range_bound.h) prove most (query, row) pairs in or out, and the
// rest are decided by the reference-order f32 distance.  The partial lists and counts are
// flat_range_scan_kernel's, so flat_range_gather_kernel and range_sort_kernel run unchanged.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "flat_range_kernels.h"

namespace alaya_amd {

struct FlatRangeMfmaPlan {
  uint64_t chunk_rows;     // rows per chunk, a multiple of kMfmaScanTileRows (exact_scan_plan.h)
  uint64_t chunks;         // row chunks (0 when n is 0)
  uint64_t sub_queries;    // queries per scan launch, a multiple of kMfmaScanQueries
  uint64_t slots;          // stored hits per (chunk, query): min(cap, chunk_rows)
  uint64_t staging_bytes;  // chunks x min(nq rounded up, sub_queries) x (slots pairs + one count)
};

// Pure host arithmetic.  n: the index's rows (the scan walks all of them; the mask words pick the eligible).
FlatRangeMfmaPlan flat_range_mfma_plan(uint64_t n, uint64_t nq, uint32_t cap, uint32_t cus);

struct FlatRangeMfmaParams {
  const float *base;        // n x stride f32 rows
  const float *norms;       // L2: |b|^2 per row; IP: unused
  uint64_t n;
  uint32_t dim, stride;
  int ip;
  float max_norm;
  const float *queries;     // as FlatRangeParams
  uint32_t q_stride;
  const float *radii;
  const uint32_t *q_list;
  uint64_t q_first;
  uint64_t nq;              // queries of this launch
  const uint32_t *words;    // the mask's words, (n + 31) / 32 of them
  const uint32_t *valid;    // the validity words, or null
  uint64_t chunk_rows, chunks;
  uint32_t cap, slots;
  float *qpad;              // (nq rounded up to 128) x qwidth: the launch's queries, zero padded (prepare)
  uint32_t qwidth;
  float *qmeta;             // 4 x (nq rounded up): |q|^2, lo, hi, radius; past nq: 0, -inf, -inf, -inf (prepare)
  uint32_t *part_n;         // as FlatRangeParams
  uint32_t *part_i;
  float *part_d;
  uint32_t *wave_stats;     // chunks x (nq rounded up) / 32 x 3: pairs verified, band pairs, pairs proven
  unsigned long long *stats;  // the three sums over the launches of a call (the reduction adds to them)
};

// pads the launch's queries and computes their norms and thresholds
hipError_t launch_flat_range_mfma_prepare(const FlatRangeMfmaParams &p, hipStream_t s);
// the scan, then the reduction of its per-wave counters into p.stats
hipError_t launch_flat_range_mfma_scan(const FlatRangeMfmaParams &p, hipStream_t s);
hipError_t launch_flat_range_mfma_clear(unsigned long long *stats, hipStream_t s);

}  // namespace alaya_amd
