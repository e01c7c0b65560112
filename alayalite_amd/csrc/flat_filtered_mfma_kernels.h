// Exact filtered k-NN on the MFMA scan (flat_filtered_mfma_kernels.hip), for masks that allow a large share of
// the rows: every row of the index is streamed as 32-row tiles -- a tile is one word of (mask AND validity AND
// below n) -- through the range MFMA scan's bf16 hi/lo split contraction, and a (query, row) pair gets the
// reference-order f32 distance only when flat_range_bound.h cannot prove it behind the query's k-th best so far.
// The partial lists are flat_filtered_scan_kernel's (chunks x nq x k, ascending by (distance, id), empty slots
// (0xffffffff, FLT_MAX)), so flat_filtered_merge_kernel runs unchanged on them.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "flat_filtered_kernels.h"

namespace alaya_amd {

struct FlatFilteredMfmaPlan {
  uint64_t chunk_rows;     // rows of the index per chunk, a multiple of kMfmaScanTileRows (exact_scan_plan.h)
  uint64_t chunks;         // row chunks (0 when n is 0)
  uint64_t sub_queries;    // queries per scan launch, a multiple of kMfmaScanQueries
  uint64_t partial_bytes;  // chunks x min(nq, sub_queries) x k (distance, id) pairs
};

// Pure host arithmetic.  n: the index's rows (the scan walks all of them; the mask words pick the eligible).
FlatFilteredMfmaPlan flat_filtered_mfma_plan(uint64_t n, uint64_t nq, uint32_t k, uint32_t cus);

struct FlatFilteredMfmaParams {
  const float *base;        // n x stride f32 rows
  const float *norms;       // L2: |b|^2 per row; IP: unused
  uint64_t n;
  uint32_t dim, stride;
  int ip;
  float max_norm;
  const float *queries;     // as FlatFilteredParams
  uint32_t q_stride;
  const uint32_t *q_list;
  uint64_t q_first;
  uint64_t nq;              // queries of this launch
  const uint32_t *words;    // the mask's words, (n + 31) / 32 of them
  const uint32_t *valid;    // the validity words, or null
  uint64_t chunk_rows, chunks;
  uint32_t k;
  float *qpad;              // (nq rounded up to 128) x qwidth: the launch's queries, zero padded (prepare)
  uint32_t qwidth;
  float *qmeta;             // 2 x (nq rounded up): |q|^2 and the first threshold, +inf; past nq: 0, -inf (prepare)
  float *part_d;            // as FlatFilteredParams: chunks x nq x k
  uint32_t *part_i;
  uint32_t *wave_stats;     // chunks x (nq rounded up) / 32 x 2: pairs verified, pairs inserted
  unsigned long long *stats;  // the two sums over the launches of a call (the reduction adds to them)
};

// pads the launch's queries and computes their norms
hipError_t launch_flat_filtered_mfma_prepare(const FlatFilteredMfmaParams &p, hipStream_t s);
// the scan, then the reduction of its per-wave counters into p.stats
hipError_t launch_flat_filtered_mfma_scan(const FlatFilteredMfmaParams &p, hipStream_t s);
hipError_t launch_flat_filtered_mfma_clear(unsigned long long *stats, hipStream_t s);

}  // namespace alaya_amd
