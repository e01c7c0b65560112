// Exact range search: every eligible row within a radius, by a row-reusing f32 scan (flat_range_kernels.hip).
// The id list is the exact filtered scan's (launch_flat_filtered_compact); the scan compares each
// reference-order f32 distance with the query's radius and appends the hits, in id-list order, to a
// partial list per (row chunk, query); a gather concatenates the chunk lists in chunk order.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "exact_scan_plan.h"

namespace alaya_amd {

constexpr uint32_t kFlatRangeMaxCap = 4096;    // stored hits per query
constexpr size_t kFlatRangeStagingCap = size_t(256) << 20;  // bytes of partial lists and counts per scan launch

struct FlatRangePlan {
  uint64_t chunk_rows;     // id-list entries per row chunk, a multiple of kScanPassRows
  uint64_t chunks;         // row chunks (0 when no row is eligible)
  uint64_t tile;           // queries per workgroup (0: the queries do not fit the LDS)
  uint64_t sub_queries;    // queries per scan launch, a multiple of the tile
  uint64_t slots;          // stored hits per (chunk, query): min(cap, chunk_rows)
  uint64_t staging_bytes;  // chunks x min(nq, sub_queries) x (slots pairs + one count)
};

// Pure host arithmetic (no device call).  forced_rows: 0, or the diagnostics' rows per chunk;
// forced_staging: 0, or the diagnostics' staging cap in bytes (raised to what one tile of one chunk needs).
FlatRangePlan flat_range_plan(uint64_t n_eligible, uint64_t nq, uint32_t cap, uint32_t stride, uint32_t cus,
                              uint64_t forced_rows, uint64_t forced_staging);
// LDS bytes of one scan workgroup: the tile's queries
size_t flat_range_lds(uint32_t tile, uint32_t stride);

struct FlatRangeParams {
  const float *base;        // n x stride f32 rows
  uint32_t dim, stride;
  int ip;                   // 1 = -(q.b) in ip_sqr_avx2's order, 0 = l2_sqr_avx2's
  const float *queries;     // rows of q_stride floats
  uint32_t q_stride;
  const float *radii;       // one per row of `queries`: a hit has d <= radius
  const uint32_t *q_list;   // query j of this launch is row q_list[q_first + j] of `queries`, `radii` and of
  uint64_t q_first;         // the outputs; q_list null = row q_first + j
  uint64_t nq;              // queries of this launch
  const uint32_t *ids;      // the ascending eligible ids
  uint64_t n_ids;
  uint64_t chunk_rows, chunks;
  uint32_t tile, cap, slots;
  uint32_t *part_n;         // chunks x nq: hits of (chunk, query), not capped
  uint32_t *part_i;         // chunks x nq x slots: the first min(hits, slots) in id-list order
  float *part_d;
  uint32_t *out_counts;     // (rows of `queries`): hits, not capped
  uint32_t *out_ids;        // (rows of `queries`) x cap: the first min(hits, cap) in id order, then empty slots
  float *out_dists;
};

hipError_t launch_flat_range_scan(const FlatRangeParams &p, hipStream_t s);
// chunks == 0: counts of 0 and empty slots for the launch's queries
hipError_t launch_flat_range_gather(const FlatRangeParams &p, hipStream_t s);

}  // namespace alaya_amd
