// Exact filtered k-NN: a row-reusing f32 scan over the rows a mask allows (flat_filtered_kernels.hip).
// Compaction of (mask AND validity) into an ascending id list, a scan over query tiles x ranges of
// that list in the reference's f32 summation order, and a merge of the per-range lists.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "exact_scan_plan.h"

namespace alaya_amd {

constexpr uint32_t kFilteredMaxK = 224;
constexpr size_t kFilteredPartialCap = size_t(256) << 20;  // bytes of partial lists per scan launch

struct FlatFilteredPlan {
  uint64_t chunk_rows;     // id-list entries per row chunk, a multiple of kScanPassRows
  uint64_t chunks;         // row chunks (0 when nothing is allowed)
  uint64_t tile;           // queries per workgroup (0: the shape does not fit the LDS)
  uint64_t sub_queries;    // queries per scan launch, a multiple of the tile
  uint64_t partial_bytes;  // chunks x min(nq, sub_queries) x k (distance, id) pairs
};

// Pure host arithmetic (no device call).  forced_rows: 0, or the diagnostics' rows per chunk.
FlatFilteredPlan flat_filtered_plan(uint64_t n_allowed, uint64_t nq, uint32_t k, uint32_t stride, uint32_t cus,
                                    uint64_t forced_rows);
// LDS bytes of one scan workgroup
size_t flat_filtered_lds(uint32_t tile, uint32_t stride, uint32_t k);

struct FlatFilteredParams {
  const float *base;        // n x stride f32 rows
  uint32_t dim, stride;
  int ip;                   // 1 = -(q.b) in ip_sqr_avx2's order, 0 = l2_sqr_avx2's
  const float *queries;     // rows of q_stride floats
  uint32_t q_stride;
  const uint32_t *q_list;   // query j of this launch is row q_list[q_first + j] of `queries` and of the
  uint64_t q_first;         // outputs; q_list null = row q_first + j
  uint64_t nq;              // queries of this launch
  const uint32_t *ids;      // the mask's ascending allowed valid ids
  uint64_t n_ids;
  uint64_t chunk_rows, chunks;
  uint32_t tile, k;
  float *part_d;            // chunks x nq x k, each list ascending by (distance, id)
  uint32_t *part_i;
  uint32_t *out_ids;        // (rows of `queries`) x k
  float *out_dists;         // nullable
};

// words: one mask's ceil(n / 32) words; valid: the validity bitmap or null (every row valid).
// block_sums: scratch of flat_filtered_blocks(n) + 1 words.  Writes the ascending ids of the set bits
// of (words AND valid) below n to `ids` and their count to *count (device memory).
uint64_t flat_filtered_blocks(uint64_t n);
hipError_t launch_flat_filtered_compact(const uint32_t *words, const uint32_t *valid, uint64_t n, uint32_t *block_sums,
                                        uint32_t *ids, uint32_t *count, hipStream_t s);
hipError_t launch_flat_filtered_scan(const FlatFilteredParams &p, hipStream_t s);
// chunks == 0: every slot of the launch's queries is written empty
hipError_t launch_flat_filtered_merge(const FlatFilteredParams &p, hipStream_t s);

}  // namespace alaya_amd
