// Exact k-NN over per-query candidate lists: a gather-and-select scan (flat_lists_kernels.hip).
// Each query brings its own list of row ids (CSR: lims, ids).  The lists are cut into pieces of at most
// `piece` entries, one wave scans one piece against that piece's query in the reference's f32 summation
// order and keeps its k best, and one wave per query merges that query's pieces.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "exact_scan_plan.h"

namespace alaya_amd {

constexpr uint32_t kListsMaxK = 224;
constexpr size_t kListsPartialCap = size_t(256) << 20;  // bytes of partial lists per scan launch
constexpr uint32_t kListsPassRows = 8;                  // candidates one wave takes per pass: one per lane group
constexpr uint32_t kListsWaves = 4;                     // waves (pieces) per scan workgroup
constexpr uint32_t kListsMinPiece = 64, kListsMaxPiece = 1024;

struct FlatListsPlan {
  uint64_t piece;          // list entries per piece, a multiple of kListsPassRows
  uint64_t sub_queries;    // queries per launch (0: the shape does not fit the LDS)
  uint64_t table;          // piece-table entries of one launch: total / piece + min(nq, sub_queries)
  uint64_t partial_bytes;  // table x k (distance, id) pairs
  uint64_t launches;       // ceil(nq / sub_queries)
};

// Pure host arithmetic (no device call).  total: list entries of the whole call -- a launch's queries hold at
// most that many, so every launch's table is sized for it and nothing is read back.  forced_piece: 0, or the
// diagnostics' piece length (rounded up to whole passes, honoured whatever the cap).
FlatListsPlan flat_lists_plan(uint64_t total, uint64_t nq, uint32_t k, uint32_t stride, uint32_t cus, uint64_t forced_piece);
// LDS bytes of one scan workgroup: a padded query and a list of k per wave
size_t flat_lists_lds(uint32_t stride, uint32_t k);

struct FlatListsPiece {
  uint64_t first;  // of `ids`
  uint32_t query;  // of the launch
  uint32_t count;  // 0: an unused table entry
};

struct FlatListsParams {
  const float *base;      // n x stride f32 rows
  uint64_t n;
  const uint32_t *valid;  // the validity bitmap or null (every row valid)
  uint32_t dim, stride;
  int ip;                 // 1 = -(q.b) in ip_sqr_avx2's order, 0 = l2_sqr_avx2's
  const float *queries;   // rows of q_stride floats
  uint32_t q_stride;
  uint64_t q_first;       // query j of this launch is row q_first + j of `queries`, `lims` and the outputs
  uint64_t nq;            // queries of this launch
  const int64_t *lims;    // query i's candidates are ids[lims[i] .. lims[i + 1]), ends clamped to [0, total]
  const uint32_t *ids;
  uint64_t total;
  uint32_t piece, k;
  uint64_t table;         // entries of `pieces`, part_d / k and part_i / k
  uint64_t *first_piece;  // nq + 1: the exclusive scan of the queries' piece counts
  FlatListsPiece *pieces;
  float *part_d;          // table x k, each list ascending by (distance, id)
  uint32_t *part_i;
  uint32_t *out_ids;      // (rows of `queries`) x k
  float *out_dists;       // nullable
};

// first_piece and the table: pieces past `table` (lims that are not non-decreasing can ask for them) are dropped
hipError_t launch_flat_lists_pieces(const FlatListsParams &p, hipStream_t s);
hipError_t launch_flat_lists_scan(const FlatListsParams &p, hipStream_t s);
hipError_t launch_flat_lists_merge(const FlatListsParams &p, hipStream_t s);

}  // namespace alaya_amd
