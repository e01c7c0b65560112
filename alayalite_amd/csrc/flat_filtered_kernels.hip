// Exact filtered k-NN for small allowed shares: skip the graph, scan the allowed rows exactly.
//
// Stands in for the reference's exact search (find_exact_gt, include/utils/evaluate.hpp:29-62) over
// the subset of rows that are valid and that a mask allows.  Every distance is computed in f32 in
// the reference's summation order from the start (l2_sqr_avx2 / ip_sqr_avx2, restated in
// exact_scan_device.h), so there is no approximate contraction, no bound, no flag and no host recompute --
// unlike the MFMA flat scan of flat_kernels.hip, whose exact_l2 / exact_ip give the same bits.
//
//   1. compaction  (mask AND validity) -> ascending id list + count: word popcounts, an exclusive scan
//                  of the per-block sums, a scatter.
//   2. scan        grid = row chunks (ranges of the id list) x query tiles; the distance pass is
//                  exact_scan_device.h's, shared with the exact range scan.  Each wave keeps its queries'
//                  k best by (distance, id) as sorted lists in LDS and writes them out at the end.
//   3. merge       one wave per query folds the chunk lists into the k outputs, empty slots
//                  (all-ones id, FLT_MAX).
//
// No workgroup waits for another.
#include "flat_filtered_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "exact_scan_device.h"

namespace alaya_amd {

using namespace exact_scan;

namespace {

constexpr uint32_t kEmptyId = 0xffffffffu;
constexpr int kCompactBlock = 256;  // threads = mask words per compaction block

__device__ __forceinline__ void ff_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// (distance, id) total order of every selection: smaller distance first, then smaller id
__device__ __forceinline__ bool ff_before(float da, uint32_t ia, float db, uint32_t ib) {
  return (da < db) | ((da == db) & (ia < ib));
}

// ---- compaction ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ff_word(const uint32_t *words, const uint32_t *valid, uint64_t n, uint64_t w) {
  const uint64_t n_words = (n + 31) / 32;
  if (w >= n_words) return 0u;
  uint32_t x = words[w];
  if (valid) x &= valid[w];
  // bits at positions >= n are ignored, whatever they hold
  if (w == n_words - 1 && (n & 31)) x &= (1u << (n & 31)) - 1u;
  return x;
}

// exclusive scan of one value per thread over a block of 256; total = the block's sum
__device__ __forceinline__ uint32_t ff_block_scan(uint32_t v, uint32_t *wave_tot, uint32_t &total) {
  const int lane = __lane_id(), wave = threadIdx.x >> 6;
  uint32_t incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  uint32_t pre = 0;
  total = 0;
  for (int w = 0; w < kCompactBlock / 64; ++w) {
    const uint32_t t = wave_tot[w];
    pre += w < wave ? t : 0u;
    total += t;
  }
  __syncthreads();
  return pre + incl - v;
}

__global__ void __launch_bounds__(kCompactBlock) flat_filtered_count_kernel(const uint32_t *words, const uint32_t *valid,
                                                                            uint64_t n, uint32_t *block_sums) {
  __shared__ uint32_t wave_tot[kCompactBlock / 64];
  const uint64_t w = static_cast<uint64_t>(blockIdx.x) * kCompactBlock + threadIdx.x;
  uint32_t total = 0;
  (void)ff_block_scan(__popc(ff_word(words, valid, n, w)), wave_tot, total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one block: block_sums[0 .. blocks) -> their exclusive scan, block_sums[blocks] = *count = the sum
__global__ void __launch_bounds__(kCompactBlock) flat_filtered_offsets_kernel(uint32_t *block_sums, uint64_t blocks,
                                                                              uint32_t *count) {
  __shared__ uint32_t wave_tot[kCompactBlock / 64];
  uint32_t running = 0;
  for (uint64_t b0 = 0; b0 < blocks; b0 += kCompactBlock) {
    const uint64_t b = b0 + threadIdx.x;
    const uint32_t v = b < blocks ? block_sums[b] : 0u;
    uint32_t total = 0;
    const uint32_t ex = ff_block_scan(v, wave_tot, total);
    if (b < blocks) block_sums[b] = running + ex;
    running += total;
  }
  if (threadIdx.x == 0) {
    block_sums[blocks] = running;
    *count = running;
  }
}

__global__ void __launch_bounds__(kCompactBlock) flat_filtered_scatter_kernel(const uint32_t *words, const uint32_t *valid,
                                                                              uint64_t n, const uint32_t *block_sums,
                                                                              uint32_t *ids) {
  __shared__ uint32_t wave_tot[kCompactBlock / 64];
  const uint64_t w = static_cast<uint64_t>(blockIdx.x) * kCompactBlock + threadIdx.x;
  uint32_t x = ff_word(words, valid, n, w);
  uint32_t total = 0;
  // the id list holds block_sums[blocks] <= n entries: every write below lands inside it
  uint32_t o = block_sums[blockIdx.x] + ff_block_scan(__popc(x), wave_tot, total);
  while (x) {
    const int b = __ffs(x) - 1;
    x &= x - 1;
    ids[o++] = static_cast<uint32_t>(w * 32 + b);
  }
}

// ---- sorted (distance, id) lists of k entries in LDS, one wave ------------------------------------
// Insert (d, id), which is before the list's last entry: every lane holds entries lane, lane + 64, ...
// (k <= 256), the ones not before the newcomer move up by one and the last drops out.
__device__ __forceinline__ void ff_insert(float *Ld, uint32_t *Li, uint32_t k, float d, uint32_t id, int lane) {
  float ed[4];
  uint32_t ei[4];
  uint32_t pos = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t e = lane + 64 * r;
    ed[r] = FLT_MAX;
    ei[r] = kEmptyId;
    if (e < k) {
      ed[r] = Ld[e];
      ei[r] = Li[e];
    }
    pos += __popcll(__ballot(e < k && ff_before(ed[r], ei[r], d, id)));
  }
  ff_wave_fence();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t e = lane + 64 * r;
    if (e >= pos && e + 1 < k) {
      Ld[e + 1] = ed[r];
      Li[e + 1] = ei[r];
    }
  }
  if (lane == 0) {  // pos < k: the caller checked the newcomer against entry k - 1
    Ld[pos] = d;
    Li[pos] = id;
  }
  ff_wave_fence();
}

}  // namespace

template <bool kIp>
__global__ void __launch_bounds__(256) flat_filtered_scan_kernel(FlatFilteredParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tile = p.tile, stride = p.stride, k = p.k;
  float *qs = reinterpret_cast<float *>(smem);                  // tile x stride, zero padded
  float *ld = qs + static_cast<size_t>(tile) * stride;          // tile x k
  uint32_t *li = reinterpret_cast<uint32_t *>(ld + tile * k);   // tile x k
  const uint64_t q_tiles = (p.nq + tile - 1) / tile;
  const uint64_t chunk = blockIdx.x / q_tiles;
  const uint64_t q0 = (blockIdx.x % q_tiles) * tile;  // first query (of the launch) of this tile
  load_query_tile(qs, tile, stride, p.dim, p.queries, p.q_stride, p.q_list, p.q_first, q0, p.nq);
  for (uint32_t i = threadIdx.x; i < tile * k; i += blockDim.x) {
    ld[i] = FLT_MAX;
    li[i] = kEmptyId;
  }
  __syncthreads();
  const int lane = __lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t g = lane >> 3, m = lane & 7;
  if (q0 + kQueries * wave >= p.nq) return;  // (no barrier below)
  const float *q = qs + static_cast<size_t>(kQueries) * wave * stride;
  float *Ld0 = ld + kQueries * wave * k;
  uint32_t *Li0 = li + kQueries * wave * k;
  const uint64_t r0 = chunk * p.chunk_rows;
  const uint64_t r1 = r0 + p.chunk_rows < p.n_ids ? r0 + p.chunk_rows : p.n_ids;  // r0 < r1: chunks cover n_ids
  const uint32_t T = p.dim >> 5;
  const uint32_t nb8 = (p.dim - 32 * T) >> 3;
  const uint32_t tail0 = 32 * T + 8 * nb8;
  for (uint64_t pb = r0; pb < r1; pb += kScanPassRows) {
    uint32_t rid[kRows];
    bool ok[kRows];
    float dist[kRows][kQueries];
    pass<kIp>(p.ids, p.base, pb, r0, r1, q, p.dim, stride, T, nb8, tail0, g, m, dist, rid, ok);
    // every lane of a group holds its rows' 16 distances; lane 0 of the group offers them
#pragma unroll
    for (int c = 0; c < kQueries; ++c) {
      if (q0 + kQueries * wave + c >= p.nq) continue;
      float *Ld = Ld0 + c * k;
      uint32_t *Li = Li0 + c * k;
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        const float d = dist[j][c];
        uint64_t offer = __ballot(m == 0 && ok[j] && ff_before(d, rid[j], Ld[k - 1], Li[k - 1]));
        while (offer) {
          const int src = __ffsll(static_cast<unsigned long long>(offer)) - 1;
          offer &= offer - 1;
          const float cd = __shfl(d, src);
          const uint32_t ci = __shfl(rid[j], src);
          if (ff_before(cd, ci, Ld[k - 1], Li[k - 1])) ff_insert(Ld, Li, k, cd, ci, lane);
        }
      }
    }
  }
  ff_wave_fence();
#pragma unroll
  for (int c = 0; c < kQueries; ++c) {
    const uint64_t qi = q0 + kQueries * wave + c;
    if (qi >= p.nq) continue;
    const uint64_t o = (chunk * p.nq + qi) * k;
    for (uint32_t e = lane; e < k; e += 64) {
      p.part_d[o + e] = Ld0[c * k + e];
      p.part_i[o + e] = Li0[c * k + e];
    }
  }
}

// One wave per query: fold the chunk lists (each ascending by (distance, id)) into one list of k and
// write it.  A chunk's entry that is not before the list's last ends that chunk: the rest are later.
__global__ void __launch_bounds__(64) flat_filtered_merge_kernel(FlatFilteredParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t k = p.k;
  float *Ld = reinterpret_cast<float *>(smem);
  uint32_t *Li = reinterpret_cast<uint32_t *>(Ld + k);
  const int lane = __lane_id();
  for (uint64_t qi = blockIdx.x; qi < p.nq; qi += gridDim.x) {
    for (uint32_t e = lane; e < k; e += 64) {
      Ld[e] = FLT_MAX;
      Li[e] = kEmptyId;
    }
    ff_wave_fence();
    for (uint64_t c = 0; c < p.chunks; ++c) {
      const uint64_t o = (c * p.nq + qi) * k;
      bool open = true;
      for (uint32_t e0 = 0; e0 < k && open; e0 += 64) {
        const uint32_t e = e0 + lane;
        const float d = e < k ? p.part_d[o + e] : FLT_MAX;
        const uint32_t id = e < k ? p.part_i[o + e] : kEmptyId;
        uint64_t offer = __ballot(e < k && ff_before(d, id, Ld[k - 1], Li[k - 1]));
        if (offer != __ballot(e < k)) open = false;  // an entry lost: so do the later ones
        while (offer) {
          const int src = __ffsll(static_cast<unsigned long long>(offer)) - 1;
          offer &= offer - 1;
          const float cd = __shfl(d, src);
          const uint32_t ci = __shfl(id, src);
          if (!ff_before(cd, ci, Ld[k - 1], Li[k - 1])) {
            open = false;
            break;
          }
          ff_insert(Ld, Li, k, cd, ci, lane);
        }
      }
    }
    // query_row(), spelled out: behind a call the compiler lays this kernel's blocks out in another order
    const uint64_t dst = (p.q_list ? p.q_list[p.q_first + qi] : p.q_first + qi) * k;
    for (uint32_t e = lane; e < k; e += 64) {
      p.out_ids[dst + e] = Li[e];
      if (p.out_dists) p.out_dists[dst + e] = Ld[e];
    }
    ff_wave_fence();
  }
}

// ---- host side -------------------------------------------------------------------------------------
size_t flat_filtered_lds(uint32_t tile, uint32_t stride, uint32_t k) {
  return static_cast<size_t>(tile) * (static_cast<size_t>(stride) * 4 + static_cast<size_t>(k) * 8);
}

FlatFilteredPlan flat_filtered_plan(uint64_t n_allowed, uint64_t nq, uint32_t k, uint32_t stride, uint32_t cus,
                                    uint64_t forced_rows) {
  FlatFilteredPlan r{};
  k = std::max<uint32_t>(k, 1);
  cus = std::max<uint32_t>(cus, 1);
  const uint32_t tile = scan_tile(nq, [&](uint32_t t) { return flat_filtered_lds(t, stride, k); });
  if (tile == 0) return r;  // does not fit
  r.tile = tile;
  uint64_t chunk_rows = scan_chunk_rows(n_allowed, nq, tile, cus, forced_rows);
  // one query tile's lists stay under the cap (only a forced chunk size can ask for more)
  const uint64_t cap_chunks = kFilteredPartialCap / (static_cast<uint64_t>(tile) * k * 8);
  if ((n_allowed + chunk_rows - 1) / chunk_rows > cap_chunks)
    chunk_rows = kScanPassRows * ((scan_passes(n_allowed) + cap_chunks - 1) / cap_chunks);
  r.chunk_rows = chunk_rows;
  r.chunks = (n_allowed + chunk_rows - 1) / chunk_rows;
  r.sub_queries = scan_sub_queries(nq, tile, r.chunks, kFilteredPartialCap, k * 8ull);  // >= tile by cap_chunks
  r.partial_bytes = r.chunks * std::min<uint64_t>(nq, r.sub_queries) * k * 8;
  return r;
}

uint64_t flat_filtered_blocks(uint64_t n) {
  const uint64_t words = (n + 31) / 32;
  return (words + kCompactBlock - 1) / kCompactBlock;
}

hipError_t launch_flat_filtered_compact(const uint32_t *words, const uint32_t *valid, uint64_t n, uint32_t *block_sums,
                                        uint32_t *ids, uint32_t *count, hipStream_t s) {
  const uint64_t blocks = flat_filtered_blocks(n);
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  if (blocks)
    hipLaunchKernelGGL(flat_filtered_count_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kCompactBlock), 0, s, words,
                       valid, n, block_sums);
  hipLaunchKernelGGL(flat_filtered_offsets_kernel, dim3(1), dim3(kCompactBlock), 0, s, block_sums, blocks, count);
  if (blocks)
    hipLaunchKernelGGL(flat_filtered_scatter_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kCompactBlock), 0, s, words,
                       valid, n, block_sums, ids);
  return hipGetLastError();
}

namespace {
template <bool kIp>
hipError_t scan_launch(const FlatFilteredParams &p, uint32_t grid, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL(flat_filtered_scan_kernel<kIp>, dim3(grid), dim3(p.tile / kScanWaveQueries * 64), lds, s, p);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_flat_filtered_scan(const FlatFilteredParams &p, hipStream_t s) {
  const uint32_t grid = scan_grid(p.tile, p.nq, p.n_ids, p.chunk_rows, p.chunks);
  if (grid == 0 || p.k == 0 || p.k > kFilteredMaxK) return hipErrorInvalidValue;
  const size_t lds = flat_filtered_lds(p.tile, p.stride, p.k);
  if (lds > kScanLdsMax) return hipErrorInvalidValue;
  return p.ip ? scan_launch<true>(p, grid, lds, s) : scan_launch<false>(p, grid, lds, s);
}

hipError_t launch_flat_filtered_merge(const FlatFilteredParams &p, hipStream_t s) {
  if (p.k == 0 || p.k > kFilteredMaxK || p.nq == 0) return hipErrorInvalidValue;
  const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(p.nq, 1u << 16));
  hipLaunchKernelGGL(flat_filtered_merge_kernel, dim3(grid), dim3(64), static_cast<size_t>(p.k) * 8, s, p);
  return hipGetLastError();
}

}  // namespace alaya_amd
