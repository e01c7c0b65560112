// Exact filtered k-NN for small allowed shares: skip the graph, scan the allowed rows exactly.
//
// Stands in for the reference's exact search (find_exact_gt, include/utils/evaluate.hpp:29-62) over
// the subset of rows that are valid and that a mask allows.  Every distance is computed in f32 in
// the reference's summation order from the start (l2_sqr_avx2 / ip_sqr_avx2, restated below), so
// there is no approximate contraction, no bound, no flag and no host recompute -- unlike the MFMA
// flat scan of flat_kernels.hip, whose exact_l2 / exact_ip give the same bits.
//
//   1. compaction  (mask AND validity) -> ascending id list + count: word popcounts, an exclusive scan
//                  of the per-block sums, a scatter.
//   2. scan        grid = row chunks (ranges of the id list) x query tiles.  A workgroup holds its tile's
//                  queries in LDS; wave w owns queries 4w..4w+3 of the tile and streams the chunk's rows
//                  32 per pass: lane group g (8 lanes) takes rows 4g..4g+3 of the pass, lane m of the
//                  group the reference's accumulators 4m..4m+3.  A lane's 16-byte slice of each of its 4
//                  rows meets the 4 queries' slices before it is dropped: 64 accumulators, 4 global and
//                  4 LDS 16-byte reads per 64 fmaf.  The waves of a workgroup read the same rows at the
//                  same time, so a row leaves memory once per tile.  Each wave keeps its queries' k best
//                  by (distance, id) as sorted lists in LDS and writes them out at the end.
//   3. merge       one wave per query folds the chunk lists into the k outputs, empty slots
//                  (all-ones id, FLT_MAX).
//
// No workgroup waits for another.
#include "flat_filtered_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

namespace alaya_amd {

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

// ---- the reference order, restated ---------------------------------------------------------------
// l2_sqr_avx2 / ip_sqr_avx2: four 8-wide accumulators over 32-element blocks (lane m of 8 owns elements
// 4m..4m+3 of each block, one fmaf per element), then the whole 8-element blocks into the first
// accumulator (lanes 0-1), the horizontal sum (xor 2, xor 4, xor 1, then (s0 + s1) + (s2 + s3)), the
// scalar tail through fmaf, and for inner products the negation last.
// Lane xor inside a group of 8 by DPP: xor 1 / 2 quad_perm, xor 4 row_ror:12 / row_ror:4 by lane bit 2.
template <int kXor>
__device__ __forceinline__ float ff_xor(float v) {
  const int x = __float_as_int(v);
  if constexpr (kXor == 1) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false));
  } else if constexpr (kXor == 2) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false));
  } else {
    const int up = __builtin_amdgcn_update_dpp(0, x, 0x12C, 0xF, 0xF, false);
    const int down = __builtin_amdgcn_update_dpp(0, x, 0x124, 0xF, 0xF, false);
    return __int_as_float((__lane_id() & 4) ? down : up);
  }
}

constexpr int kRows = 4;     // rows of a lane group per pass
constexpr int kQueries = 4;  // queries of a wave

// one 16-byte slice of each of the lane's rows against the same slice of each of the wave's queries
template <bool kIp>
__device__ __forceinline__ void ff_block(float (&acc)[kRows][kQueries][4], const float4 (&y)[kRows], const float *q,
                                         uint32_t stride, uint32_t off) {
#pragma unroll
  for (int c = 0; c < kQueries; ++c) {
    const float4 x = *reinterpret_cast<const float4 *>(q + c * stride + off);
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      if constexpr (kIp) {
        acc[j][c][0] = fmaf(x.x, y[j].x, acc[j][c][0]);
        acc[j][c][1] = fmaf(x.y, y[j].y, acc[j][c][1]);
        acc[j][c][2] = fmaf(x.z, y[j].z, acc[j][c][2]);
        acc[j][c][3] = fmaf(x.w, y[j].w, acc[j][c][3]);
      } else {
        const float d0 = x.x - y[j].x, d1 = x.y - y[j].y, d2 = x.z - y[j].z, d3 = x.w - y[j].w;
        acc[j][c][0] = fmaf(d0, d0, acc[j][c][0]);
        acc[j][c][1] = fmaf(d1, d1, acc[j][c][1]);
        acc[j][c][2] = fmaf(d2, d2, acc[j][c][2]);
        acc[j][c][3] = fmaf(d3, d3, acc[j][c][3]);
      }
    }
  }
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
  for (uint32_t i = threadIdx.x; i < tile * stride; i += blockDim.x) {
    const uint32_t ql = i / stride, e = i - ql * stride;
    float v = 0.f;
    if (q0 + ql < p.nq && e < p.dim) {
      const uint64_t src = p.q_list ? p.q_list[p.q_first + q0 + ql] : p.q_first + q0 + ql;
      v = p.queries[src * p.q_stride + e];
    }
    qs[i] = v;
  }
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
  for (uint64_t pb = r0; pb < r1; pb += kFilteredPassRows) {
    // the lane group's rows, in ascending id order; a slot past the chunk recomputes the chunk's first row
    uint32_t rid[kRows];
    bool ok[kRows];
    const float *row[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const uint64_t at = pb + g * kRows + j;
      ok[j] = at < r1;
      rid[j] = p.ids[ok[j] ? at : r0];
      row[j] = p.base + static_cast<uint64_t>(rid[j]) * stride;
    }
    float acc[kRows][kQueries][4];
#pragma unroll
    for (int j = 0; j < kRows; ++j)
#pragma unroll
      for (int c = 0; c < kQueries; ++c)
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[j][c][a] = 0.f;
    if (T > 0) {
      float4 y[kRows];
#pragma unroll
      for (int j = 0; j < kRows; ++j) y[j] = *reinterpret_cast<const float4 *>(row[j] + 4 * m);
      for (uint32_t t = 0; t < T; ++t) {
        // the next block's slices are requested before this block's arithmetic
        float4 yn[kRows];
        const uint32_t tn = t + 1 < T ? t + 1 : t;
#pragma unroll
        for (int j = 0; j < kRows; ++j) yn[j] = *reinterpret_cast<const float4 *>(row[j] + 32 * tn + 4 * m);
        ff_block<kIp>(acc, y, q, stride, 32 * t + 4 * m);
#pragma unroll
        for (int j = 0; j < kRows; ++j) y[j] = yn[j];
      }
    }
    if (m < 2) {
      for (uint32_t bb = 0; bb < nb8; ++bb) {
        const uint32_t off = 32 * T + 8 * bb + 4 * m;
        float4 y[kRows];
#pragma unroll
        for (int j = 0; j < kRows; ++j) y[j] = *reinterpret_cast<const float4 *>(row[j] + off);
        ff_block<kIp>(acc, y, q, stride, off);
      }
    }
    float dist[kRows][kQueries];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
#pragma unroll
      for (int c = 0; c < kQueries; ++c) {
        float a0 = acc[j][c][0], a1 = acc[j][c][1], a2 = acc[j][c][2], a3 = acc[j][c][3];
        a0 += ff_xor<2>(a0); a1 += ff_xor<2>(a1); a2 += ff_xor<2>(a2); a3 += ff_xor<2>(a3);
        a0 += ff_xor<4>(a0); a1 += ff_xor<4>(a1); a2 += ff_xor<4>(a2); a3 += ff_xor<4>(a3);
        const float s0 = a0 + ff_xor<1>(a0), s1 = a1 + ff_xor<1>(a1);
        const float s2 = a2 + ff_xor<1>(a2), s3 = a3 + ff_xor<1>(a3);
        float res = (s0 + s1) + (s2 + s3);
        for (uint32_t e = tail0; e < p.dim; ++e) {
          if constexpr (kIp) {
            res = fmaf(q[c * stride + e], row[j][e], res);
          } else {
            const float d = q[c * stride + e] - row[j][e];
            res = fmaf(d, d, res);
          }
        }
        dist[j][c] = kIp ? -res : res;
      }
    }
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
  // Query tile: 16 (four waves share each row read), smaller for a handful of queries, and smaller
  // where two workgroups would no longer fit a CU's LDS -- the second one hides the row loads' latency.
  uint32_t tile = nq <= 4 ? 4 : (nq <= 8 ? 8 : kFilteredMaxTile);
  while (tile > kFilteredWaveQueries && flat_filtered_lds(tile, stride, k) > kFilteredLdsMax / 2) tile /= 2;
  if (flat_filtered_lds(tile, stride, k) > kFilteredLdsMax) return r;  // tile = 0: does not fit
  r.tile = tile;
  const uint64_t q_tiles = std::max<uint64_t>(1, (nq + tile - 1) / tile);
  // no more chunks than fill the CUs twice over at this tile -- rounded down: two workgroups are resident
  // per CU, and a grid a little past 2 x cus would run a second, nearly empty round
  const uint64_t max_chunks = std::max<uint64_t>(1, 2ull * cus / q_tiles);
  const uint64_t passes = (n_allowed + kFilteredPassRows - 1) / kFilteredPassRows;
  uint64_t chunk_rows = kFilteredPassRows * std::max<uint64_t>(1, (passes + max_chunks - 1) / max_chunks);
  if (forced_rows) chunk_rows = (forced_rows + kFilteredPassRows - 1) / kFilteredPassRows * kFilteredPassRows;
  // one query tile's lists stay under the cap (only a forced chunk size can ask for more)
  const uint64_t cap_chunks = kFilteredPartialCap / (static_cast<uint64_t>(tile) * k * 8);
  if ((n_allowed + chunk_rows - 1) / chunk_rows > cap_chunks)
    chunk_rows = kFilteredPassRows * ((passes + cap_chunks - 1) / cap_chunks);
  r.chunk_rows = chunk_rows;
  r.chunks = (n_allowed + chunk_rows - 1) / chunk_rows;
  const uint64_t all = (std::max<uint64_t>(nq, 1) + tile - 1) / tile * tile;
  r.sub_queries = all;
  if (r.chunks) {
    const uint64_t fit = kFilteredPartialCap / (r.chunks * k * 8) / tile * tile;  // >= tile by cap_chunks
    r.sub_queries = std::min(all, fit);
  }
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
  hipLaunchKernelGGL(flat_filtered_scan_kernel<kIp>, dim3(grid), dim3(p.tile / kFilteredWaveQueries * 64), lds, s, p);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_flat_filtered_scan(const FlatFilteredParams &p, hipStream_t s) {
  if (p.tile != 4 && p.tile != 8 && p.tile != 16) return hipErrorInvalidValue;
  if (p.k == 0 || p.k > kFilteredMaxK || p.nq == 0 || p.chunks == 0 || p.chunk_rows == 0) return hipErrorInvalidValue;
  if (p.chunks * p.chunk_rows < p.n_ids || (p.chunks - 1) * p.chunk_rows >= p.n_ids) return hipErrorInvalidValue;
  const size_t lds = flat_filtered_lds(p.tile, p.stride, p.k);
  if (lds > kFilteredLdsMax) return hipErrorInvalidValue;
  const uint64_t grid = (p.nq + p.tile - 1) / p.tile * p.chunks;
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  return p.ip ? scan_launch<true>(p, static_cast<uint32_t>(grid), lds, s)
              : scan_launch<false>(p, static_cast<uint32_t>(grid), lds, s);
}

hipError_t launch_flat_filtered_merge(const FlatFilteredParams &p, hipStream_t s) {
  if (p.k == 0 || p.k > kFilteredMaxK || p.nq == 0) return hipErrorInvalidValue;
  const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(p.nq, 1u << 16));
  hipLaunchKernelGGL(flat_filtered_merge_kernel, dim3(grid), dim3(64), static_cast<size_t>(p.k) * 8, s, p);
  return hipGetLastError();
}

}  // namespace alaya_amd
