// Exact k-NN over per-query candidate lists: gather the listed rows, select the k nearest.
//
// Stands in for the reference's exact search (find_exact_gt, include/utils/evaluate.hpp:29-62) over a row set
// that each query names itself: query i's candidates are ids[lims[i] .. lims[i + 1]).  Every distance is f32 in
// the reference's summation order from the start (l2_sqr_avx2 / ip_sqr_avx2, restated in exact_scan_device.h),
// so nothing is approximate, flagged or recomputed.  Unlike the filtered scan, whose work item is (query tile,
// row chunk) and which reuses a row across a tile, no two queries share a row here: the work item is
// (query, piece of that query's list), and the cost is the gather of the rows.
//
//   1. pieces   flat_lists_offsets_kernel scans the queries' piece counts, flat_lists_pieces_kernel writes the
//               table of (query, first, count), count <= piece.  The table holds total / piece + nq entries,
//               a bound the host knows without reading `lims`; entries past the last piece are empty.
//   2. scan     one wave per piece, kListsWaves pieces per workgroup.  The wave's query sits in LDS in
//               load_query_tile's padded layout; its 8 lane groups take 8 candidates per pass, lane m of a
//               group the reference's accumulators 4m..4m+3 (pair_distance's split).  A lane keeps kBatch
//               16-byte slices of its row in flight and requests the next batch -- at a row's end the first
//               batch of the next pass's row, whose id was read a pass earlier and whose validity word half a
//               pass earlier -- before it works on the current one, so the next rows are on their way during
//               the reduction and the insertions.  The k best by (distance, id) live in LDS.
//   3. merge    one wave per query folds its pieces' lists into the k outputs, empty slots (all-ones id,
//               FLT_MAX).
//
// An id counts when it is below n and valid; every row load is behind that test, and a slot that fails it
// loads nothing.  A row listed twice has equal (distance bits, id) both times and is kept once: in a piece
// and in the merge an entry equal to the one at its slot is dropped.  No atomics, and no workgroup waits for
// another.
#include "flat_lists_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "exact_scan_device.h"

namespace alaya_amd {

using exact_scan::lane_xor;

namespace {

constexpr uint32_t kEmptyId = 0xffffffffu;
constexpr int kOffsetsBlock = 256;
constexpr int kBatch = 4;  // 32-element blocks of a row a lane has in flight (16 bytes each), twice while prefetching

__device__ __forceinline__ void fl_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// (distance, id) total order of every selection: smaller distance first, then smaller id
__device__ __forceinline__ bool fl_before(float da, uint32_t ia, float db, uint32_t ib) {
  return (da < db) | ((da == db) & (ia < ib));
}

// ---- pieces ---------------------------------------------------------------------------------------
// Query qi's list as [lo, lo + len): ends clamped to [0, total], a decreasing pair is empty.
__device__ __forceinline__ uint64_t fl_list(const FlatListsParams &p, uint64_t qi, uint64_t &lo) {
  const int64_t a = p.lims[p.q_first + qi], b = p.lims[p.q_first + qi + 1];
  lo = a < 0 ? 0 : std::min<uint64_t>(static_cast<uint64_t>(a), p.total);
  const uint64_t hi = b < 0 ? 0 : std::min<uint64_t>(static_cast<uint64_t>(b), p.total);
  return hi > lo ? hi - lo : 0;
}

__device__ __forceinline__ uint64_t fl_shfl_up(uint64_t v, int off) {
  const uint32_t lo = __shfl_up(static_cast<uint32_t>(v), off), hi = __shfl_up(static_cast<uint32_t>(v >> 32), off);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// one block: first_piece[0 .. nq] = the exclusive scan of ceil(len / piece), each count at most `table`
__global__ void __launch_bounds__(kOffsetsBlock) flat_lists_offsets_kernel(FlatListsParams p) {
  __shared__ uint64_t wave_tot[kOffsetsBlock / 64];
  const int lane = __lane_id(), wave = threadIdx.x >> 6;
  uint64_t running = 0;
  for (uint64_t q0 = 0; q0 < p.nq; q0 += kOffsetsBlock) {
    const uint64_t qi = q0 + threadIdx.x;
    uint64_t v = 0, lo;
    if (qi < p.nq) v = std::min<uint64_t>((fl_list(p, qi, lo) + p.piece - 1) / p.piece, p.table);
    uint64_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
      const uint64_t t = fl_shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint64_t pre = 0, total = 0;
    for (int w = 0; w < kOffsetsBlock / 64; ++w) {
      const uint64_t t = wave_tot[w];
      pre += w < wave ? t : 0;
      total += t;
    }
    __syncthreads();
    if (qi < p.nq) p.first_piece[qi] = running + pre + incl - v;
    running += total;
  }
  if (threadIdx.x == 0) p.first_piece[p.nq] = running;
}

// Table entry t: piece t - first_piece[i] of the query i that owns it, or an empty piece past the last one.
__global__ void __launch_bounds__(256) flat_lists_pieces_kernel(FlatListsParams p) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= p.table) return;
  FlatListsPiece pc{0, 0, 0};
  if (t < p.first_piece[p.nq]) {
    // the last query whose first piece is at or before t: it has a piece there, the ones after it start later
    uint64_t a = 0, b = p.nq;  // first_piece[a] <= t < first_piece[b]
    while (b - a > 1) {
      const uint64_t mid = a + (b - a) / 2;
      if (p.first_piece[mid] <= t) a = mid; else b = mid;
    }
    uint64_t lo;
    const uint64_t len = fl_list(p, a, lo);
    const uint64_t off = (t - p.first_piece[a]) * p.piece;  // < len: the query has more than t - first_piece[a] pieces
    pc.first = lo + off;
    pc.query = static_cast<uint32_t>(a);
    pc.count = static_cast<uint32_t>(std::min<uint64_t>(p.piece, len - off));
  }
  p.pieces[t] = pc;
}

// ---- a sorted (distance, id) list of k entries in LDS, one wave -------------------------------------
// Insert (d, id), which is before the list's last entry, unless the entry at its slot equals it: every lane
// holds entries lane, lane + 64, ... (k <= 256), the ones not before the newcomer move up by one and the last
// drops out.
__device__ __forceinline__ void fl_insert_unique(float *Ld, uint32_t *Li, uint32_t k, float d, uint32_t id, int lane) {
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
    pos += __popcll(__ballot(e < k && fl_before(ed[r], ei[r], d, id)));
  }
  // pos < k: the caller checked the newcomer against entry k - 1.  The same row met again has the same bits.
  const bool again = Li[pos] == id && __float_as_uint(Ld[pos]) == __float_as_uint(d);
  fl_wave_fence();
  if (again) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t e = lane + 64 * r;
    if (e >= pos && e + 1 < k) {
      Ld[e + 1] = ed[r];
      Li[e + 1] = ei[r];
    }
  }
  if (lane == 0) {
    Ld[pos] = d;
    Li[pos] = id;
  }
  fl_wave_fence();
}

// blocks tb .. tb + kBatch of a row, lane m's 16-byte slice of each; nothing is read for a slot that does not count
__device__ __forceinline__ void fl_load_batch(float4 (&y)[kBatch], const float *row, bool ok, uint32_t tb, uint32_t T,
                                              uint32_t m) {
#pragma unroll
  for (int u = 0; u < kBatch; ++u) {
    y[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok && tb + u < T) y[u] = *reinterpret_cast<const float4 *>(row + 32 * (tb + u) + 4 * m);
  }
}

template <bool kIp>
__device__ __forceinline__ void fl_step(float (&a)[4], const float4 x, const float4 y) {
  if constexpr (kIp) {
    a[0] = fmaf(x.x, y.x, a[0]); a[1] = fmaf(x.y, y.y, a[1]); a[2] = fmaf(x.z, y.z, a[2]); a[3] = fmaf(x.w, y.w, a[3]);
  } else {
    const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
    a[0] = fmaf(d0, d0, a[0]); a[1] = fmaf(d1, d1, a[1]); a[2] = fmaf(d2, d2, a[2]); a[3] = fmaf(d3, d3, a[3]);
  }
}

}  // namespace

// Built for 4 waves per SIMD: 4 workgroups of 4 waves per CU, each lane with kBatch .. 2 kBatch 16-byte loads in
// flight -- 64 .. 128 KB per CU, past what covers an HBM miss at the gather ceiling.
template <bool kIp>
__global__ void __launch_bounds__(64 * kListsWaves, 4) flat_lists_scan_kernel(FlatListsParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t stride = p.stride, k = p.k, dim = p.dim;
  const int lane = __lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t g = lane >> 3, m = lane & 7;
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kListsWaves + wave;
  if (t >= p.table) return;  // (no workgroup barrier below: a wave touches its own LDS only)
  const FlatListsPiece pc = p.pieces[t];
  if (pc.count == 0) return;
  float *q = reinterpret_cast<float *>(smem) + static_cast<size_t>(wave) * stride;  // stride floats, zero padded
  float *Ld = reinterpret_cast<float *>(smem) + static_cast<size_t>(kListsWaves) * stride + wave * k;
  uint32_t *Li = reinterpret_cast<uint32_t *>(reinterpret_cast<float *>(smem) + static_cast<size_t>(kListsWaves) * (stride + k)) + wave * k;
  const float *qrow = p.queries + (p.q_first + pc.query) * p.q_stride;
  for (uint32_t e = lane; e < stride; e += 64) q[e] = e < dim ? qrow[e] : 0.f;
  for (uint32_t e = lane; e < k; e += 64) {
    Ld[e] = FLT_MAX;
    Li[e] = kEmptyId;
  }
  fl_wave_fence();
  const uint32_t T = dim >> 5;
  const uint32_t nb8 = (dim - 32 * T) >> 3;
  const uint32_t tail0 = 32 * T + 8 * nb8;
  const uint32_t passes = (pc.count + kListsPassRows - 1) / kListsPassRows;
  // lane group g's candidate of pass ps; the all-ones id (never below n) past the piece
  auto cand = [&](uint32_t ps) {
    const uint32_t at = ps * kListsPassRows + g;
    return ps < passes && at < pc.count ? p.ids[pc.first + at] : kEmptyId;
  };
  auto valid_word = [&](uint32_t id) { return p.valid && id < p.n ? p.valid[id >> 5] : ~0u; };
  auto counts = [&](uint32_t id, uint32_t word) { return id < p.n && ((word >> (id & 31)) & 1u) != 0; };
  uint32_t id_c = cand(0), id_n = cand(1);
  bool ok_c = counts(id_c, valid_word(id_c));
  uint32_t word_n = valid_word(id_n);
  const float *row = p.base + static_cast<uint64_t>(ok_c ? id_c : 0u) * stride;
  float4 y[kBatch];
  fl_load_batch(y, row, ok_c, 0, T, m);
  for (uint32_t ps = 0; ps < passes; ++ps) {
    const uint32_t id_nn = cand(ps + 2);
    const bool ok_n = counts(id_n, word_n);
    const float *row_n = p.base + static_cast<uint64_t>(ok_n ? id_n : 0u) * stride;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (uint32_t t0 = 0; t0 < T; t0 += kBatch) {
      // the next batch is requested before this batch's arithmetic: of this row, or of the next pass's row
      float4 yn[kBatch];
      if (t0 + kBatch < T) {
        fl_load_batch(yn, row, ok_c, t0 + kBatch, T, m);
      } else {
        fl_load_batch(yn, row_n, ok_n, 0, T, m);
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        if (t0 + u < T) fl_step<kIp>(a, *reinterpret_cast<const float4 *>(q + 32 * (t0 + u) + 4 * m), y[u]);
        y[u] = yn[u];
      }
    }
    const uint32_t word_nn = valid_word(id_nn);
    if (m < 2) {
      for (uint32_t bb = 0; bb < nb8; ++bb) {
        const uint32_t off = 32 * T + 8 * bb + 4 * m;
        float4 yb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok_c) yb = *reinterpret_cast<const float4 *>(row + off);
        fl_step<kIp>(a, *reinterpret_cast<const float4 *>(q + off), yb);
      }
    }
    // every lane takes part in the group sums, whether its slot counts or not
    a[0] += lane_xor<2>(a[0]); a[1] += lane_xor<2>(a[1]); a[2] += lane_xor<2>(a[2]); a[3] += lane_xor<2>(a[3]);
    a[0] += lane_xor<4>(a[0]); a[1] += lane_xor<4>(a[1]); a[2] += lane_xor<4>(a[2]); a[3] += lane_xor<4>(a[3]);
    const float s0 = a[0] + lane_xor<1>(a[0]), s1 = a[1] + lane_xor<1>(a[1]);
    const float s2 = a[2] + lane_xor<1>(a[2]), s3 = a[3] + lane_xor<1>(a[3]);
    float res = (s0 + s1) + (s2 + s3);
    for (uint32_t e = tail0; e < dim; ++e) {
      const float b = ok_c ? row[e] : 0.f;
      if constexpr (kIp) {
        res = fmaf(q[e], b, res);
      } else {
        const float d = q[e] - b;
        res = fmaf(d, d, res);
      }
    }
    const float d = kIp ? -res : res;
    // the 8 finished distances: those not before the k-th are dropped, the rest inserted one at a time
    uint64_t offer = __ballot(m == 0 && ok_c && fl_before(d, id_c, Ld[k - 1], Li[k - 1]));
    while (offer) {
      const int src = __ffsll(static_cast<unsigned long long>(offer)) - 1;
      offer &= offer - 1;
      const float cd = __shfl(d, src);
      const uint32_t ci = __shfl(id_c, src);
      if (fl_before(cd, ci, Ld[k - 1], Li[k - 1])) fl_insert_unique(Ld, Li, k, cd, ci, lane);
    }
    id_c = id_n;
    ok_c = ok_n;
    row = row_n;
    id_n = id_nn;
    word_n = word_nn;
  }
  fl_wave_fence();
  for (uint32_t e = lane; e < k; e += 64) {
    p.part_d[t * k + e] = Ld[e];
    p.part_i[t * k + e] = Li[e];
  }
}

// One wave per query: fold its pieces' lists (each ascending by (distance, id)) into one list of k and write it.
// A piece's entry that is not before the list's last ends that piece: the rest are later.
__global__ void __launch_bounds__(64) flat_lists_merge_kernel(FlatListsParams p) {
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
    fl_wave_fence();
    const uint64_t t1 = std::min<uint64_t>(p.first_piece[qi + 1], p.table);
    for (uint64_t t = p.first_piece[qi]; t < t1; ++t) {
      bool open = true;
      for (uint32_t e0 = 0; e0 < k && open; e0 += 64) {
        const uint32_t e = e0 + lane;
        const float d = e < k ? p.part_d[t * k + e] : FLT_MAX;
        const uint32_t id = e < k ? p.part_i[t * k + e] : kEmptyId;
        uint64_t offer = __ballot(e < k && fl_before(d, id, Ld[k - 1], Li[k - 1]));
        if (offer != __ballot(e < k)) open = false;  // an entry lost: so do the later ones
        while (offer) {
          const int src = __ffsll(static_cast<unsigned long long>(offer)) - 1;
          offer &= offer - 1;
          const float cd = __shfl(d, src);
          const uint32_t ci = __shfl(id, src);
          if (!fl_before(cd, ci, Ld[k - 1], Li[k - 1])) {
            open = false;
            break;
          }
          fl_insert_unique(Ld, Li, k, cd, ci, lane);
        }
      }
    }
    const uint64_t dst = (p.q_first + qi) * k;
    for (uint32_t e = lane; e < k; e += 64) {
      p.out_ids[dst + e] = Li[e];
      if (p.out_dists) p.out_dists[dst + e] = Ld[e];
    }
    fl_wave_fence();
  }
}

// ---- host side -------------------------------------------------------------------------------------
size_t flat_lists_lds(uint32_t stride, uint32_t k) {
  return static_cast<size_t>(kListsWaves) * (static_cast<size_t>(stride) * 4 + static_cast<size_t>(k) * 8);
}

FlatListsPlan flat_lists_plan(uint64_t total, uint64_t nq, uint32_t k, uint32_t stride, uint32_t cus, uint64_t forced_piece) {
  FlatListsPlan r{};
  k = std::max<uint32_t>(k, 1);
  cus = std::max<uint32_t>(cus, 1);
  nq = std::max<uint64_t>(nq, 1);
  if (flat_lists_lds(stride, k) > kScanLdsMax) return r;  // (four workgroups fit a CU up to a stride of about 2000)
  const uint64_t pair = static_cast<uint64_t>(k) * 8;
  const auto passes_up = [](uint64_t v) { return (v + kListsPassRows - 1) / kListsPassRows * kListsPassRows; };
  uint64_t piece;
  if (forced_piece) {
    piece = passes_up(forced_piece);
  } else {
    // about four pieces for each of the 16 waves a CU holds, within [kListsMinPiece, kListsMaxPiece] ...
    piece = std::min<uint64_t>(kListsMaxPiece, std::max<uint64_t>(kListsMinPiece, passes_up(total / (64ull * cus))));
    // ... and long enough that the whole pieces' lists take at most half the cap: the other half is the queries'
    piece = std::max(piece, passes_up((total * pair + kListsPartialCap / 2 - 1) / (kListsPartialCap / 2)));
  }
  if (piece > 0x7fffffffull) return r;
  const uint64_t whole = total / piece;  // sum of floor(len / piece) <= this; each query adds at most one more
  const uint64_t room = kListsPartialCap / pair;
  r.piece = piece;
  r.sub_queries = std::min(nq, room > whole ? room - whole : 1);
  r.table = whole + r.sub_queries;
  r.partial_bytes = r.table * pair;
  r.launches = (nq + r.sub_queries - 1) / r.sub_queries;
  return r;
}

namespace {
// what every launch checks: k, the piece, a table below 2^31 that holds the bound, and the LDS
bool lists_launch_ok(const FlatListsParams &p) {
  if (p.k == 0 || p.k > kListsMaxK || p.nq == 0 || p.nq > 0xffffffffull) return false;
  if (p.piece == 0 || p.piece % kListsPassRows != 0) return false;
  if (p.table > 0x7fffffffull || p.table < p.total / p.piece + p.nq) return false;
  if (p.stride < 4 || p.stride % 4 != 0 || p.dim > p.stride) return false;
  return flat_lists_lds(p.stride, p.k) <= kScanLdsMax;
}
}  // namespace

hipError_t launch_flat_lists_pieces(const FlatListsParams &p, hipStream_t s) {
  if (!lists_launch_ok(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(flat_lists_offsets_kernel, dim3(1), dim3(kOffsetsBlock), 0, s, p);
  hipLaunchKernelGGL(flat_lists_pieces_kernel, dim3(static_cast<uint32_t>((p.table + 255) / 256)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_flat_lists_scan(const FlatListsParams &p, hipStream_t s) {
  if (!lists_launch_ok(p)) return hipErrorInvalidValue;
  const uint32_t grid = static_cast<uint32_t>((p.table + kListsWaves - 1) / kListsWaves);
  const size_t lds = flat_lists_lds(p.stride, p.k);
  if (p.ip) {
    hipLaunchKernelGGL(flat_lists_scan_kernel<true>, dim3(grid), dim3(64 * kListsWaves), lds, s, p);
  } else {
    hipLaunchKernelGGL(flat_lists_scan_kernel<false>, dim3(grid), dim3(64 * kListsWaves), lds, s, p);
  }
  return hipGetLastError();
}

hipError_t launch_flat_lists_merge(const FlatListsParams &p, hipStream_t s) {
  if (!lists_launch_ok(p)) return hipErrorInvalidValue;
  const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(p.nq, 1u << 16));
  hipLaunchKernelGGL(flat_lists_merge_kernel, dim3(grid), dim3(64), static_cast<size_t>(p.k) * 8, s, p);
  return hipGetLastError();
}

}  // namespace alaya_amd
