// Exact range search on the MFMA scan: prove most (query, row) pairs by a matrix contraction, verify the band.
//
//   1. prepare  one wave per query of the launch: the query zero padded to whole slabs, |q|^2, and the two
//               thresholds lo <= hi of flat_range_bound.h.
//   2. scan     flat_range_mfma_kernel<kIp>.  A workgroup of 4 waves owns 128 queries (32 per wave) and one
//               contiguous row chunk; the grid is XCD-aware as flat_scan_kernel's.  Rows stream through a
//               double-buffered LDS unit of 32 rows x KS = 64 columns, split into bf16 hi + lo once when the
//               unit is staged.  Per slab a wave splits its queries' slice into hi / lo A fragments (lane
//               (col, h) holds query col, columns h KS/2 .. + KS/2 of the slab) and runs a super-tile of TT = 4
//               tiles whose 32x32 accumulators (C[query][row]: row = lane & 31, query = (r & 3) + 8 (r >> 2) +
//               4 h for register r) persist across the slabs: qh.bh + qh.bl + ql.bh, three
//               v_mfma_f32_32x32x16_bf16 per 16 columns.  After the last slab d~ = (|q|^2 + |b|^2) - 2 C (L2)
//               or -C (IP); per accumulator register two compares, the tile's eligibility bit and a ballot:
//               no candidate bit set, next register.  Otherwise the register's two ballots go to a per-wave LDS
//               list that is settled after the super-tile's compares, per query of the register: the pairs that
//               need the exact distance -- the band bits, and every candidate bit while the query's count is
//               below `slots` -- are computed 8 at a time, a group of 8 lanes per pair in exact_scan_device.h's
//               order, and the hits appended in row order with plain vector stores; proven bits past
//               `slots` add their popcount.  One wave owns a (chunk, query) pair: counts are registers (lane q
//               of the wave holds query q's), nothing is atomic, no workgroup waits for another.
//   3. reduce   the per-wave counters (pairs verified, band pairs, pairs proven) summed by one workgroup.
//
// KS = 64, TT = 4: a lane holds 64 accumulators, 32 VGPRs of A fragments, 32 of the next slab's f32 slice, 48
// of thresholds and 8 of staging: 245 VGPRs + 64 AGPRs for L2, 221 + 64 for IP, no scratch, one wave per SIMD;
// KS = 128 doubles the fragment and prefetch registers and would spill.  LDS reads: a wave reads 2 x 16 bytes per lane (bh, bl) per 3 MFMAs, 2 KiB per
// 96 MFMA cycles; 4 waves, 85 bytes per cycle of the CU's 128, whatever TT -- each B fragment feeds one wave's
// 3 MFMAs.  TT amortises what is per slab: the 8 float4 loads and the 32 hi/lo splits of the A slice, over
// TT x 12 MFMAs (1536 cycles at TT = 4), and the barrier per unit stays one per 12 MFMAs.
#include "flat_range_mfma_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "exact_scan_device.h"
#include "flat_mfma_split.h"
#include "flat_range_bound.h"

namespace alaya_amd {

using exact_scan::query_row;

namespace {

constexpr int KS = kRangeMfmaKS;
constexpr int TT = kRangeMfmaTT;
constexpr int kTile = 32;
constexpr int kBPitch = KS + 8;                // bf16 per LDS row: 144 bytes, 16-byte reads spread over the banks
constexpr int kHalf = kTile * kBPitch;         // bf16 of one hi (or lo) unit
using mfma_split::bf16x4;
using mfma_split::bf16x8;
using mfma_split::f32x16;
using mfma_split::split_bf16;

__device__ __forceinline__ uint32_t read_lane(uint32_t v, int l) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), __builtin_amdgcn_readfirstlane(l)));
}

// a value every lane holds alike, as a scalar
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  const uint32_t a = __builtin_amdgcn_readfirstlane(static_cast<int>(v));
  const uint32_t b = __builtin_amdgcn_readfirstlane(static_cast<int>(v >> 32));
  return (static_cast<uint64_t>(b) << 32) | a;
}

__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace

__global__ void __launch_bounds__(256) flat_range_mfma_prepare_kernel(FlatRangeMfmaParams p) {
  const uint64_t nq_up = (p.nq + kRangeMfmaQueries - 1) / kRangeMfmaQueries * kRangeMfmaQueries;
  const uint64_t qi = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (qi >= nq_up) return;
  const int lane = __lane_id();
  const bool live = qi < p.nq;
  const uint64_t src = live ? query_row(p.q_list, p.q_first, qi) : 0;
  float sum = 0.f;
  for (uint32_t e = lane; e < p.qwidth; e += 64) {
    const float v = live && e < p.dim ? p.queries[src * p.q_stride + e] : 0.f;
    p.qpad[qi * p.qwidth + e] = v;
    sum = fmaf(v, v, sum);
  }
  for (int x = 32; x > 0; x >>= 1) sum += __shfl_xor(sum, x);
  if (lane == 0) {
    const float rad = live ? p.radii[src] : -INFINITY;
    FlatRangeBound b = flat_range_bound(p.ip != 0, rad, sum, p.max_norm, p.qwidth, kFlatSplit);
    if (!live) b.lo = b.hi = -INFINITY;
    p.qmeta[qi] = sum;
    p.qmeta[nq_up + qi] = b.lo;
    p.qmeta[2 * nq_up + qi] = b.hi;
    p.qmeta[3 * nq_up + qi] = rad;
  }
}

template <bool kIp>
__global__ void __launch_bounds__(256) flat_range_mfma_kernel(FlatRangeMfmaParams p) {
  __shared__ __attribute__((aligned(16))) __bf16 tile[2 * 2 * kHalf];  // two buffers of (hi unit, lo unit)
  __shared__ uint64_t pend[4][TT * 16][2];  // per wave: the (candidate, proven) ballots of a super-tile's registers
  const int lane = __lane_id();
  const int wave = threadIdx.x >> 6;
  const int col = lane & 31, h = lane >> 5;
  const uint32_t g = lane >> 3, m = lane & 7;
  const uint64_t nq_up = (p.nq + kRangeMfmaQueries - 1) / kRangeMfmaQueries * kRangeMfmaQueries;
  const uint32_t nqg = static_cast<uint32_t>(nq_up / kRangeMfmaQueries);
  // XCD-aware block -> (query group, chunk): the query groups of one chunk share an XCD label
  const uint32_t b = blockIdx.x;
  const uint32_t qg = (b / 8) % nqg;
  const uint64_t chunk = (b % 8) + 8ull * (b / (8 * nqg));
  if (chunk >= p.chunks) return;
  const uint64_t r0 = chunk * p.chunk_rows;
  const uint64_t r1 = min(p.n, r0 + p.chunk_rows);  // r0 < r1: the chunks cover n
  const int nslab = static_cast<int>(p.qwidth / KS);
  const uint64_t q0 = static_cast<uint64_t>(qg) * kRangeMfmaQueries + wave * 32;  // the wave's first query

  // per accumulator register: the thresholds of its query (and |q|^2 for L2)
  float lo[16], hi[16], qn[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const uint64_t qi = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
    qn[r] = kIp ? 0.f : p.qmeta[qi];
    lo[r] = p.qmeta[nq_up + qi];
    hi[r] = p.qmeta[2 * nq_up + qi];
  }
  // per lane q < 32: query q0 + q's radius and hit count
  const float radv = p.qmeta[3 * nq_up + q0 + col];
  uint32_t cntv = 0;
  uint32_t st_verified = 0, st_band = 0, st_proven = 0;
  const uint64_t lower = (1ull << lane) - 1ull;

  const float4 *qrow = reinterpret_cast<const float4 *>(p.qpad + (q0 + col) * p.qwidth + h * (KS / 2));
  float4 an[KS / 8];
  auto load_a = [&](int s) {
#pragma unroll
    for (int j = 0; j < KS / 8; ++j) an[j] = qrow[s * (KS / 4) + j];
  };

  // cooperative unit load: 32 rows x KS columns, 256 threads, float4 each; rows past n read row n - 1 (their
  // eligibility bits are clear), columns past stride are zeroed when stored
  constexpr int kVecPerRow = KS / 4;
  constexpr int kPerThread = kTile * kVecPerRow / 256;
  static_assert(kTile * kVecPerRow % 256 == 0, "whole float4s per thread");
  auto load_unit = [&](uint64_t row0, uint32_t c0, float4 (&reg)[kPerThread]) {
#pragma unroll
    for (int v = 0; v < kPerThread; ++v) {
      const int idx = threadIdx.x + v * 256;
      const uint64_t row = min<uint64_t>(row0 + idx / kVecPerRow, p.n - 1);
      const uint32_t c = min<uint32_t>(c0 + (idx % kVecPerRow) * 4, p.stride - 4);
      reg[v] = *reinterpret_cast<const float4 *>(p.base + row * p.stride + c);
    }
  };
  auto store_unit = [&](int buf, uint32_t c0, const float4 (&reg)[kPerThread]) {
#pragma unroll
    for (int v = 0; v < kPerThread; ++v) {
      const int idx = threadIdx.x + v * 256;
      const bool in = c0 + (idx % kVecPerRow) * 4 < p.stride;
      const float4 x = in ? reg[v] : make_float4(0.f, 0.f, 0.f, 0.f);
      __bf16 *th = tile + buf * 2 * kHalf + (idx / kVecPerRow) * kBPitch + (idx % kVecPerRow) * 4;
      bf16x4 hv, lv;
      __bf16 xh, xl;
      split_bf16(x.x, xh, xl); hv[0] = xh; lv[0] = xl;
      split_bf16(x.y, xh, xl); hv[1] = xh; lv[1] = xl;
      split_bf16(x.z, xh, xl); hv[2] = xh; lv[2] = xl;
      split_bf16(x.w, xh, xl); hv[3] = xh; lv[3] = xl;
      *reinterpret_cast<bf16x4 *>(th) = hv;
      *reinterpret_cast<bf16x4 *>(th + kHalf) = lv;
    }
  };

  // One query of an accumulator register: qs its slot in the wave, row0 the tile's first row, cand / sure the
  // tile's candidate and proven bits for it.  Wave-uniform.
  auto settle = [&](int qs, uint64_t row0, uint32_t cand, uint32_t sure) {
    const uint64_t qi = q0 + qs;
    if (cand == 0 || qi >= p.nq) return;
    uint32_t cnt = read_lane(cntv, qs);
    uint32_t need = cnt < p.slots ? cand : (cand & ~sure);
    const uint32_t proven = __popc(sure & ~need);
    st_verified += __popc(need);
    st_band += __popc(need & ~sure);
    st_proven += proven;
    cnt += proven;  // (proven > 0 only past `slots`: nothing more is stored, the order no longer matters)
    if (need != 0) {
      const float rad = __int_as_float(static_cast<int>(read_lane(static_cast<uint32_t>(__float_as_int(radv)), qs)));
      const float *q = p.qpad + qi * p.qwidth;
      const uint64_t part = (chunk * p.nq + qi) * p.slots;
      while (need != 0) {
        // the next 8 pairs in ascending row order, one per lane group; an idle group recomputes the first
        uint32_t mine = __builtin_ctz(need);
        bool active = false;
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
          if (need != 0) {
            const uint32_t bit = __builtin_ctz(need);
            if (g == i) {
              mine = bit;
              active = true;
            }
            need &= need - 1;
          }
        }
        const uint64_t rid = row0 + mine;  // < n: the eligibility word has no bit past n
        const float d = exact_scan::pair_distance<kIp>(q, p.base + rid * p.stride, p.dim, m);
        const bool hit = active && m == 0 && d <= rad;  // inclusive; a NaN radius or distance is no hit
        const uint64_t hb = __ballot(hit);
        if (hit) {
          const uint32_t at = cnt + __popcll(hb & lower);
          if (at < p.slots) {
            p.part_i[part + at] = static_cast<uint32_t>(rid);
            p.part_d[part + at] = d;
          }
        }
        cnt += __popcll(hb);
      }
    }
    if (lane == qs) cntv = cnt;
  };

  float4 stage[kPerThread];
  load_a(0);
  load_unit(r0, 0, stage);
  store_unit(0, 0, stage);
  __syncthreads();
  int buf = 0;
  for (uint64_t sup = r0; sup < r1; sup += kTile * TT) {
    const int ntiles = static_cast<int>(min<uint64_t>(TT, (r1 - sup + kTile - 1) / kTile));
    const bool last_sup = sup + kTile * TT >= r1;
    float bn[TT];
    uint32_t el[TT];  // the tiles' eligibility words: mask AND validity AND below n
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const uint64_t row0 = sup + kTile * t;
      bn[t] = kIp ? 0.f : p.norms[min<uint64_t>(row0 + col, p.n - 1)];
      uint32_t w = 0;
      if (row0 < r1) {
        w = p.words[row0 >> 5];
        if (p.valid != nullptr) w &= p.valid[row0 >> 5];
        if (p.n - row0 < 32) w &= (1u << (p.n - row0)) - 1u;
      }
      el[t] = w;
    }
    f32x16 c[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) c[t] = f32x16{};
    for (int s = 0; s < nslab; ++s) {
      // this slab's A fragments: k-step st of lane (col, h) holds columns s KS + h KS/2 + 8 st + j
      bf16x8 ah[KS / 16], al[KS / 16];
#pragma unroll
      for (int st = 0; st < KS / 16; ++st) {
        const float4 u = an[2 * st], w = an[2 * st + 1];
        const float v8[8] = {u.x, u.y, u.z, u.w, w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          __bf16 xh, xl;
          split_bf16(v8[j], xh, xl);
          ah[st][j] = xh;
          al[st][j] = xl;
        }
      }
      if (s + 1 < nslab || !last_sup) load_a(s + 1 < nslab ? s + 1 : 0);  // the next slab's slice in flight
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        if (t < ntiles) {  // wave-uniform, and the same in every wave of the workgroup
          // the unit after (s, t): (s, t + 1), else (s + 1, 0), else the next super-tile's (0, 0)
          uint64_t nrow = 0;
          uint32_t ncol = 0;
          bool next = true;
          if (t + 1 < ntiles) {
            nrow = sup + kTile * (t + 1);
            ncol = s * KS;
          } else if (s + 1 < nslab) {
            nrow = sup;
            ncol = (s + 1) * KS;
          } else if (!last_sup) {
            nrow = sup + kTile * TT;
            ncol = 0;
          } else {
            next = false;
          }
          if (next) load_unit(nrow, ncol, stage);
          const __bf16 *tb = tile + buf * 2 * kHalf + col * kBPitch + h * (KS / 2);
#pragma unroll
          for (int st = 0; st < KS / 16; ++st) {
            const bf16x8 bh = *reinterpret_cast<const bf16x8 *>(tb + 8 * st);
            const bf16x8 bl = *reinterpret_cast<const bf16x8 *>(tb + kHalf + 8 * st);
            c[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[st], bh, c[t], 0, 0, 0);
            c[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[st], bl, c[t], 0, 0, 0);
            c[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[st], bh, c[t], 0, 0, 0);
          }
          if (next) {
            store_unit(buf ^ 1, ncol, stage);
            buf ^= 1;
          }
          __syncthreads();
        }
      }
    }
    // thresholds: two compares, the eligibility bit and a ballot per accumulator register; the registers with
    // a candidate bit leave their two ballots in the wave's LDS list and are settled below, in (tile, register)
    // order -- for any one query that is ascending row order
    uint64_t pending = 0;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      if (t < ntiles && el[t] != 0) {
        const bool eligible = (el[t] >> col) & 1u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = kIp ? -c[t][r] : (qn[r] + bn[t]) - 2.0f * c[t][r];
          const bool cand = eligible && !(d > hi[r]);  // NaN: the band
          const uint64_t cm = __ballot(cand);
          if (cm == 0ull) continue;
          const uint64_t sm = __ballot(eligible && d <= lo[r]);
          if (lane == 0) {
            pend[wave][t * 16 + r][0] = cm;
            pend[wave][t * 16 + r][1] = sm;
          }
          pending |= 1ull << (t * 16 + r);
        }
      }
    }
    if (pending != 0ull) {
      wave_fence();
      while (pending != 0ull) {
        const int idx = __builtin_ctzll(pending);
        pending &= pending - 1ull;
        const uint64_t cm = uniform64(pend[wave][idx][0]), sm = uniform64(pend[wave][idx][1]);
        const int t = idx >> 4, r = idx & 15;
        const int qs = (r & 3) + 8 * (r >> 2);
#pragma unroll 1
        for (int hh = 0; hh < 2; ++hh)
          settle(qs + 4 * hh, sup + kTile * t, static_cast<uint32_t>(cm >> (32 * hh)), static_cast<uint32_t>(sm >> (32 * hh)));
      }
      wave_fence();
    }
  }
  // the wave's counts and counters
  if (col + q0 < p.nq && h == 0) p.part_n[chunk * p.nq + q0 + col] = cntv;
  if (lane == 0) {
    uint32_t *ws = p.wave_stats + (chunk * (nq_up / 32) + q0 / 32) * 3;
    ws[0] = st_verified;
    ws[1] = st_band;
    ws[2] = st_proven;
  }
}

// One workgroup: the per-wave counters of a scan launch added to the call's three sums.
__global__ void __launch_bounds__(256) flat_range_mfma_reduce_kernel(const uint32_t *wave_stats, uint64_t waves,
                                                                     unsigned long long *stats) {
  __shared__ unsigned long long part[3][256];
  unsigned long long s[3] = {0, 0, 0};
  for (uint64_t i = threadIdx.x; i < waves; i += 256)
    for (int j = 0; j < 3; ++j) s[j] += wave_stats[i * 3 + j];
  for (int j = 0; j < 3; ++j) part[j][threadIdx.x] = s[j];
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
    for (int i = 0; i < 256; ++i) t += part[threadIdx.x][i];
    stats[threadIdx.x] += t;
  }
}

__global__ void flat_range_mfma_clear_kernel(unsigned long long *stats) {
  if (threadIdx.x < 3) stats[threadIdx.x] = 0;
}

// ---- host side -------------------------------------------------------------------------------------
FlatRangeMfmaPlan flat_range_mfma_plan(uint64_t n, uint64_t nq, uint32_t cap, uint32_t cus) {
  FlatRangeMfmaPlan r{};
  cap = std::min<uint32_t>(std::max<uint32_t>(cap, 1), kFlatRangeMaxCap);
  cus = std::max<uint32_t>(cus, 1);
  const uint64_t all = (std::max<uint64_t>(nq, 1) + kRangeMfmaQueries - 1) / kRangeMfmaQueries * kRangeMfmaQueries;
  r.sub_queries = all;
  if (n == 0) return r;
  const uint64_t tiles = (n + kRangeMfmaTileRows - 1) / kRangeMfmaTileRows;
  // a chunk is no shorter than twice its list: of a chunk full of hits at least half are counted without a distance
  const uint64_t min_rows = (2ull * cap + kRangeMfmaTileRows - 1) / kRangeMfmaTileRows * kRangeMfmaTileRows;
  // rows per chunk for `groups` query groups in flight: no more chunks than fill the CUs twice over
  const auto rows_for = [&](uint64_t groups, uint64_t most) {
    const uint64_t max_chunks = std::max<uint64_t>(1, std::min<uint64_t>(most, 2ull * cus / groups));
    return std::max(min_rows, kRangeMfmaTileRows * ((tiles + max_chunks - 1) / max_chunks));
  };
  const auto pair_bytes = [&](uint64_t rows) { return std::min<uint64_t>(cap, rows) * 8 + 4; };
  // all the queries in one launch where their lists fit the staging cap, else half as many, down to one
  // query group -- whose chunks are then as few as fit (the cap holds one group of one chunk at any list)
  uint64_t sub = all, rows = 0;
  for (;;) {
    rows = rows_for(sub / kRangeMfmaQueries, tiles);
    const uint64_t chunks = (n + rows - 1) / rows;
    if (chunks * sub * pair_bytes(rows) <= kFlatRangeStagingCap) break;
    if (sub == kRangeMfmaQueries) {
      const uint64_t most = std::max<uint64_t>(1, kFlatRangeStagingCap / (sub * (static_cast<uint64_t>(cap) * 8 + 4)));
      rows = rows_for(1, most);
      break;
    }
    sub = std::max<uint64_t>(kRangeMfmaQueries, sub / 2 / kRangeMfmaQueries * kRangeMfmaQueries);
  }
  r.chunk_rows = rows;
  r.chunks = (n + rows - 1) / rows;
  r.sub_queries = sub;
  r.slots = std::min<uint64_t>(cap, rows);
  r.staging_bytes = r.chunks * std::min(all, sub) * pair_bytes(rows);
  return r;
}

hipError_t launch_flat_range_mfma_prepare(const FlatRangeMfmaParams &p, hipStream_t s) {
  if (p.nq == 0 || p.qwidth == 0 || p.qwidth % kRangeMfmaKS != 0 || p.qwidth < p.dim) return hipErrorInvalidValue;
  const uint64_t nq_up = (p.nq + kRangeMfmaQueries - 1) / kRangeMfmaQueries * kRangeMfmaQueries;
  hipLaunchKernelGGL(flat_range_mfma_prepare_kernel, dim3(static_cast<uint32_t>(nq_up / 4)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_flat_range_mfma_scan(const FlatRangeMfmaParams &p, hipStream_t s) {
  if (p.nq == 0 || p.n == 0 || p.chunks == 0 || p.chunk_rows == 0 || p.chunk_rows % kRangeMfmaTileRows != 0)
    return hipErrorInvalidValue;
  if (p.chunks * p.chunk_rows < p.n || (p.chunks - 1) * p.chunk_rows >= p.n) return hipErrorInvalidValue;
  if (p.cap == 0 || p.cap > kFlatRangeMaxCap || p.slots == 0 || p.slots > p.cap) return hipErrorInvalidValue;
  if (p.stride < 4 || p.stride % 4 != 0 || p.qwidth != flat_range_mfma_width(p.stride) || p.dim > p.stride)
    return hipErrorInvalidValue;
  const uint64_t nqg = (p.nq + kRangeMfmaQueries - 1) / kRangeMfmaQueries;
  const uint64_t grid = 8 * nqg * ((p.chunks + 7) / 8);
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  if (p.ip)
    hipLaunchKernelGGL(flat_range_mfma_kernel<true>, dim3(static_cast<uint32_t>(grid)), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(flat_range_mfma_kernel<false>, dim3(static_cast<uint32_t>(grid)), dim3(256), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(flat_range_mfma_reduce_kernel, dim3(1), dim3(256), 0, s, p.wave_stats, p.chunks * nqg * 4, p.stats);
  return hipGetLastError();
}

hipError_t launch_flat_range_mfma_clear(unsigned long long *stats, hipStream_t s) {
  hipLaunchKernelGGL(flat_range_mfma_clear_kernel, dim3(1), dim3(64), 0, s, stats);
  return hipGetLastError();
}

}  // namespace alaya_amd
