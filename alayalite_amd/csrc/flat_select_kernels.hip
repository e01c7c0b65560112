// Exact k-NN for k above the register-list limit: a histogram-select scan on the MFMA units.
//
//   scan    flat_select_hist_kernel<kIp>: the work split and the streaming pass that flat_mfma_scan.h describes,
//           with the eligibility word validity AND below n, and d~ in the same operation order, so a pair's d~
//           has the bits the range scan will compare.  The epilogue:
//             histogram mode  each query of the workgroup has a window [lo, hi) and an inverse bin width in LDS
//                             and a histogram of 256 bins + a `below` counter there (128 x 257 x 4 B = 128.5 KB
//                             beside the 18 KB of tile buffers: one workgroup per CU, which the scan runs at
//                             anyway -- its waves hold ~250 VGPRs).  Per accumulator register a lane holds one
//                             (query, row) pair: eligible and d~ < lo adds 1 to `below`, lo <= d~ < hi adds 1 to
//                             bin min(floor((d~ - lo) inv), 255) with an LDS atomic; the rest is dropped (a NaN
//                             compares false twice).  The pitch of 257 words spreads the 32 queries of a wave
//                             over the banks; lanes of one query that meet in a bin are serialised by the LDS,
//                             which costs little once the window is narrow: most pairs lie above hi.  At the end of
//                             the chunk the non-zero counters are added to the call's histograms with global
//                             vector atomics: integer sums, the same whatever the order.
//             span mode       per accumulator register a running min / max of the eligible d~, reduced over
//                             the 32 rows of a tile by shuffles at the end of the chunk and folded into the
//                             call's per-query (min, max) with atomic min / max on order-preserving keys; the
//                             workgroups of query group 0 count the eligible rows they met.
//           p.sup_step > 1 walks every sup_step-th super-tile of the chunk: a strided sample of whole tiles.
//   pick    one thread per query: the bin b that holds rank k (below + bins 0..b >= k), its upper edge e and
//           lower edge lo' as *floats found by bisection on the bin function itself* -- e is the smallest float
//           whose bin is above b -- so "d~ < e" is exactly "counted in `below` or bins 0..b" whatever the
//           roundings of (d~ - lo) inv, and the next window [lo', e) holds exactly bin b's pairs.
//   radius  one thread per query: the smallest f32 radius r with flat_range_bound(r).lo >= e, by bisection on
//           the ordered floats (lo is monotone in r).  Every pair counted below e is then proven inside r.
//   cut     the first k of each sorted list.
#include "flat_select_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "flat_mfma_scan.h"
#include "flat_range_bound.h"

namespace alaya_amd {

namespace {

using namespace mfma_scan;

constexpr int kBins = kSelectBins;
constexpr int kPitch = kSelectPitch;

// floats as unsigned keys in the floats' order (-inf lowest; -0 just below +0)
__device__ __forceinline__ uint32_t float_key(float x) {
  const uint32_t b = static_cast<uint32_t>(__float_as_int(x));
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __int_as_float(static_cast<int>((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k));
}

// The bin of d in the window that starts at lo: non-decreasing in d (a rounded subtraction, a rounded product
// with inv >= 0, a clamp and a truncation are each monotone; a NaN from 0 x inf or inf x 0 clamps to bin 0,
// which only lo itself or a window without a finite width can produce).
__device__ __forceinline__ int select_bin(float d, float lo, float inv) {
  return static_cast<int>(fminf(fmaxf((d - lo) * inv, 0.f), static_cast<float>(kBins - 1)));
}

// the smallest float in [lo, hi] whose bin is at least t, or hi where none is
__device__ float bin_edge(float lo, float hi, float inv, int t) {
  if (select_bin(hi, lo, inv) < t) return hi;
  uint32_t a = float_key(lo), b = float_key(hi);
  while (a < b) {
    const uint32_t mid = a + (b - a) / 2;
    if (select_bin(key_float(mid), lo, inv) >= t) b = mid; else a = mid + 1;
  }
  return key_float(a);
}

__device__ __forceinline__ float window_inv(float lo, float hi) { return static_cast<float>(kBins) / (hi - lo); }

}  // namespace

template <bool kIp>
__global__ void __launch_bounds__(256) flat_select_hist_kernel(FlatSelectParams p) {
  __shared__ __attribute__((aligned(16))) __bf16 tile[kTileLds];
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // histogram mode: 128 x 257 counters, 3 x 128 window floats
  uint32_t *hist = reinterpret_cast<uint32_t *>(smem);
  float *win = reinterpret_cast<float *>(smem + sizeof(uint32_t) * kMfmaScanQueries * kPitch);
  const int lane = __lane_id();
  const int wave = threadIdx.x >> 6;
  const int col = lane & 31, h = lane >> 5;
  const uint64_t nq_up = mfma_scan_queries_up(p.nq);
  const uint32_t nqg = static_cast<uint32_t>(nq_up / kMfmaScanQueries);
  // XCD-aware block -> (query group, chunk): the query groups of one chunk share an XCD label
  const uint32_t b = blockIdx.x;
  const uint32_t qg = (b / 8) % nqg;
  const uint64_t chunk = (b % 8) + 8ull * (b / (8 * nqg));
  if (chunk >= p.chunks) return;
  const uint64_t r0 = chunk * p.chunk_rows;
  const uint64_t r1 = min(p.n, r0 + p.chunk_rows);  // r0 < r1: the chunks cover n
  const uint64_t sup_rows = static_cast<uint64_t>(kTile * TT) * p.sup_step;
  const int nslab = static_cast<int>(p.qwidth / KS);
  const uint64_t qg0 = static_cast<uint64_t>(qg) * kMfmaScanQueries;
  const uint64_t q0 = qg0 + wave * 32;  // the wave's first query
  const bool span = p.span != 0;        // uniform over the launch

  if (!span) {
    for (int i = threadIdx.x; i < static_cast<int>(kMfmaScanQueries) * kPitch; i += 256) hist[i] = 0;
    for (int i = threadIdx.x; i < static_cast<int>(kMfmaScanQueries) * 3; i += 256)
      win[i] = p.win[static_cast<uint64_t>(i / kMfmaScanQueries) * nq_up + qg0 + i % kMfmaScanQueries];
  }
  // per accumulator register: |q|^2 of its query (L2), and the span mode's running min / max
  float qn[16], mn[16], mx[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    qn[r] = kIp ? 0.f : p.qmeta[query_slot(q0, r, h)];
    mn[r] = INFINITY;
    mx[r] = -INFINITY;
  }
  uint32_t met = 0;  // eligible rows of the chunk's scanned tiles

  const float4 *qrow = reinterpret_cast<const float4 *>(p.qpad + (q0 + col) * p.qwidth + h * (KS / 2));
  float4 an[KS / 8];
  auto load_a = [&](int s) {
#pragma unroll
    for (int j = 0; j < KS / 8; ++j) an[j] = qrow[s * (KS / 4) + j];
  };

  // cooperative unit load: 32 rows x KS columns, 256 threads, float4 each; rows past n read row n - 1 (their
  // eligibility bits are clear), columns past stride are zeroed when stored
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

  float4 stage[kPerThread];
  load_a(0);
  load_unit(r0, 0, stage);
  store_unit(0, 0, stage);
  __syncthreads();  // (and the cleared histograms, the windows)
  int buf = 0;
  for (uint64_t sup = r0; sup < r1; sup += sup_rows) {
    const int ntiles = static_cast<int>(min<uint64_t>(TT, (r1 - sup + kTile - 1) / kTile));
    const bool last_sup = sup + sup_rows >= r1;
    float bn[TT];
    uint32_t el[TT];  // the tiles' eligibility words: validity AND below n
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const uint64_t row0 = sup + kTile * t;
      bn[t] = kIp ? 0.f : p.norms[min<uint64_t>(row0 + col, p.n - 1)];
      uint32_t w = 0;
      if (row0 < r1) {
        w = p.valid != nullptr ? p.valid[row0 >> 5] : 0xffffffffu;
        if (p.n - row0 < 32) w &= (1u << (p.n - row0)) - 1u;
      }
      el[t] = w;
      met += __popc(w);
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
          // the unit after (s, t): (s, t + 1), else (s + 1, 0), else the next scanned super-tile's (0, 0)
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
            nrow = sup + sup_rows;
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
    // the epilogue: a lane holds the pair (query (r & 3) + 8 (r >> 2) + 4 h of the wave, row col of tile t) in
    // register r of tile t
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      if (t < ntiles && el[t] != 0) {
        const bool eligible = (el[t] >> col) & 1u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = approx_distance<kIp>(qn[r], bn[t], c[t][r]);
          if (span) {
            mn[r] = fminf(mn[r], eligible ? d : INFINITY);
            mx[r] = fmaxf(mx[r], eligible ? d : -INFINITY);
          } else if (eligible) {
            const int qs = query_slot(wave * 32, r, h);
            const float wl = win[qs], wh = win[kMfmaScanQueries + qs], iv = win[2 * kMfmaScanQueries + qs];
            if (d < wl)
              atomicAdd(&hist[qs * kPitch + kBins], 1u);
            else if (d < wh)
              atomicAdd(&hist[qs * kPitch + select_bin(d, wl, iv)], 1u);
          }
        }
      }
    }
  }
  if (span) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float a = mn[r], z = mx[r];
      for (int x = 16; x > 0; x >>= 1) {  // over the 32 rows; the two halves hold different queries
        a = fminf(a, __shfl_xor(a, x));
        z = fmaxf(z, __shfl_xor(z, x));
      }
      if (col == 0 && a <= z) {  // (an empty or all-NaN register: nothing)
        const uint64_t qi = query_slot(q0, r, h);
        atomicMin(&p.span_keys[qi], float_key(a));
        atomicMax(&p.span_keys[nq_up + qi], float_key(z));
      }
    }
    if (qg == 0 && threadIdx.x == 0 && met != 0) atomicAdd(p.eligible, met);
  } else {
    __syncthreads();
    for (int i = threadIdx.x; i < static_cast<int>(kMfmaScanQueries) * kPitch; i += 256) {
      const uint32_t v = hist[i];
      if (v != 0) atomicAdd(&p.hist[qg0 * kPitch + i], v);
    }
  }
}

// ---- the small kernels: one thread per query of the launch (rounded up to whole query groups) --------
__global__ void flat_select_init_kernel(FlatSelectParams p, uint64_t nq_up) {
  const uint64_t q = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q == 0) *p.eligible = 0;
  if (q >= nq_up) return;
  p.span_keys[q] = 0xffffffffu;
  p.span_keys[nq_up + q] = 0u;
  p.win[q] = p.win[nq_up + q] = p.win[2 * nq_up + q] = 0.f;
  p.done[q] = q < p.nq ? kSelectRunning : kSelectDone;
  p.edge[q] = INFINITY;
  p.cum[q] = 0;
}

__global__ void flat_select_clear_kernel(uint32_t *hist, uint64_t words) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < words) hist[i] = 0;
}

// the first window [min, the float after max): every sampled eligible d~ lies in it
__global__ void flat_select_window_kernel(FlatSelectParams p, uint64_t nq_up) {
  const uint64_t q = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q >= p.nq) return;
  const uint32_t ka = p.span_keys[q], kz = p.span_keys[nq_up + q];
  if (ka > kz) {  // no comparable d~ at all
    p.done[q] = kSelectFallback;
    return;
  }
  const float lo = key_float(ka), hi = flat_range_step(key_float(kz), true);
  if (!(lo < hi)) {  // max = +inf
    p.done[q] = kSelectFallback;
    return;
  }
  p.win[q] = lo;
  p.win[nq_up + q] = hi;
  p.win[2 * nq_up + q] = window_inv(lo, hi);
}

__global__ void flat_select_pick_kernel(FlatSelectParams p, uint64_t nq_up, uint32_t k, uint32_t target, int sample) {
  const uint64_t q = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q >= p.nq || p.done[q] != kSelectRunning) return;
  const uint32_t *hq = p.hist + q * kPitch;
  const float lo = p.win[q], hi = p.win[nq_up + q], inv = p.win[2 * nq_up + q];
  uint64_t c = hq[kBins];
  if (c >= k) {  // rank k lies below the window (rows the sample missed): lo is an edge, nothing narrower is known
    if (sample) return;
    p.edge[q] = lo;
    p.cum[q] = static_cast<uint32_t>(min<uint64_t>(c, 0xffffffffull));
    p.done[q] = kSelectDone;
    return;
  }
  int bin = -1;
  for (int i = 0; i < kBins; ++i) {
    c += hq[i];
    if (c >= k) {
      bin = i;
      break;
    }
  }
  if (bin < 0) {  // fewer than k comparable pairs below hi
    p.done[q] = kSelectFallback;
    return;
  }
  const float e = bin == kBins - 1 ? hi : bin_edge(lo, hi, inv, bin + 1);
  if (sample) {  // at least k sampled rows have d~ < e, so at least k rows have: [lo, e) is the window to count
    p.win[nq_up + q] = e;
    p.win[2 * nq_up + q] = window_inv(lo, e);
    return;
  }
  const float nlo = bin == 0 ? lo : bin_edge(lo, hi, inv, bin);
  p.edge[q] = e;
  p.cum[q] = static_cast<uint32_t>(min<uint64_t>(c, 0xffffffffull));
  if (c <= target || (nlo == lo && e == hi) || !(nlo < e)) {  // met, or the bin cannot be split: ties in d~
    p.done[q] = kSelectDone;
    return;
  }
  p.win[q] = nlo;
  p.win[nq_up + q] = e;
  p.win[2 * nq_up + q] = window_inv(nlo, e);
}

// the smallest radius whose proven-inside threshold reaches the edge; +inf where there is no edge or no bound
__global__ void flat_select_radius_kernel(FlatSelectParams p, int all_inf) {
  const uint64_t q = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q >= p.nq) return;
  float r = INFINITY;
  const float e = p.edge[q];
  if (!all_inf && p.done[q] != kSelectFallback && e < INFINITY) {
    const float qn = p.qmeta[q];
    const auto reaches = [&](float rad) {
      return flat_range_bound(p.ip != 0, rad, qn, p.max_norm, p.qwidth, kFlatSplit).lo >= e;
    };
    if (reaches(INFINITY)) {
      uint32_t a = float_key(e), b = float_key(INFINITY);  // lo(r) <= r: no radius below e reaches it
      while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (reaches(key_float(mid))) b = mid; else a = mid + 1;
      }
      r = key_float(a);
    }
  }
  p.radii[q] = r;
}

__global__ void flat_select_cut_kernel(const uint32_t *counts, const uint32_t *ids, const float *dists, uint32_t cap,
                                       uint32_t k, uint32_t *out_ids, float *out_dists) {
  const uint64_t q = blockIdx.x;
  const uint32_t have = min(min(counts[q], cap), k);
  for (uint32_t j = threadIdx.x; j < k; j += blockDim.x) {
    out_ids[q * k + j] = j < have ? ids[q * cap + j] : 0xffffffffu;
    out_dists[q * k + j] = j < have ? dists[q * cap + j] : FLT_MAX;
  }
}

// ---- host side -------------------------------------------------------------------------------------
namespace {
uint64_t select_nq_up(const FlatSelectParams &p) { return mfma_scan_queries_up(p.nq); }
uint32_t per_query_grid(uint64_t nq_up) { return static_cast<uint32_t>((nq_up + 255) / 256); }
bool per_query_ok(const FlatSelectParams &p) { return p.nq != 0 && p.nq <= 0x7fffffffull; }
}  // namespace

hipError_t launch_flat_select_init(const FlatSelectParams &p, hipStream_t s) {
  if (!per_query_ok(p)) return hipErrorInvalidValue;
  const uint64_t nq_up = select_nq_up(p);
  hipLaunchKernelGGL(flat_select_init_kernel, dim3(per_query_grid(nq_up)), dim3(256), 0, s, p, nq_up);
  return hipGetLastError();
}

hipError_t launch_flat_select_scan(const FlatSelectParams &p, hipStream_t s) {
  const uint32_t grid = mfma_scan_grid(p.nq, p.n, p.chunk_rows, p.chunks, p.dim, p.stride, p.qwidth);
  if (grid == 0) return hipErrorInvalidValue;
  if (p.sup_step == 0 || p.sup_step > 0xffffu) return hipErrorInvalidValue;
  const size_t lds = p.span ? 0 : kSelectHistLds;
  if (p.ip)
    hipLaunchKernelGGL(flat_select_hist_kernel<true>, dim3(grid), dim3(256), lds, s, p);
  else
    hipLaunchKernelGGL(flat_select_hist_kernel<false>, dim3(grid), dim3(256), lds, s, p);
  return hipGetLastError();
}

hipError_t launch_flat_select_window(const FlatSelectParams &p, hipStream_t s) {
  if (!per_query_ok(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(flat_select_window_kernel, dim3(per_query_grid(p.nq)), dim3(256), 0, s, p, select_nq_up(p));
  return hipGetLastError();
}

hipError_t launch_flat_select_clear(const FlatSelectParams &p, hipStream_t s) {
  if (!per_query_ok(p)) return hipErrorInvalidValue;
  const uint64_t words = select_nq_up(p) * kSelectPitch;
  hipLaunchKernelGGL(flat_select_clear_kernel, dim3(static_cast<uint32_t>((words + 255) / 256)), dim3(256), 0, s, p.hist, words);
  return hipGetLastError();
}

hipError_t launch_flat_select_pick(const FlatSelectParams &p, uint32_t k, uint32_t target, int sample, hipStream_t s) {
  if (!per_query_ok(p) || k == 0 || target < k) return hipErrorInvalidValue;
  hipLaunchKernelGGL(flat_select_pick_kernel, dim3(per_query_grid(p.nq)), dim3(256), 0, s, p, select_nq_up(p), k, target, sample);
  return hipGetLastError();
}

hipError_t launch_flat_select_radius(const FlatSelectParams &p, int all_inf, hipStream_t s) {
  if (!per_query_ok(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(flat_select_radius_kernel, dim3(per_query_grid(p.nq)), dim3(256), 0, s, p, all_inf);
  return hipGetLastError();
}

hipError_t launch_flat_select_cut(const uint32_t *counts, const uint32_t *ids, const float *dists, uint32_t cap, uint64_t nq,
                                  uint32_t k, uint32_t *out_ids, float *out_dists, hipStream_t s) {
  if (nq == 0 || nq > 0x7fffffffull || k == 0 || k > cap) return hipErrorInvalidValue;
  hipLaunchKernelGGL(flat_select_cut_kernel, dim3(static_cast<uint32_t>(nq)), dim3(256), 0, s, counts, ids, dists, cap, k,
                     out_ids, out_dists);
  return hipGetLastError();
}

}  // namespace alaya_amd
