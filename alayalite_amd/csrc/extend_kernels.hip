// MI355X (gfx950) device code for the rows alaya_index_extend_graph appends (see extend_kernels.h).
// Both kernels touch a few bytes per appended element once per call: plain grid-stride loops.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "extend_kernels.h"

namespace alaya_amd {

namespace {

constexpr int kThreads = 256;
constexpr uint64_t kMaxBlocks = 4096;

// one thread per bitmap word that holds a bit of [first, end); the two edge words are shared with
// rows outside the range, so every word takes an atomic OR of the bits it owns
__global__ void __launch_bounds__(kThreads) set_valid_range_kernel(uint32_t *valid, uint64_t first, uint64_t end) {
  const uint64_t w0 = first >> 5, w1 = (end - 1) >> 5;
  for (uint64_t w = w0 + static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; w <= w1;
       w += static_cast<uint64_t>(gridDim.x) * kThreads) {
    const uint64_t lo = std::max<uint64_t>(first, w << 5) - (w << 5);   // 0..31
    const uint64_t hi = std::min<uint64_t>(end, (w + 1) << 5) - (w << 5);  // 1..32
    const uint32_t mask = static_cast<uint32_t>(((1ull << hi) - 1ull) & ~((1ull << lo) - 1ull));
    atomicOr(&valid[w], mask);
  }
}

__device__ __forceinline__ uint32_t sq8_code(float v, float mn, float mx) {
  if (mx == mn) return 0u;
  if (v >= mx) return 255u;
  if (v <= mn) return 0u;
  return static_cast<uint32_t>(static_cast<uint8_t>(((v - mn) / (mx - mn)) * 255));
}

// one thread per 4 consecutive codes of a row (one aligned 32-bit store)
__global__ void __launch_bounds__(kThreads) sq8_encode_rows_kernel(const float *base, uint32_t stride, uint32_t dim,
                                                                   const float *min_v, const float *max_v,
                                                                   uint8_t *codes, uint32_t code_stride,
                                                                   uint64_t first, uint64_t count) {
  const uint32_t quads = code_stride / 4;
  const uint64_t items = count * quads;
  for (uint64_t it = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; it < items;
       it += static_cast<uint64_t>(gridDim.x) * kThreads) {
    const uint64_t row = first + it / quads;
    const uint32_t j0 = static_cast<uint32_t>(it % quads) * 4;
    const float *src = base + row * stride;
    uint32_t word = 0;
    for (uint32_t b = 0; b < 4; ++b) {
      const uint32_t j = j0 + b;
      if (j < dim) word |= sq8_code(src[j], min_v[j], max_v[j]) << (8 * b);
    }
    *reinterpret_cast<uint32_t *>(codes + row * code_stride + j0) = word;
  }
}

int blocks_for(uint64_t items) {
  return static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>(kMaxBlocks, (items + kThreads - 1) / kThreads)));
}

}  // namespace

hipError_t launch_set_valid_range(uint32_t *valid, uint64_t first, uint64_t count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  const uint64_t end = first + count;
  const uint64_t words = ((end - 1) >> 5) - (first >> 5) + 1;
  hipLaunchKernelGGL(set_valid_range_kernel, dim3(blocks_for(words)), dim3(kThreads), 0, stream, valid, first, end);
  return hipGetLastError();
}

hipError_t launch_sq8_encode_rows(const float *base, uint32_t stride, uint32_t dim, const float *min_v,
                                  const float *max_v, uint8_t *codes, uint32_t code_stride, uint64_t first,
                                  uint64_t count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  if (code_stride % 4 != 0 || code_stride < dim) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sq8_encode_rows_kernel, dim3(blocks_for(count * (code_stride / 4))), dim3(kThreads), 0, stream,
                     base, stride, dim, min_v, max_v, codes, code_stride, first, count);
  return hipGetLastError();
}

}  // namespace alaya_amd
