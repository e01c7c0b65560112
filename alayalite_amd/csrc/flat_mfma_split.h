// The bf16 hi/lo split of the exact MFMA scans (flat_range_mfma_kernels.hip, flat_select_kernels.hip): x = hi + lo
// + a residual below 2^-16 |x|, and the fragment types of v_mfma_f32_32x32x16_bf16.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace alaya_amd {
namespace mfma_split {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split_bf16(float x, __bf16 &hi, __bf16 &lo) {
  hi = static_cast<__bf16>(x);
  lo = static_cast<__bf16>(x - static_cast<float>(hi));
}

}  // namespace mfma_split
}  // namespace alaya_amd
