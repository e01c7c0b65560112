// Launch interface of the small kernels behind alaya_index_extend_graph (extend_kernels.hip): what an
// appended block of rows needs besides the build kernels (build_kernels.h) -- its validity bits and,
// on an SQ8 index, its codes.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace alaya_amd {

// Set bits [first, first + count) of the validity bitmap (bit i%32 of word i/32).  The bitmap must
// hold word (first + count - 1) / 32.
hipError_t launch_set_valid_range(uint32_t *valid, uint64_t first, uint64_t count, hipStream_t stream);

// SQ8 codes of rows [first, first + count) from the f32 rows in HBM (`stride` floats per row) into
// the code array (`code_stride` bytes per row, a multiple of 4; bytes past `dim` are written as 0).
// SQ8Quantizer::quantize per element, alaya_sq8_encode's f32 operation order: mx == mn -> 0,
// v >= mx -> 255, v <= mn -> 0, else (uint8)(((v - mn) / (mx - mn)) * 255) with an IEEE division.
hipError_t launch_sq8_encode_rows(const float *base, uint32_t stride, uint32_t dim, const float *min_v,
                                  const float *max_v, uint8_t *codes, uint32_t code_stride, uint64_t first,
                                  uint64_t count, hipStream_t stream);

}  // namespace alaya_amd
