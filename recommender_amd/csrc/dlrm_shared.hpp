// dlrm_shared.hpp — what the DLRM kernel files share: the compact pair order of the interaction
// row and the pointer shuffle of the gather (interaction.hip, the training kernels; dlrm_score.hip,
// the serving kernel, places its pairs by compact_index), and the RS_Q8 element (dlrm_score.hip
// and embedding_q8.hip).
#pragma once
#include "common.hpp"

namespace rs {

// compact output index of kept pair (i,j) (row-major boolean_mask order, ctr/layers.py:39-42)
__device__ __forceinline__ int compact_index(int i, int j, int F, int self_i) {
  return self_i ? (i * (i + 1) / 2 + j) : (i * F - i * (i + 1) / 2 + (j - i - 1));
}
__host__ __device__ inline int out_width(int F, int self_i, int skip_gather) {
  return skip_gather ? F * F : (self_i ? F * (F + 1) / 2 : F * (F - 1) / 2);
}

// invert compact_index for the non-self (i < j) layout: row i starts at i*F - i(i+1)/2
__device__ __forceinline__ void compact_pair(int o, int F, int self_i, int& i, int& j) {
  if (self_i) {  // o = i(i+1)/2 + j, j <= i
    int ii = (int)((sqrtf(8.f * o + 1.f) - 1.f) * 0.5f);
    while (ii * (ii + 1) / 2 > o) --ii;
    while ((ii + 1) * (ii + 2) / 2 <= o) ++ii;
    i = ii;
    j = o - ii * (ii + 1) / 2;
  } else {
    const float b = 2.f * F - 1.f;
    int ii = (int)((b - sqrtf(b * b - 8.f * o)) * 0.5f);
    if (ii < 0) ii = 0;
    while (ii > 0 && ii * F - ii * (ii + 1) / 2 > o) --ii;
    while ((ii + 1) * F - (ii + 1) * (ii + 2) / 2 <= o) ++ii;
    i = ii;
    j = o - (ii * F - ii * (ii + 1) / 2) + ii + 1;
  }
}

__device__ __forceinline__ const float* shfl_ptr(const float* p, int src) {
  return reinterpret_cast<const float*>(__shfl(reinterpret_cast<long long>(p), src));
}

// code k (0..3) of the four in word w of an RS_Q8 row, dequantised: one rounded multiply, one
// rounded add, never an fma (include/recsys_hip.h a-1c)
__device__ __forceinline__ float q8_value(uint32_t w, int k, float scale, float bias) {
  return __fadd_rn(__fmul_rn((float)((w >> (8 * k)) & 0xffu), scale), bias);
}

}  // namespace rs
