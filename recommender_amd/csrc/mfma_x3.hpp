// mfma_x3.hpp — fp32 products on the bf16 MFMA: each operand is split into three bf16 parts and
// the six largest cross products are accumulated in fp32 (gemm.hip, the DLRM train kernel).
#pragma once
#include "common.hpp"

namespace rs {

// x = h + m + l with h, m, l bf16 (one v_cvt_pk_bf16_f32 and one v_pk_add_f32 per step, round to
// nearest): the two residuals are exact in fp32 and l carries x's bits below 2^-16 |x| to
// 2^-24 |x|.
__device__ __forceinline__ void split_pair(const f2 x, bf2& h, bf2& m, bf2& l) {
  h = __builtin_convertvector(x, bf2);
  const f2 r1 = x - __builtin_convertvector(h, f2);
  m = __builtin_convertvector(r1, bf2);
  l = __builtin_convertvector(r1 - __builtin_convertvector(m, f2), bf2);
}

// c + A·B from the split operands: the six products down to 2^-16 |a||b|, smallest first
__device__ __forceinline__ f4 mfma6(const bf8& ah, const bf8& am, const bf8& al, const bf8& bh,
                                    const bf8& bm, const bf8& bl, f4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bm, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bm, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bh, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
}

}  // namespace rs
