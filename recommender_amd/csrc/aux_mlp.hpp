// aux_mlp.hpp — the Dense(80σ) → Dense(40σ) → Dense(1) net on v_mfma_f32_16x16x4_f32 (exact
// f32), shared by the DIEN auxiliary loss (dien_aux.hip) and DIN's local activation unit
// (din_activation.hip).
//
// MFMA layout: activations are kept TRANSPOSED — a 16-row tile is the N side, units the M side —
// so the C layout of one layer (lane = (row j, unit group kq), 4 consecutive units per lane) is
// directly the B operand of the next layer when the K axis is walked as (tile u, register r): no
// transposes between layers. Weights sit in LDS and are read as A operands with the matching
// permutation.
#pragma once
#include "common.hpp"

namespace rs {
namespace {

constexpr int kN1 = 80, kN2 = 40;  // AuxiliaryNet([80, 40, 1])
constexpr int kT1 = 5, kT2 = 3;    // 16-unit tiles of the two hidden layers (40 padded to 48)
constexpr int kMaxIn = 80, kMaxKS = kMaxIn / 4;
constexpr int kW1S = 81, kW2S = 49;  // LDS row strides: W1 [In][80], W2 [80][48] (bank spread)
constexpr int kS1 = 81, kS2 = 49;    // wave scratch strides: [16 rows][80] and [16 rows][48]
constexpr int kWaves = 4;

struct AuxLds {
  float w1[kMaxIn * kW1S];
  float w2[kN1 * kW2S];
  float b1[kN1], b2[48], w3[48];
};

// σ with the hardware exp2 / reciprocal (≈1-2 ulp; the parity tests bound the net at 1e-5)
__device__ __forceinline__ float aux_sigm(float x) {
  return __builtin_amdgcn_rcpf(1.f + __expf(-x));
}

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// W1 [In][80] into LDS rows of stride kW1S, zero rows from In to `rows`
__device__ __forceinline__ void stage_w1(float* w1s, int rows, int In, const float* W1) {
  for (int i = threadIdx.x; i < rows * kN1; i += blockDim.x) {
    const int f = i / kN1, u = i % kN1;
    w1s[f * kW1S + u] = f < In ? W1[f * kN1 + u] : 0.f;
  }
}

// W2 [80][40] into LDS rows of stride kW2S, columns padded to 48 with zeros
__device__ __forceinline__ void stage_w2(float* w2s, const float* W2) {
  for (int i = threadIdx.x; i < kN1 * 48; i += blockDim.x) {
    const int u = i / 48, v = i % 48;
    w2s[u * kW2S + v] = v < kN2 ? W2[u * kN2 + v] : 0.f;
  }
}

// b2 and W3, padded to 48 with zeros
__device__ __forceinline__ void stage_b2_w3(float* b2s, float* w3s, const float* b2,
                                            const float* W3) {
  for (int i = threadIdx.x; i < 48; i += blockDim.x) {
    b2s[i] = i < kN2 ? b2[i] : 0.f;
    w3s[i] = i < kN2 ? W3[i] : 0.f;
  }
}

// Layer 1 without its bias: h1ᵀ = W1ᵀ·xᵀ for the tile's row j = lane & 15; xv[k] is feature
// 4k + kq of the row (C layout, 5 tiles)
template <int KS>
__device__ __forceinline__ void mlp3_layer1(const float* w1s, const float (&xv)[KS], int j, int kq,
                                            f4 (&h1)[kT1]) {
#pragma unroll
  for (int u = 0; u < kT1; ++u) h1[u] = f4{0.f, 0.f, 0.f, 0.f};
  const float* w1 = w1s + kq * kW1S + j;
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    const float* w = w1 + 4 * k * kW1S;  // A: W1[4k + kq][16u + j]
#pragma unroll
    for (int u = 0; u < kT1; ++u) h1[u] = mfma4(w[16 * u], xv[k], h1[u]);
  }
}

// From the activated h1: h2 (3 tiles, activated) and the logit of row j (identical in the four
// kq lanes of the row)
__device__ __forceinline__ float mlp3_tail(const float* w2s, const float* b2s, const float* w3s,
                                           const float* b3, int j, int kq, const f4 (&h1)[kT1],
                                           f4 (&h2)[kT2]) {
#pragma unroll
  for (int m = 0; m < kT2; ++m) h2[m] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < kT1; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* w = w2s + (16 * u + 4 * kq + r) * kW2S + j;  // A: W2[16u+4kq+r][16m + j]
#pragma unroll
      for (int m = 0; m < kT2; ++m) h2[m] = mfma4(w[16 * m], h1[u][r], h2[m]);
    }
  float p = 0.f;
#pragma unroll
  for (int m = 0; m < kT2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int v = 16 * m + 4 * kq + r;
      h2[m][r] = aux_sigm(h2[m][r] + b2s[v]);
      p = fmaf(h2[m][r], w3s[v], p);
    }
  p += __shfl_xor(p, 16);
  p += __shfl_xor(p, 32);
  return p + b3[0];
}

__device__ __forceinline__ void store4(float* p, f4 v) {  // 16-byte aligned global rows
  *reinterpret_cast<f4*>(p) = v;
}
__device__ __forceinline__ void lds4(float* p, f4 v) {  // odd-stride LDS tile: 4 dword writes
  p[0] = v[0];
  p[1] = v[1];
  p[2] = v[2];
  p[3] = v[3];
}

}  // namespace
}  // namespace rs
