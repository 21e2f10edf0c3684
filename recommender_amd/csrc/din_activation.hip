// din_activation.hip — DIN's LocalActivationUnit (dien/layers.py:34-59) forward and backward as
// fused kernels on the exact-f32 MFMA layer core of the DIEN aux net (aux_mlp.hpp).
//
// Per example b (target t = target[b]) and history step h = his[b, step]:
//   w[b,step] = σ(σ([t, h, t−h, t⊙h]·W1 + b1)·W2 + b2)·W3 + b3,  rep[b] = Σ_step m·w·h
// The FOLDED form is built: with W1 = [Wa; Wb; Wc; Wd] (four [D, 80] blocks)
//   z1 = [h, t⊙h]·[Wb − Wc; Wd] + (b1 + t·(Wa + Wc))
// so a row is an aux-net row with In = 2D and a per-example layer-1 bias c_b = b1 + t_b·(Wa+Wc).
// A prep kernel writes W1f = [Wb − Wc; Wd; Wa + Wc] ([3D, 80]) and c [B, 80] (one thread per
// (b, unit), features in order: an example's bias does not depend on the rest of the batch).
//
// Work: one wave per example, four examples per block round, persistent blocks with the weights
// staged once. Only 16-step tiles that hold a valid step are evaluated (masks may have holes: a
// tile is live if any of its rows is). A masked row is SELECTED to zero where it is read, so it
// adds exactly 0 whatever its history row holds.
//
// Backward: recomputes the forward of each live tile; d3 = m·(drep·h), then dz2, dz1 as the aux
// net. The input gradient runs against all 3D rows of W1f: the [h] and [t⊙h] parts give dhis, the
// [t⊙h] and [t] parts summed over the example's rows give dtarget (registers, tile order). The
// weight gradients run against x = [h, t⊙h, t, 1]: rows [2D, 3D) are Σ_b t_b ⊗ Σ_step dz1, the
// target-side term of dWa and dWc, and row 3D is db1. Per-block partials in MFMA C tiles, folded
// in a fixed order (fold_two_level), then unfolded to the reference's W1 row order.
#include <algorithm>

#include "aux_mlp.hpp"

namespace rs {

namespace {

constexpr int kFwdBlocksPerCU = 3;  // 43 KB of LDS each
constexpr int kTilesW2 = kT1 * kT2;  // dW2: 5 × 3 tiles

struct DinArgs {
  const float* target;  // [B, D]
  const float* his;     // [B, L, D]
  const uint8_t* mask;  // [B, L]
  int64_t B;
  int L;
  const float *W1f, *cb;             // workspace: [3D, 80] folded weights, [B, 80] biases
  const float *W2, *b2, *W3, *b3;    // [80, 40], [40], [40], [1]
};

template <int D>
__global__ __launch_bounds__(256) void din_prep_kernel(const float* __restrict__ W1,
                                                       const float* __restrict__ b1,
                                                       const float* __restrict__ target, int64_t B,
                                                       float* __restrict__ W1f,
                                                       float* __restrict__ cb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3 * D * kN1) {
    const int f = (int)(i / kN1), u = (int)(i % kN1);
    float v;
    if (f < D) v = W1[(D + f) * kN1 + u] - W1[(2 * D + f) * kN1 + u];      // Wb − Wc
    else if (f < 2 * D) v = W1[(2 * D + f) * kN1 + u];                      // Wd
    else v = W1[(f - 2 * D) * kN1 + u] + W1[f * kN1 + u];                   // Wa + Wc
    W1f[i] = v;
  }
  if (i < B * kN1) {
    const int64_t b = i / kN1;
    const int u = (int)(i % kN1);
    float acc = b1[u];
    for (int d = 0; d < D; ++d)
      acc = fmaf(target[b * D + d], W1[d * kN1 + u] + W1[(2 * D + d) * kN1 + u], acc);
    cb[i] = acc;
  }
}

// ---------------------------------------------------------------------------------------
// forward: wave = example; rep accumulated per lane (row j, features kq + 4s) over the live
// tiles in order, then summed over the 16 rows by a fixed butterfly
// ---------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void din_fwd_kernel(DinArgs a, float* __restrict__ rep) {
  __shared__ AuxLds s;  // b1 unused: the bias is per example
  stage_w1(s.w1, kMaxIn, 2 * D, a.W1f);
  stage_w2(s.w2, a.W2);
  stage_b2_w3(s.b2, s.w3, a.b2, a.W3);
  __syncthreads();
  const int lane = threadIdx.x & 63, j = lane & 15, kq = lane >> 4, wave = threadIdx.x >> 6;
  constexpr int Q = D / 4;
  const int L = a.L;
  const int NT = (L + 15) / 16;
  const int64_t n_rounds = (a.B + kWaves - 1) / kWaves;
  for (int64_t rd = blockIdx.x; rd < n_rounds; rd += gridDim.x) {
    const int64_t b = rd * kWaves + wave;
    if (b >= a.B) continue;  // wave-uniform; no block barrier in the loop
    f4 cbv[kT1];
#pragma unroll
    for (int u = 0; u < kT1; ++u)
      cbv[u] = *reinterpret_cast<const f4*>(a.cb + b * kN1 + 16 * u + 4 * kq);
    float tv[Q], racc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      tv[q] = a.target[b * D + kq + 4 * q];
      racc[q] = 0.f;
    }
    for (int tile = 0; tile < NT; ++tile) {
      const int t = 16 * tile + j;
      const int tc = t < L ? t : 0;  // loads unguarded from an in-bounds row, masked at use
      const bool m = t < L && a.mask[b * L + tc] != 0;
      if (__ballot(m) == 0) continue;  // no valid row: the tile adds exactly 0
      float xv[2 * Q];
      const float* hr = a.his + (b * L + tc) * (int64_t)D + kq;
#pragma unroll
      for (int q = 0; q < Q; ++q) xv[q] = hr[4 * q];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        xv[q] = m ? xv[q] : 0.f;
        xv[Q + q] = tv[q] * xv[q];
      }
      f4 h1[kT1], h2[kT2];
      mlp3_layer1<2 * Q>(s.w1, xv, j, kq, h1);
#pragma unroll
      for (int u = 0; u < kT1; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) h1[u][r] = aux_sigm(h1[u][r] + cbv[u][r]);
      const float z = mlp3_tail(s.w2, s.b2, s.w3, a.b3, j, kq, h1, h2);
      const float w = m ? z : 0.f;
#pragma unroll
      for (int q = 0; q < Q; ++q) racc[q] = fmaf(w, xv[q], racc[q]);
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
#pragma unroll
      for (int q = 0; q < Q; ++q) racc[q] += __shfl_xor(racc[q], off);
    if (j == 0) {
#pragma unroll
      for (int q = 0; q < Q; ++q) rep[b * D + kq + 4 * q] = racc[q];
    }
  }
}

// ---------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------
template <int D>
struct DinCfg {
  static constexpr int In2 = 2 * D, In3 = 3 * D;
  static constexpr int XT = (In3 + 1 + 15) / 16;  // dW1 feature tiles over [h, t⊙h, t, 1]
  static constexpr int XD = (In3 + 15) / 16;      // input-gradient tiles over [h, t⊙h, t]
  static constexpr int W1R = 16 * XT;             // W1f rows in LDS (zero from 3D)
  static constexpr int NTV = W1R - In2;           // [t, 1, 0...]: the row-independent features
  static constexpr int TW1 = XT * kT1;
  static constexpr int TPW = (TW1 + kTilesW2 + kWaves - 1) / kWaves;  // tiles per wave
  static constexpr int DS = D + 1;                // stride of the [16][D] t⊙h gradient tile
  static_assert(D % 4 == 0 && In2 <= kMaxIn - 4, "width");
};

template <int D>
struct DinSet {
  float x[16 * kS1];  // [row][feature]: [h, t⊙h]
  float h1[16 * kS1];
  float dz1[16 * kS1];
  float dz2[16 * kS2];
  float h2[16 * kS2];
  float d3[16];
  float dxth[16 * DinCfg<D>::DS];  // the row's gradient of its t⊙h features
  float tv[DinCfg<D>::NTV];        // [t_b, 1, 0...]
  float dts[2 * D];                // dtarget parts: Σ dx_{t⊙h}⊙h | Σ dx_t
};

template <int D>
struct DinBwdLds {
  float w1[DinCfg<D>::W1R * kW1S];
  float w2[kN1 * kW2S];
  float b2[48], w3[48];
  DinSet<D> st[kWaves];
  int live[kWaves];
};

static_assert(sizeof(DinBwdLds<36>) <= 160 * 1024 && sizeof(DinBwdLds<16>) <= 160 * 1024,
              "the backward's LDS plan must fit one CU");

__host__ __device__ inline int din_n_fold(int D) {  // [dW1f 3D×80 | db1 | dW2 | db2 | dW3 | db3]
  return 3 * D * kN1 + kN1 + kN1 * kN2 + kN2 + kN2 + 1;
}
__host__ __device__ inline int din_n_param(int D) {
  return 4 * D * kN1 + kN1 + kN1 * kN2 + kN2 + kN2 + 1;
}

template <int D>
__global__ __launch_bounds__(256) void din_bwd_kernel(DinArgs a, const float* __restrict__ drep,
                                                      float* __restrict__ dtarget,
                                                      float* __restrict__ dhis,
                                                      float* __restrict__ part) {
  using Cf = DinCfg<D>;
  extern __shared__ float dyn[];
  DinBwdLds<D>& S = *reinterpret_cast<DinBwdLds<D>*>(dyn);
  stage_w1(S.w1, Cf::W1R, Cf::In3, a.W1f);
  stage_w2(S.w2, a.W2);
  stage_b2_w3(S.b2, S.w3, a.b2, a.W3);
  const int lane = threadIdx.x & 63, j = lane & 15, kq = lane >> 4, wave = threadIdx.x >> 6;
  constexpr int Q = D / 4;
  constexpr int XH = (D + 15) / 16;  // input-gradient tiles that hold h features
  const int L = a.L;
  const int NT = (L + 15) / 16;
  DinSet<D>& T = S.st[wave];

  f4 acc[Cf::TPW];
#pragma unroll
  for (int q = 0; q < Cf::TPW; ++q) acc[q] = f4{0.f, 0.f, 0.f, 0.f};
  float vacc = 0.f;  // thread q < 81: dW3[q] (q < 40), db2[q-40] (q < 80), db3 (q = 80)
  __syncthreads();

  const int64_t n_rounds = (a.B + kWaves - 1) / kWaves;
  for (int64_t rd = blockIdx.x; rd < n_rounds; rd += gridDim.x) {
    const int64_t b = rd * kWaves + wave;
    const bool bv = b < a.B;
    const int64_t bc = bv ? b : 0;  // a wave past the batch reads example 0's, uses nothing
    f4 cbv[kT1];
#pragma unroll
    for (int u = 0; u < kT1; ++u)
      cbv[u] = *reinterpret_cast<const f4*>(a.cb + bc * kN1 + 16 * u + 4 * kq);
    float tv[Q], dv[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      tv[q] = a.target[bc * D + kq + 4 * q];
      dv[q] = drep[bc * D + kq + 4 * q];
    }
    f4 t4[XH], dr4[XH];  // target / drep at the lane's h features 16x + 4kq .. +3
#pragma unroll
    for (int x = 0; x < XH; ++x) {
      const int f0 = 16 * x + 4 * kq;
      t4[x] = *reinterpret_cast<const f4*>(a.target + bc * D + (f0 < D ? f0 : 0));
      dr4[x] = *reinterpret_cast<const f4*>(drep + bc * D + (f0 < D ? f0 : 0));
    }
    for (int i = lane; i < Cf::NTV; i += 64)
      T.tv[i] = i < D ? a.target[bc * D + i] : i == D ? 1.f : 0.f;
    f4 dtacc[Cf::XD];  // per lane (row j): Σ_tiles of the t⊙h / t feature gradients
#pragma unroll
    for (int x = 0; x < Cf::XD; ++x) dtacc[x] = f4{0.f, 0.f, 0.f, 0.f};

    for (int tile = 0; tile < NT; ++tile) {
      const int t = 16 * tile + j;
      const int tc = t < L ? t : 0;
      const bool m = bv && t < L && a.mask[bc * L + tc] != 0;
      const bool live = __ballot(m) != 0;
      if (lane == 0) S.live[wave] = live ? 1 : 0;
      f4 dxh[XH];
      float wgt = 0.f;
      if (live) {
        const float* hrow = a.his + (bc * L + tc) * (int64_t)D;
        float xv[2 * Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) xv[q] = hrow[kq + 4 * q];
        f4 h4[Cf::XD];  // the row's h at the lane's t⊙h features
#pragma unroll
        for (int x = 0; x < Cf::XD; ++x) {
          const int f0 = 16 * x + 4 * kq;
          if (16 * x + 15 >= D && 16 * x < 2 * D)
            h4[x] = *reinterpret_cast<const f4*>(hrow + (f0 >= D && f0 < 2 * D ? f0 - D : 0));
        }
        float d3 = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          xv[q] = m ? xv[q] : 0.f;
          xv[Q + q] = tv[q] * xv[q];
          d3 = fmaf(dv[q], xv[q], d3);
        }
        d3 += __shfl_xor(d3, 16);
        d3 += __shfl_xor(d3, 32);
        d3 = m ? d3 : 0.f;  // dL/dw of the row: drep·h
#pragma unroll
        for (int k = 0; k < 2 * Q; ++k) T.x[j * kS1 + 4 * k + kq] = xv[k];
        f4 h1[kT1], h2[kT2];
        mlp3_layer1<2 * Q>(S.w1, xv, j, kq, h1);
#pragma unroll
        for (int u = 0; u < kT1; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) h1[u][r] = aux_sigm(h1[u][r] + cbv[u][r]);
        const float z = mlp3_tail(S.w2, S.b2, S.w3, a.b3, j, kq, h1, h2);
        wgt = m ? z : 0.f;
        f4 dz2[kT2];
#pragma unroll
        for (int mm = 0; mm < kT2; ++mm)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int v = 16 * mm + 4 * kq + r;
            dz2[mm][r] = d3 * S.w3[v] * (h2[mm][r] * (1.f - h2[mm][r]));
          }
#pragma unroll
        for (int mm = 0; mm < kT2; ++mm) {
          lds4(T.dz2 + j * kS2 + 16 * mm + 4 * kq, dz2[mm]);
          lds4(T.h2 + j * kS2 + 16 * mm + 4 * kq, h2[mm]);
        }
        if (kq == 0) T.d3[j] = d3;
        // dh1ᵀ = W2 · dz2ᵀ, then dz1 = dh1 ⊙ h1(1 − h1)
        f4 dz1[kT1];
#pragma unroll
        for (int u = 0; u < kT1; ++u) {
          f4 c = f4{0.f, 0.f, 0.f, 0.f};
          const float* w = S.w2 + (16 * u + j) * kW2S + 4 * kq;  // A: W2[16u + j][16m + 4kq + r]
#pragma unroll
          for (int mm = 0; mm < kT2; ++mm)
#pragma unroll
            for (int r = 0; r < 4; ++r) c = mfma4(w[16 * mm + r], dz2[mm][r], c);
#pragma unroll
          for (int r = 0; r < 4; ++r) dz1[u][r] = c[r] * (h1[u][r] * (1.f - h1[u][r]));
          lds4(T.h1 + j * kS1 + 16 * u + 4 * kq, h1[u]);
          lds4(T.dz1 + j * kS1 + 16 * u + 4 * kq, dz1[u]);
        }
        // dXᵀ = W1f · dz1ᵀ over [h, t⊙h, t]: lane holds features 16x + 4kq .. +3 of row j
#pragma unroll
        for (int x = 0; x < Cf::XD; ++x) {
          f4 c = f4{0.f, 0.f, 0.f, 0.f};
          const float* w = S.w1 + (16 * x + j) * kW1S + 4 * kq;  // A: W1f[16x + j][16u + 4kq + r]
#pragma unroll
          for (int u = 0; u < kT1; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) c = mfma4(w[16 * u + r], dz1[u][r], c);
          const int f0 = 16 * x + 4 * kq;
          if (x < XH) dxh[x < XH ? x : 0] = c;  // used where f0 < D
          if (16 * x + 15 >= D) {
            f4 v = f4{0.f, 0.f, 0.f, 0.f};
            if (f0 >= D && f0 < 2 * D) {
              lds4(T.dxth + j * Cf::DS + (f0 - D), c);
              if (16 * x < 2 * D) {
                const f4 hh = h4[x];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = c[r] * (m ? hh[r] : 0.f);
              }
            } else if (f0 >= 2 * D && f0 < 3 * D) {
              v = c;
            }
            dtacc[x] += v;
          }
        }
      }
      __syncthreads();
      // dhis rows of this tile: dx_h + dx_{t⊙h}⊙t + w·drep at valid steps, exactly 0 elsewhere
      if (bv && t < L) {
#pragma unroll
        for (int x = 0; x < XH; ++x) {
          const int f0 = 16 * x + 4 * kq;
          if (f0 < D) {
            f4 v = f4{0.f, 0.f, 0.f, 0.f};
            if (live && m) {
              const float* o = T.dxth + j * Cf::DS + f0;
              v = dxh[x] + f4{o[0], o[1], o[2], o[3]} * t4[x] + dr4[x] * wgt;
            }
            store4(dhis + (b * L + t) * (int64_t)D + f0, v);
          }
        }
      }
      const bool any = (S.live[0] | S.live[1] | S.live[2] | S.live[3]) != 0;
      if (any) {
        // this wave's weight-gradient tiles over the round's live sets (K = rows)
#pragma unroll
        for (int q = 0; q < Cf::TPW; ++q) {
          const int tq = wave * Cf::TPW + q;
          if (tq >= Cf::TW1 + kTilesW2) continue;
#pragma unroll 1
          for (int sidx = 0; sidx < kWaves; ++sidx) {
            if (!S.live[sidx]) continue;
            const DinSet<D>& U = S.st[sidx];
            if (tq < Cf::TW1) {  // dW1f[16x + i][16u + n] += Σ_rows xaug[row][16x + i]·dz1[row][16u + n]
              const int x = tq / kT1, u = tq % kT1;
              const int f = 16 * x + j;
              const bool fx = f < Cf::In2;  // [h, t⊙h] per row; [t, 1] per example
              const float tval = U.tv[fx ? 0 : f - Cf::In2];
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const int row = 4 * k + kq;
                const float xa = U.x[row * kS1 + (fx ? f : 0)];
                acc[q] = mfma4(fx ? xa : tval, U.dz1[row * kS1 + 16 * u + j], acc[q]);
              }
            } else {  // dW2[16u + i][16m + n] += Σ_rows h1[row][16u + i]·dz2[row][16m + n]
              const int t2 = tq - Cf::TW1;
              const int u = t2 / kT2, mm = t2 % kT2;
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const int row = 4 * k + kq;
                acc[q] = mfma4(U.h1[row * kS1 + 16 * u + j], U.dz2[row * kS2 + 16 * mm + j], acc[q]);
              }
            }
          }
        }
        {  // dW3 / db2 / db3 on the vector unit: one output per thread
          const int q = threadIdx.x;
          if (q <= 2 * kN2) {
            for (int sidx = 0; sidx < kWaves; ++sidx) {
              if (!S.live[sidx]) continue;
              const DinSet<D>& U = S.st[sidx];
              float va[16], vb[16];
#pragma unroll
              for (int row = 0; row < 16; ++row) {
                va[row] = q < kN2 ? U.h2[row * kS2 + q] : q < 2 * kN2 ? U.dz2[row * kS2 + (q - kN2)] : 1.f;
                vb[row] = q < kN2 || q == 2 * kN2 ? U.d3[row] : 1.f;
              }
#pragma unroll
              for (int row = 0; row < 16; ++row) vacc = fmaf(va[row], vb[row], vacc);
            }
          }
        }
      }
      __syncthreads();  // the set tiles and live flags are rewritten next tile
    }

    // dtarget[b] = Σ_rows dx_{t⊙h}⊙h + Σ_rows dx_t: rows by a fixed butterfly, then the two parts
#pragma unroll
    for (int x = 0; x < Cf::XD; ++x) {
      if (16 * x + 15 < D) continue;
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) dtacc[x][r] += __shfl_xor(dtacc[x][r], off);
      const int f0 = 16 * x + 4 * kq;
      if (j == 0 && f0 >= D && f0 < 3 * D) lds4(T.dts + (f0 - D), dtacc[x]);
    }
    __syncthreads();
    if (bv && lane < D) dtarget[b * D + lane] = T.dts[lane] + T.dts[D + lane];
    // T.dts and T.tv are rewritten a round later, behind the tile loop's barriers (NT >= 1)
  }

  // this block's partial gradients: [dW1f 3D×80 | db1 80 | dW2 80×40 | db2 40 | dW3 40 | db3 1]
  float* out = part + (int64_t)blockIdx.x * din_n_fold(D);
  float* o_b1 = out + Cf::In3 * kN1;
  float* o_w2 = o_b1 + kN1;
  float* o_b2 = o_w2 + kN1 * kN2;
  float* o_w3 = o_b2 + kN2;
#pragma unroll
  for (int q = 0; q < Cf::TPW; ++q) {
    const int tq = wave * Cf::TPW + q;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (tq < Cf::TW1) {
        const int x = tq / kT1, u = tq % kT1;
        const int f = 16 * x + 4 * kq + r, un = 16 * u + j;
        if (f < Cf::In3) out[f * kN1 + un] = acc[q][r];
        else if (f == Cf::In3) o_b1[un] = acc[q][r];
      } else if (tq < Cf::TW1 + kTilesW2) {
        const int t2 = tq - Cf::TW1;
        const int u = t2 / kT2, mm = t2 % kT2;
        const int un = 16 * u + 4 * kq + r, v = 16 * mm + j;
        if (v < kN2) o_w2[un * kN2 + v] = acc[q][r];
      }
    }
  }
  const int q = threadIdx.x;
  if (q < kN2) o_w3[q] = vacc;
  else if (q < 2 * kN2) o_b2[q - kN2] = vacc;
  else if (q == 2 * kN2) o_w3[kN2] = vacc;  // db3 follows dW3
}

// folded gradients G = [G_h; G_th; G_t] → dW1 = [dWa = G_t; dWb = G_h; dWc = G_t − G_h;
// dWd = G_th] in the reference's row order; the other parameters copied
__global__ void din_unfold_kernel(const float* __restrict__ g, int D, float* __restrict__ dparams) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n1 = 4 * D * kN1;
  if (i >= din_n_param(D)) return;
  if (i >= n1) {
    dparams[i] = g[i - n1 + 3 * D * kN1];
    return;
  }
  const int f = i / kN1, u = i % kN1;
  const int seg = f / D, d = f % D;
  const float gh = g[d * kN1 + u], gth = g[(D + d) * kN1 + u], gt = g[(2 * D + d) * kN1 + u];
  dparams[i] = seg == 0 ? gt : seg == 1 ? gh : seg == 2 ? gt - gh : gth;
}

struct DinWs {  // workspace carve: folded W1 | biases | partials | fold scratch | folded gradients
  size_t w1f, cb, part, part2, fold, total;
};
DinWs din_ws_layout(int64_t B, int32_t D) {
  const size_t np = (size_t)din_n_fold(D);
  DinWs w;
  w.w1f = 0;
  w.cb = align_up(w.w1f + (size_t)3 * D * kN1 * 4, 256);
  w.part = align_up(w.cb + (size_t)B * kN1 * 4, 256);
  w.part2 = align_up(w.part + (size_t)device_cus() * np * 4, 256);
  w.fold = align_up(w.part2 + 32 * np * 4, 256);
  w.total = align_up(w.fold + np * 4, 256);
  return w;
}

bool din_built(int32_t D) { return D == 36 || D == 16; }

int32_t check_din(const float* target, const float* his, const uint8_t* mask, int64_t B, int32_t L,
                  int32_t D, const float* W1, const float* b1, const float* W2, const float* b2,
                  const float* W3, const float* b3, const void* workspace, size_t ws_bytes) {
  RS_CHECK_ARG(B >= 0 && B < (1LL << 31) / kN1 && L >= 1 && L <= 4096 && D > 0,
               "din activation: bad sizes (B >= 0, 1 <= L <= 4096)");
  if (!din_built(D)) {
    set_error("din activation: D = %d not built (36, 16)", D);
    return RS_E_UNSUPPORTED;
  }
  RS_CHECK_ARG(target && his && mask && W1 && b1 && W2 && b2 && W3 && b3 && workspace,
               "din activation: null pointer");
  if (ws_bytes < din_ws_layout(B, D).total) {
    set_error("din activation: workspace too small (%zu < %zu bytes)", ws_bytes,
              din_ws_layout(B, D).total);
    return RS_E_WORKSPACE;
  }
  return RS_OK;
}

template <int D>
int32_t din_prep(const float* W1, const float* b1, const float* target, int64_t B, float* w1f,
                 float* cb, hipStream_t st) {
  const int64_t n = std::max<int64_t>(B * kN1, 3 * D * kN1);
  din_prep_kernel<D><<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(W1, b1, target, B, w1f, cb);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" size_t rs_din_activation_workspace_size(int64_t B, int32_t L, int32_t D) {
  (void)L;
  if (B < 0 || D <= 0) return 0;
  return din_ws_layout(B, D).total;
}

extern "C" int32_t rs_din_activation_fwd(const float* target, const float* his,
                                         const uint8_t* mask, int64_t B, int32_t L, int32_t D,
                                         const float* W1, const float* b1, const float* W2,
                                         const float* b2, const float* W3, const float* b3,
                                         float* rep, void* workspace, size_t ws_bytes,
                                         void* stream) {
  if (int32_t e = check_din(target, his, mask, B, L, D, W1, b1, W2, b2, W3, b3, workspace, ws_bytes))
    return e;
  RS_CHECK_ARG(rep, "din activation: null pointer");
  if (B == 0) return RS_OK;
  hipStream_t st = as_stream(stream);
  const DinWs wl = din_ws_layout(B, D);
  char* wsb = static_cast<char*>(workspace);
  float* w1f = reinterpret_cast<float*>(wsb + wl.w1f);
  float* cb = reinterpret_cast<float*>(wsb + wl.cb);
  DinArgs a{target, his, mask, B, L, w1f, cb, W2, b2, W3, b3};
  // persistent over rounds of kWaves examples, 3 resident blocks per CU
  const unsigned grid =
      (unsigned)std::min<int64_t>(ceil_div(B, kWaves), (int64_t)kFwdBlocksPerCU * device_cus());
  if (D == 36) {
    if (int32_t e = din_prep<36>(W1, b1, target, B, w1f, cb, st)) return e;
    din_fwd_kernel<36><<<grid, 64 * kWaves, 0, st>>>(a, rep);
  } else {
    if (int32_t e = din_prep<16>(W1, b1, target, B, w1f, cb, st)) return e;
    din_fwd_kernel<16><<<grid, 64 * kWaves, 0, st>>>(a, rep);
  }
  RS_CHECK_LAUNCH();
  return RS_OK;
}

extern "C" int32_t rs_din_activation_bwd(const float* target, const float* his,
                                         const uint8_t* mask, int64_t B, int32_t L, int32_t D,
                                         const float* W1, const float* b1, const float* W2,
                                         const float* b2, const float* W3, const float* b3,
                                         const float* drep, float* dtarget, float* dhis,
                                         float* dparams, void* workspace, size_t ws_bytes,
                                         void* stream) {
  if (int32_t e = check_din(target, his, mask, B, L, D, W1, b1, W2, b2, W3, b3, workspace, ws_bytes))
    return e;
  RS_CHECK_ARG(drep && dtarget && dhis && dparams, "din activation: null pointer");
  hipStream_t st = as_stream(stream);
  if (B == 0) {
    RS_CHECK_HIP(hipMemsetAsync(dparams, 0, (size_t)din_n_param(D) * 4, st));
    return RS_OK;
  }
  const DinWs wl = din_ws_layout(B, D);
  char* wsb = static_cast<char*>(workspace);
  float* w1f = reinterpret_cast<float*>(wsb + wl.w1f);
  float* cb = reinterpret_cast<float*>(wsb + wl.cb);
  float* part = reinterpret_cast<float*>(wsb + wl.part);
  float* part2 = reinterpret_cast<float*>(wsb + wl.part2);
  float* fold = reinterpret_cast<float*>(wsb + wl.fold);
  DinArgs a{target, his, mask, B, L, w1f, cb, W2, b2, W3, b3};
  // persistent over rounds of kWaves examples, one block per CU (the set tiles fill its LDS)
  const int nb = (int)std::min<int64_t>(ceil_div(B, kWaves), device_cus());
  auto run = [&](auto kern, size_t lds) -> int32_t {
    RS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<(unsigned)nb, 64 * kWaves, lds, st>>>(a, drep, dtarget, dhis, part);
    RS_CHECK_LAUNCH();
    return RS_OK;
  };
  int32_t rc;
  if (D == 36) {
    if (int32_t e = din_prep<36>(W1, b1, target, B, w1f, cb, st)) return e;
    rc = run(din_bwd_kernel<36>, sizeof(DinBwdLds<36>));
  } else {
    if (int32_t e = din_prep<16>(W1, b1, target, B, w1f, cb, st)) return e;
    rc = run(din_bwd_kernel<16>, sizeof(DinBwdLds<16>));
  }
  if (rc) return rc;
  const int np = din_n_fold(D);
  if (int32_t e = fold_two_level(part, nb, np, part2, fold, st)) return e;
  din_unfold_kernel<<<(unsigned)ceil_div(din_n_param(D), 256), 256, 0, st>>>(fold, D, dparams);
  RS_CHECK_LAUNCH();
  return RS_OK;
}
