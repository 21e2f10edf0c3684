// pinsage_infer.hip — one PinSage Convolve layer over the whole catalogue, fused (gfx950).
//
// Layer-wise inference (pinsage/inference/inference.py:8-41) has no block machinery: the dst
// nodes are all the items in order, the src nodes are the same items, and the "block" is the
// [n_items, k] neighbour table of rs_pinsage_neighbors. Per item i, in one pass:
//   nv  = Σ_j (float)cnt[i,j] · u[nbr[i,j]] / max(Σ_j cnt[i,j], 1)   (slot order; the
//         rs_weighted_mean_agg_fwd contract: products rounded, then summed)
//   z   = [nv ; h[i]] · w2 + b2, optional relu
//   out = z / ‖z‖₂ (norm == 1), a zero row staying zero
// nv, the concat and z never reach HBM.
//
// Shape of the kernel: a block of 256 threads walks tiles of kTile = 64 consecutive items
// (grid-stride), with fc_2's kernel and bias staged in LDS once per block (rows padded to a
// multiple of 4 columns, so a wave reads 4 weights with one broadcast 16-byte LDS read).
//   A  the tile's nbr / cnt rows are copied to LDS (coalesced) and validated there: -1 or a
//      zero count = empty slot, any other id outside [0, n_items) = skipped + RS_ERRBIT_OOB;
//      h's rows (contiguous in HBM) are copied into the x tile beside where nv goes.
//   B  (item, 4-column chunk) per lane: the k u-rows are gathered with 16-byte loads (8 lanes
//      cover the 128-byte row of hidden = 32), summed in slot order, divided, written to x.
//   C  (item = lane, 4 output columns per wave-uniform column group): K = hidden + d_in
//      explicit fmaf steps per output in row order of w2, from the bias; x is read with an odd
//      row stride (no bank conflict), w2 by broadcast.
//   D  per row: Σ z² in column order, sqrt; then the tile's [rows, d_out] outputs are written
//      coalesced, divided by the row's norm.
// A row's result depends on that row's inputs only — no atomics on data, no cross-row
// reduction — so it is run-to-run identical and independent of n_items, of the tiling and of
// the grid.
//
// fc_2 on the VALU (fmaf), not the exact-f32 MFMA: at the default sizes a row moves 792 B for
// 1 792 FLOP (2.3 FLOP/B, against ≈ 20 FLOP/B where the fp32 vector rate meets HBM), so the
// matrix core would not shorten the kernel, and fmaf keeps one fixed, documented summation
// order per output for every shape ("Layer-wise PinSage inference").
#include <cmath>

#include "common.hpp"

namespace rs {

constexpr int kTile = RS_PINSAGE_INFER_TILE;
constexpr int kInferThreads = 256;
static_assert(kTile == kWave, "phase C maps one item to one lane of a wave");

struct InferLds {
  int ldw;       // w2 row stride in LDS: d_out rounded up to 4
  int ldx;       // x row stride: K made odd
  int ldz;       // z row stride: ldw + 1 (odd)
  size_t w_off, b_off, x_off, s_off;  // float offsets: w2 [K, ldw], b2 [ldw], x [kTile, ldx],
                                      // then the region shared by nbr/cnt (A, B) and z/norm (C, D)
  size_t floats;
};

inline InferLds infer_lds(int d_in, int hidden, int k, int d_out) {
  InferLds l;
  const int K = hidden + d_in;
  l.ldw = (d_out + 3) / 4 * 4;
  l.ldx = K | 1;
  l.ldz = l.ldw + 1;
  l.w_off = 0;
  l.b_off = (size_t)K * l.ldw;
  l.x_off = l.b_off + l.ldw;
  l.s_off = l.x_off + (size_t)kTile * l.ldx;
  l.s_off = (l.s_off + 3) / 4 * 4;
  const size_t ids = (size_t)2 * kTile * k;
  const size_t zs = (size_t)kTile * l.ldz + kTile;
  l.floats = l.s_off + (ids > zs ? ids : zs);
  return l;
}

__global__ __launch_bounds__(kInferThreads) void pinsage_infer_kernel(
    const float* __restrict__ h, int64_t n_items, int d_in, const float* __restrict__ u,
    int hidden, const int32_t* __restrict__ nbr, const int32_t* __restrict__ cnt, int k,
    const float* __restrict__ w2, const float* __restrict__ b2, int d_out, int relu, int norm,
    int vec_u, int vec_h, InferLds L, float* __restrict__ out, int32_t* err_flag) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ws = lds + L.w_off;
  float* bs = lds + L.b_off;
  float* xs = lds + L.x_off;
  int32_t* ids = reinterpret_cast<int32_t*>(lds + L.s_off);  // [kTile, k]: id or -1
  int32_t* cts = ids + kTile * k;                            // [kTile, k]
  float* zs = lds + L.s_off;                                 // [kTile, ldz] (after B)
  float* nrm = zs + kTile * L.ldz;                           // [kTile]
  const int tid = threadIdx.x;
  const int K = hidden + d_in;

  // fc_2's kernel and bias, once per block (padding columns 0)
  for (int e = tid; e < K * L.ldw; e += kInferThreads) {
    const int r = e / L.ldw, c = e - r * L.ldw;
    ws[e] = c < d_out ? w2[r * d_out + c] : 0.f;
  }
  for (int c = tid; c < L.ldw; c += kInferThreads) bs[c] = c < d_out ? b2[c] : 0.f;

  const int64_t n_tiles = (n_items + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t i0 = tile * kTile;
    const int rows = (int)(n_items - i0 < kTile ? n_items - i0 : kTile);
    __syncthreads();  // the previous tile's z / norm reads are done (and w2 is staged)

    // ---- A: neighbour slots (validated) and h rows into LDS -------------------------------
    bool oob = false;
    for (int e = tid; e < rows * k; e += kInferThreads) {
      const int32_t id = nbr[i0 * k + e];
      const int32_t c = cnt[i0 * k + e];
      const bool in = id >= 0 && (int64_t)id < n_items;
      if (!in && id != -1) oob = true;
      ids[e] = (in && c != 0) ? id : -1;
      cts[e] = c;
    }
    if (oob) flag_oob(err_flag);
    if (vec_h) {
      const int q = d_in >> 2;
      const float4* src = reinterpret_cast<const float4*>(h + i0 * d_in);
      for (int e = tid; e < rows * q; e += kInferThreads) {
        const int r = e / q, c = (e - r * q) << 2;
        const float4 v = src[e];
        float* d = xs + r * L.ldx + hidden + c;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
      }
    } else {
      for (int e = tid; e < rows * d_in; e += kInferThreads) {
        const int r = e / d_in, c = e - r * d_in;
        xs[r * L.ldx + hidden + c] = h[i0 * d_in + e];
      }
    }
    __syncthreads();

    // ---- B: nv = weighted mean of the neighbours' u rows, slot order -----------------------
    {
      const int nch = (hidden + 3) >> 2;
      for (int e = tid; e < rows * nch; e += kInferThreads) {
        const int r = e / nch, c0 = (e - r * nch) << 2;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, wsum = 0.f;
        const int32_t* rid = ids + r * k;
        const int32_t* rct = cts + r * k;
        if (vec_u) {
#pragma unroll 4
          for (int j = 0; j < k; ++j) {
            const int32_t id = rid[j];
            if (id < 0) continue;
            const float w = (float)rct[j];
            const float4 v = *reinterpret_cast<const float4*>(u + (int64_t)id * hidden + c0);
            a0 += w * v.x, a1 += w * v.y, a2 += w * v.z, a3 += w * v.w;
            wsum += w;
          }
        } else {
          const int nc = hidden - c0 < 4 ? hidden - c0 : 4;
          for (int j = 0; j < k; ++j) {
            const int32_t id = rid[j];
            if (id < 0) continue;
            const float w = (float)rct[j];
            const float* p = u + (int64_t)id * hidden + c0;
            a0 += w * p[0];
            if (nc > 1) a1 += w * p[1];
            if (nc > 2) a2 += w * p[2];
            if (nc > 3) a3 += w * p[3];
            wsum += w;
          }
        }
        const float den = fmaxf(wsum, 1.f);
        float* d = xs + r * L.ldx + c0;
        d[0] = a0 / den;
        if (c0 + 1 < hidden) d[1] = a1 / den;
        if (c0 + 2 < hidden) d[2] = a2 / den;
        if (c0 + 3 < hidden) d[3] = a3 / den;
      }
    }
    __syncthreads();

    // ---- C: z = [nv ; h] · w2 + b2 (fmaf in w2 row order), relu -----------------------------
    {
      const int ng = L.ldw >> 2;
      for (int e = tid; e < kTile * ng; e += kInferThreads) {
        const int r = e & (kTile - 1), c0 = (e / kTile) << 2;  // c0 is wave-uniform
        if (r >= rows) continue;
        const float4 b = *reinterpret_cast<const float4*>(bs + c0);
        float z0 = b.x, z1 = b.y, z2 = b.z, z3 = b.w;
        const float* x = xs + r * L.ldx;
        const float* w = ws + c0;
#pragma unroll 4
        for (int kk = 0; kk < K; ++kk) {
          const float xv = x[kk];
          const float4 wv = *reinterpret_cast<const float4*>(w + kk * L.ldw);
          z0 = fmaf(xv, wv.x, z0);
          z1 = fmaf(xv, wv.y, z1);
          z2 = fmaf(xv, wv.z, z2);
          z3 = fmaf(xv, wv.w, z3);
        }
        if (relu) z0 = fmaxf(z0, 0.f), z1 = fmaxf(z1, 0.f), z2 = fmaxf(z2, 0.f), z3 = fmaxf(z3, 0.f);
        float* d = zs + r * L.ldz + c0;
        d[0] = z0, d[1] = z1, d[2] = z2, d[3] = z3;  // padding columns land in the row's pad
      }
    }
    __syncthreads();

    // ---- D: per-row L2 norm, coalesced store -------------------------------------------------
    if (norm) {
      if (tid < rows) {
        const float* z = zs + tid * L.ldz;
        float ss = 0.f;
        for (int c = 0; c < d_out; ++c) ss = fmaf(z[c], z[c], ss);
        nrm[tid] = sqrtf(ss);
      }
      __syncthreads();
    }
    for (int e = tid; e < rows * d_out; e += kInferThreads) {
      const int r = e / d_out, c = e - r * d_out;
      float v = zs[r * L.ldz + c];
      if (norm) {
        const float n = nrm[r];
        v = n > 0.f ? v / n : 0.f;  // a zero row stays zero (the Spark UDF's 0 / 0 gives NaN)
      }
      out[i0 * d_out + e] = v;
    }
  }
}

}  // namespace rs

using namespace rs;

extern "C" int32_t rs_pinsage_infer_layer(const float* h, int64_t n_items, int32_t d_in,
                                          const float* u, int32_t hidden, const int32_t* nbr,
                                          const int32_t* cnt, int32_t k, const float* w2,
                                          const float* b2, int32_t d_out, int32_t relu,
                                          int32_t norm, float* out, int32_t* err_flag,
                                          void* stream) {
  RS_CHECK_ARG(n_items >= 0 && d_in >= 1 && hidden >= 1 && k >= 1 && d_out >= 1,
               "rs_pinsage_infer_layer: bad sizes");
  RS_CHECK_ARG(norm == 0 || norm == 1, "rs_pinsage_infer_layer: norm must be 0 (none) or 1 (row)");
  if (d_in > RS_PINSAGE_INFER_MAX_DIN || hidden > RS_PINSAGE_INFER_MAX_HIDDEN ||
      d_out > RS_PINSAGE_INFER_MAX_DOUT || k > RS_PINSAGE_INFER_MAX_K) {
    set_error("rs_pinsage_infer_layer: the fused form takes d_in <= %d, hidden <= %d, "
              "d_out <= %d, k <= %d (got %d, %d, %d, %d)",
              RS_PINSAGE_INFER_MAX_DIN, RS_PINSAGE_INFER_MAX_HIDDEN, RS_PINSAGE_INFER_MAX_DOUT,
              RS_PINSAGE_INFER_MAX_K, d_in, hidden, d_out, k);
    return RS_E_UNSUPPORTED;
  }
  if (n_items == 0) return RS_OK;
  RS_CHECK_ARG(h && u && nbr && cnt && w2 && b2 && out, "rs_pinsage_infer_layer: null pointer");
  const InferLds L = infer_lds(d_in, hidden, k, d_out);
  const size_t lds_bytes = L.floats * sizeof(float);
  if (lds_bytes > 64 * 1024)
    RS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pinsage_infer_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  const int vec_u = hidden % 4 == 0 && reinterpret_cast<uintptr_t>(u) % 16 == 0;
  const int vec_h = d_in % 4 == 0 && reinterpret_cast<uintptr_t>(h) % 16 == 0;
  // as many blocks as stay resident (LDS-bound, at most 8 per CU of 256), tiles grid-strided
  int64_t per_cu = (int64_t)(160 * 1024) / (int64_t)lds_bytes;
  per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
  const int64_t n_tiles = ceil_div(n_items, kTile);
  const int64_t grid = n_tiles < 256 * per_cu ? n_tiles : 256 * per_cu;
  pinsage_infer_kernel<<<(unsigned)grid, kInferThreads, lds_bytes, as_stream(stream)>>>(
      h, n_items, d_in, u, hidden, nbr, cnt, k, w2, b2, d_out, relu != 0, norm, vec_u, vec_h, L,
      out, err_flag);
  RS_CHECK_LAUNCH();
  return RS_OK;
}
