// item_softmax.hip — softmax cross-entropy of query rows against a matrix of item rows
// (recsys_hip.h, "Softmax cross-entropy over item rows"), forward and backward, without the
// [n_queries, n_items] logits matrix: the forward keeps an online log-sum-exp, the backward
// recomputes every logits tile from the rows and lse.
//
//   item_softmax_prep     per query row: the resolved target (-1 when outside [0, n_items)), the
//                         target's id and, for the backward, grad_loss · inv_temp.
//   item_softmax_kernel   one block = 32 "own" rows × one contiguous range (a "split") of the
//                         "streamed" rows. The own tile sits in LDS for the block's life; each of
//                         the 4 waves takes every fourth 32-row tile of the range. A tile's rows go
//                         global → registers (16 bytes per lane where alignment allows) and
//                         v_mfma_f32_32x32x2_f32 computes the transposed tile T[streamed][own], so a
//                         lane holds 16 streamed rows' logits of ONE own row.
//       MODE 0 (forward)  own = queries. A lane folds its 16 logits into one running (max, sum)
//                         pair; the lane that meets its row's target keeps the logit. At the end
//                         the 8 pairs of a row (4 waves × 2 lane halves) merge in a fixed order and
//                         (max, sum, target logit) go to the workspace slot of (split, row).
//       MODE 1 (dQueries) own = queries, streamed = items; MODE 2 (dItems) own = items, streamed =
//                         queries. The 16 logits become c = g · inv_temp · (p - [j == t]) in place:
//                         in the transposed tile they already are the A operand (own row × streamed
//                         row) of the second product, so c never leaves the registers. The B
//                         operand is the streamed tile again, read 32 columns of a row at a time
//                         (it is in cache). The 4 waves' gradient tiles are added in wave order
//                         through LDS; the block writes the output rows (one split) or its
//                         workspace slot (more).
//   item_softmax_merge    forward: the splits' (max, sum) pairs merged in ascending split order,
//                         lse and loss written.
//   item_softmax_fold     backward, more than one split: the splits' partial rows added in
//                         ascending split order.
// No floating-point atomics; no block waits for another; the host never synchronises.
#include <cmath>

#include "common.hpp"

namespace rs {
namespace {

constexpr int kT = 32;  // tile edge: own rows per block, streamed rows per wave tile
constexpr int kIsWaves = 4;
constexpr int kIsThreads = kIsWaves * kWave;
constexpr int kIsDimMax = 256;
constexpr int kIsSplitMax = 1024;
constexpr int kIsAutoSplitMax = 16;
constexpr int kMetaFloats = 6 * kT;  // per wave: two float, one int32, one int64 array of 32

struct IsArgs {
  const float* q;
  int64_t q_ld;
  int32_t nq;
  const float* v;
  int64_t v_ld;
  int32_t nv;
  int32_t dim;
  float inv_temp;
  const float* bias;    // may be NULL
  const int64_t* ids;   // may be NULL
  const int32_t* tgt;   // [nq] resolved targets, -1: none
  const int64_t* tid;   // [nq] ids[tgt] (read only when ids != NULL)
  const float* lse;     // backward
  const float* gs;      // backward: grad_loss * inv_temp
  int32_t n_splits;
  int32_t x_tiles;
  float* out;           // forward: [n_splits][nq][3]; backward: rows, or [n_splits][n_own][dim]
  int64_t out_ld;
  int64_t split_stride;  // backward: floats between two splits' partials (0: the output itself)
};

// exp(a - b) for a <= b, with equal infinities giving 1 (their difference is NaN)
__device__ __forceinline__ float exp_diff(float a, float b) { return a == b ? 1.f : expf(a - b); }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__global__ __launch_bounds__(256) void item_softmax_prep_kernel(
    const int32_t* __restrict__ targets, const int64_t* __restrict__ ids,
    const float* __restrict__ grad_loss, float inv_temp, int32_t nq, int32_t nv,
    int32_t* __restrict__ tgt, int64_t* __restrict__ tid, float* __restrict__ gs) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nq) return;
  const int64_t t = targets ? (int64_t)targets[r] : r;
  const bool ok = t >= 0 && t < nv;
  tgt[r] = ok ? (int32_t)t : -1;
  tid[r] = ids && ok ? ids[t] : 0;
  if (grad_loss) gs[r] = grad_loss[r] * inv_temp;
}

// NB = 32-column blocks of the gradient tile a wave accumulates (unused by the forward)
template <int MODE, bool FAST, int NB>
__global__ __launch_bounds__(kIsThreads) void item_softmax_kernel(const IsArgs a) {
  constexpr bool OWN_Q = MODE != 2;
  extern __shared__ __align__(16) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int mrow = lane & 31, half = lane >> 5;
  const int32_t dim = a.dim;
  const int dq = (dim + 7) & ~7;  // the dot product runs over 8 columns per group, zeros past dim
  const int XS = dq + 4;
  // per wave: the streamed tile's row data
  float* mA = lds + wid * kMetaFloats;
  float* mB = mA + kT;
  int32_t* mT = reinterpret_cast<int32_t*>(mB + kT);
  int64_t* mId = reinterpret_cast<int64_t*>(mT + kT);
  float* red = lds + kIsWaves * kMetaFloats;  // forward: [8][32] max, [8][32] sum, [32] target
  float* Xs = red + 17 * kT;                  // [32][XS]; afterwards the gradient tile [32][32 NB]

  const float* X = OWN_Q ? a.q : a.v;
  const float* Y = OWN_Q ? a.v : a.q;
  const int64_t x_ld = OWN_Q ? a.q_ld : a.v_ld, y_ld = OWN_Q ? a.v_ld : a.q_ld;
  const int32_t nx = OWN_Q ? a.nq : a.nv, ny = OWN_Q ? a.nv : a.nq;
  const int32_t sp = blockIdx.x / a.x_tiles;
  const int64_t x0 = (int64_t)(blockIdx.x - sp * a.x_tiles) * kT;  // + 31 may pass 2^31
  const int32_t per = ny / a.n_splits;
  const int32_t lo = sp * per, hi = sp == a.n_splits - 1 ? ny : lo + per;

  for (int e = tid; e < kT * dq; e += kIsThreads) {
    const int row = e / dq, col = e - row * dq;
    Xs[row * XS + col] =
        x0 + row < nx && col < dim ? X[(x0 + row) * x_ld + col] : 0.f;
  }
  if (MODE == 0 && tid < kT) red[16 * kT + tid] = NAN;

  // this lane's own row
  const int64_t xr = x0 + mrow;
  const bool xok = xr < nx;
  int32_t x_t = -1;
  int64_t x_id = 0;
  float x_f = 0.f, x_gs = 0.f;  // OWN_Q: lse, g * inv_temp; else: bias
  if (OWN_Q) {
    if (xok) x_t = a.tgt[xr];
    if (a.ids && x_t >= 0) x_id = a.tid[xr];
    if (MODE == 1 && xok) {
      x_f = a.lse[xr];
      x_gs = a.gs[xr];
    }
  } else if (xok) {
    if (a.bias) x_f = a.bias[xr];
    if (a.ids) x_id = a.ids[xr];
  }
  __syncthreads();

  float run_m = -INFINITY, run_s = 0.f;
  f32x16 acc2[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc2[b] = f32x16{};

  const int32_t n_tiles = hi > lo ? (int32_t)(((int64_t)hi - lo + kT - 1) / kT) : 0;
  for (int32_t ti = wid; ti < n_tiles; ti += kIsWaves) {
    const int64_t yb = (int64_t)lo + (int64_t)ti * kT;
    if (lane < kT) {
      const int64_t yr = yb + lane;
      const bool ok = yr < hi;
      if (OWN_Q) {
        mA[lane] = a.bias && ok ? a.bias[yr] : 0.f;
        mId[lane] = a.ids && ok ? a.ids[yr] : 0;
      } else {
        const int32_t t = ok ? a.tgt[yr] : -1;
        mT[lane] = t;
        mA[lane] = ok ? a.lse[yr] : 0.f;
        mB[lane] = ok ? a.gs[yr] : 0.f;
        mId[lane] = a.ids && t >= 0 ? a.tid[yr] : 0;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // T[streamed][own]: column c of the product sits in step (c / 8, c % 4), lane half
    // (c / 4) % 2, for both operands; a row past the range's end re-reads the last row (FAST)
    // or reads zeros, and its logits are never used
    f32x16 acc = {};
    {
      const bool rok = yb + mrow < hi;
      const float* yp = Y + (rok ? yb + mrow : (int64_t)hi - 1) * y_ld;
      const float* xp = Xs + mrow * XS + 4 * half;
      for (int c0 = 0; c0 < dq; c0 += 8) {
        const int col = c0 + 4 * half;
        float4 y4;
        if constexpr (FAST) {
          y4 = *reinterpret_cast<const float4*>(yp + min(col, dim - 4));
          if (col >= dim) y4 = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          y4 = make_float4(0.f, 0.f, 0.f, 0.f);
          if (rok && col < dim) {
            y4.x = yp[col];
            if (col + 1 < dim) y4.y = yp[col + 1];
            if (col + 2 < dim) y4.z = yp[col + 2];
            if (col + 3 < dim) y4.w = yp[col + 3];
          }
        }
        const float4 x4 = *reinterpret_cast<const float4*>(xp + c0);
        acc = mfma(y4.x, x4.x, acc);
        acc = mfma(y4.y, x4.y, acc);
        acc = mfma(y4.z, x4.z, acc);
        acc = mfma(y4.w, x4.w, acc);
      }
    }

    // register r of the tile: streamed row 8 (r / 4) + 4 half + r % 4, own row mrow
    float tile_m = -INFINITY;
    bool kept[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int yy = 8 * (r >> 2) + 4 * half + (r & 3);
      const int64_t yr = yb + yy;
      const bool yok = yr < hi;
      int32_t t;
      int64_t j, id_j, id_t;
      float bias_j, lse_i = 0.f, gs_i = 0.f;
      if (OWN_Q) {
        t = x_t;
        j = yr;
        id_j = mId[yy];
        id_t = x_id;
        bias_j = mA[yy];
        lse_i = x_f;
        gs_i = x_gs;
      } else {
        t = mT[yy];
        j = xr;
        id_j = x_id;
        id_t = mId[yy];
        bias_j = x_f;
        lse_i = mA[yy];
        gs_i = mB[yy];
      }
      const bool valid = xok && yok && t >= 0;
      const bool is_t = j == t;
      kept[r] = valid && (is_t || !a.ids || id_j != id_t);
      const float z = a.inv_temp * acc[r] - bias_j;
      if (MODE == 0) {
        acc[r] = z;
        if (kept[r]) tile_m = fmaxf(tile_m, z);  // a NaN is not a maximum; it reaches the sum
        if (valid && is_t) red[16 * kT + mrow] = z;
      } else {
        const float p = kept[r] ? expf(z - lse_i) : 0.f;
        acc[r] = valid ? gs_i * (p - (is_t ? 1.f : 0.f)) : 0.f;
      }
    }
    if (MODE == 0) {
      const float m = fmaxf(run_m, tile_m);
      run_s *= exp_diff(run_m, m);
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kept[r]) run_s += exp_diff(acc[r], m);
      run_m = m;
    } else {
      // grad[own][d] += sum over the streamed rows of c · Y[row][d]: step r takes, per lane half,
      // the streamed row register r belongs to, so acc[r] is the A operand as it stands
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int d = 32 * b + mrow;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t yr = yb + 8 * (r >> 2) + 4 * half + (r & 3);
          const float y = d < dim && yr < hi ? Y[yr * y_ld + d] : 0.f;
          acc2[b] = mfma(acc[r], y, acc2[b]);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  if (MODE == 0) {
    red[(2 * wid + half) * kT + mrow] = run_m;
    red[(8 + 2 * wid + half) * kT + mrow] = run_s;
    __syncthreads();
    if (tid < kT && x0 + tid < nx) {
      float m = -INFINITY, s = 0.f;
#pragma unroll
      for (int p = 0; p < 8; ++p) m = fmaxf(m, red[p * kT + tid]);
#pragma unroll
      for (int p = 0; p < 8; ++p) s += red[(8 + p) * kT + tid] * exp_diff(red[p * kT + tid], m);
      float* o = a.out + ((int64_t)sp * a.nq + x0 + tid) * 3;
      o[0] = m;
      o[1] = s;
      o[2] = red[16 * kT + tid];
    }
    return;
  }

  // the four waves' tiles, added in wave order; register r of block b is own row
  // 8 (r / 4) + 4 half + r % 4, column 32 b + mrow
  constexpr int OS = 32 * NB;
  float* Ob = Xs;
  for (int w = 0; w < kIsWaves; ++w) {
    __syncthreads();  // w == 0: every wave is done with Xs
    if (wid == w) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float* o = Ob + (8 * (r >> 2) + 4 * half + (r & 3)) * OS + 32 * b + mrow;
          *o = w == 0 ? acc2[b][r] : *o + acc2[b][r];
        }
    }
  }
  __syncthreads();
  float* out = a.out + (int64_t)sp * a.split_stride;
  for (int e = tid; e < kT * dim; e += kIsThreads) {
    const int row = e / dim, col = e - row * dim;
    if (x0 + row < nx) out[(x0 + row) * a.out_ld + col] = Ob[row * OS + col];
  }
}

__global__ __launch_bounds__(256) void item_softmax_merge_kernel(
    const float* __restrict__ part, const int32_t* __restrict__ tgt, int32_t nq, int32_t nv,
    int32_t n_splits, float* __restrict__ loss, float* __restrict__ lse) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nq) return;
  const int32_t t = tgt[r];
  if (t < 0) {
    loss[r] = NAN;
    lse[r] = NAN;
    return;
  }
  float m = -INFINITY, s = 0.f;
  for (int32_t sp = 0; sp < n_splits; ++sp) m = fmaxf(m, part[((int64_t)sp * nq + r) * 3]);
  for (int32_t sp = 0; sp < n_splits; ++sp) {
    const float* p = part + ((int64_t)sp * nq + r) * 3;
    s += p[1] * exp_diff(p[0], m);
  }
  const int32_t per = nv / n_splits;
  const int32_t st = per > 0 && t / per < n_splits - 1 ? t / per : n_splits - 1;
  const float l = m + logf(s);
  lse[r] = l;
  loss[r] = l - part[((int64_t)st * nq + r) * 3 + 2];
}

__global__ __launch_bounds__(256) void item_softmax_fold_kernel(const float* __restrict__ part,
                                                                int64_t n_rows, int32_t dim,
                                                                int32_t n_splits,
                                                                float* __restrict__ out,
                                                                int64_t out_ld) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_rows * dim) return;
  const int64_t row = e / dim;
  float s = part[e];
  for (int32_t sp = 1; sp < n_splits; ++sp) s += part[(int64_t)sp * n_rows * dim + e];
  out[row * out_ld + (e - row * dim)] = s;
}

// the streamed ranges of a kernel: the forced count, or enough blocks for two per CU with
// ranges of at least 1024 rows
int32_t is_pick_splits(int64_t n_own, int64_t n_stream, int32_t n_splits) {
  if (n_splits > 0) return n_splits;
  if (n_own <= 0 || n_stream <= 0) return 1;
  int64_t s = ceil_div(2 * (int64_t)device_cus(), ceil_div(n_own, kT));
  s = s < n_stream / 1024 ? s : n_stream / 1024;
  s = s < kIsAutoSplitMax ? s : kIsAutoSplitMax;
  return (int32_t)(s < 1 ? 1 : s);
}

struct IsWs {
  int32_t* tgt;
  int64_t* tid;
  float* gs;
  float* stats;   // [sq][nq][3]
  float* part_q;  // [sq][nq][dim] when sq > 1
  float* part_v;  // [sv][nv][dim] when sv > 1
  int32_t sq, sv;
};

IsWs is_ws(Carver& c, int32_t nq, int64_t nv, int32_t dim, int32_t n_splits) {
  IsWs w;
  w.sq = is_pick_splits(nq, nv, n_splits);
  w.sv = is_pick_splits(nv, nq, n_splits);
  w.tgt = c.take<int32_t>((size_t)nq);
  w.tid = c.take<int64_t>((size_t)nq);
  w.gs = c.take<float>((size_t)nq);
  w.stats = c.take<float>((size_t)w.sq * (size_t)nq * 3);
  w.part_q = c.take<float>(w.sq > 1 ? (size_t)w.sq * (size_t)nq * (size_t)dim : 0);
  w.part_v = c.take<float>(w.sv > 1 ? (size_t)w.sv * (size_t)nv * (size_t)dim : 0);
  return w;
}

size_t is_lds_bytes(int32_t dim, int nb) {
  const int dq = (dim + 7) & ~7;
  const size_t tile = (size_t)kT * (dq + 4), grad = (size_t)kT * 32 * nb;
  return sizeof(float) * (kIsWaves * kMetaFloats + 17 * kT + (tile > grad ? tile : grad));
}

template <int MODE, bool FAST, int NB>
int32_t is_launch_as(const IsArgs& a, hipStream_t st) {
  const size_t lds = is_lds_bytes(a.dim, MODE == 0 ? 0 : NB);
  item_softmax_kernel<MODE, FAST, NB>
      <<<(unsigned)((int64_t)a.x_tiles * a.n_splits), kIsThreads, lds, st>>>(a);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

template <int MODE, bool FAST>
int32_t is_launch_nb(const IsArgs& a, hipStream_t st) {
  if constexpr (MODE == 0) {
    return is_launch_as<0, FAST, 1>(a, st);
  } else {
    switch ((a.dim + 31) / 32) {
      case 1: return is_launch_as<MODE, FAST, 1>(a, st);
      case 2: return is_launch_as<MODE, FAST, 2>(a, st);
      case 3: return is_launch_as<MODE, FAST, 3>(a, st);
      case 4: return is_launch_as<MODE, FAST, 4>(a, st);
      case 5: return is_launch_as<MODE, FAST, 5>(a, st);
      case 6: return is_launch_as<MODE, FAST, 6>(a, st);
      case 7: return is_launch_as<MODE, FAST, 7>(a, st);
      default: return is_launch_as<MODE, FAST, 8>(a, st);
    }
  }
}

// 16-byte loads of the streamed rows when their base, ld and dim allow it
template <int MODE>
int32_t is_launch(const IsArgs& a, hipStream_t st) {
  const float* y = MODE == 2 ? a.q : a.v;
  const int64_t y_ld = MODE == 2 ? a.q_ld : a.v_ld;
  const bool fast =
      (y_ld & 3) == 0 && (a.dim & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  return fast ? is_launch_nb<MODE, true>(a, st) : is_launch_nb<MODE, false>(a, st);
}

int32_t is_check(const char* fn, const float* queries, int64_t q_ld, int32_t n_queries,
                 const float* items, int64_t i_ld, int64_t n_items, int32_t dim,
                 const int32_t* targets, float inv_temp, int32_t n_splits) {
  RS_CHECK_ARG(dim >= 1 && dim <= kIsDimMax, "%s: need 1 <= dim <= 256, got %d", fn, dim);
  RS_CHECK_ARG(q_ld >= dim && i_ld >= dim, "%s: q_ld and i_ld must be >= dim", fn);
  RS_CHECK_ARG(n_queries >= 0 && n_items >= 0 && n_items < ((int64_t)1 << 31),
               "%s: need n_queries >= 0 and 0 <= n_items < 2^31", fn);
  RS_CHECK_ARG(n_splits >= 0 && n_splits <= kIsSplitMax, "%s: need 0 <= n_splits <= %d, got %d",
               fn, kIsSplitMax, n_splits);
  RS_CHECK_ARG(std::isfinite(inv_temp), "%s: inv_temp is not finite", fn);
  if (n_queries == 0) return RS_OK;
  RS_CHECK_ARG(n_items >= 1, "%s: no items", fn);
  RS_CHECK_ARG(queries != nullptr && items != nullptr, "%s: queries / items is NULL", fn);
  RS_CHECK_ARG(targets != nullptr || n_queries <= n_items,
               "%s: targets is NULL (row r's target is column r) with %d queries over %lld items",
               fn, n_queries, (long long)n_items);
  return RS_OK;
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" size_t rs_item_softmax_workspace_size(int32_t n_queries, int64_t n_items, int32_t dim,
                                                 int32_t n_splits) {
  if (n_queries <= 0 || n_items <= 0 || dim <= 0 || n_splits < 0 || n_splits > kIsSplitMax)
    return 0;
  Carver c(nullptr, 0);
  is_ws(c, n_queries, n_items, dim, n_splits);
  return c.off + 256;
}

extern "C" int32_t rs_item_softmax_fwd(const float* queries, int64_t q_ld, int32_t n_queries,
                                       const float* items, int64_t i_ld, int64_t n_items,
                                       int32_t dim, const int32_t* targets, float inv_temp,
                                       const float* col_bias, const int64_t* col_ids,
                                       int32_t n_splits, float* loss, float* lse, void* workspace,
                                       size_t ws_bytes, void* stream) {
  const int32_t rc = is_check("rs_item_softmax_fwd", queries, q_ld, n_queries, items, i_ld,
                              n_items, dim, targets, inv_temp, n_splits);
  if (rc != RS_OK || n_queries == 0) return rc;
  RS_CHECK_ARG(loss != nullptr && lse != nullptr, "rs_item_softmax_fwd: loss / lse is NULL");
  Carver c(workspace, ws_bytes);
  const IsWs w = is_ws(c, n_queries, n_items, dim, n_splits);
  RS_CHECK_ARG(workspace != nullptr && c.ok(),
               "rs_item_softmax_fwd: workspace of %zu bytes, need %zu", ws_bytes, c.off);
  const int64_t x_tiles = ceil_div(n_queries, kT);
  RS_CHECK_ARG(x_tiles * w.sq < ((int64_t)1 << 31), "rs_item_softmax_fwd: too many blocks");
  hipStream_t st = as_stream(stream);
  const unsigned rows_grid = (unsigned)ceil_div(n_queries, 256);
  item_softmax_prep_kernel<<<rows_grid, 256, 0, st>>>(targets, col_ids, nullptr, inv_temp,
                                                      n_queries, (int32_t)n_items, w.tgt, w.tid,
                                                      w.gs);
  RS_CHECK_LAUNCH();
  IsArgs a = {};
  a.q = queries;
  a.q_ld = q_ld;
  a.nq = n_queries;
  a.v = items;
  a.v_ld = i_ld;
  a.nv = (int32_t)n_items;
  a.dim = dim;
  a.inv_temp = inv_temp;
  a.bias = col_bias;
  a.ids = col_ids;
  a.tgt = w.tgt;
  a.tid = w.tid;
  a.n_splits = w.sq;
  a.x_tiles = (int32_t)x_tiles;
  a.out = w.stats;
  const int32_t rc2 = is_launch<0>(a, st);
  if (rc2 != RS_OK) return rc2;
  item_softmax_merge_kernel<<<rows_grid, 256, 0, st>>>(w.stats, w.tgt, n_queries,
                                                       (int32_t)n_items, w.sq, loss, lse);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

extern "C" int32_t rs_item_softmax_bwd(const float* queries, int64_t q_ld, int32_t n_queries,
                                       const float* items, int64_t i_ld, int64_t n_items,
                                       int32_t dim, const int32_t* targets, float inv_temp,
                                       const float* col_bias, const int64_t* col_ids,
                                       int32_t n_splits, const float* lse, const float* grad_loss,
                                       float* grad_queries, int64_t gq_ld, float* grad_items,
                                       int64_t gi_ld, void* workspace, size_t ws_bytes,
                                       void* stream) {
  const int32_t rc = is_check("rs_item_softmax_bwd", queries, q_ld, n_queries, items, i_ld,
                              n_items, dim, targets, inv_temp, n_splits);
  if (rc != RS_OK || n_queries == 0) return rc;
  RS_CHECK_ARG(lse != nullptr && grad_loss != nullptr,
               "rs_item_softmax_bwd: lse / grad_loss is NULL");
  RS_CHECK_ARG(grad_queries != nullptr || grad_items != nullptr,
               "rs_item_softmax_bwd: grad_queries and grad_items are both NULL");
  RS_CHECK_ARG((grad_queries == nullptr || gq_ld >= dim) && (grad_items == nullptr || gi_ld >= dim),
               "rs_item_softmax_bwd: gq_ld and gi_ld must be >= dim");
  Carver c(workspace, ws_bytes);
  const IsWs w = is_ws(c, n_queries, n_items, dim, n_splits);
  RS_CHECK_ARG(workspace != nullptr && c.ok(),
               "rs_item_softmax_bwd: workspace of %zu bytes, need %zu", ws_bytes, c.off);
  const int64_t q_tiles = ceil_div(n_queries, kT), v_tiles = ceil_div(n_items, kT);
  RS_CHECK_ARG(q_tiles * w.sq < ((int64_t)1 << 31) && v_tiles * w.sv < ((int64_t)1 << 31),
               "rs_item_softmax_bwd: too many blocks");
  hipStream_t st = as_stream(stream);
  item_softmax_prep_kernel<<<(unsigned)ceil_div(n_queries, 256), 256, 0, st>>>(
      targets, col_ids, grad_loss, inv_temp, n_queries, (int32_t)n_items, w.tgt, w.tid, w.gs);
  RS_CHECK_LAUNCH();
  IsArgs a = {};
  a.q = queries;
  a.q_ld = q_ld;
  a.nq = n_queries;
  a.v = items;
  a.v_ld = i_ld;
  a.nv = (int32_t)n_items;
  a.dim = dim;
  a.inv_temp = inv_temp;
  a.bias = col_bias;
  a.ids = col_ids;
  a.tgt = w.tgt;
  a.tid = w.tid;
  a.lse = lse;
  a.gs = w.gs;
  if (grad_queries) {
    a.n_splits = w.sq;
    a.x_tiles = (int32_t)q_tiles;
    a.out = w.sq > 1 ? w.part_q : grad_queries;
    a.out_ld = w.sq > 1 ? dim : gq_ld;
    a.split_stride = w.sq > 1 ? (int64_t)n_queries * dim : 0;
    const int32_t r1 = is_launch<1>(a, st);
    if (r1 != RS_OK) return r1;
    if (w.sq > 1) {
      item_softmax_fold_kernel<<<(unsigned)ceil_div((int64_t)n_queries * dim, 256), 256, 0, st>>>(
          w.part_q, n_queries, dim, w.sq, grad_queries, gq_ld);
      RS_CHECK_LAUNCH();
    }
  }
  if (grad_items) {
    a.n_splits = w.sv;
    a.x_tiles = (int32_t)v_tiles;
    a.out = w.sv > 1 ? w.part_v : grad_items;
    a.out_ld = w.sv > 1 ? dim : gi_ld;
    a.split_stride = w.sv > 1 ? n_items * dim : 0;
    const int32_t r2 = is_launch<2>(a, st);
    if (r2 != RS_OK) return r2;
    if (w.sv > 1) {
      item_softmax_fold_kernel<<<(unsigned)ceil_div(n_items * dim, 256), 256, 0, st>>>(
          w.part_v, n_items, dim, w.sv, grad_items, gi_ld);
      RS_CHECK_LAUNCH();
    }
  }
  return RS_OK;
}
