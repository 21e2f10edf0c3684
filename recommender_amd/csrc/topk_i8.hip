// topk_i8.hip — two-stage retrieval (recsys_hip.h, "Int8 candidate retrieval with an exact
// re-rank"): symmetric per-row int8 codes, an int8 MFMA candidate scan over the whole catalogue
// and the exact fp32 re-rank of the few candidates it keeps.
//
//   i8_quantize_kernel  a lane group per row: |x| maximum, scale = amax / 127, the codes; the
//                       whole code row is written, padding bytes as 0.
//   topk_i8_kernel      topk_ip_kernel's block (32 queries × one item range, 4 waves, 32-item
//                       tiles) and its whole selection machinery (topk_select.hpp), with the
//                       scoring replaced. The prologue quantises the block's 32 query rows into
//                       an int8 LDS tile (pad columns 0) and every lane takes its A fragments
//                       from it into registers for the block's life. An integer sum is exact in
//                       any order, so (a) the K order is free: half h of a lane owns the
//                       contiguous bytes [16 P h, 16 P (h + 1)) of its row (P = ceil(dim / 32)
//                       K chunks), on the query and on the item side alike, and chunk c
//                       multiplies fragment c of both halves; and (b) the B operand needs no
//                       LDS stage: a fragment is 16 contiguous bytes of one code row, global →
//                       registers, the next round's tile in flight while this one multiplies.
//                       P v_mfma_i32_32x32x32_i8 give the 32 × 32 integer scores; a lane then
//                       holds 16 queries' sums of one item, converts each (exact, |I| <= 2^22)
//                       and multiplies by its item's scale: the key. From there on the code is
//                       topk_ip_kernel's: threshold, LDS append, compaction, the final lists.
//   rerank_ip_kernel    one wave per query, a lane per candidate: candidate rows are loaded by
//                       half-waves, 32 columns at a time, into a wave-private LDS stage, each
//                       lane runs its candidate's ascending fmaf chain, one wave_sort orders
//                       them.
#include "topk_select.hpp"

namespace rs {
namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ bool nonfinite(float x) {
  return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

// the code of a finite x under a scale > 0: IEEE division, ties to even, clamped (a subnormal
// scale can put the quotient past 127); -128 is never produced
__device__ __forceinline__ int32_t i8_code(float x, float scale) {
  return (int32_t)fminf(fmaxf(rintf(__fdiv_rn(x, scale)), -127.f), 127.f);
}

// ---- quantise: one group of 2^lpr_log2 lanes per row, PW code bytes per store ---------------
template <int PW>
__global__ __launch_bounds__(256) void i8_quantize_kernel(const float* __restrict__ table,
                                                          int64_t ld, int64_t n_rows, int dim,
                                                          int8_t* __restrict__ codes,
                                                          int64_t c_ld, float* __restrict__ scales,
                                                          int32_t* err_flag, int lpr_log2) {
  constexpr int NW = PW / 4;
  const int lpr = 1 << lpr_log2;
  const int gl = threadIdx.x & (lpr - 1);
  const int64_t gpb = blockDim.x >> lpr_log2;
  const int64_t groups = (int64_t)gridDim.x * gpb;
  const int64_t pieces = c_ld / PW;  // the whole row is written, padding included
  bool flagged = false;
  for (int64_t r = (int64_t)blockIdx.x * gpb + (threadIdx.x >> lpr_log2); r < n_rows;
       r += groups) {
    const float* src = table + r * ld;
    float amax = 0.f;
    int bad = 0;
    for (int col = gl; col < dim; col += lpr) {
      const float x = src[col];
      amax = fmaxf(amax, fabsf(x));
      bad |= nonfinite(x);
    }
    // the group's lanes run this loop together: the exchange stays inside the group
    for (int m = 1; m < lpr; m <<= 1) {
      amax = fmaxf(amax, __shfl_xor(amax, m));
      bad |= __shfl_xor(bad, m);
    }
    const float scale = bad ? 0.f : __fdiv_rn(amax, 127.f);
    flagged |= bad != 0;
    if (gl == 0) scales[r] = scale;
    int8_t* crow = codes + r * c_ld;
    for (int64_t piece = gl; piece < pieces; piece += lpr) {
      uint32_t w[NW];
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        w[j] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t col = piece * PW + 4 * j + k;
          if (col < dim && scale != 0.f)
            w[j] |= ((uint32_t)i8_code(src[col], scale) & 0xffu) << (8 * k);
        }
      }
      if constexpr (PW == 16)
        *reinterpret_cast<uint4*>(crow + piece * PW) = make_uint4(w[0], w[1], w[2], w[3]);
      else
        *reinterpret_cast<uint32_t*>(crow + piece * PW) = w[0];
    }
  }
  if (__any(flagged) && (threadIdx.x & 63) == 0 && err_flag)
    atomicOr(err_flag, RS_ERRBIT_NONFINITE);
}

// ---- the candidate scan --------------------------------------------------------------------
struct TopkI8Args {
  const float* queries;
  int64_t q_ld;
  int32_t n_queries;
  const int8_t* codes;
  int64_t c_ld;
  const float* scales;
  int32_t n_items;
  int32_t dim;
  int64_t excl_base;
  const int64_t* excl_indptr;
  const int32_t* excl_items;
  const int32_t* excl_one;
  int32_t k;
  int32_t n_splits;
  int32_t q_tiles;
  int32_t* out_items;  // n_splits == 1: the outputs; else the workspace lists
  float* out_keys;     // may be NULL when n_splits == 1
};

// the bytes of a 4-byte word of which the first nv lie below dim
__device__ __forceinline__ uint32_t word_mask(int nv) {
  return nv >= 4 ? 0xffffffffu : nv <= 0 ? 0u : (1u << (8 * nv)) - 1u;
}

constexpr size_t kI8LdsBytes = sizeof(float) * ((size_t)kTileQ * kCap * 2 + (size_t)kTileQ * 4);

// P = ceil(dim / 32) K chunks; WIDE: 16-byte loads of the code rows, else 4-byte loads
template <int P, bool WIDE>
__global__ __launch_bounds__(kIpThreads) void topk_i8_kernel(const TopkI8Args a) {
  constexpr int DK = 32 * P;   // K, padded
  constexpr int QS = DK + 16;  // bytes of an LDS query row: 16-byte aligned, rows 4 banks apart
  static_assert((size_t)kTileQ * QS <= sizeof(float) * kTileQ * kCap, "the tile fits the alias");
  extern __shared__ __align__(16) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int32_t dim = a.dim;
  float* cand_s = lds;
  int32_t* cand_i = reinterpret_cast<int32_t*>(cand_s + kTileQ * kCap);
  int32_t* cnt = cand_i + kTileQ * kCap;
  float* th_s = reinterpret_cast<float*>(cnt + kTileQ);
  int32_t* th_i = reinterpret_cast<int32_t*>(th_s + kTileQ);
  int32_t* ex1 = th_i + kTileQ;
  // the int8 query tile lives in the candidate lists' space until every lane has its fragments
  int8_t* Q8 = reinterpret_cast<int8_t*>(lds);

  const int32_t sp = blockIdx.x / a.q_tiles;
  const int32_t q0 = (blockIdx.x - sp * a.q_tiles) * kTileQ;
  const int32_t nq = min(kTileQ, a.n_queries - q0);
  const int32_t per = a.n_items / a.n_splits;
  const int32_t lo = sp * per;
  const int32_t hi = sp == a.n_splits - 1 ? a.n_items : lo + per;

  {  // 8 lanes quantise one query row by the rule of rs_quantize_rows_i8; rows past nq are 0
    const int row = tid >> 3, gl = tid & 7;
    const bool live = row < nq;
    const float* src = a.queries + (int64_t)(q0 + (live ? row : 0)) * a.q_ld;
    float amax = 0.f;
    int bad = 0;
    for (int col = gl; col < dim; col += 8) {
      const float x = src[col];
      amax = fmaxf(amax, fabsf(x));
      bad |= nonfinite(x);
    }
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
      amax = fmaxf(amax, __shfl_xor(amax, m));
      bad |= __shfl_xor(bad, m);
    }
    const float scale = bad || !live ? 0.f : __fdiv_rn(amax, 127.f);
    for (int col = gl; col < DK; col += 8) {
      int32_t c = 0;
      if (col < dim && scale != 0.f) c = i8_code(src[col], scale);
      Q8[row * QS + col] = (int8_t)c;
    }
  }
  if (tid < kTileQ) {
    cnt[tid] = 0;
    th_i[tid] = INT_MAX;
    th_s[tid] = tid < nq ? -INFINITY : INFINITY;  // rows past the last query take nothing
    ex1[tid] = a.excl_one && tid < nq ? a.excl_one[q0 + tid] : -1;
  }
  __syncthreads();

  // lane (mrow, half) owns bytes [16 P half, 16 P (half + 1)) of row mrow: fragment c of chunk c
  const int mrow = lane & 31, half = lane >> 5;
  i32x4 qa[P];
#pragma unroll
  for (int c = 0; c < P; ++c)
    qa[c] = *reinterpret_cast<const i32x4*>(Q8 + mrow * QS + 16 * (P * half + c));
  __syncthreads();  // the tile is in registers: the candidate lists may be written

  const int32_t n_tiles = (hi - lo + kTileI - 1) / kTileI;
  const int32_t n_rounds = (n_tiles + kIpWaves - 1) / kIpWaves;

  // This lane's P fragments of the item at tile row mrow, and the item's scale. Unconditional
  // loads and nothing that reads them, so all are in flight together. A row past the range's end
  // re-reads the last row (its keys are never looked at); a fragment (WIDE) or word that starts
  // at or past dim re-reads the row's first and is masked to 0 when it is used, so nothing past
  // round_up(dim, 16) (WIDE) or round_up(dim, 4) bytes of a row is read: both are <= c_ld.
  auto fetch = [&](int64_t jb, i32x4 (&dst)[P], float& sc) {
    const int64_t j = jb + mrow;
    const int64_t jc = j < hi ? j : (int64_t)hi - 1;
    const int8_t* row = a.codes + jc * a.c_ld;
#pragma unroll
    for (int c = 0; c < P; ++c) {
      const int o = 16 * (P * half + c);
      if constexpr (WIDE) {
        dst[c] = *reinterpret_cast<const i32x4*>(row + (o < dim ? o : 0));
      } else {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int ow = o + 4 * w;
          dst[c][w] = *reinterpret_cast<const int32_t*>(row + (ow < dim ? ow : 0));
        }
      }
    }
    sc = a.scales[jc];
  };

  i32x4 cur[P], nxt[P];
  float cur_sc, nxt_sc;
  fetch((int64_t)lo + wid * kTileI, cur, cur_sc);
  for (int32_t round = 0; round < n_rounds; ++round) {
    const int64_t jb64 = (int64_t)lo + ((int64_t)round * kIpWaves + wid) * kTileI;
    const bool active = jb64 < hi;
    const int32_t jb = active ? (int32_t)jb64 : hi;
    fetch(jb64 + kRound, nxt, nxt_sc);  // past the last tile: the range's last row, never used
    i32x16 acc = {};
    if (active) {  // wave-uniform: the MFMA runs for the whole wave, tail lanes included
#pragma unroll
      for (int c = 0; c < P; ++c) {
        const int o = 16 * (P * half + c);
        i32x4 b;
#pragma unroll
        for (int w = 0; w < 4; ++w) b[w] = cur[c][w] & (int32_t)word_mask(dim - (o + 4 * w));
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(qa[c], b, acc, 0, 0, 0);
      }
    }
    if (active && jb + mrow < hi) {
      const int32_t j = jb + mrow;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 t4 = *reinterpret_cast<const float4*>(th_s + 8 * g + 4 * half);
        const float th[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = 8 * g + 4 * half + u;  // the query row of accumulator register 4 g + u
          const float s = __fmul_rn((float)acc[4 * g + u], cur_sc);
          if (s < th[u]) continue;  // nearly every pair; false for a NaN on either side
          if (i < nq && better(s, j, th[u], th_i[i]) && j != ex1[i]) {
            const int32_t slot = atomicAdd(&cnt[i], 1);
            if (slot < kCap) {  // always: a list enters a round with count + kRound <= kCap
              cand_s[i * kCap + slot] = s;
              cand_i[i * kCap + slot] = j;
            }
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < P; ++c) cur[c] = nxt[c];
    cur_sc = nxt_sc;
    __syncthreads();
    const uint64_t full = __ballot(lane < nq && cnt[lane & (kTileQ - 1)] + kRound > kCap);
    for (int q = wid; q < nq; q += kIpWaves)
      if ((full >> q) & 1)
        compact_query(q, lane, a.k, cand_s, cand_i, cnt, th_s, th_i, a.excl_indptr,
                      a.excl_items, a.excl_base + q0 + q, nullptr, nullptr, false);
    __syncthreads();
  }
  const bool final = a.n_splits == 1;
  for (int q = wid; q < nq; q += kIpWaves) {
    const int64_t o = ((int64_t)(q0 + q) * a.n_splits + sp) * a.k;
    compact_query(q, lane, a.k, cand_s, cand_i, cnt, th_s, th_i, a.excl_indptr, a.excl_items,
                  a.excl_base + q0 + q, a.out_items + o, a.out_keys ? a.out_keys + o : nullptr,
                  final);
  }
}

template <int P, bool WIDE>
int32_t launch_topk_i8_as(const TopkI8Args& a, int64_t grid, hipStream_t st) {
  RS_CHECK_HIP(hipFuncSetAttribute((const void*)topk_i8_kernel<P, WIDE>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kI8LdsBytes));
  topk_i8_kernel<P, WIDE><<<(unsigned)grid, kIpThreads, kI8LdsBytes, st>>>(a);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

template <int P>
int32_t launch_topk_i8(const TopkI8Args& a, int64_t grid, hipStream_t st) {
  const bool wide = (a.c_ld & 15) == 0 && (reinterpret_cast<uintptr_t>(a.codes) & 15) == 0;
  return wide ? launch_topk_i8_as<P, true>(a, grid, st) : launch_topk_i8_as<P, false>(a, grid, st);
}

int32_t launch_topk_i8_dim(const TopkI8Args& a, int64_t grid, hipStream_t st) {
  switch ((a.dim + 31) / 32) {
    case 1: return launch_topk_i8<1>(a, grid, st);
    case 2: return launch_topk_i8<2>(a, grid, st);
    case 3: return launch_topk_i8<3>(a, grid, st);
    case 4: return launch_topk_i8<4>(a, grid, st);
    case 5: return launch_topk_i8<5>(a, grid, st);
    case 6: return launch_topk_i8<6>(a, grid, st);
    case 7: return launch_topk_i8<7>(a, grid, st);
    default: return launch_topk_i8<8>(a, grid, st);
  }
}

// ---- the exact re-rank ---------------------------------------------------------------------
constexpr int kRrCols = 32;            // columns staged at a time
constexpr int kRrStride = kRrCols + 1; // odd: the 64 candidates' rows of a column fall in 64 banks

__global__ __launch_bounds__(kIpThreads) void rerank_ip_kernel(
    const float* __restrict__ queries, int64_t q_ld, int32_t n_queries,
    const float* __restrict__ items, int64_t i_ld, int32_t n_items, int32_t dim,
    const int32_t* __restrict__ cand, int32_t kc, int32_t k, int32_t* __restrict__ out_items,
    float* __restrict__ out_scores) {
  __shared__ float stage[kIpWaves][kWave * kRrStride];
  __shared__ float qrow[kIpWaves][kDimMax];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * kIpWaves + wid;
  if (r >= n_queries) return;  // whole waves; nothing below synchronises across waves
  float* st = stage[wid];
  float* q = qrow[wid];
  for (int d = lane; d < dim; d += kWave) q[d] = queries[r * q_ld + d];
  const int32_t id = lane < kc ? cand[r * kc + lane] : -1;
  const bool ok = id >= 0 && id < n_items;  // anything else (-1 is the scan's padding) is skipped
  const int sub = lane & (kRrCols - 1), hw = lane >> 5;
  float acc = 0.f;
  for (int c0 = 0; c0 < dim; c0 += kRrCols) {
    // a half-wave loads 32 columns of one candidate's row: candidates 2 t and 2 t + 1 together
    for (int t = 0; 2 * t < kc; ++t) {
      const int cl = 2 * t + hw;
      const int32_t cid = __shfl(id, cl, kWave);
      float x = 0.f;
      if (cid >= 0 && cid < n_items && c0 + sub < dim) x = items[(int64_t)cid * i_ld + c0 + sub];
      st[cl * kRrStride + sub] = x;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the score contract: one fmaf per column, ascending, from +0
    const int nc = min(kRrCols, dim - c0);
    for (int d = 0; d < nc; ++d) acc = __fmaf_rn(q[c0 + d], st[lane * kRrStride + d], acc);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  float v[1] = {ok ? acc : -INFINITY};
  int32_t ix[1] = {ok ? id : INT_MAX};
  wave_sort<1>(v, ix, lane);
  if (lane < k) {
    const bool pad = ix[0] == INT_MAX;
    out_items[r * k + lane] = pad ? -1 : ix[0];
    if (out_scores) out_scores[r * k + lane] = pad ? -INFINITY : v[0];
  }
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" size_t rs_i8_row_bytes(int32_t dim) {
  return dim <= 0 ? 0 : align_up((size_t)dim, 16);
}

extern "C" int32_t rs_quantize_rows_i8(const float* table, int64_t ld, int64_t n_rows, int32_t dim,
                                       int8_t* codes, int64_t c_ld, float* scales,
                                       int32_t* err_flag, void* stream) {
  RS_CHECK_ARG(dim >= 1 && n_rows >= 0, "rs_quantize_rows_i8: need dim >= 1 and n_rows >= 0");
  RS_CHECK_ARG(ld >= dim && c_ld >= dim && (c_ld & 3) == 0,
               "rs_quantize_rows_i8: need ld >= dim, c_ld >= dim and c_ld %% 4 == 0");
  RS_CHECK_ARG((reinterpret_cast<uintptr_t>(codes) & 3) == 0,
               "rs_quantize_rows_i8: codes must be 4-byte aligned");
  if (n_rows == 0) return RS_OK;
  RS_CHECK_ARG(table != nullptr && codes != nullptr && scales != nullptr,
               "rs_quantize_rows_i8: table / codes / scales is NULL");
  hipStream_t st = as_stream(stream);
  const bool wide = (c_ld & 15) == 0 && (reinterpret_cast<uintptr_t>(codes) & 15) == 0;
  const int pw = wide ? 16 : 4;
  int lpr_log2 = 0;
  while (lpr_log2 < 6 && (pw << lpr_log2) < dim) ++lpr_log2;
  const int64_t rows_per_block = 256 >> lpr_log2;
  int64_t blocks = ceil_div(n_rows, rows_per_block);
  blocks = blocks < (1 << 20) ? blocks : (1 << 20);
  if (wide)
    i8_quantize_kernel<16><<<(unsigned)blocks, 256, 0, st>>>(table, ld, n_rows, dim, codes, c_ld,
                                                             scales, err_flag, lpr_log2);
  else
    i8_quantize_kernel<4><<<(unsigned)blocks, 256, 0, st>>>(table, ld, n_rows, dim, codes, c_ld,
                                                            scales, err_flag, lpr_log2);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

extern "C" size_t rs_topk_ip_i8_workspace_size(int32_t n_queries, int64_t n_items, int32_t kc,
                                               int32_t n_splits) {
  if (n_queries <= 0 || n_items <= 0 || kc <= 0 || n_splits < 0) return 0;
  return ws_bytes_for(n_queries, pick_splits(n_queries, n_items, n_splits), kc);
}

extern "C" int32_t rs_topk_ip_i8(const float* queries, int64_t q_ld, int32_t n_queries,
                                 const int8_t* codes, int64_t c_ld, const float* scales,
                                 int64_t n_items, int32_t dim, int64_t excl_base,
                                 const int64_t* excl_indptr, const int32_t* excl_items,
                                 const int32_t* excl_one, int32_t kc, int32_t n_splits,
                                 int32_t* out_items, float* out_keys, void* workspace,
                                 size_t ws_bytes, void* stream) {
  RS_CHECK_ARG(kc >= 1 && kc <= kKMax, "rs_topk_ip_i8: need 1 <= kc <= 64, got %d", kc);
  RS_CHECK_ARG(dim >= 1 && dim <= kDimMax, "rs_topk_ip_i8: need 1 <= dim <= 256, got %d", dim);
  RS_CHECK_ARG(q_ld >= dim && c_ld >= dim, "rs_topk_ip_i8: q_ld and c_ld must be >= dim");
  RS_CHECK_ARG((c_ld & 3) == 0 && (reinterpret_cast<uintptr_t>(codes) & 3) == 0,
               "rs_topk_ip_i8: need c_ld %% 4 == 0 and codes 4-byte aligned");
  RS_CHECK_ARG(n_queries >= 0 && n_items >= 0 && n_items < ((int64_t)1 << 31),
               "rs_topk_ip_i8: need n_queries >= 0 and 0 <= n_items < 2^31");
  RS_CHECK_ARG(n_splits >= 0 && (n_items == 0 || n_splits <= n_items),
               "rs_topk_ip_i8: need 0 <= n_splits <= n_items");
  RS_CHECK_ARG(excl_base >= 0, "rs_topk_ip_i8: excl_base < 0");
  if (n_queries == 0) return RS_OK;
  RS_CHECK_ARG(out_items != nullptr, "rs_topk_ip_i8: out_items is NULL");
  hipStream_t st = as_stream(stream);
  if (n_items == 0) {
    const int64_t n = (int64_t)n_queries * kc;
    topk_ip_pad_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(n, out_items, out_keys);
    RS_CHECK_LAUNCH();
    return RS_OK;
  }
  RS_CHECK_ARG(queries != nullptr && codes != nullptr && scales != nullptr,
               "rs_topk_ip_i8: queries / codes / scales is NULL");
  const int64_t splits = pick_splits(n_queries, n_items, n_splits);
  const int64_t q_tiles = ceil_div(n_queries, kTileQ);
  RS_CHECK_ARG(q_tiles * splits < ((int64_t)1 << 31), "rs_topk_ip_i8: too many blocks");
  const size_t need = ws_bytes_for(n_queries, splits, kc);
  RS_CHECK_ARG(need == 0 || (workspace != nullptr && ws_bytes >= need),
               "rs_topk_ip_i8: workspace of %zu bytes, need %zu", ws_bytes, need);
  TopkI8Args a;
  a.queries = queries;
  a.q_ld = q_ld;
  a.n_queries = n_queries;
  a.codes = codes;
  a.c_ld = c_ld;
  a.scales = scales;
  a.n_items = (int32_t)n_items;
  a.dim = dim;
  a.excl_base = excl_base;
  a.excl_indptr = excl_indptr;
  a.excl_items = excl_items;
  a.excl_one = excl_one;
  a.k = kc;
  a.n_splits = (int32_t)splits;
  a.q_tiles = (int32_t)q_tiles;
  int32_t* ws_items = static_cast<int32_t*>(workspace);
  float* ws_keys = reinterpret_cast<float*>(static_cast<char*>(workspace) + need / 2);
  a.out_items = splits == 1 ? out_items : ws_items;
  a.out_keys = splits == 1 ? out_keys : ws_keys;
  const int32_t rc = launch_topk_i8_dim(a, q_tiles * splits, st);
  if (rc != RS_OK || splits == 1) return rc;
  topk_ip_merge_kernel<<<(unsigned)ceil_div(n_queries, kIpWaves), kIpThreads, 0, st>>>(
      ws_items, ws_keys, n_queries, nullptr, 1, 0, (int32_t)splits, kc, out_items, out_keys);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

extern "C" int32_t rs_rerank_ip(const float* queries, int64_t q_ld, int32_t n_queries,
                                const float* items, int64_t i_ld, int64_t n_items, int32_t dim,
                                const int32_t* cand, int32_t kc, int32_t k, int32_t* out_items,
                                float* out_scores, void* stream) {
  RS_CHECK_ARG(k >= 1 && k <= kc && kc <= kKMax, "rs_rerank_ip: need 1 <= k <= kc <= 64");
  RS_CHECK_ARG(dim >= 1 && dim <= kDimMax, "rs_rerank_ip: need 1 <= dim <= 256, got %d", dim);
  RS_CHECK_ARG(q_ld >= dim && i_ld >= dim, "rs_rerank_ip: q_ld and i_ld must be >= dim");
  RS_CHECK_ARG(n_queries >= 0 && n_items >= 0 && n_items < ((int64_t)1 << 31),
               "rs_rerank_ip: need n_queries >= 0 and 0 <= n_items < 2^31");
  if (n_queries == 0) return RS_OK;
  RS_CHECK_ARG(queries != nullptr && cand != nullptr && out_items != nullptr,
               "rs_rerank_ip: queries / cand / out_items is NULL");
  RS_CHECK_ARG(items != nullptr || n_items == 0, "rs_rerank_ip: items is NULL");
  rerank_ip_kernel<<<(unsigned)ceil_div(n_queries, kIpWaves), kIpThreads, 0, as_stream(stream)>>>(
      queries, q_ld, n_queries, items, i_ld, (int32_t)n_items, dim, cand, kc, k, out_items,
      out_scores);
  RS_CHECK_LAUNCH();
  return RS_OK;
}
