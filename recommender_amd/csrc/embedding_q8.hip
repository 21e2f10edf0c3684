// embedding_q8.hip — row-wise int8 embedding tables for serving (RS_Q8, include/recsys_hip.h
// a-1c): quantise an fp32 table, dequantise it, gather rows of it, pool bags of it.
//
// A quantised row is q_ld bytes: scale (fp32), bias (fp32), dim uint8 codes, zero padding.
// Quantise writes it in the row's own aligned pieces of PW bytes (piece j = bytes [j * PW,
// (j + 1) * PW), columns [j * PW - 8, j * PW - 8 + PW)): PW = 16 when the base and q_ld allow
// 16-byte stores (piece 0 is the header and 8 codes), PW = 4 otherwise. Both give the same bits.
// The readers take the codes in pieces of PW bytes from byte 8 on (piece j = columns [j * PW,
// (j + 1) * PW)), and every lane reads the 8-byte header itself (the same cache line as piece 0).
// Measured at D = 128 and 64 (profiles/embedding_q8_bench.txt): the lookup is fastest
// with PW = 4 (a lane's four floats are one 16-byte store, so a group's stores are contiguous;
// with 16-byte pieces each lane stored 64 bytes of its own and the lookup ran 0.84x the fp32
// gather instead of 1.23x); the bag, which stores once per bag, with PW = 8 (16 lanes per
// D = 128 row, all busy; 16-byte pieces left 7 of 16 idle: 1.37x against 1.87x). The bag falls
// back to PW = 4 when the base or q_ld is not a multiple of 8: the same bits.
// A lane group of 1 << lpr_log2 lanes owns a row or a bag, lane l taking pieces l, l + lanes, ...
// Four rows are requested before any is consumed, as in embedding.hip's gather and
// embedding_bag.hip's walk, and every load is unguarded from an address that is always valid.
// The bag keeps embedding_bag.hip's order of additions: the position order alone.
// No atomics except the error flag's OR; plain vector stores only.
#include <algorithm>
#include <cmath>

#include "dlrm_shared.hpp"
#include "row_io.hpp"

namespace rs {
namespace {

template <int PW>
struct Piece;
template <>
struct Piece<16> {
  static __device__ __forceinline__ void store(uint8_t* p, const uint32_t (&w)[4]) {
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};
template <>
struct Piece<8> {
  static __device__ __forceinline__ void load(const uint8_t* p, uint32_t (&w)[2]) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    w[0] = t.x; w[1] = t.y;
  }
  static __device__ __forceinline__ void header(const uint8_t* row, float& scale, float& bias) {
    const float2 h = *reinterpret_cast<const float2*>(row);
    scale = h.x; bias = h.y;
  }
};
template <>
struct Piece<4> {
  static __device__ __forceinline__ void load(const uint8_t* p, uint32_t (&w)[1]) {
    w[0] = *reinterpret_cast<const uint32_t*>(p);
  }
  static __device__ __forceinline__ void store(uint8_t* p, const uint32_t (&w)[1]) {
    *reinterpret_cast<uint32_t*>(p) = w[0];
  }
  static __device__ __forceinline__ void header(const uint8_t* row, float& scale, float& bias) {
    scale = *reinterpret_cast<const float*>(row);
    bias = *reinterpret_cast<const float*>(row + 4);
  }
};

// v[k] = code k of the piece, dequantised: one rounded multiply, one rounded add, never an fma
template <int PW>
__device__ __forceinline__ void dequant_piece(const uint32_t (&w)[PW / 4], float scale, float bias,
                                              float (&v)[PW]) {
#pragma unroll
  for (int j = 0; j < PW / 4; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      v[4 * j + k] = q8_value(w[j], k, scale, bias);
}

// the piece's columns [col0, col0 + PW) that lie in [0, dim), to row o; col0 is a multiple of 4
template <int PW, bool OUT4>
__device__ __forceinline__ void store_cols(float* __restrict__ o, int col0, int dim,
                                           const float (&v)[PW]) {
#pragma unroll
  for (int j = 0; j < PW / 4; ++j) {
    const int c4 = col0 + 4 * j;
    if (OUT4 && c4 >= 0 && c4 + 4 <= dim) {
      *reinterpret_cast<float4*>(o + c4) =
          make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c4 + k >= 0 && c4 + k < dim) o[c4 + k] = v[4 * j + k];
    }
  }
}

constexpr int kHeader = 8;  // the readers' piece 0 starts at the codes

__device__ __forceinline__ bool nonfinite(float x) {
  return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

// ---- quantise: one lane group per row, min / max reduction, then the codes -----------------
template <int PW>
__global__ __launch_bounds__(256) void q8_quantize_kernel(const float* __restrict__ table,
                                                          int64_t ld, int64_t n_rows, int dim,
                                                          uint8_t* __restrict__ qt, int64_t q_ld,
                                                          int32_t* err_flag, int lpr_log2,
                                                          int chunks) {
  constexpr int NW = PW / 4;
  const int lpr = 1 << lpr_log2;
  const int gl = threadIdx.x & (lpr - 1);
  const int64_t gpb = blockDim.x >> lpr_log2;
  const int64_t groups = (int64_t)gridDim.x * gpb;
  const int pieces = (int)(q_ld / PW);  // the whole row is written, padding included
  bool flagged = false;
  for (int64_t r = (int64_t)blockIdx.x * gpb + (threadIdx.x >> lpr_log2); r < n_rows;
       r += groups) {
    const float* src = table + r * ld;
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int c = 0; c < chunks; ++c) {
      const int col0 = (gl + c * lpr) * PW - 8;
#pragma unroll
      for (int k = 0; k < PW; ++k) {
        const int col = col0 + k;
        const bool ok = col >= 0 && col < dim;
        const float x = src[ok ? col : 0];
        if (ok) {
          lo = fminf(lo, x);
          hi = fmaxf(hi, x);
          bad |= nonfinite(x);
        }
      }
    }
    // the group's lanes run this loop together: the exchange stays inside the group
    for (int m = 1; m < lpr; m <<= 1) {
      lo = fminf(lo, __shfl_xor(lo, m));
      hi = fmaxf(hi, __shfl_xor(hi, m));
      bad |= __shfl_xor(bad, m);
    }
    lo = lo + 0.f;  // -0 -> +0
    hi = hi + 0.f;
    const float range = __fsub_rn(hi, lo);
    bad |= nonfinite(range);
    float scale = __fdiv_rn(range, 255.f);
    if (bad) {
      scale = 0.f;
      lo = 0.f;
      flagged = true;
    }
    uint8_t* qrow = qt + r * q_ld;
    for (int c = 0; c < chunks; ++c) {
      const int piece = gl + c * lpr;
      const int col0 = piece * PW - 8;
      uint32_t w[NW];
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        w[j] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int col = col0 + 4 * j + k;
          const bool ok = col >= 0 && col < dim;
          const float x = src[ok ? col : 0];
          uint32_t code = 0;
          if (ok && scale != 0.f) {
            const float q = rintf(__fdiv_rn(__fsub_rn(x, lo), scale));
            code = (uint32_t)fminf(fmaxf(q, 0.f), 255.f);
          }
          w[j] |= code << (8 * k);
        }
        const int word = piece * NW + j;  // words 0 and 1 of the row are the header
        if (word == 0) w[j] = __float_as_uint(scale);
        if (word == 1) w[j] = __float_as_uint(lo);
      }
      if (piece < pieces) Piece<PW>::store(qrow + (int64_t)piece * PW, w);
    }
  }
  if (__any(flagged) && (threadIdx.x & 63) == 0 && err_flag)
    atomicOr(err_flag, RS_ERRBIT_NONFINITE);
}

// ---- lookup (IDENT: row p itself, the dequantise) ------------------------------------------
template <int PW, bool OUT4, typename IdT, bool IDENT>
__global__ __launch_bounds__(256) void q8_lookup_kernel(
    const uint8_t* __restrict__ qt, int64_t n_rows, int dim, int64_t q_ld,
    const IdT* __restrict__ ids, int64_t n_ids, const int64_t* __restrict__ slot_offsets,
    int32_t n_slots, float* __restrict__ out, int64_t out_ld, int32_t* err_flag, int lpr_log2,
    int chunks) {
  constexpr int U = 4, NW = PW / 4;
  const int lpr = 1 << lpr_log2;
  const int gl = threadIdx.x & (lpr - 1);
  const int64_t gpb = blockDim.x >> lpr_log2;
  const int64_t groups = (int64_t)gridDim.x * gpb;
  const int64_t g = (int64_t)blockIdx.x * gpb + (threadIdx.x >> lpr_log2);
  const int pieces = (dim + PW - 1) / PW;
  bool oob = false;
  for (int64_t base = g; base < n_ids; base += groups * U) {
    // an entry past the ids re-reads position `base`, an out-of-range id reads table row 0
    int64_t row[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t p = base + u * groups;
      const int64_t pc = p < n_ids ? p : base;
      if constexpr (IDENT) {
        row[u] = pc;
        in[u] = true;
      } else {
        const int64_t id = static_cast<int64_t>(ids[pc]);
        int64_t lo = 0, card = n_rows;
        if (slot_offsets) {
          const int s = (int)(pc % n_slots);
          lo = slot_offsets[s];
          card = slot_offsets[s + 1] - lo;
        }
        in[u] = id >= 0 && id < card;
        row[u] = in[u] ? lo + id : 0;
        oob |= p < n_ids && !in[u];
      }
    }
    for (int c = 0; c < chunks; ++c) {
      const int piece = gl + c * lpr;
      const int pc = piece < pieces ? piece : 0;  // lanes past the row read piece 0, never stored
      uint32_t w[U][NW];
      float scale[U], bias[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint8_t* rp = qt + row[u] * q_ld;
        Piece<PW>::header(rp, scale[u], bias[u]);
        Piece<PW>::load(rp + kHeader + (int64_t)pc * PW, w[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = base + u * groups;
        if (p < n_ids && piece < pieces) {
          float v[PW];
          dequant_piece<PW>(w[u], scale[u], bias[u], v);
          if (!in[u]) {
#pragma unroll
            for (int k = 0; k < PW; ++k) v[k] = 0.f;
          }
          store_cols<PW, OUT4>(out + p * out_ld, piece * PW, dim, v);
        }
      }
    }
  }
  if (__any(oob) && (threadIdx.x & 63) == 0) flag_oob(err_flag);
}

// ---- bag: embedding_bag.hip's bag_fwd_kernel over dequantised pieces ------------------------
template <int PW, bool OUT4, typename IdT>
__global__ __launch_bounds__(256) void q8_bag_kernel(
    const uint8_t* __restrict__ qt, int64_t q_ld, int64_t n_rows, int dim,
    const IdT* __restrict__ ids, int64_t n_ids, const int64_t* __restrict__ offsets,
    int64_t n_bags, int32_t bag_len, const uint8_t* __restrict__ valid,
    const float* __restrict__ weights, int32_t mode, const int64_t* __restrict__ slot_offsets,
    int32_t n_slots, float* __restrict__ out, int64_t out_ld, float* __restrict__ bag_scale,
    int32_t* err_flag, int lpr_log2, int chunks) {
  constexpr int U = 4, NW = PW / 4;
  const int lpr = 1 << lpr_log2;
  const int gl = threadIdx.x & (lpr - 1);
  const int64_t gpb = blockDim.x >> lpr_log2;
  const int64_t groups = (int64_t)gridDim.x * gpb;
  const int pieces = (dim + PW - 1) / PW;
  bool bad = false;
  // without a mask or weights the flag / weight loads still go out, from the ids' own bytes, and
  // are ignored (embedding_bag.hip: a branch around a load serialises the batch's loads)
  const uint8_t* vp = valid ? valid : reinterpret_cast<const uint8_t*>(ids);
  const float* wp = weights ? weights : reinterpret_cast<const float*>(ids);
  for (int64_t b = (int64_t)blockIdx.x * gpb + (threadIdx.x >> lpr_log2); b < n_bags;
       b += groups) {
    int64_t s, e;
    if (!offsets) {
      s = b * bag_len;
      e = s + bag_len;
    } else {
      s = offsets[b];
      e = offsets[b + 1];
      if (s < 0 || e > n_ids || s > e) {  // reversed, or leaving [0, n_ids]: empty and reported
        s = e = 0;
        bad = true;
      }
    }
    int64_t lo = 0, card = n_rows;
    if (slot_offsets) {
      const int sl = (int)(b % n_slots);
      lo = slot_offsets[sl];
      card = slot_offsets[sl + 1] - lo;
    }
    int64_t count = 0;
    for (int c = 0; c < chunks; ++c) {
      const int piece = gl + c * lpr;
      const int pc = piece < pieces ? piece : 0;
      float acc[PW];
#pragma unroll
      for (int k = 0; k < PW; ++k) acc[k] = 0.f;
      count = 0;
      for (int64_t p0 = s; p0 < e; p0 += U) {
        // unguarded loads from always-valid addresses: an entry past the bag re-reads position
        // s, a dead or out-of-range one reads table row 0
        int64_t id[U];
        uint8_t vl[U];
        float wt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t p = p0 + u < e ? p0 + u : s;
          id[u] = static_cast<int64_t>(ids[p]);
          vl[u] = vp[p];
          wt[u] = wp[p];
        }
        uint32_t w[U][NW];
        float scale[U], bias[U];
        bool live[U], in[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          live[u] = p0 + u < e && (!valid || vl[u] != 0);
          in[u] = id[u] >= 0 && id[u] < card;
          const int64_t r = (live[u] && in[u]) ? lo + id[u] : 0;
          const uint8_t* rp = qt + r * q_ld;
          Piece<PW>::header(rp, scale[u], bias[u]);
          Piece<PW>::load(rp + kHeader + (int64_t)pc * PW, w[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (live[u]) {
            ++count;
            bad |= !in[u];
            float v[PW];
            dequant_piece<PW>(w[u], scale[u], bias[u], v);
#pragma unroll
            for (int k = 0; k < PW; ++k) {
              float t = in[u] ? v[k] : 0.f;
              if (weights) t = __fmul_rn(wt[u], t);
              acc[k] = __fadd_rn(acc[k], t);
            }
          }
        }
      }
      if (piece < pieces) {
        if (mode == RS_BAG_MEAN) {
          const float n = (float)count;
#pragma unroll
          for (int k = 0; k < PW; ++k) acc[k] = count > 0 ? __fdiv_rn(acc[k], n) : 0.f;
        }
        store_cols<PW, OUT4>(out + b * out_ld, piece * PW, dim, acc);
      }
    }
    if (bag_scale && gl == 0) bag_scale[b] = count > 0 ? __fdiv_rn(1.f, (float)count) : 0.f;
  }
  flag_oob_wave(bad, err_flag);
}

// q_ld >= 8 + dim, a multiple of 4; the table 4-byte aligned (the header is two floats)
int32_t check_q8(const void* qtable, int32_t dim, int64_t q_ld) {
  RS_CHECK_ARG(dim > 0, "dim must be > 0");
  RS_CHECK_ARG(q_ld >= 8 + (int64_t)dim, "q_ld must be >= 8 + dim");
  RS_CHECK_ARG(q_ld % 4 == 0, "q_ld must be a multiple of 4");
  RS_CHECK_ARG(reinterpret_cast<uintptr_t>(qtable) % 4 == 0, "qtable must be 4-byte aligned");
  return RS_OK;
}

// quantise: 16-byte pieces when every row starts 16-byte aligned
bool q8_wide(const void* qtable, int64_t q_ld) {
  return reinterpret_cast<uintptr_t>(qtable) % 16 == 0 && q_ld % 16 == 0;
}

bool out_vec4(const float* out, int64_t out_ld) {
  return reinterpret_cast<uintptr_t>(out) % 16 == 0 && out_ld % 4 == 0;
}

// the gather and the dequantise (ids == nullptr: row p of the output is row p of the table)
int32_t q8_lookup(const uint8_t* qtable, int64_t n_rows, int32_t dim, int64_t q_ld,
                  const void* ids, int32_t id_dtype, int64_t n_ids, const int64_t* slot_offsets,
                  int32_t n_slots, float* out, int64_t out_ld, int32_t* err_flag,
                  hipStream_t st) {
  const bool o4 = out_vec4(out, out_ld);
  const LaneGroup g = lane_group(((int64_t)dim + 3) / 4);
  const int gpb = 256 >> g.lpr_log2;
  const int blocks = (int)std::min<int64_t>(ceil_div(n_ids, gpb * 4), 256 * 16);
#define RS_Q8_LOOKUP(O4, T, IDENT)                                                              \
  q8_lookup_kernel<4, O4, T, IDENT><<<blocks, 256, 0, st>>>(                                    \
      qtable, n_rows, dim, q_ld, static_cast<const T*>(ids), n_ids, slot_offsets, n_slots, out, \
      out_ld, err_flag, g.lpr_log2, g.chunks)
#define RS_Q8_LOOKUP_IDS(O4)                                            \
  do {                                                                  \
    if (!ids) RS_Q8_LOOKUP(O4, int32_t, true);                          \
    else if (id_dtype == RS_ID_I64) RS_Q8_LOOKUP(O4, int64_t, false);   \
    else RS_Q8_LOOKUP(O4, int32_t, false);                              \
  } while (0)
  if (o4) RS_Q8_LOOKUP_IDS(true);
  else RS_Q8_LOOKUP_IDS(false);
#undef RS_Q8_LOOKUP_IDS
#undef RS_Q8_LOOKUP
  RS_CHECK_LAUNCH();
  return RS_OK;
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" size_t rs_q8_row_bytes(int32_t dim) {
  return dim > 0 ? align_up(8 + (size_t)dim, 16) : 0;
}

extern "C" int32_t rs_quantize_rows_q8(const float* table, int64_t ld, int64_t n_rows, int32_t dim,
                                       uint8_t* qtable, int64_t q_ld, int32_t* err_flag,
                                       void* stream) {
  if (int32_t st = check_q8(qtable, dim, q_ld)) return st;
  RS_CHECK_ARG(ld >= dim, "ld must be >= dim");
  RS_CHECK_ARG(n_rows >= 0, "n_rows must be >= 0");
  if (n_rows == 0) return RS_OK;
  RS_CHECK_ARG(table && qtable, "null pointer");
  const bool wide = q8_wide(qtable, q_ld);
  const LaneGroup g = lane_group(q_ld / (wide ? 16 : 4));
  const int gpb = 256 >> g.lpr_log2;
  const int blocks = (int)std::min<int64_t>(ceil_div(n_rows, gpb), 256 * 64);
  hipStream_t st = as_stream(stream);
  if (wide)
    q8_quantize_kernel<16><<<blocks, 256, 0, st>>>(table, ld, n_rows, dim, qtable, q_ld, err_flag,
                                                   g.lpr_log2, g.chunks);
  else
    q8_quantize_kernel<4><<<blocks, 256, 0, st>>>(table, ld, n_rows, dim, qtable, q_ld, err_flag,
                                                  g.lpr_log2, g.chunks);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

extern "C" int32_t rs_dequantize_rows_q8(const uint8_t* qtable, int64_t n_rows, int32_t dim,
                                         int64_t q_ld, float* out, int64_t out_ld, void* stream) {
  if (int32_t st = check_q8(qtable, dim, q_ld)) return st;
  RS_CHECK_ARG(out_ld >= dim, "out_ld must be >= dim");
  RS_CHECK_ARG(n_rows >= 0, "n_rows must be >= 0");
  if (n_rows == 0) return RS_OK;
  RS_CHECK_ARG(qtable && out, "null pointer");
  return q8_lookup(qtable, n_rows, dim, q_ld, nullptr, RS_ID_I32, n_rows, nullptr, 1, out, out_ld,
                   nullptr, as_stream(stream));
}

extern "C" int32_t rs_embedding_q8_fwd(const uint8_t* qtable, int64_t n_rows, int32_t dim,
                                       int64_t q_ld, const void* ids, int32_t id_dtype,
                                       int64_t n_ids, const int64_t* slot_offsets, int32_t n_slots,
                                       float* out, int64_t out_ld, int32_t* err_flag,
                                       void* stream) {
  if (int32_t st = check_q8(qtable, dim, q_ld)) return st;
  RS_CHECK_ARG(out_ld >= dim, "out_ld must be >= dim");
  RS_CHECK_ARG(n_ids >= 0, "n_ids must be >= 0");
  RS_CHECK_ARG(n_slots >= 1, "n_slots must be >= 1");
  RS_CHECK_ARG(id_dtype == RS_ID_I32 || id_dtype == RS_ID_I64, "bad id dtype");
  RS_CHECK_ARG(n_ids == 0 || (qtable && ids && out), "null pointer");
  if (n_ids == 0) return RS_OK;
  // row 0 is what an out-of-range id reads (and discards): it has to exist
  RS_CHECK_ARG(n_rows > 0, "n_rows must be > 0");
  return q8_lookup(qtable, n_rows, dim, q_ld, ids, id_dtype, n_ids, slot_offsets, n_slots, out,
                   out_ld, err_flag, as_stream(stream));
}

extern "C" int32_t rs_embedding_bag_q8_fwd(const uint8_t* qtable, int64_t q_ld, int64_t n_rows,
                                           int32_t dim, const void* ids, int32_t id_dtype,
                                           int64_t n_ids, const int64_t* offsets, int64_t n_bags,
                                           int32_t bag_len, const uint8_t* valid,
                                           const float* per_sample_weights, int32_t mode,
                                           const int64_t* slot_offsets, int32_t n_slots, float* out,
                                           int64_t out_ld, float* bag_scale, int32_t* err_flag,
                                           void* stream) {
  if (int32_t st = check_q8(qtable, dim, q_ld)) return st;
  RS_CHECK_ARG(n_rows > 0, "n_rows must be > 0");
  RS_CHECK_ARG(out_ld >= dim, "out_ld must be >= dim");
  RS_CHECK_ARG(n_slots >= 1, "n_slots must be >= 1");
  RS_CHECK_ARG(id_dtype == RS_ID_I32 || id_dtype == RS_ID_I64, "bad id dtype");
  RS_CHECK_ARG(mode == RS_BAG_SUM || mode == RS_BAG_MEAN, "mode must be RS_BAG_SUM or RS_BAG_MEAN");
  RS_CHECK_ARG(!(per_sample_weights && mode == RS_BAG_MEAN),
               "per_sample_weights go with RS_BAG_SUM only");
  RS_CHECK_ARG(n_ids >= 0 && n_bags >= 0, "n_ids and n_bags must be >= 0");
  if (!offsets) {
    RS_CHECK_ARG(bag_len >= 0, "bag_len must be >= 0");
    RS_CHECK_ARG(n_ids == n_bags * (int64_t)bag_len,
                 "without offsets n_ids (%lld) must be n_bags * bag_len (%lld * %d)",
                 (long long)n_ids, (long long)n_bags, bag_len);
  }
  if (n_bags == 0) return RS_OK;
  RS_CHECK_ARG(qtable && out && (n_ids == 0 || ids), "null pointer");
  const bool o4 = out_vec4(out, out_ld);
  // 8-byte pieces when every row's codes start 8-byte aligned
  const int pw = (reinterpret_cast<uintptr_t>(qtable) | (uintptr_t)q_ld) % 8 == 0 ? 8 : 4;
  const LaneGroup g = lane_group(((int64_t)dim + pw - 1) / pw);
  const int gpb = 256 >> g.lpr_log2;
  const int blocks = (int)std::min<int64_t>(ceil_div(n_bags, gpb), 256 * 64);
  hipStream_t st = as_stream(stream);
#define RS_Q8_BAG(PW, O4, T)                                                                    \
  q8_bag_kernel<PW, O4, T><<<blocks, 256, 0, st>>>(                                             \
      qtable, q_ld, n_rows, dim, static_cast<const T*>(ids), n_ids, offsets, n_bags, bag_len,   \
      valid, per_sample_weights, mode, slot_offsets, n_slots, out, out_ld, bag_scale, err_flag, \
      g.lpr_log2, g.chunks)
#define RS_Q8_BAG_IDS(PW, O4)                                    \
  do {                                                           \
    if (id_dtype == RS_ID_I64) RS_Q8_BAG(PW, O4, int64_t);       \
    else RS_Q8_BAG(PW, O4, int32_t);                             \
  } while (0)
  switch (pw * 2 + o4) {
    case 17: RS_Q8_BAG_IDS(8, true); break;
    case 16: RS_Q8_BAG_IDS(8, false); break;
    case 9: RS_Q8_BAG_IDS(4, true); break;
    default: RS_Q8_BAG_IDS(4, false); break;
  }
#undef RS_Q8_BAG_IDS
#undef RS_Q8_BAG
  RS_CHECK_LAUNCH();
  return RS_OK;
}
