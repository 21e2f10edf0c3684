// dlrm_score.hip — DLRM scoring for serving (include/recsys_hip.h a-4, rs_dlrm_score and
// rs_dlrm_score_q8): ids in, one prediction per example out. The lookup, the concat with the
// bottom MLP's row, the strict-upper pairs of X·Xᵀ and the composed top MLP (ctr/model.py:49-57)
// run in the wave that holds the example, and nothing but y[b] is stored: the [B, F(F-1)/2 + D]
// interaction row of rs_dlrm_interaction_fwd_head never reaches HBM.
//
// One kernel, templated on D (128, 64) and on the row source:
//   kF32      fp32 table rows, 16-byte loads (the loads of inter_fwd_mfma);
//   kQ8Word   RS_Q8 rows, the lane's four codes of MFMA step t as one 4-byte load at byte
//             8 + 4g + 16t: D / 16 loads per row, serves every legal (base, q_ld);
//   kQ8Wide   RS_Q8 rows, the row's codes as 16-byte loads (lane g takes the D / 4 bytes from
//             byte 8 + g·D/4), then a 4x4 word transposition among the four lanes that share a
//             row (lanes r, r + 16, r + 32, r + 48) on v_permlane32_swap / v_permlane16_swap:
//             D / 64 loads per row; needs the base and q_ld to be multiples of 8.
// The two RS_Q8 forms hand the same words to the same lanes, so they give the same bits.
//
// Arithmetic: exactly inter_fwd_mfma<D, GatherSrc, true, true>'s (interaction.hip). Lane (r, g)
// (r = lane % 16, g = lane / 16) feeds columns 4g + 16t + c of rows r and 16 + r to step (t, c)
// of three v_mfma_f32_16x16x4_f32 chains; the pairs go through LDS, each to its compact position,
// to the lane that owns position o = lane + 64t; the head is a rounded multiply and a rounded add per
// term (that kernel's ISA has v_mul_f32 + v_add_f32 there, never an fma; here it is written with
// __fmul_rn / __fadd_rn so it does not depend on the compiler's contraction), pairs first, then
// the dense part, then the xor butterfly from 32 down to 1, then + c, then the activation.
// An RS_Q8 element is q8_value(): __fadd_rn(__fmul_rn((float)code, scale), bias).
//
// Shape: one wave per example, four per block, every global load of the example issued before
// anything is consumed. Lanes whose row is absent (an out-of-range id, a row past F) read
// the example's dense row (fp32) or row 0 (RS_Q8, as do the dense row's lanes) and discard it,
// so no table load sits behind a branch; with an RS_Q8 table the dense row's four lanes read it
// as fp32 besides. Plain vector stores only; no atomics
// except the error flag's OR.
#include "dlrm_shared.hpp"

namespace rs {
namespace {

enum RowSrc { kF32 = 0, kQ8Word = 1, kQ8Wide = 2 };

struct ScoreArgs {
  const float* table;     // kF32
  const uint8_t* qtable;  // kQ8*
  int64_t q_ld;
  int64_t n_rows;
  const void* ids;
  int32_t id_dtype;
  int32_t n_slots;
  const int64_t* slot_offsets;
  const float* dense;  // [batch, D]
  const float* q;      // [F(F-1)/2 + D]
  const float* c;      // [1]
  float* y;            // [batch]
  int32_t act;
  int32_t* err_flag;
};

// lanes r, r + 16, r + 32, r + 48 hold a 4x4 word matrix [lane / 16][register]: transpose it
// (the 2x2 blocks across the wave's halves, then each block across its 16-lane rows)
__device__ __forceinline__ void transpose4(uint32_t (&v)[4]) {
  auto s = __builtin_amdgcn_permlane32_swap(v[0], v[2], false, false);
  v[0] = s[0]; v[2] = s[1];
  s = __builtin_amdgcn_permlane32_swap(v[1], v[3], false, false);
  v[1] = s[0]; v[3] = s[1];
  s = __builtin_amdgcn_permlane16_swap(v[0], v[1], false, false);
  v[0] = s[0]; v[1] = s[1];
  s = __builtin_amdgcn_permlane16_swap(v[2], v[3], false, false);
  v[2] = s[0]; v[3] = s[1];
}

// the D / 16 words of one RS_Q8 row that lane (r, g) feeds to the MFMA steps: w[t] = the four
// codes at byte 8 + 4g + 16t. WIDE: two (D = 128) or one (D = 64) 16-byte loads, 8-byte aligned.
template <int D, bool WIDE>
struct Q8Row {
  static constexpr int NT = D / 16;
  static constexpr int NV = D / 64;  // 16-byte loads per lane
  uint32_t raw[NT];
  float scale, bias;
  __device__ __forceinline__ void load(const uint8_t* row, int g) {
    if constexpr (WIDE) {
      const float2 h = *reinterpret_cast<const float2*>(row);
      scale = h.x; bias = h.y;
      const uint8_t* p =
          static_cast<const uint8_t*>(__builtin_assume_aligned(row + 8 + g * (D / 4), 8));
#pragma unroll
      for (int j = 0; j < NV; ++j) __builtin_memcpy(&raw[4 * j], p + 16 * j, 16);
    } else {
      scale = *reinterpret_cast<const float*>(row);
      bias = *reinterpret_cast<const float*>(row + 4);
#pragma unroll
      for (int t = 0; t < NT; ++t)
        raw[t] = *reinterpret_cast<const uint32_t*>(row + 8 + 4 * g + 16 * t);
    }
  }
  // after every load of the example is out: w[t] as the MFMA order wants it
  __device__ __forceinline__ void words(uint32_t (&w)[NT]) {
    if constexpr (WIDE) {
      // raw[4j + i] is word i of piece t = NV·g + j; after the transposition register gs of
      // group j holds lane gs's word (this lane's g) of piece NV·gs + j
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        uint32_t v[4] = {raw[4 * j], raw[4 * j + 1], raw[4 * j + 2], raw[4 * j + 3]};
        transpose4(v);
#pragma unroll
        for (int gs = 0; gs < 4; ++gs) w[NV * gs + j] = v[gs];
      }
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t) w[t] = raw[t];
    }
  }
};

// k ? x : y by component (a ternary over two float4 objects becomes a select of their addresses,
// which puts both in scratch)
__device__ __forceinline__ float4 sel4(bool k, const float4& x, const float4& y) {
  return make_float4(k ? x.x : y.x, k ? x.y : y.y, k ? x.z : y.z, k ? x.w : y.w);
}

template <int D, int SRC>
__global__ __launch_bounds__(256) void dlrm_score_kernel(ScoreArgs a, int64_t batch, int F) {
  constexpr int NT = D / 16;
  __shared__ float zl[4][512];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= batch) return;
  const int r = lane & 15, g = lane >> 4;
  const int S = a.n_slots;
  const int nzc = F * (F - 1) / 2;
  // this lane's q entries (pair o = lane + 64t, dense d = lane + 64t) and dense entries, ahead
  // of the gathers so their latency hides behind the row loads
  constexpr int kHz = 8, kHd = (D + 63) / 64;
  float qz[kHz], qd[kHd], dnv[kHd];
  const float* dn = a.dense + b * D;
#pragma unroll
  for (int t = 0; t < kHz; ++t) qz[t] = lane + 64 * t < nzc ? a.q[lane + 64 * t] : 0.f;
#pragma unroll
  for (int t = 0; t < kHd; ++t) {
    const bool in = lane + 64 * t < D;
    qd[t] = in ? a.q[nzc + lane + 64 * t] : 0.f;
    dnv[t] = in ? dn[lane + 64 * t] : 0.f;
  }
  const float cc = a.c[0];
  // lane k < S resolves row k once; the MFMA lanes fetch the row by shuffle (-1: no table row)
  // (global_row's rule; the slot of position b·S + lane is the lane, so no division)
  long long mine = -1;
  bool oob = false;
  if (lane < S) {
    const int64_t id = load_id(a.ids, a.id_dtype, b * S + lane);
    int64_t lo = 0, card = a.n_rows;
    if (a.slot_offsets) {
      lo = a.slot_offsets[lane];
      card = a.slot_offsets[lane + 1] - lo;
    }
    oob = id < 0 || id >= card;
    mine = oob ? -1 : lo + id;
  }
  const long long r0 = __shfl(mine, r), r1 = __shfl(mine, 16 + r);
  const bool t0 = r0 >= 0, t1 = r1 >= 0;  // a live table row
  const bool d0 = r == S, d1 = 16 + r == S;  // the dense row
  float4 a0[NT], a1[NT];
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (SRC == kF32) {
    // unguarded loads: a lane without a row reads the example's dense row and discards it
    const float* p0 = t0 ? a.table + r0 * D : dn;
    const float* p1 = t1 ? a.table + r1 * D : dn;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = g * 4 + 16 * t;
      a0[t] = *reinterpret_cast<const float4*>(p0 + col);
      a1[t] = *reinterpret_cast<const float4*>(p1 + col);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (!(t0 || d0)) a0[t] = zero4;
      if (!(t1 || d1)) a1[t] = zero4;
    }
  } else {
    Q8Row<D, SRC == kQ8Wide> h0, h1;
    h0.load(a.qtable + (t0 ? r0 : 0) * a.q_ld, g);
    h1.load(a.qtable + (t1 ? r1 : 0) * a.q_ld, g);
    float4 dv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) dv[t] = zero4;
    if (d0 || d1) {
#pragma unroll
      for (int t = 0; t < NT; ++t) dv[t] = *reinterpret_cast<const float4*>(dn + g * 4 + 16 * t);
    }
    uint32_t w0[NT], w1[NT];
    h0.words(w0);
    h1.words(w1);
    // a lane without a table row dequantises with scale = bias = 0: code·0 + 0 is +0 exactly
    const float s0 = t0 ? h0.scale : 0.f, b0 = t0 ? h0.bias : 0.f;
    const float s1 = t1 ? h1.scale : 0.f, b1 = t1 ? h1.bias : 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      a0[t] = make_float4(q8_value(w0[t], 0, s0, b0), q8_value(w0[t], 1, s0, b0),
                          q8_value(w0[t], 2, s0, b0), q8_value(w0[t], 3, s0, b0));
      a1[t] = make_float4(q8_value(w1[t], 0, s1, b1), q8_value(w1[t], 1, s1, b1),
                          q8_value(w1[t], 2, s1, b1), q8_value(w1[t], 3, s1, b1));
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      a0[t] = sel4(d0, dv[t], a0[t]);
      a1[t] = sel4(d1, dv[t], a1[t]);
    }
  }
  f4 c00 = {0.f, 0.f, 0.f, 0.f}, c01 = c00, c11 = c00;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float x0[4] = {a0[t].x, a0[t].y, a0[t].z, a0[t].w};
    const float x1[4] = {a1[t].x, a1[t].y, a1[t].z, a1[t].w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[c], x0[c], c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[c], x1[c], c01, 0, 0, 0);
      c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[c], x1[c], c11, 0, 0, 0);
    }
  }
  // C layout: lane holds G[4g + reg][r] of each block. The lane that holds pair (i, j), i < j < F,
  // knows its compact position (compact_index) and writes it there, so the lane that owns
  // position o = lane + 64t reads z[o]: no inverse of the pair order (compact_pair's square root
  // and loops cost the wave more issue slots than its MFMA chain). Every position below nzc is
  // written exactly once; nzc <= 496.
  float* z = zl[wave];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int i = 4 * g + reg;
    if (i < r && r < F) z[compact_index(i, r, F, 0)] = c00[reg];
    if (16 + r < F) z[compact_index(i, 16 + r, F, 0)] = c01[reg];
    if (i < r && 16 + r < F) z[compact_index(16 + i, 16 + r, F, 0)] = c11[reg];
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  float hacc = 0.f;  // this lane's share of row·q (F <= 32: nzc <= 496 < 64·kHz)
#pragma unroll
  for (int t = 0; t < kHz; ++t) {
    const int o = lane + 64 * t;
    if (o < nzc) hacc = __fadd_rn(hacc, __fmul_rn(z[o], qz[t]));
  }
#pragma unroll
  for (int t = 0; t < kHd; ++t)
    if (lane + 64 * t < D) hacc = __fadd_rn(hacc, __fmul_rn(dnv[t], qd[t]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) hacc = __fadd_rn(hacc, __shfl_xor(hacc, off));
  if (lane == 0) {
    const float v = __fadd_rn(hacc, cc);
    a.y[b] = a.act == 2 ? 1.f / (1.f + expf(-v)) : (a.act == 1 ? fmaxf(v, 0.f) : v);
  }
  if (__any(oob) && lane == 0) flag_oob(a.err_flag);
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what both entry points check after their table; RS_OK with batch == 0 means "nothing to do"
int32_t check_score(const void* table, int64_t n_rows, int32_t D, const void* ids,
                    int32_t id_dtype, int32_t n_slots, const float* dense, int64_t batch,
                    const float* q, const float* c, int32_t act, const float* y) {
  RS_CHECK_ARG(batch >= 0, "batch must be >= 0");
  RS_CHECK_ARG(n_slots >= 1, "n_slots must be >= 1");
  RS_CHECK_ARG(n_slots + 1 <= 32, "at most 31 slots (F = n_slots + 1 <= 32)");
  RS_CHECK_ARG(id_dtype == RS_ID_I32 || id_dtype == RS_ID_I64, "bad id dtype");
  RS_CHECK_ARG(act >= 0 && act <= 2, "bad activation");
  RS_CHECK_ARG(batch == 0 || (table && ids && dense && q && c && y), "null pointer");
  RS_CHECK_ARG(al16(dense), "dense must be 16-byte aligned");
  // row 0 is what an absent RS_Q8 row reads (and discards): it has to exist
  RS_CHECK_ARG(batch == 0 || n_rows > 0, "n_rows must be > 0");
  if (D != 128 && D != 64) {
    set_error("dlrm score: D = %d not built (128, 64)", D);
    return RS_E_UNSUPPORTED;
  }
  return RS_OK;
}

template <int SRC>
int32_t launch_score(const ScoreArgs& a, int32_t D, int64_t batch, hipStream_t st) {
  const int F = a.n_slots + 1;
  const unsigned blocks = (unsigned)ceil_div(batch, 4);
  if (D == 128) dlrm_score_kernel<128, SRC><<<blocks, 256, 0, st>>>(a, batch, F);
  else dlrm_score_kernel<64, SRC><<<blocks, 256, 0, st>>>(a, batch, F);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" int32_t rs_dlrm_score(const float* table, int64_t n_rows, int32_t D, const void* ids,
                                 int32_t id_dtype, int32_t n_slots, const int64_t* slot_offsets,
                                 const float* dense, int64_t batch, const float* q, const float* c,
                                 int32_t act, float* y, int32_t* err_flag, void* stream) {
  RS_CHECK_ARG(al16(table), "table must be 16-byte aligned");
  if (int32_t st = check_score(table, n_rows, D, ids, id_dtype, n_slots, dense, batch, q, c, act, y))
    return st;
  if (batch == 0) return RS_OK;
  const ScoreArgs a{table, nullptr, 0, n_rows, ids, id_dtype, n_slots, slot_offsets,
                    dense, q, c, y, act, err_flag};
  return launch_score<kF32>(a, D, batch, as_stream(stream));
}

extern "C" int32_t rs_dlrm_score_q8(const uint8_t* qtable, int64_t q_ld, int64_t n_rows, int32_t D,
                                    const void* ids, int32_t id_dtype, int32_t n_slots,
                                    const int64_t* slot_offsets, const float* dense, int64_t batch,
                                    const float* q, const float* c, int32_t act, float* y,
                                    int32_t* err_flag, void* stream) {
  RS_CHECK_ARG(D > 0 && q_ld >= 8 + (int64_t)D, "q_ld must be >= 8 + D");
  RS_CHECK_ARG(q_ld % 4 == 0, "q_ld must be a multiple of 4");
  RS_CHECK_ARG(reinterpret_cast<uintptr_t>(qtable) % 4 == 0, "qtable must be 4-byte aligned");
  if (int32_t st =
          check_score(qtable, n_rows, D, ids, id_dtype, n_slots, dense, batch, q, c, act, y))
    return st;
  if (batch == 0) return RS_OK;
  const ScoreArgs a{nullptr, qtable, q_ld, n_rows, ids, id_dtype, n_slots, slot_offsets,
                    dense, q, c, y, act, err_flag};
  // 16-byte loads when every row's codes start 8-byte aligned; the same bits either way
  const bool wide = (reinterpret_cast<uintptr_t>(qtable) | (uintptr_t)q_ld) % 8 == 0;
  return wide ? launch_score<kQ8Wide>(a, D, batch, as_stream(stream))
              : launch_score<kQ8Word>(a, D, batch, as_stream(stream));
}
