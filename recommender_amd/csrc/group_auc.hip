// group_auc.hip — exact per-group AUC counts (GAUC, the metric DIN / DIEN are judged by:
// the impression-weighted mean of each user's own Mann-Whitney AUC), include/recsys_hip.h
// rs_group_auc. The one-group case is the exact, ungridded pooled AUC.
//
// Everything is integer: per group the kernel leaves n, #positives and
//   w2 = Σ_{positive a, negative b} 2·[pred_a > pred_b] + [pred_a == pred_b]   (= 2·U),
// so the result does not depend on the order partial sums meet in; the division is the host's.
//
// Passes (all on the caller's stream, no host sync):
//   1. pred → order-preserving uint32 key (-0 → +0, NaN → 0xFFFFFFFF), value = position;
//   2. stable LSD sorts, least significant key first: radix_sort_pairs on the prediction key,
//      then on the group word gathered through the permutation (int64: low word, then high word;
//      the most significant word has its sign bit flipped, so the order is the signed one);
//   3. head flags over (group) and (group, pred) plus the negative flag, three exclusive scans
//      (each keeps its total behind the array, at index n);
//   4. heads scatter their position: run_start[run], group_start[group], group_key, w2 = 0;
//   5. one thread per tie run: with negcum the scanned negative flag,
//        neg_before = negcum[run_start] - negcum[group_start]
//        neg_in     = negcum[run_end] - negcum[run_start],  pos_in = len - neg_in
//        contribution = pos_in · (2·neg_before + neg_in)
//      folded over equal groups across the wave (segmented shuffle scan) and across the block's
//      16 waves (LDS), then one 64-bit integer atomic per (block, group): a single group of 2^22
//      runs issues 4096 atomics, not 2^22. The same kernel's first n_groups threads write
//      group_n / group_pos from the scans at the group boundaries.
#include "common.hpp"

namespace rs {

namespace {

constexpr int64_t kFullKey = 0xFFFFFFFFll;  // radix_sort_pairs: all 32 key bits, four 8-bit passes
constexpr int kRunThreads = 1024, kRunWaves = kRunThreads / kWave;

// float32 → uint32 with the order of the values: -0 is +0, negative values have every bit
// flipped, the others the top bit set; NaN is the largest key
__device__ __forceinline__ uint32_t pred_key(float p, bool& nan) {
  uint32_t b = __float_as_uint(p);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) {
    nan = true;
    return 0xFFFFFFFFu;
  }
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void gauc_pred_key_kernel(const float* __restrict__ pred, int64_t n,
                                                            uint32_t* __restrict__ keys,
                                                            int32_t* __restrict__ pos,
                                                            int32_t* __restrict__ err_flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool nan = false;
  if (i < n) {
    keys[i] = pred_key(pred[i], nan);
    pos[i] = (int32_t)i;
  }
  // one OR per wave that saw a NaN
  if (__any(nan) && (threadIdx.x & 63) == 0 && err_flag) atomicOr(err_flag, RS_ERRBIT_NONFINITE);
}

// the sort key of one 32-bit word of the group id at sorted place j. word 0: an int32 id (sign
// flipped); 1: the low word of an int64 id; 2: its high word (sign flipped)
__global__ __launch_bounds__(256) void gauc_group_word_kernel(const void* __restrict__ group,
                                                              const int32_t* __restrict__ perm,
                                                              int64_t n, int word,
                                                              uint32_t* __restrict__ keys) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t p = perm[j];
  uint32_t k;
  if (word == 0) {
    k = (uint32_t) static_cast<const int32_t*>(group)[p] ^ 0x80000000u;
  } else {
    const uint64_t g = (uint64_t) static_cast<const int64_t*>(group)[p];
    k = word == 1 ? (uint32_t)g : ((uint32_t)(g >> 32) ^ 0x80000000u);
  }
  keys[j] = k;
}

// sg[j] = place j starts a group, sr[j] = it starts a tie run (same group, same prediction key),
// sn[j] = its example is a negative
__global__ __launch_bounds__(256) void gauc_flags_kernel(
    const float* __restrict__ pred, const float* __restrict__ label, const void* __restrict__ group,
    int32_t dtype, const int32_t* __restrict__ perm, int64_t n, int32_t* __restrict__ sg,
    int32_t* __restrict__ sr, int32_t* __restrict__ sn) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t p = perm[j];
  const int32_t q = perm[j > 0 ? j - 1 : 0];
  bool nan = false;
  const int64_t g = group ? load_id(group, dtype, p) : 0, gq = group ? load_id(group, dtype, q) : 0;
  const uint32_t k = pred_key(pred[p], nan), kq = pred_key(pred[q], nan);
  const bool hg = j == 0 || g != gq;
  sg[j] = hg;
  sr[j] = hg || k != kq;
  sn[j] = !(label[p] != 0.f);
}

// after the scans (sg, sr exclusive, totals at [n]): every head writes where it stands
__global__ __launch_bounds__(256) void gauc_heads_kernel(
    const int32_t* __restrict__ sg, const int32_t* __restrict__ sr, const void* __restrict__ group,
    int32_t dtype, const int32_t* __restrict__ perm, int64_t n, int32_t* __restrict__ run_start,
    int32_t* __restrict__ group_start, int64_t* __restrict__ group_key,
    unsigned long long* __restrict__ group_w2) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t r = sr[j], gi = sg[j];
  if (sr[j + 1] != r) run_start[r] = (int32_t)j;
  if (sg[j + 1] != gi) {
    group_start[gi] = (int32_t)j;
    group_key[gi] = group ? load_id(group, dtype, perm[j]) : 0;
    group_w2[gi] = 0ull;
  }
}

__global__ __launch_bounds__(kRunThreads) void gauc_runs_kernel(
    const int32_t* __restrict__ sg, const int32_t* __restrict__ sr, const int32_t* __restrict__ sn,
    int64_t n, const int32_t* __restrict__ run_start, const int32_t* __restrict__ group_start,
    int32_t* __restrict__ group_n, int32_t* __restrict__ group_pos,
    unsigned long long* __restrict__ group_w2, int32_t* __restrict__ n_groups_out) {
  __shared__ int32_t first_g[kRunWaves], tail_g[kRunWaves], whole[kRunWaves];
  __shared__ unsigned long long tail_sum[kRunWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * kRunThreads + threadIdx.x;
  const int32_t n_groups = sg[n], n_runs = sr[n];
  if (t == 0) *n_groups_out = n_groups;
  if (t < n_groups) {
    const int32_t s = group_start[t];
    const int32_t e = t + 1 < n_groups ? group_start[t + 1] : (int32_t)n;
    group_n[t] = e - s;
    group_pos[t] = (e - s) - (sn[e] - sn[s]);
  }
  int32_t gi = -1;  // lanes past the last run: a segment of their own that adds nothing
  unsigned long long x = 0ull;
  if (t < n_runs) {
    const int32_t s = run_start[t];
    const int32_t e = t + 1 < n_runs ? run_start[t + 1] : (int32_t)n;
    gi = sg[s + 1] - 1;
    const int32_t ns = sn[s];
    const uint64_t neg_before = (uint64_t)(ns - sn[group_start[gi]]);
    const uint64_t neg_in = (uint64_t)(sn[e] - ns);
    const uint64_t pos_in = (uint64_t)(e - s) - neg_in;
    x = pos_in * (2ull * neg_before + neg_in);
  }
  // inclusive scan inside each stretch of lanes with one group (the runs are in group order)
  const int32_t g_up = __shfl_up(gi, 1);
  const uint64_t heads = __ballot(lane == 0 || gi != g_up);
  const int seg_start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long y = __shfl_up(x, off);
    if (lane - off >= seg_start) x += y;
  }
  const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  if (lane == 0) first_g[wave] = gi;
  if (lane == 63) {
    tail_g[wave] = gi;
    tail_sum[wave] = x;
    whole[wave] = heads == 1ull;
  }
  __syncthreads();
  if (!tail || gi < 0) return;
  // a stretch that goes on in the next wave is added there
  if (lane == 63 && wave + 1 < kRunWaves && first_g[wave + 1] == gi) return;
  if (seg_start == 0) {
    for (int w = wave - 1; w >= 0 && tail_g[w] == gi; --w) {
      x += tail_sum[w];
      if (!whole[w]) break;
    }
  }
  if (x) atomicAdd(group_w2 + gi, x);
}

struct GaucWs {
  uint32_t *k0, *k1;
  int32_t *v0, *v1, *sg, *sr, *sn;
  char *sort_ws, *scan_ws;
};

GaucWs gauc_ws(Carver& c, int64_t n) {
  GaucWs w;
  w.k0 = c.take<uint32_t>(n);
  w.k1 = c.take<uint32_t>(n);
  w.v0 = c.take<int32_t>(n);
  w.v1 = c.take<int32_t>(n);
  w.sg = c.take<int32_t>(n + 1);
  w.sr = c.take<int32_t>(n + 1);
  w.sn = c.take<int32_t>(n + 1);
  w.sort_ws = c.take<char>(radix_sort_ws_size(n));
  w.scan_ws = c.take<char>(exclusive_scan_ws_size(n));
  return w;
}

}  // namespace

}  // namespace rs

using namespace rs;

extern "C" size_t rs_group_auc_workspace_size(int64_t n) {
  if (n <= 0) return 0;
  Carver c(nullptr, 0);
  gauc_ws(c, n);
  return c.off;
}

extern "C" int32_t rs_group_auc(const float* pred, const float* label, const void* group,
                                int32_t group_dtype, int64_t n, int64_t* group_key,
                                int32_t* group_n, int32_t* group_pos,
                                unsigned long long* group_w2, int32_t* n_groups, int32_t* err_flag,
                                void* workspace, size_t ws_bytes, void* stream) {
  RS_CHECK_ARG(n >= 0 && n <= 0x7FFFFFFFll, "rs_group_auc: n = %lld outside [0, 2^31)", (long long)n);
  RS_CHECK_ARG(!group || group_dtype == RS_ID_I32 || group_dtype == RS_ID_I64,
               "rs_group_auc: group_dtype %d", group_dtype);
  RS_CHECK_ARG(n_groups, "rs_group_auc: null n_groups");
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    RS_CHECK_HIP(hipMemsetAsync(n_groups, 0, sizeof(int32_t), st));
    return RS_OK;
  }
  RS_CHECK_ARG(pred && label && group_key && group_n && group_pos && group_w2 && workspace,
               "rs_group_auc: null pointer");
  Carver c(workspace, ws_bytes);
  const GaucWs w = gauc_ws(c, n);
  if (!c.ok()) {
    set_error("rs_group_auc: workspace too small: need %zu have %zu", c.off, ws_bytes);
    return RS_E_WORKSPACE;
  }
  const size_t sort_bytes = radix_sort_ws_size(n), scan_bytes = exclusive_scan_ws_size(n);
  const unsigned grid = (unsigned)ceil_div(n, 256);
  gauc_pred_key_kernel<<<grid, 256, 0, st>>>(pred, n, w.k0, w.v0, err_flag);
  RS_CHECK_LAUNCH();
  int32_t s = radix_sort_pairs(w.k0, w.v0, w.k1, w.v1, n, kFullKey, w.sort_ws, sort_bytes, st);
  if (s) return s;
  // perm: the positions in (group, pred) order; spare: the other position buffer
  int32_t *perm = w.v1, *spare = w.v0;
  if (group) {
    const int n_words = group_dtype == RS_ID_I64 ? 2 : 1;
    for (int k = 0; k < n_words; ++k) {
      gauc_group_word_kernel<<<grid, 256, 0, st>>>(group, perm, n, n_words == 1 ? 0 : k + 1, w.k0);
      RS_CHECK_LAUNCH();
      s = radix_sort_pairs(w.k0, perm, w.k1, spare, n, kFullKey, w.sort_ws, sort_bytes, st);
      if (s) return s;
      int32_t* t = perm;
      perm = spare;
      spare = t;
    }
  }
  gauc_flags_kernel<<<grid, 256, 0, st>>>(pred, label, group, group_dtype, perm, n, w.sg, w.sr, w.sn);
  RS_CHECK_LAUNCH();
  for (int32_t* a : {w.sg, w.sr, w.sn}) {
    s = exclusive_scan_i32(a, a, n, a + n, w.scan_ws, scan_bytes, st);
    if (s) return s;
  }
  // the key buffers and the spare positions are free now
  int32_t* run_start = reinterpret_cast<int32_t*>(w.k0);
  int32_t* group_start = spare;
  gauc_heads_kernel<<<grid, 256, 0, st>>>(w.sg, w.sr, group, group_dtype, perm, n, run_start,
                                          group_start, group_key, group_w2);
  RS_CHECK_LAUNCH();
  gauc_runs_kernel<<<(unsigned)ceil_div(n, kRunThreads), kRunThreads, 0, st>>>(
      w.sg, w.sr, w.sn, n, run_start, group_start, group_n, group_pos, group_w2, n_groups);
  RS_CHECK_LAUNCH();
  return RS_OK;
}
