// topk_select.hpp — the selection machinery the top-k retrieval kernels share (topk_ip.hip: the
// fp32 scan and its IVF form; topk_i8.hip: the int8 candidate scan and the exact re-rank): the
// block shape, the total order as one integer, the wave-wide sorts and merges, the compaction of
// a query's LDS candidate list with the exclusion walk, the merge of the per-range lists, the
// padding kernel and the choice of item ranges with its workspace.
//
// Order: (rank desc, item asc) with rank = the score, NaN ranking as -inf; a total order over
// distinct items, so the result does not depend on the order candidates arrive in.
//
// Everything sits in an anonymous namespace: each file that includes this gets its own copy of
// the kernels, as it would of any helper.
#pragma once
#include <climits>

#include "common.hpp"

namespace rs {
namespace {

constexpr int kTileQ = 32;                  // queries per block (MFMA rows)
constexpr int kTileI = 32;                  // items per wave tile (MFMA columns)
constexpr int kIpWaves = 4;
constexpr int kIpThreads = kIpWaves * kWave;
constexpr int kRound = kIpWaves * kTileI;   // most appends to one query's list per round
constexpr int kKMax = 64;
constexpr int kCap = kKMax + kRound;        // candidate slots per query
constexpr int kDimMax = 256;
constexpr int kAutoSplitMax = 64;

__device__ __forceinline__ float rank_of(float s) { return s != s ? -INFINITY : s; }

// The total order as one integer: a larger key is a better pair. High word: the rank (NaN as
// -inf, -0 as +0) mapped so that unsigned order is float order; low word: ~item, so the smaller
// item wins a tie (items are >= 0; the padding item INT_MAX maps lowest). One 64-bit compare
// and no branch per exchange of the sorts.
__device__ __forceinline__ uint64_t order_key(float s, int32_t ix) {
  const uint32_t b = __float_as_uint(rank_of(s) + 0.f);
  const uint32_t u = b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
  return ((uint64_t)u << 32) | (uint32_t)~ix;
}

__device__ __forceinline__ bool better(float a, int32_t ia, float b, int32_t ib) {
  return order_key(a, ia) > order_key(b, ib);
}

// N independent bitonic sorts of one (score, item) per lane across the wave, best first; the N
// lists advance step by step together, so their cross-lane exchanges overlap
template <int N>
__device__ __forceinline__ void wave_sort(float (&v)[N], int32_t (&ix)[N], int lane) {
#pragma unroll
  for (int k = 2; k <= kWave; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const bool keep_better = ((lane & k) == 0) == ((lane & j) == 0);
#pragma unroll
      for (int c = 0; c < N; ++c) {
        const float ov = __shfl_xor(v[c], j, kWave);
        const int32_t oi = __shfl_xor(ix[c], j, kWave);
        const uint64_t mine = order_key(v[c], ix[c]), theirs = order_key(ov, oi);
        const bool take = keep_better ? theirs > mine : mine > theirs;
        v[c] = take ? ov : v[c];
        ix[c] = take ? oi : ix[c];
      }
    }
  }
}

// (v, ix) and (bv, bi) both sorted best first across the wave → (v, ix) = the best 64 of the
// 128, sorted: lane l keeps the better of a[l] and b[63 - l] (a bitonic sequence holding the
// best 64), then one bitonic merge.
__device__ __forceinline__ void wave_merge_top(float& v, int32_t& ix, float bv, int32_t bi,
                                               int lane) {
  const float rv = __shfl(bv, kWave - 1 - lane, kWave);
  const int32_t ri = __shfl(bi, kWave - 1 - lane, kWave);
  const bool first = order_key(rv, ri) > order_key(v, ix);
  v = first ? rv : v;
  ix = first ? ri : ix;
#pragma unroll
  for (int j = kWave >> 1; j > 0; j >>= 1) {
    const float ov = __shfl_xor(v, j, kWave);
    const int32_t oi = __shfl_xor(ix, j, kWave);
    const uint64_t mine = order_key(v, ix), theirs = order_key(ov, oi);
    const bool take = (lane & j) == 0 ? theirs > mine : mine > theirs;
    v = take ? ov : v;
    ix = take ? oi : ix;
  }
}

// One wave reduces query row q's candidate list to its best k non-excluded entries (sorted, at
// slots [0, k)), sets its count and, once k are known, its threshold. out_i != nullptr: also
// writes the k entries (best first) to out_i / out_s (out_s may be NULL); `final` turns the
// padding (INT_MAX, -inf) into (-1, -inf).
__device__ __forceinline__ void compact_query(int q, int lane, int32_t k, float* cand_s,
                                              int32_t* cand_i, int32_t* cnt, float* th_s,
                                              int32_t* th_i, const int64_t* excl_indptr,
                                              const int32_t* excl_items, int64_t excl_row,
                                              int32_t* out_i, float* out_s, bool final) {
  float* cs = cand_s + q * kCap;
  int32_t* ci = cand_i + q * kCap;
  const int32_t n = min(__builtin_amdgcn_readfirstlane(cnt[q]), kCap);
  constexpr int NC = kCap / kWave;
  float v[NC];
  int32_t ix[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int idx = c * kWave + lane;
    v[c] = idx < n ? cs[idx] : -INFINITY;
    ix[c] = idx < n ? ci[idx] : INT_MAX;
  }
  if (excl_indptr && n > 0) {
    const int64_t lo = excl_indptr[excl_row], hi = excl_indptr[excl_row + 1];
    const int32_t* row = excl_items + lo;
    const int64_t len64 = hi > lo ? hi - lo : 0;
    const int32_t len =
        __builtin_amdgcn_readfirstlane(len64 < INT_MAX ? (int32_t)len64 : INT_MAX);
    bool hit[NC] = {};
    for (int32_t e = 0; e < len; e += kWave) {
      const int32_t x = e + lane < len ? row[e + lane] : -1;  // -1 matches no candidate
      const int32_t m = min(kWave, len - e);
      for (int32_t t = 0; t < m; ++t) {
        const int32_t y = __builtin_amdgcn_readlane(x, t);
#pragma unroll
        for (int c = 0; c < NC; ++c) hit[c] |= ix[c] == y;
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (hit[c]) {
        v[c] = -INFINITY;
        ix[c] = INT_MAX;
      }
  }
  wave_sort<NC>(v, ix, lane);
#pragma unroll
  for (int c = 1; c < NC; ++c)
    if (n > c * kWave) wave_merge_top(v[0], ix[0], v[c], ix[c], lane);
  const bool keep = lane < k && ix[0] != INT_MAX;  // the padding sorts last: a prefix
  const int32_t nk = __popcll(__ballot(keep));
  const float kv = __shfl(v[0], k - 1, kWave);
  const int32_t ki = __shfl(ix[0], k - 1, kWave);
  __builtin_amdgcn_wave_barrier();  // every lane's reads of the list are done
  if (lane < k) {
    cs[lane] = v[0];
    ci[lane] = ix[0];
  }
  if (lane == 0) {
    cnt[q] = nk;
    if (nk >= k) {
      th_s[q] = kv;
      th_i[q] = ki;
    }
  }
  if (out_i && lane < k) {
    const bool pad = ix[0] == INT_MAX;
    out_i[lane] = pad && final ? -1 : ix[0];
    if (out_s) out_s[lane] = pad ? -INFINITY : v[0];
  }
}

// one wave per query: its nprobe groups of n_splits sorted lists of k → the best k. probes ==
// NULL (rs_topk_ip, rs_topk_ip_i8): one group. Otherwise group p exists when probes[r, p] names
// a list; the slots of the others were written by no block and are not read.
__global__ __launch_bounds__(kIpThreads) void topk_ip_merge_kernel(
    const int32_t* __restrict__ ws_items, const float* __restrict__ ws_scores, int32_t n_queries,
    const int32_t* __restrict__ probes, int32_t nprobe, int64_t n_lists, int32_t n_splits,
    int32_t k, int32_t* __restrict__ out_items, float* __restrict__ out_scores) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kIpWaves + (threadIdx.x >> 6);
  if (r >= n_queries) return;
  float v = -INFINITY;
  int32_t ix = INT_MAX;
  for (int32_t p = 0; p < nprobe; ++p) {
    if (probes) {
      const int32_t l = probes[r * nprobe + p];
      if (l < 0 || l >= n_lists) continue;
    }
    for (int32_t sp = 0; sp < n_splits; ++sp) {
      const int64_t o = ((r * nprobe + p) * n_splits + sp) * k + lane;
      const float bv = lane < k ? ws_scores[o] : -INFINITY;
      const int32_t bi = lane < k ? ws_items[o] : INT_MAX;
      wave_merge_top(v, ix, bv, bi, lane);
    }
  }
  if (lane < k) {
    const bool pad = ix == INT_MAX;
    out_items[r * k + lane] = pad ? -1 : ix;
    if (out_scores) out_scores[r * k + lane] = pad ? -INFINITY : v;
  }
}

__global__ __launch_bounds__(256) void topk_ip_pad_kernel(int64_t n, int32_t* __restrict__ items,
                                                          float* __restrict__ scores) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  items[i] = -1;
  if (scores) scores[i] = -INFINITY;
}

// the item ranges of a call: the forced count, or enough blocks for two per CU with ranges of
// at least 1024 items
int64_t pick_splits(int32_t n_queries, int64_t n_items, int32_t n_splits) {
  if (n_splits > 0) return n_splits;
  if (n_queries <= 0 || n_items <= 0) return 1;
  const int64_t q_tiles = ceil_div(n_queries, kTileQ);
  int64_t s = ceil_div(2 * (int64_t)device_cus(), q_tiles);
  s = s < n_items / 1024 ? s : n_items / 1024;
  s = s < kAutoSplitMax ? s : kAutoSplitMax;
  return s < 1 ? 1 : s;
}

size_t ws_bytes_for(int32_t n_queries, int64_t splits, int32_t k) {
  if (splits <= 1 || n_queries <= 0) return 0;
  return 2 * align_up((size_t)n_queries * (size_t)splits * (size_t)k * 4, 256);
}

}  // namespace
}  // namespace rs
