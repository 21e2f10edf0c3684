// topk_ip.hip — fused top-k inner-product retrieval over an item catalogue (recsys_hip.h,
// "Top-k inner-product retrieval"): the k best items of every query by q · x, with a per-query
// exclusion set, without the [n_queries, n_items] score matrix.
//
//   topk_ip_kernel   one block = 32 queries × one contiguous item range (a "split"). The query
//                    tile sits in LDS for the block's life. Each of the 4 waves streams 32-item
//                    tiles: the tile's rows go global → registers (prefetched one stage ahead) →
//                    a wave-private LDS stage, 64 columns at a time, and v_mfma_f32_32x32x2_f32
//                    runs the 32 × 32 scores down the columns in ascending order: per (query,
//                    item) one accumulator, one fmaf-equivalent step per column, never split.
//                    A lane then holds 16 queries' scores of one item. A score that beats its
//                    query's threshold (the k-th best (score, item) kept so far; -inf before k
//                    are known) is appended to the query's LDS candidate list with an LDS atomic.
//                    After every round (4 tiles, ≤ 128 appends per query) a list that could
//                    overflow in the next round (count + 128 > 192) is compacted by one wave:
//                    exclusion (the CSR row is walked once, 64 ids per load, against the ≤ 192
//                    candidates in registers), three 64-lane bitonic sorts run side by side, two
//                    top-64 merges; the best k stay and the threshold is refreshed. Overflow
//                    cannot happen, so there is no retry. The exclusion test therefore runs only
//                    on candidates that beat the threshold, a few hundred per query however
//                    large the range. A compaction is a latency-bound chain of cross-lane
//                    exchanges that holds its block at the round's barrier: it, not the scoring,
//                    is what small-dim shapes pay for.
//   topk_ip_merge    n_splits > 1: every block left its k (item, score) pairs in the workspace;
//                    one wave per query merges the n_splits sorted lists by the same order.
//
//
// rs_ivf_topk_ip scans inverted lists with the same kernel (IVF = true): a block's 32 query rows
// are gathered through an index (the block's tile of the probes that name one list), its item
// range is one of list_splits sub-ranges of that list, a candidate is appended under its
// reported id item_ids[j], and the k pairs go to the workspace slot of (query, probe,
// sub-range). The work list is made on the device:
//   rs_sort_ids        the flattened probes, grouped by list (stable; values outside
//                      [0, n_lists) last);
//   ivf_bounds         first sorted position of every list;
//   ivf_tile_counts    ceil(probes of the list / 32), then an exclusive scan (tile bases, total);
//   ivf_work           one entry per tile: (list, first sorted position, queries);
//   topk_ip_kernel     a grid of the host-known bound; blocks past the total return;
//   ivf_merge          one wave per query merges its nprobe · list_splits lists, skipping the
//                      probes that name no list (no block wrote their slots).
//
// The order, the sorts, compact_query, the merge and pad kernels and the choice of item ranges
// are topk_select.hpp's, shared with the int8 candidate scan (topk_i8.hip).
#include "topk_select.hpp"

namespace rs {
namespace {

constexpr int kIvfProbeMax = 64;
constexpr int kIvfSlotsMax = RS_IVF_MAX_SLOTS;  // nprobe * list_splits
constexpr int kIvfAutoSplitMax = 8;

struct TopkIpArgs {
  const float* queries;
  int64_t q_ld;
  int32_t n_queries;
  const float* items;
  int64_t i_ld;
  int32_t n_items;
  int32_t dim;
  int64_t excl_base;
  const int64_t* excl_indptr;
  const int32_t* excl_items;
  const int32_t* excl_one;
  int32_t k;
  int32_t n_splits;
  int32_t q_tiles;
  int32_t* out_items;   // n_splits == 1: the outputs; else the workspace lists
  float* out_scores;    // may be NULL when n_splits == 1
  // IVF only (n_splits = list_splits, q_tiles unused, the outputs are the workspace lists)
  const int4* work;            // (list, first sorted position, queries, -) per tile
  const int32_t* n_work;       // device: tiles in work
  const int32_t* sorted_pos;   // flattened probe position r * nprobe + p, grouped by list
  int64_t n_probes;            // n_queries * nprobe
  int32_t nprobe;
  const int64_t* list_offsets;
  int64_t n_lists;
  const int32_t* item_ids;     // may be NULL: the stored row
};

// W = 4 << LOGW4 columns are staged at a time (the power of two ≥ dim, at most 64).
template <int LOGW4, bool FAST, bool IVF>
__global__ __launch_bounds__(kIpThreads) void topk_ip_kernel(const TopkIpArgs a) {
  constexpr int W = 4 << LOGW4;
  constexpr int W4 = 1 << LOGW4;  // float4 slots per staged row
  constexpr int SS = W + 1;       // odd row strides: the 32 rows of a column fall in 32 banks
  constexpr int NSLOT = (kTileI * W4 + kWave - 1) / kWave;
  extern __shared__ __align__(16) float lds[];  // every sub-array below starts 128-byte aligned
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int32_t dim = a.dim;
  constexpr int G = W / 2 < 8 ? W / 2 : 8;  // MFMA steps per operand group
  constexpr int GC = 2 * G;                 // = ip_group_cols(W)
  const int dq = (dim + GC - 1) / GC * GC;
  const int QS = dq + 1;
  float* Qs = lds;
  float* st = Qs + kTileQ * QS + wid * (kTileI * SS);
  float* cand_s = Qs + kTileQ * QS + kIpWaves * kTileI * SS;
  int32_t* cand_i = reinterpret_cast<int32_t*>(cand_s + kTileQ * kCap);
  int32_t* cnt = cand_i + kTileQ * kCap;
  float* th_s = reinterpret_cast<float*>(cnt + kTileQ);
  int32_t* th_i = reinterpret_cast<int32_t*>(th_s + kTileQ);
  int32_t* ex1 = th_i + kTileQ;
  int32_t* qix = ex1 + kTileQ;  // IVF: the flattened probe position of every query row

  int32_t sp, q0, nq, lo, hi;
  if constexpr (IVF) {
    // one tile of the work list × one sub-range of its list, clipped to [0, n_items]
    const int32_t w = blockIdx.x / a.n_splits;
    sp = blockIdx.x - w * a.n_splits;
    if (w >= *a.n_work) return;
    const int4 wk = a.work[w];
    const int64_t l = wk.x;
    q0 = 0;
    nq = l >= 0 && l < a.n_lists ? max(0, min(kTileQ, wk.z)) : 0;
    if (tid < kTileQ) {
      const int64_t sp_pos = (int64_t)wk.y + tid;
      int32_t flat = -1;
      if (tid < nq && wk.y >= 0 && sp_pos < a.n_probes) flat = a.sorted_pos[sp_pos];
      qix[tid] = flat >= 0 && flat < a.n_probes ? flat : -1;  // -1: a dead row
    }
    int64_t l0 = 0, l1 = 0;
    if (nq > 0) {
      l0 = a.list_offsets[l];
      l1 = a.list_offsets[l + 1];
    }
    l0 = l0 < 0 ? 0 : (l0 > a.n_items ? a.n_items : l0);
    l1 = l1 < 0 ? 0 : (l1 > a.n_items ? a.n_items : l1);
    const int32_t len = l1 > l0 ? (int32_t)(l1 - l0) : 0;
    const int32_t per = len / a.n_splits;
    lo = (int32_t)l0 + sp * per;
    hi = sp == a.n_splits - 1 ? (int32_t)l0 + len : lo + per;
    __syncthreads();
  } else {
    sp = blockIdx.x / a.q_tiles;
    q0 = (blockIdx.x - sp * a.q_tiles) * kTileQ;
    nq = min(kTileQ, a.n_queries - q0);
    const int32_t per = a.n_items / a.n_splits;
    lo = sp * per;
    hi = sp == a.n_splits - 1 ? a.n_items : lo + per;
  }
  // the query of tile row `row` (IVF: -1 for a dead row)
  auto query_of = [&](int row) -> int32_t {
    if constexpr (IVF) {
      const int32_t flat = qix[row];
      return flat < 0 ? -1 : flat / a.nprobe;
    } else {
      return q0 + row;
    }
  };

  // The pad column of an odd dim holds -0 (the staged items' holds +0): the padded step adds a
  // -0 product, the identity for every acc, a -0 included (which a negative product that
  // underflows leaves; +0 there would turn it into +0).
  for (int e = tid; e < kTileQ * dq; e += kIpThreads) {
    const int row = e / dq, col = e - row * dq;
    const float pad = col < dim ? 0.f : -0.f;
    if constexpr (IVF) {
      const int32_t r = row < nq ? query_of(row) : -1;
      Qs[row * QS + col] = r >= 0 && col < dim ? a.queries[(int64_t)r * a.q_ld + col] : pad;
    } else {
      Qs[row * QS + col] =
          row < nq && col < dim ? a.queries[(int64_t)(q0 + row) * a.q_ld + col] : pad;
    }
  }
  if (tid < kTileQ) {
    cnt[tid] = 0;
    th_i[tid] = INT_MAX;
    if constexpr (IVF) {
      const int32_t r = tid < nq ? query_of(tid) : -1;
      th_s[tid] = r >= 0 ? -INFINITY : INFINITY;  // dead rows take nothing
      ex1[tid] = a.excl_one && r >= 0 ? a.excl_one[r] : -1;
    } else {
      th_s[tid] = tid < nq ? -INFINITY : INFINITY;  // rows past the last query take nothing
      ex1[tid] = a.excl_one && tid < nq ? a.excl_one[q0 + tid] : -1;
    }
  }
  __syncthreads();

  // IVF: a sub-range may be empty (n_tiles == 0: nothing is fetched, the lists stay empty)
  const int32_t n_tiles = hi > lo ? (hi - lo + kTileI - 1) / kTileI : 0;
  const int32_t n_rounds = (n_tiles + kIpWaves - 1) / kIpWaves;
  const int32_t n_chunks = (dim + W - 1) / W;

  // This lane's float4 slots of columns [c0, c0 + W) of the tile at item jb.
  // FAST (items 16-byte aligned, i_ld and dim multiples of 4): unconditional loads and nothing
  // that reads them, so all are in flight together and stay so until stage() (a select or a
  // branch on the way made the compiler wait for each load before issuing the next). A row
  // past the range's end re-reads the last row (its scores are never looked at), a slot past
  // dim the row's last four columns (stage() zeroes it).
  // Otherwise: guarded element loads, zeros past the range's end and past dim.
  float4 pre[NSLOT];
  auto fetch = [&](int64_t jb, int32_t c0) {
#pragma unroll
    for (int t = 0; t < NSLOT; ++t) {
      const int slot = lane + kWave * t;
      const int row = (slot >> LOGW4) & (kTileI - 1), col = c0 + 4 * (slot & (W4 - 1));
      const int64_t j = jb + row;
      if constexpr (FAST) {
        const int64_t jc = j < hi ? j : (int64_t)hi - 1;
        pre[t] = *reinterpret_cast<const float4*>(a.items + jc * a.i_ld + min(col, dim - 4));
      } else {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < hi && col < dim) {
          const float* p = a.items + j * a.i_ld + col;
          x.x = p[0];
          if (col + 1 < dim) x.y = p[1];
          if (col + 2 < dim) x.z = p[2];
          if (col + 3 < dim) x.w = p[3];
        }
        pre[t] = x;
      }
    }
  };
  auto stage = [&](int32_t c0) {
#pragma unroll
    for (int t = 0; t < NSLOT; ++t) {
      const int slot = lane + kWave * t;
      if (slot < kTileI * W4) {
        float* d = st + (slot >> LOGW4) * SS + 4 * (slot & (W4 - 1));
        const bool ok = c0 + 4 * (slot & (W4 - 1)) < dim;
        d[0] = ok ? pre[t].x : 0.f;
        d[1] = ok ? pre[t].y : 0.f;
        d[2] = ok ? pre[t].z : 0.f;
        d[3] = ok ? pre[t].w : 0.f;
      }
    }
  };

  const int mrow = lane & 31, half = lane >> 5;
  if (!IVF || n_tiles > 0) fetch((int64_t)lo + wid * kTileI, 0);
  for (int32_t round = 0; round < n_rounds; ++round) {
    const int64_t jb64 = (int64_t)lo + ((int64_t)round * kIpWaves + wid) * kTileI;
    const bool active = jb64 < hi;
    const int32_t jb = active ? (int32_t)jb64 : hi;
    f32x16 acc = {};
    for (int32_t c = 0; c < n_chunks; ++c) {
      stage(c * W);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      {  // the next stage's rows are in flight while this one multiplies (past the last tile:
         // the range's last row again, or nothing, never used)
        const bool last = c + 1 == n_chunks;
        fetch(last ? jb64 + kRound : jb64, last ? 0 : (c + 1) * W);
      }
      if (active) {
        const int c0 = c * W;
        const float* qa = Qs + mrow * QS + c0 + half;
        const float* xb = st + mrow * SS + half;
        // G steps (GC columns) at a time, the next group's operands read while this one
        // multiplies; the columns past dim hold -0 (queries) and +0 (items): identity steps
        const int groups = (min(W, dim - c0) + GC - 1) / GC;
        float fa[G], fb[G];
#pragma unroll
        for (int s = 0; s < G; ++s) {
          fa[s] = qa[2 * s];
          fb[s] = xb[2 * s];
        }
        for (int g = 0; g < groups; ++g) {
          const int nx = (g + 1 < groups ? g + 1 : g) * GC;  // the last group is read twice
          float na[G], nfb[G];
#pragma unroll
          for (int s = 0; s < G; ++s) {
            na[s] = qa[nx + 2 * s];
            nfb[s] = xb[nx + 2 * s];
          }
#pragma unroll
          for (int s = 0; s < G; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], fb[s], acc, 0, 0, 0);
#pragma unroll
          for (int s = 0; s < G; ++s) {
            fa[s] = na[s];
            fb[s] = nfb[s];
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
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
          const float s = acc[4 * g + u];
          if (s < th[u]) continue;  // nearly every pair; false for a NaN on either side
          if constexpr (IVF) {
            // th_s is +inf for a dead row, so only an +inf or a live row's score gets here
            if (i >= nq || qix[i] < 0) continue;
            const int32_t id = a.item_ids ? a.item_ids[j] : j;  // j < hi <= n_items
            if (better(s, id, th[u], th_i[i]) && id != ex1[i]) {
              const int32_t slot = atomicAdd(&cnt[i], 1);
              if (slot < kCap) {
                cand_s[i * kCap + slot] = s;
                cand_i[i * kCap + slot] = id;
              }
            }
          } else if (i < nq && better(s, j, th[u], th_i[i]) && j != ex1[i]) {
            const int32_t slot = atomicAdd(&cnt[i], 1);
            if (slot < kCap) {  // always: a list enters a round with count + kRound <= kCap
              cand_s[i * kCap + slot] = s;
              cand_i[i * kCap + slot] = j;
            }
          }
        }
      }
    }
    __syncthreads();
    const uint64_t full = __ballot(lane < nq && cnt[lane & (kTileQ - 1)] + kRound > kCap);
    for (int q = wid; q < nq; q += kIpWaves)
      if ((full >> q) & 1)
        compact_query(q, lane, a.k, cand_s, cand_i, cnt, th_s, th_i, a.excl_indptr,
                      a.excl_items, a.excl_base + query_of(q), nullptr, nullptr, false);
    __syncthreads();
  }
  if constexpr (IVF) {
    // the slot of (query, probe, sub-range); a dead row has none
    for (int q = wid; q < nq; q += kIpWaves) {
      const int32_t flat = qix[q];
      if (flat < 0) continue;
      const int64_t o = ((int64_t)flat * a.n_splits + sp) * a.k;
      compact_query(q, lane, a.k, cand_s, cand_i, cnt, th_s, th_i, a.excl_indptr, a.excl_items,
                    a.excl_base + flat / a.nprobe, a.out_items + o, a.out_scores + o, false);
    }
    return;
  }
  const bool final = a.n_splits == 1;
  for (int q = wid; q < nq; q += kIpWaves) {
    const int64_t o = ((int64_t)(q0 + q) * a.n_splits + sp) * a.k;
    compact_query(q, lane, a.k, cand_s, cand_i, cnt, th_s, th_i, a.excl_indptr, a.excl_items,
                  a.excl_base + q0 + q, a.out_items + o, a.out_scores ? a.out_scores + o : nullptr,
                  final);
  }
}

// ---- the IVF work list ----------------------------------------------------------------
// sorted[n] ascending with the sentinel n_lists last → first[l] = the first position whose
// value is >= l, for l in [0, n_lists]: list l's probes are positions [first[l], first[l+1]).
// Position p writes the entries of (sorted[p-1], sorted[p]]; position n those up to n_lists.
__global__ __launch_bounds__(256) void ivf_bounds_kernel(const uint32_t* __restrict__ sorted,
                                                         int64_t n, int64_t n_lists,
                                                         int32_t* __restrict__ first) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n) return;
  const int64_t cur = p < n ? min((int64_t)sorted[p], n_lists) : n_lists;
  const int64_t prev = p > 0 ? min((int64_t)sorted[p - 1], n_lists) : -1;
  for (int64_t l = prev + 1; l <= cur; ++l) first[l] = (int32_t)p;
}

__global__ __launch_bounds__(256) void ivf_tile_counts_kernel(const int32_t* __restrict__ first,
                                                              int64_t n_lists,
                                                              int32_t* __restrict__ tiles) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_lists) return;
  const int32_t c = first[l + 1] - first[l];
  tiles[l] = c > 0 ? (c + kTileQ - 1) / kTileQ : 0;
}

// the position that opens a tile of its list writes the tile's entry
__global__ __launch_bounds__(256) void ivf_work_kernel(const uint32_t* __restrict__ sorted,
                                                       int64_t n, int64_t n_lists,
                                                       const int32_t* __restrict__ first,
                                                       const int32_t* __restrict__ tile_base,
                                                       int64_t work_cap, int4* __restrict__ work) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t l = sorted[p];
  if (l >= n_lists) return;
  const int32_t rel = (int32_t)p - first[l];
  if (rel < 0 || rel % kTileQ) return;
  const int64_t w = (int64_t)tile_base[l] + rel / kTileQ;
  if (w < 0 || w >= work_cap) return;  // never: work_cap bounds the tiles of any probe array
  work[w] = make_int4((int32_t)l, (int32_t)p, min(kTileQ, first[l + 1] - (int32_t)p), 0);
}

int ip_group_cols(int W) { return W < 16 ? W : 16; }

// the five 32-entry arrays: count, threshold score and item, excl_one, and the IVF query index
size_t ip_lds_bytes(int32_t dim, int W) {
  const int gc = ip_group_cols(W);
  const int dq = (dim + gc - 1) / gc * gc;
  return sizeof(float) * ((size_t)kTileQ * (dq + 1) + (size_t)kIpWaves * kTileI * (W + 1) +
                          (size_t)kTileQ * kCap * 2 + (size_t)kTileQ * 5);
}

// grid: q_tiles * n_splits blocks (IVF: the bound on the work list's tiles, times list_splits)
template <int LOGW4, bool FAST, bool IVF>
int32_t launch_topk_ip_as(const TopkIpArgs& a, int64_t grid, hipStream_t st) {
  const size_t lds = ip_lds_bytes(a.dim, 4 << LOGW4);
  if (lds > 48 * 1024)
    RS_CHECK_HIP(hipFuncSetAttribute((const void*)topk_ip_kernel<LOGW4, FAST, IVF>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  topk_ip_kernel<LOGW4, FAST, IVF><<<(unsigned)grid, kIpThreads, lds, st>>>(a);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

template <int LOGW4, bool IVF>
int32_t launch_topk_ip(const TopkIpArgs& a, int64_t grid, hipStream_t st) {
  const bool fast = (a.i_ld & 3) == 0 && (a.dim & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(a.items) & 15) == 0;
  return fast ? launch_topk_ip_as<LOGW4, true, IVF>(a, grid, st)
              : launch_topk_ip_as<LOGW4, false, IVF>(a, grid, st);
}

template <bool IVF>
int32_t launch_topk_ip_dim(const TopkIpArgs& a, int64_t grid, hipStream_t st) {
  if (a.dim <= 4) return launch_topk_ip<0, IVF>(a, grid, st);
  if (a.dim <= 8) return launch_topk_ip<1, IVF>(a, grid, st);
  if (a.dim <= 16) return launch_topk_ip<2, IVF>(a, grid, st);
  if (a.dim <= 32) return launch_topk_ip<3, IVF>(a, grid, st);
  return launch_topk_ip<4, IVF>(a, grid, st);
}

// ---- IVF: sub-ranges per list, grid bound, workspace ---------------------------------
// list_splits = 0: enough blocks for two per CU, sub-ranges of at least 1024 rows of an average
// list, at most kIvfAutoSplitMax and at most what nprobe leaves of kIvfSlotsMax. n_items < 0
// (the workspace query, which does not know it): without the list-length limit, which gives the
// largest value the call could choose.
int64_t ivf_pick_splits(int32_t n_queries, int32_t nprobe, int64_t n_lists, int64_t n_items,
                        int32_t list_splits) {
  if (list_splits > 0) return list_splits;
  int64_t cap = kIvfSlotsMax / (nprobe > 0 ? nprobe : 1);
  cap = cap < kIvfAutoSplitMax ? cap : kIvfAutoSplitMax;
  if (cap < 1) cap = 1;
  if (n_queries <= 0 || n_lists <= 0) return 1;
  const int64_t np = (int64_t)n_queries * nprobe;
  const int64_t tiles = (np < n_lists ? np : n_lists) + np / kTileQ;  // at most; at least np / 32
  int64_t s = ceil_div(2 * (int64_t)device_cus(), tiles > 0 ? tiles : 1);
  const int64_t by_len = n_items < 0 ? cap : n_items / n_lists / 1024;
  s = s < by_len ? s : by_len;
  s = s < cap ? s : cap;
  return s < 1 ? 1 : s;
}

int64_t ivf_work_cap(int32_t n_queries, int32_t nprobe, int64_t n_lists) {
  const int64_t np = (int64_t)n_queries * nprobe;
  return (np < n_lists ? np : n_lists) + np / kTileQ + 1;
}

struct IvfWs {
  int32_t* items;       // [n_queries * nprobe * splits * k]
  float* scores;
  uint32_t* sorted;     // [n_queries * nprobe] list of every probe, ascending, sentinel n_lists
  int32_t* sorted_pos;  // its flattened position
  int32_t* first;       // [n_lists + 1]
  int32_t* tiles;       // [n_lists] tile counts, scanned in place to tile bases
  int32_t* n_work;      // [1] total tiles, [1] the sort's error flag (unused)
  int4* work;           // [ivf_work_cap]
  void* scan_ws;
  void* sort_ws;
  size_t sort_bytes;
};

IvfWs ivf_ws(Carver& c, int32_t n_queries, int32_t nprobe, int64_t n_lists, int32_t k,
             int64_t splits) {
  const size_t np = (size_t)n_queries * (size_t)nprobe;
  IvfWs w;
  w.items = c.take<int32_t>(np * (size_t)splits * (size_t)k);
  w.scores = c.take<float>(np * (size_t)splits * (size_t)k);
  w.sorted = c.take<uint32_t>(np);
  w.sorted_pos = c.take<int32_t>(np);
  w.first = c.take<int32_t>((size_t)n_lists + 1);
  w.tiles = c.take<int32_t>((size_t)n_lists);
  w.n_work = c.take<int32_t>(2);
  w.work = c.take<int4>((size_t)ivf_work_cap(n_queries, nprobe, n_lists));
  w.scan_ws = c.take<char>(exclusive_scan_ws_size(n_lists));
  w.sort_bytes = rs_sort_ids_workspace_size((int64_t)np);
  w.sort_ws = c.take<char>(w.sort_bytes);
  return w;
}

bool ivf_sizes_ok(int32_t n_queries, int32_t nprobe, int64_t n_lists, int32_t k,
                  int32_t list_splits) {
  return n_queries >= 0 && nprobe >= 1 && nprobe <= kIvfProbeMax && n_lists >= 0 &&
         n_lists < ((int64_t)1 << 31) - 1 && k >= 1 && k <= kKMax && list_splits >= 0 &&
         (int64_t)nprobe * list_splits <= kIvfSlotsMax &&
         (int64_t)n_queries * nprobe < ((int64_t)1 << 31);
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" size_t rs_topk_ip_workspace_size(int32_t n_queries, int64_t n_items, int32_t k,
                                            int32_t n_splits) {
  if (n_queries <= 0 || n_items <= 0 || k <= 0 || n_splits < 0) return 0;
  return ws_bytes_for(n_queries, pick_splits(n_queries, n_items, n_splits), k);
}

extern "C" int32_t rs_topk_ip(const float* queries, int64_t q_ld, int32_t n_queries,
                              const float* items, int64_t i_ld, int64_t n_items, int32_t dim,
                              int64_t excl_base, const int64_t* excl_indptr,
                              const int32_t* excl_items, const int32_t* excl_one, int32_t k,
                              int32_t n_splits, int32_t* out_items, float* out_scores,
                              void* workspace, size_t ws_bytes, void* stream) {
  RS_CHECK_ARG(k >= 1 && k <= kKMax, "rs_topk_ip: need 1 <= k <= 64, got %d", k);
  RS_CHECK_ARG(dim >= 1 && dim <= kDimMax, "rs_topk_ip: need 1 <= dim <= 256, got %d", dim);
  RS_CHECK_ARG(q_ld >= dim && i_ld >= dim, "rs_topk_ip: q_ld and i_ld must be >= dim");
  RS_CHECK_ARG(n_queries >= 0 && n_items >= 0 && n_items < ((int64_t)1 << 31),
               "rs_topk_ip: need n_queries >= 0 and 0 <= n_items < 2^31");
  RS_CHECK_ARG(n_splits >= 0 && (n_items == 0 || n_splits <= n_items),
               "rs_topk_ip: need 0 <= n_splits <= n_items");
  RS_CHECK_ARG(excl_base >= 0, "rs_topk_ip: excl_base < 0");
  if (n_queries == 0) return RS_OK;
  RS_CHECK_ARG(out_items != nullptr, "rs_topk_ip: out_items is NULL");
  hipStream_t st = as_stream(stream);
  if (n_items == 0) {
    const int64_t n = (int64_t)n_queries * k;
    topk_ip_pad_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(n, out_items, out_scores);
    RS_CHECK_LAUNCH();
    return RS_OK;
  }
  RS_CHECK_ARG(queries != nullptr && items != nullptr, "rs_topk_ip: queries / items is NULL");
  const int64_t splits = pick_splits(n_queries, n_items, n_splits);
  const int64_t q_tiles = ceil_div(n_queries, kTileQ);
  RS_CHECK_ARG(q_tiles * splits < ((int64_t)1 << 31), "rs_topk_ip: too many blocks");
  const size_t need = ws_bytes_for(n_queries, splits, k);
  RS_CHECK_ARG(need == 0 || (workspace != nullptr && ws_bytes >= need),
               "rs_topk_ip: workspace of %zu bytes, need %zu", ws_bytes, need);
  TopkIpArgs a;
  a.queries = queries;
  a.q_ld = q_ld;
  a.n_queries = n_queries;
  a.items = items;
  a.i_ld = i_ld;
  a.n_items = (int32_t)n_items;
  a.dim = dim;
  a.excl_base = excl_base;
  a.excl_indptr = excl_indptr;
  a.excl_items = excl_items;
  a.excl_one = excl_one;
  a.k = k;
  a.n_splits = (int32_t)splits;
  a.q_tiles = (int32_t)q_tiles;
  int32_t* ws_items = static_cast<int32_t*>(workspace);
  float* ws_scores = reinterpret_cast<float*>(static_cast<char*>(workspace) + need / 2);
  a.out_items = splits == 1 ? out_items : ws_items;
  a.out_scores = splits == 1 ? out_scores : ws_scores;
  a.work = nullptr;
  a.n_work = nullptr;
  a.sorted_pos = nullptr;
  a.n_probes = 0;
  a.nprobe = 1;
  a.list_offsets = nullptr;
  a.n_lists = 0;
  a.item_ids = nullptr;
  const int32_t rc = launch_topk_ip_dim<false>(a, q_tiles * splits, st);
  if (rc != RS_OK || splits == 1) return rc;
  topk_ip_merge_kernel<<<(unsigned)ceil_div(n_queries, kIpWaves), kIpThreads, 0, st>>>(
      ws_items, ws_scores, n_queries, nullptr, 1, 0, (int32_t)splits, k, out_items, out_scores);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

extern "C" size_t rs_ivf_topk_ip_workspace_size(int32_t n_queries, int32_t nprobe,
                                                int64_t n_lists, int32_t k,
                                                int32_t list_splits) {
  if (!ivf_sizes_ok(n_queries, nprobe, n_lists, k, list_splits) || n_queries == 0 ||
      n_lists == 0)
    return 0;
  Carver c(nullptr, 0);
  ivf_ws(c, n_queries, nprobe, n_lists, k,
         ivf_pick_splits(n_queries, nprobe, n_lists, -1, list_splits));
  return c.off + 256;
}

extern "C" int32_t rs_ivf_topk_ip(const float* queries, int64_t q_ld, int32_t n_queries,
                                  const int32_t* probes, int32_t nprobe,
                                  const int64_t* list_offsets, int64_t n_lists,
                                  const int32_t* item_ids, const float* vectors, int64_t v_ld,
                                  int64_t n_items, int32_t dim, int64_t excl_base,
                                  const int64_t* excl_indptr, const int32_t* excl_items,
                                  const int32_t* excl_one, int32_t k, int32_t list_splits,
                                  int32_t* out_items, float* out_scores, void* workspace,
                                  size_t ws_bytes, void* stream) {
  RS_CHECK_ARG(k >= 1 && k <= kKMax, "rs_ivf_topk_ip: need 1 <= k <= 64, got %d", k);
  RS_CHECK_ARG(dim >= 1 && dim <= kDimMax, "rs_ivf_topk_ip: need 1 <= dim <= 256, got %d", dim);
  RS_CHECK_ARG(q_ld >= dim && v_ld >= dim, "rs_ivf_topk_ip: q_ld and v_ld must be >= dim");
  RS_CHECK_ARG(nprobe >= 1 && nprobe <= kIvfProbeMax,
               "rs_ivf_topk_ip: need 1 <= nprobe <= 64, got %d", nprobe);
  RS_CHECK_ARG(n_queries >= 0 && n_lists >= 0 && n_items >= 0 && n_items < ((int64_t)1 << 31),
               "rs_ivf_topk_ip: need n_queries, n_lists >= 0 and 0 <= n_items < 2^31");
  RS_CHECK_ARG(list_splits >= 0 && (int64_t)nprobe * list_splits <= kIvfSlotsMax,
               "rs_ivf_topk_ip: need list_splits >= 0 and nprobe * list_splits <= %d",
               kIvfSlotsMax);
  RS_CHECK_ARG(ivf_sizes_ok(n_queries, nprobe, n_lists, k, list_splits),
               "rs_ivf_topk_ip: n_lists or n_queries * nprobe reaches 2^31");
  RS_CHECK_ARG(excl_base >= 0, "rs_ivf_topk_ip: excl_base < 0");
  if (n_queries == 0) return RS_OK;
  RS_CHECK_ARG(out_items != nullptr, "rs_ivf_topk_ip: out_items is NULL");
  hipStream_t st = as_stream(stream);
  if (n_items == 0 || n_lists == 0) {
    const int64_t n = (int64_t)n_queries * k;
    topk_ip_pad_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(n, out_items, out_scores);
    RS_CHECK_LAUNCH();
    return RS_OK;
  }
  RS_CHECK_ARG(queries != nullptr && probes != nullptr && list_offsets != nullptr &&
                   vectors != nullptr,
               "rs_ivf_topk_ip: queries / probes / list_offsets / vectors is NULL");
  const int64_t splits = ivf_pick_splits(n_queries, nprobe, n_lists, n_items, list_splits);
  const int64_t np = (int64_t)n_queries * nprobe;
  const int64_t work_cap = ivf_work_cap(n_queries, nprobe, n_lists);
  RS_CHECK_ARG(work_cap * splits < ((int64_t)1 << 31), "rs_ivf_topk_ip: too many blocks");
  Carver c(workspace, ws_bytes);
  const IvfWs w = ivf_ws(c, n_queries, nprobe, n_lists, k, splits);
  RS_CHECK_ARG(workspace != nullptr && c.ok(), "rs_ivf_topk_ip: workspace of %zu bytes, need %zu",
               ws_bytes, c.off);
  // the probes grouped by list; -1 and every other value outside [0, n_lists) sort last
  int32_t rc = rs_sort_ids(probes, RS_ID_I32, np, nullptr, 1, n_lists, w.sorted, w.sorted_pos,
                           nullptr, w.n_work + 1, w.sort_ws, w.sort_bytes, stream);
  if (rc != RS_OK) return rc;
  ivf_bounds_kernel<<<(unsigned)ceil_div(np + 1, 256), 256, 0, st>>>(w.sorted, np, n_lists,
                                                                      w.first);
  RS_CHECK_LAUNCH();
  ivf_tile_counts_kernel<<<(unsigned)ceil_div(n_lists, 256), 256, 0, st>>>(w.first, n_lists,
                                                                           w.tiles);
  RS_CHECK_LAUNCH();
  rc = exclusive_scan_i32(w.tiles, w.tiles, n_lists, w.n_work, w.scan_ws,
                          exclusive_scan_ws_size(n_lists), st);
  if (rc != RS_OK) return rc;
  ivf_work_kernel<<<(unsigned)ceil_div(np, 256), 256, 0, st>>>(w.sorted, np, n_lists, w.first,
                                                               w.tiles, work_cap, w.work);
  RS_CHECK_LAUNCH();
  TopkIpArgs a;
  a.queries = queries;
  a.q_ld = q_ld;
  a.n_queries = n_queries;
  a.items = vectors;
  a.i_ld = v_ld;
  a.n_items = (int32_t)n_items;
  a.dim = dim;
  a.excl_base = excl_base;
  a.excl_indptr = excl_indptr;
  a.excl_items = excl_items;
  a.excl_one = excl_one;
  a.k = k;
  a.n_splits = (int32_t)splits;
  a.q_tiles = 0;
  a.out_items = w.items;
  a.out_scores = w.scores;
  a.work = w.work;
  a.n_work = w.n_work;
  a.sorted_pos = w.sorted_pos;
  a.n_probes = np;
  a.nprobe = nprobe;
  a.list_offsets = list_offsets;
  a.n_lists = n_lists;
  a.item_ids = item_ids;
  rc = launch_topk_ip_dim<true>(a, work_cap * splits, st);
  if (rc != RS_OK) return rc;
  topk_ip_merge_kernel<<<(unsigned)ceil_div(n_queries, kIpWaves), kIpThreads, 0, st>>>(
      w.items, w.scores, n_queries, probes, nprobe, n_lists, (int32_t)splits, k, out_items,
      out_scores);
  RS_CHECK_LAUNCH();
  return RS_OK;
}
