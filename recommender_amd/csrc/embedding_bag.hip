// embedding_bag.hip — jagged sum / mean lookup (EmbeddingBag) and the two helpers of its
// backward: the position -> bag remap that lets rs_embedding_apply_scaled do the bag backward
// without ever forming the [n_ids, dim] gradient, and the expansion that forms it for the
// consumers that want ordinary (ids, rows) gradients.
//
// Forward: a lane group of 1 << lpr_log2 lanes owns a bag (the gather's row layout: VEC floats
// per lane, 16 / 8 / 4 bytes) and walks its positions in ascending order, four at a time: the
// four ids, then the four table rows, are requested before the four ordered adds, so the rows
// fly together. The order of the additions is the position order alone — part of the contract
// (include/recsys_hip.h), which is why a long bag is not split over lane groups.
// No atomics except the error flag's OR.
#include <algorithm>

#include "row_io.hpp"

namespace rs {
namespace {

// [s, e) of bag b; a reversed range or one that leaves [0, n_ids] is empty and reported
__device__ __forceinline__ bool bag_range(const int64_t* __restrict__ offsets, int64_t b,
                                          int32_t bag_len, int64_t n_ids, int64_t& s, int64_t& e) {
  if (!offsets) {
    s = b * bag_len;
    e = s + bag_len;
    return true;
  }
  s = offsets[b];
  e = offsets[b + 1];
  if (s < 0 || e > n_ids || s > e) {
    s = e = 0;
    return false;
  }
  return true;
}

// the bag holding position p, -1 if none: p / bag_len, or the last b with offsets[b] <= p
// (empty bags share their start with the bag after them, which is the one found)
__device__ __forceinline__ int64_t bag_of(const int64_t* __restrict__ offsets, int64_t n_bags,
                                          int32_t bag_len, int64_t n_ids, int64_t p) {
  if (p < 0 || p >= n_ids || n_bags <= 0) return -1;
  if (!offsets) return bag_len > 0 ? p / bag_len : -1;
  int64_t lo = 0, hi = n_bags;  // first b in [0, n_bags] with offsets[b] > p
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (offsets[mid] <= p) lo = mid + 1; else hi = mid;
  }
  const int64_t b = lo - 1;
  if (b < 0 || b >= n_bags) return -1;
  return (offsets[b] <= p && p < offsets[b + 1]) ? b : -1;
}

template <int VEC, typename IdT>
__global__ __launch_bounds__(256) void bag_fwd_kernel(
    const float* __restrict__ table, int64_t n_rows, int dim, const IdT* __restrict__ ids,
    int64_t n_ids, const int64_t* __restrict__ offsets, int64_t n_bags,
    int32_t bag_len, const uint8_t* __restrict__ valid, const float* __restrict__ weights,
    int32_t mode, const int64_t* __restrict__ slot_offsets, int32_t n_slots,
    float* __restrict__ out, int64_t out_ld, float* __restrict__ bag_scale, int32_t* err_flag,
    int lpr_log2, int chunks) {
  constexpr int U = 4;
  const int lpr = 1 << lpr_log2;
  const int gl = threadIdx.x & (lpr - 1);
  const int64_t gpb = blockDim.x >> lpr_log2;
  const int64_t groups = (int64_t)gridDim.x * gpb;
  bool bad = false;
  // without a mask or weights the flag / weight loads still go out, from the ids' own bytes
  // (position p < n_ids lies inside them as a byte and as a float) and are ignored: a branch
  // around a load makes the compiler wait for every load issued before the join, and the four
  // ids of a batch would come in one after the other
  const uint8_t* vp = valid ? valid : reinterpret_cast<const uint8_t*>(ids);
  const float* wp = weights ? weights : reinterpret_cast<const float*>(ids);
  for (int64_t b = (int64_t)blockIdx.x * gpb + (threadIdx.x >> lpr_log2); b < n_bags;
       b += groups) {
    int64_t s, e;
    bad |= !bag_range(offsets, b, bag_len, n_ids, s, e);
    // the bag's table: slot b % n_slots of the slab (global_row's rule with the bag as position)
    int64_t lo = 0, card = n_rows;
    if (slot_offsets) {
      const int sl = (int)(b % n_slots);
      lo = slot_offsets[sl];
      card = slot_offsets[sl + 1] - lo;
    }
    int64_t count = 0;
    for (int c = 0; c < chunks; ++c) {
      const int col = (gl + c * lpr) * VEC;
      const int colc = col < dim ? col : 0;  // lanes past the row read column 0, never stored
      float acc[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
      count = 0;
      for (int64_t p0 = s; p0 < e; p0 += U) {
        // every load below is unguarded from an address that is always valid: an entry past
        // the bag re-reads position s, a dead or out-of-range one reads table row 0
        int64_t id[U];
        uint8_t vl[U];
        float w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t p = p0 + u < e ? p0 + u : s;
          id[u] = static_cast<int64_t>(ids[p]);
          vl[u] = vp[p];
          w[u] = wp[p];
        }
        float v[U][VEC];
        bool live[U], in[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          live[u] = p0 + u < e && (!valid || vl[u] != 0);
          in[u] = id[u] >= 0 && id[u] < card;
          const int64_t r = (live[u] && in[u]) ? lo + id[u] : 0;
          RowIO<VEC>::load(table + r * dim + colc, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (live[u]) {
            ++count;
            bad |= !in[u];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
              float t = in[u] ? v[u][k] : 0.f;
              if (weights) t = __fmul_rn(w[u], t);
              acc[k] = __fadd_rn(acc[k], t);
            }
          }
        }
      }
      if (col < dim) {
        if (mode == RS_BAG_MEAN) {
          const float n = (float)count;
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] = count > 0 ? __fdiv_rn(acc[k], n) : 0.f;
        }
        RowIO<VEC>::store(out + b * out_ld + col, acc);
      }
    }
    if (bag_scale && gl == 0) bag_scale[b] = count > 0 ? __fdiv_rn(1.f, (float)count) : 0.f;
  }
  flag_oob_wave(bad, err_flag);
}

__global__ __launch_bounds__(256) void bag_remap_kernel(const int32_t* __restrict__ sorted_pos,
                                                        int64_t n_ids,
                                                        const int64_t* __restrict__ offsets,
                                                        int64_t n_bags, int32_t bag_len,
                                                        int32_t* __restrict__ bag_pos) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_ids;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = bag_of(offsets, n_bags, bag_len, n_ids, sorted_pos[i]);
    bag_pos[i] = b < 0 ? 0 : (int32_t)b;
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void bag_expand_kernel(
    const float* __restrict__ dout, int64_t dout_ld, int dim, int64_t n_ids,
    const int64_t* __restrict__ offsets, int64_t n_bags, int32_t bag_len,
    const float* __restrict__ bag_scale, const float* __restrict__ weights,
    float* __restrict__ grad_rows, int lpr_log2, int chunks) {
  const int lpr = 1 << lpr_log2;
  const int gl = threadIdx.x & (lpr - 1);
  const int64_t gpb = blockDim.x >> lpr_log2;
  const int64_t groups = (int64_t)gridDim.x * gpb;
  for (int64_t p = (int64_t)blockIdx.x * gpb + (threadIdx.x >> lpr_log2); p < n_ids;
       p += groups) {
    const int64_t b = bag_of(offsets, n_bags, bag_len, n_ids, p);
    const float sc = (b >= 0 && bag_scale) ? bag_scale[b] : 1.f;
    const float w = weights ? weights[p] : 1.f;
    for (int c = 0; c < chunks; ++c) {
      const int col = (gl + c * lpr) * VEC;
      if (col >= dim) continue;
      float g[VEC];
      if (b >= 0) {
        RowIO<VEC>::load(dout + b * dout_ld + col, g);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          if (bag_scale) g[k] = __fmul_rn(sc, g[k]);
          if (weights) g[k] = __fmul_rn(w, g[k]);
        }
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) g[k] = 0.f;
      }
      RowIO<VEC>::store(grad_rows + p * dim + col, g);
    }
  }
}

int32_t check_layout(const int64_t* offsets, int64_t n_ids, int64_t n_bags, int32_t bag_len) {
  RS_CHECK_ARG(n_ids >= 0 && n_bags >= 0, "n_ids and n_bags must be >= 0");
  if (!offsets) {
    RS_CHECK_ARG(bag_len >= 0, "bag_len must be >= 0");
    RS_CHECK_ARG(n_ids == n_bags * (int64_t)bag_len,
                 "without offsets n_ids (%lld) must be n_bags * bag_len (%lld * %d)",
                 (long long)n_ids, (long long)n_bags, bag_len);
  }
  return RS_OK;
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" int32_t rs_embedding_bag_fwd(const float* table, int64_t n_rows, int32_t dim,
                                        const void* ids, int32_t id_dtype, int64_t n_ids,
                                        const int64_t* offsets, int64_t n_bags, int32_t bag_len,
                                        const uint8_t* valid, const float* per_sample_weights,
                                        int32_t mode, const int64_t* slot_offsets, int32_t n_slots,
                                        float* out, int64_t out_ld, float* bag_scale,
                                        int32_t* err_flag, void* stream) {
  RS_CHECK_ARG(dim > 0, "dim must be > 0");
  RS_CHECK_ARG(n_rows > 0, "n_rows must be > 0");
  RS_CHECK_ARG(out_ld >= dim, "out_ld must be >= dim");
  RS_CHECK_ARG(n_slots >= 1, "n_slots must be >= 1");
  RS_CHECK_ARG(id_dtype == RS_ID_I32 || id_dtype == RS_ID_I64, "bad id dtype");
  RS_CHECK_ARG(mode == RS_BAG_SUM || mode == RS_BAG_MEAN, "mode must be RS_BAG_SUM or RS_BAG_MEAN");
  RS_CHECK_ARG(!(per_sample_weights && mode == RS_BAG_MEAN),
               "per_sample_weights go with RS_BAG_SUM only");
  if (int32_t st = check_layout(offsets, n_ids, n_bags, bag_len)) return st;
  if (n_bags == 0) return RS_OK;
  RS_CHECK_ARG(table && out && (n_ids == 0 || ids), "null pointer");
  const void* ptrs[3] = {table, out, reinterpret_cast<const void*>((uintptr_t)out_ld * 4)};
  const RowGeom g = row_geom(dim, ptrs, 3);
  const int gpb = 256 >> g.lpr_log2;
  const int blocks = (int)std::min<int64_t>(ceil_div(n_bags, gpb), 256 * 64);
  hipStream_t st = as_stream(stream);
#define RS_BAG_FWD(V, T)                                                                      \
  bag_fwd_kernel<V, T><<<blocks, 256, 0, st>>>(                                                \
      table, n_rows, dim, static_cast<const T*>(ids), n_ids, offsets, n_bags, bag_len, valid, \
      per_sample_weights, mode, slot_offsets, n_slots, out, out_ld, bag_scale, err_flag,      \
      g.lpr_log2, g.chunks)
  switch (g.vec * 2 + (id_dtype == RS_ID_I64)) {
    case 9: RS_BAG_FWD(4, int64_t); break;
    case 8: RS_BAG_FWD(4, int32_t); break;
    case 5: RS_BAG_FWD(2, int64_t); break;
    case 4: RS_BAG_FWD(2, int32_t); break;
    case 3: RS_BAG_FWD(1, int64_t); break;
    default: RS_BAG_FWD(1, int32_t); break;
  }
#undef RS_BAG_FWD
  RS_CHECK_LAUNCH();
  return RS_OK;
}

extern "C" int32_t rs_embedding_bag_remap_pos(const int32_t* sorted_pos, int64_t n_ids,
                                              const int64_t* offsets, int64_t n_bags,
                                              int32_t bag_len, int32_t* bag_pos, void* stream) {
  if (int32_t st = check_layout(offsets, n_ids, n_bags, bag_len)) return st;
  RS_CHECK_ARG(n_bags <= 0x7FFFFFFFll, "n_bags must fit int32 positions");
  if (n_ids == 0) return RS_OK;
  RS_CHECK_ARG(sorted_pos && bag_pos, "null pointer");
  const int blocks = (int)std::min<int64_t>(ceil_div(n_ids, 256), 256 * 32);
  bag_remap_kernel<<<blocks, 256, 0, as_stream(stream)>>>(sorted_pos, n_ids, offsets, n_bags,
                                                          bag_len, bag_pos);
  RS_CHECK_LAUNCH();
  return RS_OK;
}

extern "C" int32_t rs_embedding_bag_expand_grad(const float* dout, int64_t dout_ld, int32_t dim,
                                                int64_t n_ids, const int64_t* offsets,
                                                int64_t n_bags, int32_t bag_len,
                                                const float* bag_scale,
                                                const float* per_sample_weights, float* grad_rows,
                                                void* stream) {
  RS_CHECK_ARG(dim > 0, "dim must be > 0");
  RS_CHECK_ARG(dout_ld >= dim, "dout_ld must be >= dim");
  if (int32_t st = check_layout(offsets, n_ids, n_bags, bag_len)) return st;
  if (n_ids == 0) return RS_OK;
  RS_CHECK_ARG(grad_rows && (n_bags == 0 || dout), "null pointer");
  const void* ptrs[3] = {dout ? dout : grad_rows, grad_rows,
                         reinterpret_cast<const void*>((uintptr_t)dout_ld * 4)};
  const RowGeom g = row_geom(dim, ptrs, 3);
  const int gpb = 256 >> g.lpr_log2;
  const int blocks = (int)std::min<int64_t>(ceil_div(n_ids, gpb), 256 * 64);
  hipStream_t st = as_stream(stream);
#define RS_BAG_EXPAND(V)                                                                         \
  bag_expand_kernel<V><<<blocks, 256, 0, st>>>(dout, dout_ld, dim, n_ids, offsets, n_bags,       \
                                               bag_len, bag_scale, per_sample_weights, grad_rows, \
                                               g.lpr_log2, g.chunks)
  switch (g.vec) {
    case 4: RS_BAG_EXPAND(4); break;
    case 2: RS_BAG_EXPAND(2); break;
    default: RS_BAG_EXPAND(1); break;
  }
#undef RS_BAG_EXPAND
  RS_CHECK_LAUNCH();
  return RS_OK;
}
