// row_io.hpp — vector row I/O and the lane-group layout of the embedding kernels: a row of `dim`
// fp32 is covered by a lane group of LPR lanes (a power of two <= 64), each lane moving VEC floats
// (16 B when dim % 4 == 0 and everything is aligned for it) per chunk.
#pragma once
#include "common.hpp"

namespace rs {

template <int VEC>
struct RowIO;
template <>
struct RowIO<4> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
    float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <>
struct RowIO<2> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[2]) {
    float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[2]) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  }
};
template <>
struct RowIO<1> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[1]) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float (&v)[1]) { *p = v[0]; }
};
// a read-once stream (the walk's gradient rows): non-temporal, so it does not evict the
// table rows and tile partials that are read again
template <int VEC>
__device__ __forceinline__ void load_stream(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    f4 t = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    RowIO<VEC>::load(p, v);
  }
}

// the smallest power-of-two lane group (64 lanes at most) that covers `pieces` per-lane pieces
// of a row, and the chunks each of its lanes then walks
struct LaneGroup {
  int lpr_log2, chunks;
};
inline LaneGroup lane_group(int64_t pieces) {
  int lpr = 1, l2 = 0;
  while (lpr < pieces && lpr < 64) { lpr <<= 1; ++l2; }
  return {l2, (int)((pieces + lpr - 1) / lpr)};
}

struct RowGeom {
  int vec, lpr_log2;
  int chunks;  // column chunks of (lanes * vec) floats per row
  int cpl;     // chunks rounded up to a power of two (the CPL the kernels are built for)
};
// the widest vector that dim and every address in ptrs allow (base pointers, and row strides in
// bytes passed as addresses), over the lane group of dim / vec pieces
inline RowGeom row_geom(int dim, const void* const* ptrs, int nptr) {
  int vec = (dim % 4 == 0) ? 4 : (dim % 2 == 0 ? 2 : 1);
  for (int i = 0; i < nptr; ++i) {
    uintptr_t a = reinterpret_cast<uintptr_t>(ptrs[i]);
    while (vec > 1 && (a % (vec * 4)) != 0) vec >>= 1;
  }
  const LaneGroup g = lane_group(dim / vec);
  int c = 1;
  while (c < g.chunks) c <<= 1;
  return {vec, g.lpr_log2, g.chunks, c};
}

}  // namespace rs
