// common.hpp — shared helpers for the gfx950 kernels behind include/recsys_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/recsys_hip.h"

namespace rs {

// ---- host-side error reporting (thread-local, see rs_last_error) --------------------
void set_error(const char* fmt, ...);

#define RS_CHECK_ARG(cond, ...)        \
  do {                                 \
    if (!(cond)) {                     \
      ::rs::set_error(__VA_ARGS__);    \
      return RS_E_INVALID;             \
    }                                  \
  } while (0)

#define RS_CHECK_HIP(expr)                                                              \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      ::rs::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return RS_E_HIP;                                                                  \
    }                                                                                   \
  } while (0)

// after a kernel launch: catch launch-configuration errors without synchronising
#define RS_CHECK_LAUNCH() RS_CHECK_HIP(hipGetLastError())

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// workspace carving: 256-B aligned sub-buffers
struct Carver {
  char* base;
  size_t off = 0;
  size_t cap;
  Carver(void* p, size_t c) : base(static_cast<char*>(p)), cap(c) {}
  template <typename T>
  T* take(size_t n) {
    off = align_up(off, 256);
    T* r = reinterpret_cast<T*>(base ? base + off : nullptr);
    off += n * sizeof(T);
    return r;
  }
  bool ok() const { return off <= cap; }
};

// compute units of the current device (256 if it cannot be asked), read once per process
inline int device_cus() {
  static const int n = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0) {
      (void)hipGetLastError();
      return 256;
    }
    return cus;
  }();
  return n;
}

// ---- device-wide primitives other kernel files call (sort.hip unless noted) ---------
int32_t radix_sort_pairs(uint32_t* keys_in, int32_t* vals_in, uint32_t* keys_out,
                         int32_t* vals_out, int64_t n, int64_t n_rows, void* ws, size_t ws_bytes,
                         hipStream_t st);
size_t radix_sort_ws_size(int64_t n);
int32_t exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t n, int32_t* total, void* ws,
                           size_t ws_bytes, hipStream_t st);
size_t exclusive_scan_ws_size(int64_t n);
// fixed two-level fold of nchunks partial rows [N] into out[N] (dense.hip); part2 holds
// 32 x N floats of scratch
int32_t fold_two_level(const float* part, int nchunks, int N, float* part2, float* out,
                       hipStream_t st);

// ---- device helpers ------------------------------------------------------------------
constexpr int kWave = 64;

// register vectors (clang ext_vector_type: element-wise arithmetic, MFMA operands and results)
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ int64_t load_id(const void* ids, int32_t dtype, int64_t i) {
  return dtype == RS_ID_I64 ? static_cast<const int64_t*>(ids)[i]
                            : static_cast<int64_t>(static_cast<const int32_t*>(ids)[i]);
}

// Global row of the id at flattened position p (slot = p % n_slots). Returns -1 if the id
// is outside its table (TF-GPU: zero row, SURVEY §8.1 "OOB ids").
__device__ __forceinline__ int64_t global_row(const void* ids, int32_t dtype, int64_t p,
                                              const int64_t* slot_offsets, int32_t n_slots,
                                              int64_t n_rows) {
  int64_t id = load_id(ids, dtype, p);
  if (slot_offsets) {
    int s = static_cast<int>(p % n_slots);
    int64_t lo = slot_offsets[s], hi = slot_offsets[s + 1];
    if (id < 0 || id >= hi - lo) return -1;
    return lo + id;
  }
  if (id < 0 || id >= n_rows) return -1;
  return id;
}

__device__ __forceinline__ void flag_oob(int32_t* err_flag) {
  if (err_flag) atomicOr(err_flag, RS_ERRBIT_OOB);
}
// one OR per wave if any of its lanes saw an out-of-table id
__device__ __forceinline__ void flag_oob_wave(bool oob, int32_t* err_flag) {
  if (__any(oob) && (threadIdx.x & 63) == 0) flag_oob(err_flag);
}

// full-wave xor butterflies: every lane ends with the result, summed in one fixed order
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
// lane k's value (k wave-uniform), as a scalar operand
__device__ __forceinline__ float read_lane(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

}  // namespace rs
