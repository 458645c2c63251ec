// Shared device/host helpers for the neusky_amd HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NSKY_OK 0
#define NSKY_ERR_ARG -1
#define NSKY_ERR_LAUNCH -2

void nsky_set_error(const char* fmt, ...);

#define NSKY_CHECK_ARG(cond, ...)                \
  do {                                           \
    if (!(cond)) {                               \
      nsky_set_error(__VA_ARGS__);               \
      return NSKY_ERR_ARG;                       \
    }                                            \
  } while (0)

#define NSKY_CHECK_LAUNCH(name)                                             \
  do {                                                                      \
    hipError_t e_ = hipGetLastError();                                      \
    if (e_ != hipSuccess) {                                                 \
      nsky_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
      return NSKY_ERR_LAUNCH;                                               \
    }                                                                       \
  } while (0)

static inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// a grid of n workgroups, capped at per_cu for each of the 256 CUs (the kernels stride over what is left); never empty
static inline unsigned capped_grid(int64_t n, int per_cu) { return (unsigned)(n < 1 ? 1 : n < 256 * (int64_t)per_cu ? n : 256 * (int64_t)per_cu); }

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ float4 ldg4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void stg4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// 16 bytes per lane global -> LDS.  The LDS-DMA is hidden from hipcc's waitcnt bookkeeping (it would drain vmcnt(0) before every
// ds_read otherwise); M0 is saved and restored inside the statement.  Completion is counted by hand: vmcnt_wait<N>().
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
template <int N>
__device__ __forceinline__ void vmcnt_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// consecutive hardware workgroup ids go round-robin over the 8 XCDs (each with a private L2): hand every XCD one contiguous run of
// logical ids (a bijection of [0, total)), so the workgroups that re-read the same operand rows share an L2
__device__ __forceinline__ int xcd_contiguous(int id, int total) {
  const int q = total >> 3, r = total & 7, x = id & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (id >> 3);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
