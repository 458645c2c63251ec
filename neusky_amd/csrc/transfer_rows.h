// The stored rows of a radiance transfer (csrc/transfer.hip: T; csrc/transfer_sh.hip: T and C), each piece exactly once: how a row stored
// as fp32 or as scaled fp16 is read, and the power of two a fp16 row is scaled by.  Both agree with relight.transfer.pack_fp16.
#pragma once
#include <hip/hip_fp16.h>

#include "common.h"

__device__ __forceinline__ float half_bits_to_float(unsigned short h) { return __half2float(__ushort_as_half(h)); }
__device__ __forceinline__ float half_lo(unsigned w) { return half_bits_to_float((unsigned short)(w & 0xffffu)); }
__device__ __forceinline__ float half_hi(unsigned w) { return half_bits_to_float((unsigned short)(w >> 16)); }

// element `elem` of the stored rows
template <bool HALF>
__device__ __forceinline__ float row_element(const void* T, int64_t elem) {
  return HALF ? __half2float(((const __half*)T)[elem]) : ((const float*)T)[elem];
}

// 4 elements from `elem` on as one access: 8 bytes of fp16, 16 bytes of fp32 (aligned)
template <bool HALF>
__device__ __forceinline__ float4 row_load4(const void* T, int64_t elem) {
  if (HALF) {
    const uint2 raw = *(const uint2*)((const __half*)T + elem);
    return make_float4(half_lo(raw.x), half_hi(raw.x), half_lo(raw.y), half_hi(raw.y));
  }
  return *(const float4*)((const float*)T + elem);
}

// one 16-byte access (aligned): 8 elements of fp16, 4 of fp32, decoded where they are used
template <bool HALF>
struct RowVec;
template <>
struct RowVec<false> {
  static constexpr int kElems = 4;
  float4 raw;
  __device__ __forceinline__ void load(const void* T, int64_t elem) { raw = *(const float4*)((const float*)T + elem); }
  __device__ __forceinline__ float get(int e) const { return e == 0 ? raw.x : e == 1 ? raw.y : e == 2 ? raw.z : raw.w; }
};
template <>
struct RowVec<true> {
  static constexpr int kElems = 8;
  uint4 raw;
  __device__ __forceinline__ void load(const void* T, int64_t elem) { raw = *(const uint4*)((const __half*)T + elem); }
  __device__ __forceinline__ float get(int e) const {
    const unsigned w = e < 2 ? raw.x : e < 4 ? raw.y : e < 6 ? raw.z : raw.w;
    return (e & 1) ? half_hi(w) : half_lo(w);
  }
};

// the scale of pack_fp16: a row maximum mx = m 2^x with m in [0.5, 1) -> -x, so that the stored row is T 2^(-x), a power-of-two scale
// (exact); a zero or non-finite maximum takes 0.  In the precision its caller holds the maximum in.
__device__ __forceinline__ int row_exponent(float mx) {
  int ex = 0;
  if (mx > 0.0f && mx < __builtin_inff()) {
    frexpf(mx, &ex);
    ex = -ex;
  }
  return ex;
}
__device__ __forceinline__ int row_exponent(double mx) {
  int ex = 0;
  if (mx > 0.0 && mx < (double)__builtin_inff()) {
    frexp(mx, &ex);
    ex = -ex;
  }
  return ex;
}
