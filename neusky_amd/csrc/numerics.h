// The arithmetic that defines the project's precision contract, each piece exactly once: the fp16 hi + residual split on power-of-two
// pre-scaled operands (~2^-22 per product), the transcendental approximations both kernel sets (`f32` per-layer, `splith` chains)
// share, the sRGB transfer curve and the tile-native layout.  Parity between the kernel sets rests on every file calling THESE
// definitions.  Device-inline; common.h is the only include.
#pragma once
#include "common.h"

// power-of-two scale s with m s in [2^14, 2^15) (m = largest magnitude of the operand; the fp16 residual of every element within 2^-13
// of the largest stays a normal number: the matrix cores flush fp16 subnormals); returns s, inv = 1 / s.  m = 0 or not finite: 1.
__device__ __forceinline__ float pow2_scale(float m, float& inv) {
  if (!(m > 0.0f) || !(m < 3.0e38f)) { inv = 1.0f; return 1.0f; }
  int e;
  (void)frexpf(m, &e);  // m < 2^e
  e = max(-100, min(100, e));
  inv = ldexpf(1.0f, e - 15);
  return ldexpf(1.0f, 15 - e);
}

// x = hi + lo with hi = fp16(x), lo = fp16(x - hi) (x - hi is exact in fp32): the operands of hi hi + hi lo + lo hi
__device__ __forceinline__ void split8(const float (&x)[8], f16x8& hi, f16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const _Float16 xh = (_Float16)x[j];
    hi[j] = xh;
    lo[j] = (_Float16)(x[j] - (float)xh);
  }
}

// sin and cos with Cody-Waite reduction to [-pi/4, pi/4] + minimax polynomials (|err| < 2e-7 for |x| < 1e4): ~20 VALU ops instead of
// the ocml slow path; the FiLM epilogues' |x| = |freq * z + phase| ~ 1e2
__device__ __forceinline__ void sincos_cw(float x, float& s, float& c) {
  const float k = rintf(x * 0.6366197723675814f);  // x * 2/pi
  float r = fmaf(-k, 1.5707962513e+00f, x);
  r = fmaf(-k, 7.5497894159e-08f, r);
  r = fmaf(-k, 5.3903029534e-15f, r);
  const float r2 = r * r;
  float sp = fmaf(r2, 2.7183114939e-06f, -1.9839334836e-04f);
  sp = fmaf(sp, r2, 8.3333293855e-03f);
  sp = fmaf(sp, r2, -1.6666666567e-01f);
  sp = fmaf(sp * r2, r, r);
  float cp = fmaf(r2, 2.4433157117e-05f, -1.3887316255e-03f);
  cp = fmaf(cp, r2, 4.1666645683e-02f);
  cp = fmaf(cp, r2, -0.5f);
  cp = fmaf(cp, r2, 1.0f);
  const int q = (int)k;
  const float ss = (q & 1) ? cp : sp;
  const float cc = (q & 1) ? sp : cp;
  s = (q & 2) ? -ss : ss;
  c = ((q + 1) & 2) ? -cc : cc;
}

// One of the two alone (the chain forward needs the sine, the FiLM backward the cosine): reduction by multiples of pi to
// [-pi/2, pi/2] (two-term Cody-Waite: the fused multiply-adds keep the products exact, the third term of pi is k 1e-15), ONE
// polynomial, the sign from the parity of k.  14 instructions instead of 23; |err| < 1.4e-7 on the reduced range (fitted and
// checked in float32 arithmetic), the reduction adds |k| 1e-15.
__device__ __forceinline__ float sin_cw(float x) {
  const float k = rintf(x * 0.31830988618379067f);
  float r = fmaf(-k, 3.14159274101257324f, x);
  r = fmaf(-k, -8.74227766e-08f, r);
  const float r2 = r * r;
  float p = fmaf(r2, 2.6348141091e-06f, -1.9822760078e-04f);
  p = fmaf(p, r2, 8.3332424983e-03f);
  p = fmaf(p, r2, -1.6666665673e-01f);
  const float s = fmaf(p * r2, r, r);
  return __int_as_float(__float_as_int(s) ^ ((int)k << 31));
}
__device__ __forceinline__ float cos_cw(float x) {
  const float k = rintf(x * 0.31830988618379067f);
  float r = fmaf(-k, 3.14159274101257324f, x);
  r = fmaf(-k, -8.74227766e-08f, r);
  const float r2 = r * r;
  float p = fmaf(r2, -2.6297973932e-07f, 2.4774602934e-05f);
  p = fmaf(p, r2, -1.3888651738e-03f);
  p = fmaf(p, r2, 4.1666660458e-02f);
  p = fmaf(p, r2, -0.5f);
  const float c = fmaf(p, r2, 1.0f);
  return __int_as_float(__float_as_int(c) ^ ((int)k << 31));
}

// softplus_beta(v) and sigmoid(beta v) from ONE exponential: t = exp(-|beta v|) in (0, 1];
// softplus = (max(beta v, 0) + log1p(t)) / beta, sigmoid = 1/(1+t) or t/(1+t).  log1p(t) = log(u) * t / (u - 1) with
// u = fl(1 + t) cancels the rounding of 1 + t (few-ulp result for every t); hardware exp2/log2/rcp based.
// torch.nn.functional.softplus semantics: beta v > 20 returns v itself (sdf_albedo_field.py geo network, beta = 100).
__device__ __forceinline__ void softplus_sig(float v, float beta, float inv_beta, float& sp, float& sg) {
  const float bv = beta * v;
  const float t = __expf(-fabsf(bv));
  const float u = 1.0f + t, um1 = u - 1.0f;
  const float r = __builtin_amdgcn_rcpf(u);
  const float l = um1 == 0.0f ? t : __logf(u) * (t * __builtin_amdgcn_rcpf(um1));
  sp = bv > 20.0f ? v : (fmaxf(bv, 0.0f) + l) * inv_beta;
  sg = bv >= 0.0f ? r : t * r;
}
__device__ __forceinline__ float softplus_b(float v, float beta, float inv_beta) {  // the softplus alone
  float sp, sg;
  softplus_sig(v, beta, inv_beta, sp, sg);
  return sp;
}

// linear -> sRGB (utils.py:25-30): the curve before its clamp, the clamped curve, and the clamped curve's derivative
__device__ __forceinline__ float srgb_raw(float x) {
  return x <= 0.0031308f ? 12.92f * x : 1.055f * powf(fabsf(x), 1.0f / 2.4f) - 0.055f;
}
__device__ __forceinline__ float srgb_fwd(float x) { return fminf(fmaxf(srgb_raw(x), 0.0f), 1.0f); }
__device__ __forceinline__ float srgb_bwd(float x) {
  const float y = srgb_raw(x);
  if (y < 0.0f || y > 1.0f) return 0.0f;
  if (x <= 0.0031308f) return 12.92f;
  return 1.055f / 2.4f * powf(fabsf(x), 1.0f / 2.4f - 1.0f);
}

// Tile-native activation layout ("native"; THE description: chain.h and include/neusky_hip.h point here).  A [rows, width] fp32
// matrix (rows padded to a multiple of 32, width % 32 == 0) is cut into 32-row x 32-feature blocks of 4 KB, block (R, t) at float
// offset (R * (width / 32) + t) * 1024, and inside a block element (row c, feature f) sits at
// (f / 8) * 256 + (c + 32 * ((f / 4) & 1)) * 4 + (f & 3): exactly the accumulator layout of v_mfma_f32_32x32x16 (register
// 4 g + q of lane (c, h) = feature 8 g + 4 h + q of batch row c), so a wave stores / loads a tile with four 1 KB-contiguous
// float4 instructions (chain.h store_tile / load_tile) and the lane that stored a piece is the lane that reads it back.
// native_offset: float offset of element (row k, feature t), t % 4 == 0, of such a matrix with nnt = width / 32 tiles per row.
__device__ __forceinline__ long native_offset(int k, int t, int nnt) {
  return ((long)(k >> 5) * nnt + (t >> 5)) * 1024 + ((t & 31) >> 3) * 256 + ((k & 31) + 32 * ((t >> 2) & 1)) * 4;
}
