// What the kernels that take lights in batches share (csrc/sun.hip, lights.hip, transfer.hip, transfer_sh.hip), each piece exactly once:
// the rule that cuts K lights into passes, the dispatch of a run-time count or storage to a template argument, and the per-ray transfer
// sum of a sun and of a lamp.
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "common.h"

// f(std::integral_constant<int, N>{}) for the first N of Ns with n <= N (the last N takes what is left); f's return code is passed on
template <int N, int... Ns, typename F>
int with_count(int n, F&& f) {
  if constexpr (sizeof...(Ns) == 0) return f(std::integral_constant<int, N>{});
  else return n <= N ? f(std::integral_constant<int, N>{}) : with_count<Ns...>(n, f);
}

// f(std::bool_constant<HALF>{}): the fp16 and the fp32 instantiation of a launch
template <typename F>
int with_storage(bool half, F&& f) {
  return half ? f(std::true_type{}) : f(std::false_type{});
}

template <typename F, int... I>
int pass_of(int kb, int k0, F& f, std::integer_sequence<int, I...>) {
  return with_count<(I + 1)...>(kb, [&](auto c) { return f(k0, c); });
}

// K lights in passes of `per_pass` <= MAX: f(k0, std::integral_constant<int, KB>{}) for the pass of KB = min(per_pass, K - k0) lights
// that starts at light k0.  The first code that is not NSKY_OK ends the loop and is returned.
template <int MAX, typename F>
int for_each_pass(int K, F&& f, int per_pass = MAX) {
  for (int k0 = 0; k0 < K; k0 += per_pass) {
    const int rc = pass_of(std::min(per_pass, K - k0), k0, f, std::make_integer_sequence<int, MAX>{});
    if (rc != NSKY_OK) return rc;
  }
  return NSKY_OK;
}

// t[k,r,c] = sum_s w[r,s] alb[r,s,c] factor_k(n[r,s], x[r,s]): one wave per ray, lanes stride the samples, a sample is read once per pass
// and meets the KB lights of the pass, held in scalar registers; a lane keeps 3 KB fp32 sums, finished with wave_sum and stored by lane 0.
// Light: kFloats (floats of a light in `lights`), kPositions (whether factor reads x: `positions` is not touched otherwise),
// load(const float*) and factor(nx, ny, nz, x, y, z) -> the fp32 factor, formed in fp64 and rounded once.
template <int KB, typename Light>
__global__ __launch_bounds__(256) void ray_transfer_kernel(const float* __restrict__ positions, const float* __restrict__ albedo,
                                                           const float* __restrict__ normals, const float* __restrict__ weights,
                                                           const float* __restrict__ lights, int64_t R, int S, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Light light[KB];  // (uniform: scalar registers)
#pragma unroll
  for (int k = 0; k < KB; ++k) light[k].load(lights + k * Light::kFloats);
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < R; r += (int64_t)gridDim.x * 4) {
    float a[KB][3];
#pragma unroll
    for (int k = 0; k < KB; ++k) a[k][0] = a[k][1] = a[k][2] = 0.0f;
    for (int s = lane; s < S; s += 64) {
      const int64_t i = r * S + s, o = i * 3;
      const float w = weights[i];
      const float g0 = w * albedo[o], g1 = w * albedo[o + 1], g2 = w * albedo[o + 2];
      const double nx = normals[o], ny = normals[o + 1], nz = normals[o + 2];
      double x = 0.0, y = 0.0, z = 0.0;
      if constexpr (Light::kPositions) x = positions[o], y = positions[o + 1], z = positions[o + 2];
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const float factor = light[k].factor(nx, ny, nz, x, y, z);
        a[k][0] = fmaf(g0, factor, a[k][0]);
        a[k][1] = fmaf(g1, factor, a[k][1]);
        a[k][2] = fmaf(g2, factor, a[k][2]);
      }
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a[k][c] = wave_sum(a[k][c]);
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const int64_t o = ((int64_t)k * R + r) * 3;
        out[o] = a[k][0];
        out[o + 1] = a[k][1];
        out[o + 2] = a[k][2];
      }
    }
  }
}

// out [K][R][3] under the K lights of `lights`, up to 8 a pass; `name`: the entry point, for its launch error
template <typename Light>
int launch_ray_transfer(const char* name, const float* positions, const float* albedo, const float* normals, const float* weights,
                        const float* lights, int64_t R, int S, int K, float* out, hipStream_t st) {
  return for_each_pass<8>(K, [&](int k0, auto kb) {
    hipLaunchKernelGGL((ray_transfer_kernel<decltype(kb)::value, Light>), dim3(capped_grid((R + 3) / 4, 8)), dim3(256), 0, st, positions, albedo,
                       normals, weights, lights + (int64_t)k0 * Light::kFloats, R, S, out + (int64_t)k0 * R * 3);
    NSKY_CHECK_LAUNCH(name);
    return NSKY_OK;
  });
}
