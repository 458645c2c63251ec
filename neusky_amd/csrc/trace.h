// What the kernels of a shadow march share (csrc/sphere_trace.hip: the march; csrc/lights.hip: the begin of rays that end at a lamp), each
// piece exactly once: the layout of the state and of the parameter block, the start point of a ray off a rendered surface, the store of
// a begun ray and the V-wide accesses of the march.  Definitions and the march rule: include/neusky_hip.h.
//   state   fp32 [6][T], one plane each: the start point x (3), t, m, and a flag word (int32 bits: the status, 0x100 = outside).
//           Structure of arrays: lane l of a wave touches element l of each plane.
//   params  fp32 [6] in device memory: eps, relax, min_step, tan_half, radius, bias.
#pragma once
#include <algorithm>

#include "common.h"
#include "../../include/neusky_hip.h"

enum { S_X = 0, S_Y, S_Z, S_T, S_M, S_FLAGS };  // the state's planes
constexpr int kOutside = 0x100, kStatusMask = 0xff;
enum { P_EPS = 0, P_RELAX, P_MIN_STEP, P_TAN_HALF, P_RADIUS, P_BIAS };

static inline unsigned grid_for(int64_t threads) { return capped_grid((threads + 255) / 256, 8); }

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ bool beyond(float px, float py, float pz, float radius2) {
  return fmaf(pz, pz, fmaf(py, py, px * px)) >= radius2;
}

// the start point of a shadow ray off a rendered surface: o + depth d, lifted `bias` along the unit normal.  o, d, n: the ray's rows.
// The normal is normalised in fp64, once per ray: n^ is then the rounding of the unit normal, and x within 1.5 ulp of its largest
// term.  No rendered normal (zero or non-finite length): the lift is along fallback(x, y, z, nx, ny, nz), the caller's unit vector
// towards its light from the unlifted point.
template <typename Fallback>
__device__ __forceinline__ void lifted_start(const float* __restrict__ o, const float* __restrict__ d, float depth,
                                             const float* __restrict__ n, float bias, Fallback fallback, float& x, float& y, float& z) {
  x = fmaf(depth, d[0], o[0]), y = fmaf(depth, d[1], o[1]), z = fmaf(depth, d[2], o[2]);
  float nx = n[0], ny = n[1], nz = n[2];
  const double nn = (double)nx * nx + (double)ny * ny + (double)nz * nz;
  if (nn > 0.0 && nn < (double)INFINITY) {
    const double inv = 1.0 / sqrt(nn);
    nx = (float)(nx * inv), ny = (float)(ny * inv), nz = (float)(nz * inv);
  } else {
    fallback(x, y, z, nx, ny, nz);
  }
  x = fmaf(bias, nx, x), y = fmaf(bias, ny, y), z = fmaf(bias, nz, z);
}

// ray i of T begun at x: the six planes, its first point, and rule step 1 of iteration 0 (t = 0: the ray starts beyond the radius, or
// has `ended` by a rule of its caller's)
__device__ __forceinline__ void store_begun(float* __restrict__ state, float* __restrict__ points, int64_t T, int64_t i, float x, float y,
                                            float z, float radius2, bool ended = false) {
  state[S_X * T + i] = x;
  state[S_Y * T + i] = y;
  state[S_Z * T + i] = z;
  state[S_T * T + i] = 0.0f;
  state[S_M * T + i] = 1.0f;
  reinterpret_cast<int32_t*>(state)[S_FLAGS * T + i] = ended || beyond(x, y, z, radius2) ? NSKY_TRACE_ESCAPED : NSKY_TRACE_ALIVE;
  points[i * 3] = x;
  points[i * 3 + 1] = y;
  points[i * 3 + 2] = z;
}

// V consecutive elements as one access: 16 bytes when V == 4 (both addresses 16-byte aligned), 4 bytes when V == 1
template <int V, typename E> struct Wide { using type = E; };
template <> struct Wide<4, float> { using type = float4; };
template <> struct Wide<4, int32_t> { using type = int4; };

template <int V, typename E>
__device__ __forceinline__ void load_v(E* dst, const E* __restrict__ src) {
  using W = typename Wide<V, E>::type;
  *reinterpret_cast<W*>(dst) = *reinterpret_cast<const W*>(src);
}

template <int V, typename E>
__device__ __forceinline__ void store_v(E* __restrict__ dst, const E* src) {
  using W = typename Wide<V, E>::type;
  *reinterpret_cast<W*>(dst) = *reinterpret_cast<const W*>(src);
}

// V rows of [.][3], 3 V consecutive floats, as three accesses
template <int V>
__device__ __forceinline__ void load_rows(float* dst, const float* __restrict__ src) {
#pragma unroll
  for (int j = 0; j < 3; ++j) load_v<V>(dst + j * V, src + j * V);
}

template <int V>
__device__ __forceinline__ void store_rows(float* __restrict__ dst, const float* src) {
#pragma unroll
  for (int j = 0; j < 3; ++j) store_v<V>(dst + j * V, src + j * V);
}

// V consecutive rays of the state in registers
template <int V>
struct Rays {
  alignas(16) float x[V], y[V], z[V], t[V], m[V];
  alignas(16) int32_t flags[V];
};

// what a march reads of rays i .. i + V - 1, and what it writes back: a ray's start point never changes
template <int V>
__device__ __forceinline__ void load_marching(const float* __restrict__ state, int64_t T, int64_t i, Rays<V>& r) {
  load_v<V>(r.t, state + S_T * T + i);
  load_v<V>(r.m, state + S_M * T + i);
  load_v<V>(r.flags, reinterpret_cast<const int32_t*>(state) + S_FLAGS * T + i);
}

template <int V>
__device__ __forceinline__ void load_rays(const float* __restrict__ state, int64_t T, int64_t i, Rays<V>& r) {
  load_v<V>(r.x, state + S_X * T + i);
  load_v<V>(r.y, state + S_Y * T + i);
  load_v<V>(r.z, state + S_Z * T + i);
  load_marching<V>(state, T, i, r);
}

template <int V>
__device__ __forceinline__ void store_marching(float* __restrict__ state, int64_t T, int64_t i, const Rays<V>& r) {
  store_v<V>(state + S_T * T + i, r.t);
  store_v<V>(state + S_M * T + i, r.m);
  store_v<V>(reinterpret_cast<int32_t*>(state) + S_FLAGS * T + i, r.flags);
}
