// Sphere-traced shadow rays through the SDF (neusky_amd/relight/shadows.py).  Definitions and the march rule: include/neusky_hip.h.
//
// The march is a host loop of N rounds: the field evaluates the sdf at every ray's point (hash encode + sdf value chain, existing
// kernels), then `step` applies the rule to all T rays and writes the next points.  The shape is static, so the loop captures in a graph.
//   state      fp32 [6][T], one plane each: the start point x (3), t, m, and a flag word (int32 bits: the status, 0x100 = outside).
//              Structure of arrays: lane l of a wave touches element l of each plane.
//   begin      one thread per ray: x = o + depth d + bias n^ (or the given start point), t = 0, m = 1, ALIVE unless |x| >= radius.
//   step       one thread per ray, or per 4 consecutive rays with 16-byte accesses when T % 4 == 0 and every pointer is 16-byte aligned
//              (28 bytes read and 24 written per ray either way).  Every ray's point is rewritten as fma(t, s, x): a dead ray's t no
//              longer changes, so it keeps its last point to the bit.
//   step_bounded  the step of rays that end at a light (csrc/lights.hip): a direction, a t_end and a tan_half of each ray's own.
//   finish     state -> vis = m, status (int8; ALIVE -> EXHAUSTED), t.
// No atomics, no reductions: every output is bitwise repeatable.  Flat indices are 64-bit.  Nothing here synchronises with the host.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr int kOutside = 0x100, kStatusMask = 0xff;
enum { P_EPS = 0, P_RELAX, P_MIN_STEP, P_TAN_HALF, P_RADIUS, P_BIAS };

struct Params {
  float eps, relax, min_step, tan_half, radius2;
};

__device__ __forceinline__ Params load_params(const float* __restrict__ p) {
  return {p[P_EPS], p[P_RELAX], p[P_MIN_STEP], p[P_TAN_HALF], p[P_RADIUS] * p[P_RADIUS]};
}

__device__ __forceinline__ bool beyond(float px, float py, float pz, float radius2) {
  return fmaf(pz, pz, fmaf(py, py, px * px)) >= radius2;
}

// o, d, n [R][3] and depth [R] (d, depth, n all NULL: o holds the start points); dirs [T / dir_div][3]: ray i has direction i / dir_div
// and start row i % R
__global__ __launch_bounds__(256) void begin_kernel(const float* __restrict__ o, const float* __restrict__ d, const float* __restrict__ depth,
                                                    const float* __restrict__ n, const float* __restrict__ dirs, int64_t R, int64_t T,
                                                    int64_t dir_div, const float* __restrict__ params, float* __restrict__ state,
                                                    float* __restrict__ points) {
  const float radius2 = params[P_RADIUS] * params[P_RADIUS], bias = params[P_BIAS];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i % R * 3, k = i / dir_div * 3;
    float x = o[r], y = o[r + 1], z = o[r + 2];
    if (d) {
      const float t = depth[i % R];
      float nx = n[r], ny = n[r + 1], nz = n[r + 2];
      // (normalised in fp64, once per ray: n^ is then the rounding of the unit normal, and x within 1.5 ulp of its largest term)
      const double nn = (double)nx * nx + (double)ny * ny + (double)nz * nz;
      if (nn > 0.0 && nn < (double)INFINITY) {
        const double inv = 1.0 / sqrt(nn);
        nx = (float)(nx * inv), ny = (float)(ny * inv), nz = (float)(nz * inv);
      } else {  // no rendered normal: lift the point towards the light
        nx = dirs[k], ny = dirs[k + 1], nz = dirs[k + 2];
      }
      x = fmaf(bias, nx, fmaf(t, d[r], x));
      y = fmaf(bias, ny, fmaf(t, d[r + 1], y));
      z = fmaf(bias, nz, fmaf(t, d[r + 2], z));
    }
    state[i] = x;
    state[T + i] = y;
    state[2 * T + i] = z;
    state[3 * T + i] = 0.0f;
    state[4 * T + i] = 1.0f;
    reinterpret_cast<int32_t*>(state)[5 * T + i] = beyond(x, y, z, radius2) ? NSKY_TRACE_ESCAPED : NSKY_TRACE_ALIVE;
    points[i * 3] = x;
    points[i * 3 + 1] = y;
    points[i * 3 + 2] = z;
  }
}

// rule steps 3-6 of round `it` for the sdf f at the ray's point, then the next point and rule step 1 of round it + 1 (no round follows
// the last one: a ray alive after it is exhausted, wherever its next point would lie)
// BOUNDED (a ray towards a light inside the scene, csrc/lights.hip): the ray also ends at t_end, and its penumbra has a width of its own
template <bool BOUNDED = false>
__device__ __forceinline__ void march_ray(const Params& P, float f, float x, float y, float z, float sx, float sy, float sz, int it, int steps,
                                          int grace, float& t, float& m, int& flags, float& px, float& py, float& pz, float t_end = 0.0f,
                                          float ray_tan_half = 0.0f) {
  const float tan_half = BOUNDED ? ray_tan_half : P.tan_half;
  if ((flags & kStatusMask) == NSKY_TRACE_ALIVE) {
    if (f >= P.eps) flags |= kOutside;
    const bool outside = (flags & kOutside) != 0;
    if (f < P.eps && (outside || it >= grace)) {
      flags = (flags & ~kStatusMask) | NSKY_TRACE_HIT;
      m = 0.0f;
    } else {
      if (outside && tan_half > 0.0f && t > 0.0f) m = fminf(m, fminf(fmaxf(f / (t * tan_half), 0.0f), 1.0f));
      t += fmaxf(fabsf(f) * P.relax, P.min_step);
    }
  }
  px = fmaf(t, sx, x);
  py = fmaf(t, sy, y);
  pz = fmaf(t, sz, z);
  bool leaves = beyond(px, py, pz, P.radius2);
  if constexpr (BOUNDED) leaves = leaves || t >= t_end;
  if ((flags & kStatusMask) == NSKY_TRACE_ALIVE && it + 1 < steps && leaves) flags = (flags & ~kStatusMask) | NSKY_TRACE_ESCAPED;
}

template <int V>
__global__ __launch_bounds__(256) void step_kernel(float* __restrict__ state, const float* __restrict__ sdf, const float* __restrict__ dirs,
                                                   int64_t T, int64_t dir_div, const float* __restrict__ params, int it, int steps, int grace,
                                                   float* __restrict__ points) {
  const Params P = load_params(params);
  const int64_t groups = T / V;  // (V == 4: T % 4 == 0)
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t i = g * V;
    alignas(16) float x[V], y[V], z[V], t[V], m[V], f[V], p[3 * V];
    alignas(16) int flags[V];
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(x) = *reinterpret_cast<const float4*>(state + i);
      *reinterpret_cast<float4*>(y) = *reinterpret_cast<const float4*>(state + T + i);
      *reinterpret_cast<float4*>(z) = *reinterpret_cast<const float4*>(state + 2 * T + i);
      *reinterpret_cast<float4*>(t) = *reinterpret_cast<const float4*>(state + 3 * T + i);
      *reinterpret_cast<float4*>(m) = *reinterpret_cast<const float4*>(state + 4 * T + i);
      *reinterpret_cast<int4*>(flags) = *reinterpret_cast<const int4*>(state + 5 * T + i);
      *reinterpret_cast<float4*>(f) = *reinterpret_cast<const float4*>(sdf + i);
    } else {
      x[0] = state[i], y[0] = state[T + i], z[0] = state[2 * T + i], t[0] = state[3 * T + i], m[0] = state[4 * T + i];
      flags[0] = reinterpret_cast<const int32_t*>(state)[5 * T + i];
      f[0] = sdf[i];
    }
    int64_t row = i / dir_div, left = dir_div - (i - row * dir_div);  // one division for the V rays: `left` of them still share `row`
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int64_t k = row * 3;
      if (--left == 0) ++row, left = dir_div;
      march_ray(P, f[v], x[v], y[v], z[v], dirs[k], dirs[k + 1], dirs[k + 2], it, steps, grace, t[v], m[v], flags[v], p[3 * v], p[3 * v + 1],
                p[3 * v + 2]);
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(state + 3 * T + i) = *reinterpret_cast<const float4*>(t);
      *reinterpret_cast<float4*>(state + 4 * T + i) = *reinterpret_cast<const float4*>(m);
      *reinterpret_cast<int4*>(state + 5 * T + i) = *reinterpret_cast<const int4*>(flags);
      float4* out = reinterpret_cast<float4*>(points + i * 3);
      out[0] = *reinterpret_cast<const float4*>(p);
      out[1] = *reinterpret_cast<const float4*>(p + 4);
      out[2] = *reinterpret_cast<const float4*>(p + 8);
    } else {
      state[3 * T + i] = t[0], state[4 * T + i] = m[0];
      reinterpret_cast<int32_t*>(state)[5 * T + i] = flags[0];
      points[i * 3] = p[0], points[i * 3 + 1] = p[1], points[i * 3 + 2] = p[2];
    }
  }
}

// the step of rays that end at a light: direction row i of ray i, bounds [2][T] = t_end, tan_half (nsky_light_trace_begin)
template <int V>
__global__ __launch_bounds__(256) void step_bounded_kernel(float* __restrict__ state, const float* __restrict__ sdf,
                                                           const float* __restrict__ dirs, const float* __restrict__ bounds, int64_t T,
                                                           const float* __restrict__ params, int it, int steps, int grace,
                                                           float* __restrict__ points) {
  const Params P = load_params(params);
  const int64_t groups = T / V;  // (V == 4: T % 4 == 0)
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t i = g * V;
    alignas(16) float x[V], y[V], z[V], t[V], m[V], f[V], te[V], th[V], s[3 * V], p[3 * V];
    alignas(16) int flags[V];
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(x) = *reinterpret_cast<const float4*>(state + i);
      *reinterpret_cast<float4*>(y) = *reinterpret_cast<const float4*>(state + T + i);
      *reinterpret_cast<float4*>(z) = *reinterpret_cast<const float4*>(state + 2 * T + i);
      *reinterpret_cast<float4*>(t) = *reinterpret_cast<const float4*>(state + 3 * T + i);
      *reinterpret_cast<float4*>(m) = *reinterpret_cast<const float4*>(state + 4 * T + i);
      *reinterpret_cast<int4*>(flags) = *reinterpret_cast<const int4*>(state + 5 * T + i);
      *reinterpret_cast<float4*>(f) = *reinterpret_cast<const float4*>(sdf + i);
      *reinterpret_cast<float4*>(te) = *reinterpret_cast<const float4*>(bounds + i);
      *reinterpret_cast<float4*>(th) = *reinterpret_cast<const float4*>(bounds + T + i);
      const float4* in = reinterpret_cast<const float4*>(dirs + i * 3);
      *reinterpret_cast<float4*>(s) = in[0];
      *reinterpret_cast<float4*>(s + 4) = in[1];
      *reinterpret_cast<float4*>(s + 8) = in[2];
    } else {
      x[0] = state[i], y[0] = state[T + i], z[0] = state[2 * T + i], t[0] = state[3 * T + i], m[0] = state[4 * T + i];
      flags[0] = reinterpret_cast<const int32_t*>(state)[5 * T + i];
      f[0] = sdf[i], te[0] = bounds[i], th[0] = bounds[T + i];
      s[0] = dirs[i * 3], s[1] = dirs[i * 3 + 1], s[2] = dirs[i * 3 + 2];
    }
#pragma unroll
    for (int v = 0; v < V; ++v)
      march_ray<true>(P, f[v], x[v], y[v], z[v], s[3 * v], s[3 * v + 1], s[3 * v + 2], it, steps, grace, t[v], m[v], flags[v], p[3 * v],
                      p[3 * v + 1], p[3 * v + 2], te[v], th[v]);
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(state + 3 * T + i) = *reinterpret_cast<const float4*>(t);
      *reinterpret_cast<float4*>(state + 4 * T + i) = *reinterpret_cast<const float4*>(m);
      *reinterpret_cast<int4*>(state + 5 * T + i) = *reinterpret_cast<const int4*>(flags);
      float4* out = reinterpret_cast<float4*>(points + i * 3);
      out[0] = *reinterpret_cast<const float4*>(p);
      out[1] = *reinterpret_cast<const float4*>(p + 4);
      out[2] = *reinterpret_cast<const float4*>(p + 8);
    } else {
      state[3 * T + i] = t[0], state[4 * T + i] = m[0];
      reinterpret_cast<int32_t*>(state)[5 * T + i] = flags[0];
      points[i * 3] = p[0], points[i * 3 + 1] = p[1], points[i * 3 + 2] = p[2];
    }
  }
}

template <int V>
__global__ __launch_bounds__(256) void finish_kernel(const float* __restrict__ state, int64_t T, float* __restrict__ vis,
                                                     int8_t* __restrict__ status, float* __restrict__ t_out) {
  const int64_t groups = T / V;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t i = g * V;
    if constexpr (V == 4) {
      const int4 fl = *reinterpret_cast<const int4*>(state + 5 * T + i);
      *reinterpret_cast<float4*>(vis + i) = *reinterpret_cast<const float4*>(state + 4 * T + i);
      *reinterpret_cast<float4*>(t_out + i) = *reinterpret_cast<const float4*>(state + 3 * T + i);
      const int s[4] = {fl.x & kStatusMask, fl.y & kStatusMask, fl.z & kStatusMask, fl.w & kStatusMask};
      uint32_t packed = 0;
#pragma unroll
      for (int v = 0; v < 4; ++v) packed |= (uint32_t)(s[v] == NSKY_TRACE_ALIVE ? NSKY_TRACE_EXHAUSTED : s[v]) << (8 * v);
      *reinterpret_cast<uint32_t*>(status + i) = packed;
    } else {
      const int s = reinterpret_cast<const int32_t*>(state)[5 * T + i] & kStatusMask;
      vis[i] = state[4 * T + i];
      t_out[i] = state[3 * T + i];
      status[i] = (int8_t)(s == NSKY_TRACE_ALIVE ? NSKY_TRACE_EXHAUSTED : s);
    }
  }
}

unsigned grid_for(int64_t threads) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((threads + 255) / 256, 256 * 8)); }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int launch_begin(const char* name, const float* o, const float* d, const float* depth, const float* n, const float* dirs, int64_t R, int64_t T,
                 int64_t dir_div, const float* params, float* state, float* points, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && T >= 0 && dir_div >= 1, "%s: R %ld, T %ld, dir_div %ld", name, (long)R, (long)T, (long)dir_div);
  if (T == 0) return NSKY_OK;
  NSKY_CHECK_ARG(R >= 1 && T % R == 0, "%s: T %ld is no multiple of R %ld", name, (long)T, (long)R);
  NSKY_CHECK_ARG(o && dirs && params && state && points, "%s: NULL origins / directions / params / state / points", name);
  hipLaunchKernelGGL(begin_kernel, dim3(grid_for(T)), dim3(256), 0, (hipStream_t)stream, o, d, depth, n, dirs, R, T, dir_div, params, state,
                     points);
  NSKY_CHECK_LAUNCH(name);
  return NSKY_OK;
}

}  // namespace

extern "C" int nsky_sphere_trace_begin(const float* origins, const float* directions, const float* depth, const float* normals,
                                       const float* suns, int64_t R, int32_t K, const float* params, float* state, float* points,
                                       nsky_stream_t stream) {
  NSKY_CHECK_ARG(K >= 0, "nsky_sphere_trace_begin: K %d", (int)K);
  NSKY_CHECK_ARG(R == 0 || K == 0 || (directions && depth && normals), "nsky_sphere_trace_begin: NULL directions / depth / normals");
  return launch_begin("nsky_sphere_trace_begin", origins, directions, depth, normals, suns, R, (int64_t)K * R, std::max<int64_t>(R, 1), params,
                      state, points, stream);
}

extern "C" int nsky_sphere_trace_begin_points(const float* starts, const float* directions, int64_t M, int64_t T, int64_t dir_div,
                                              const float* params, float* state, float* points, nsky_stream_t stream) {
  return launch_begin("nsky_sphere_trace_begin_points", starts, nullptr, nullptr, nullptr, directions, M, T, dir_div, params, state, points,
                      stream);
}

extern "C" int nsky_sphere_trace_step(float* state, const float* sdf, const float* directions, int64_t T, int64_t dir_div, const float* params,
                                      int32_t iteration, int32_t steps, int32_t grace, float* points, nsky_stream_t stream) {
  NSKY_CHECK_ARG(T >= 0 && dir_div >= 1 && iteration >= 0 && iteration < steps && grace >= 0,
                 "nsky_sphere_trace_step: T %ld, dir_div %ld, iteration %d of %d, grace %d", (long)T, (long)dir_div, (int)iteration, (int)steps,
                 (int)grace);
  if (T == 0) return NSKY_OK;
  NSKY_CHECK_ARG(state && sdf && directions && params && points, "nsky_sphere_trace_step: NULL state / sdf / directions / params / points");
  hipStream_t st = (hipStream_t)stream;
  if (T % 4 == 0 && aligned16(state) && aligned16(sdf) && aligned16(points))
    hipLaunchKernelGGL(step_kernel<4>, dim3(grid_for(T / 4)), dim3(256), 0, st, state, sdf, directions, T, dir_div, params, (int)iteration,
                       (int)steps, (int)grace, points);
  else
    hipLaunchKernelGGL(step_kernel<1>, dim3(grid_for(T)), dim3(256), 0, st, state, sdf, directions, T, dir_div, params, (int)iteration,
                       (int)steps, (int)grace, points);
  NSKY_CHECK_LAUNCH("nsky_sphere_trace_step");
  return NSKY_OK;
}

extern "C" int nsky_sphere_trace_step_bounded(float* state, const float* sdf, const float* ray_dirs, const float* bounds, int64_t T,
                                              const float* params, int32_t iteration, int32_t steps, int32_t grace, float* points,
                                              nsky_stream_t stream) {
  NSKY_CHECK_ARG(T >= 0 && iteration >= 0 && iteration < steps && grace >= 0, "nsky_sphere_trace_step_bounded: T %ld, iteration %d of %d, grace %d",
                 (long)T, (int)iteration, (int)steps, (int)grace);
  if (T == 0) return NSKY_OK;
  NSKY_CHECK_ARG(state && sdf && ray_dirs && bounds && params && points,
                 "nsky_sphere_trace_step_bounded: NULL state / sdf / ray_dirs / bounds / params / points");
  hipStream_t st = (hipStream_t)stream;
  if (T % 4 == 0 && aligned16(state) && aligned16(sdf) && aligned16(points) && aligned16(ray_dirs) && aligned16(bounds))
    hipLaunchKernelGGL(step_bounded_kernel<4>, dim3(grid_for(T / 4)), dim3(256), 0, st, state, sdf, ray_dirs, bounds, T, params, (int)iteration,
                       (int)steps, (int)grace, points);
  else
    hipLaunchKernelGGL(step_bounded_kernel<1>, dim3(grid_for(T)), dim3(256), 0, st, state, sdf, ray_dirs, bounds, T, params, (int)iteration,
                       (int)steps, (int)grace, points);
  NSKY_CHECK_LAUNCH("nsky_sphere_trace_step_bounded");
  return NSKY_OK;
}

extern "C" int nsky_sphere_trace_finish(const float* state, int64_t T, float* vis, int8_t* status, float* t, nsky_stream_t stream) {
  NSKY_CHECK_ARG(T >= 0, "nsky_sphere_trace_finish: T %ld", (long)T);
  if (T == 0) return NSKY_OK;
  NSKY_CHECK_ARG(state && vis && status && t, "nsky_sphere_trace_finish: NULL state / vis / status / t");
  hipStream_t st = (hipStream_t)stream;
  if (T % 4 == 0 && aligned16(state) && aligned16(vis) && aligned16(status) && aligned16(t))
    hipLaunchKernelGGL(finish_kernel<4>, dim3(grid_for(T / 4)), dim3(256), 0, st, state, T, vis, status, t);
  else
    hipLaunchKernelGGL(finish_kernel<1>, dim3(grid_for(T)), dim3(256), 0, st, state, T, vis, status, t);
  NSKY_CHECK_LAUNCH("nsky_sphere_trace_finish");
  return NSKY_OK;
}
