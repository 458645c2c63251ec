// Sphere-traced shadow rays through the SDF (neusky_amd/relight/shadows.py).  Definitions and the march rule: include/neusky_hip.h.
//
// The march is a host loop of N rounds: the field evaluates the sdf at every ray's point (hash encode + sdf value chain, existing
// kernels), then `step` applies the rule to all T rays and writes the next points.  The shape is static, so the loop captures in a graph.
//   state      fp32 [6][T] (csrc/trace.h, with what csrc/lights.hip shares: the start point of a ray and the store of a begun one).
//   begin      one thread per ray: x = o + depth d + bias n^ (or the given start point), t = 0, m = 1, ALIVE unless |x| >= radius.
//   step       one kernel, one thread per ray, or per 4 consecutive rays with 16-byte accesses when T % 4 == 0 and every pointer is 16-byte
//              aligned (28 bytes read and 24 written per ray either way).  Every ray's point is rewritten as fma(t, s, x): a dead ray's t
//              no longer changes, so it keeps its last point to the bit.  With `bounds` it is the step of rays that end at a light
//              (csrc/lights.hip): a direction row, a t_end and a tan_half of each ray's own, 20 more bytes read per ray.
//   finish     state -> vis = m, status (int8; ALIVE -> EXHAUSTED), t.
// No atomics, no reductions: every output is bitwise repeatable.  Flat indices are 64-bit.  Nothing here synchronises with the host.
#include <cstdint>

#include "trace.h"

namespace {

struct Params {
  float eps, relax, min_step, tan_half, radius2;
};

__device__ __forceinline__ Params load_params(const float* __restrict__ p) {
  return {p[P_EPS], p[P_RELAX], p[P_MIN_STEP], p[P_TAN_HALF], p[P_RADIUS] * p[P_RADIUS]};
}

// o, d, n [R][3] and depth [R] (d, depth, n all NULL: o holds the start points); dirs [T / dir_div][3]: ray i has direction i / dir_div
// and start row i % R
__global__ __launch_bounds__(256) void begin_kernel(const float* __restrict__ o, const float* __restrict__ d, const float* __restrict__ depth,
                                                    const float* __restrict__ n, const float* __restrict__ dirs, int64_t R, int64_t T,
                                                    int64_t dir_div, const float* __restrict__ params, float* __restrict__ state,
                                                    float* __restrict__ points) {
  const float radius2 = params[P_RADIUS] * params[P_RADIUS], bias = params[P_BIAS];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i % R * 3;
    const float* s = dirs + i / dir_div * 3;
    float x = o[r], y = o[r + 1], z = o[r + 2];
    if (d)  // (no rendered normal: the point is lifted along the sun's direction)
      lifted_start(o + r, d + r, depth[i % R], n + r, bias,
                   [s](float, float, float, float& nx, float& ny, float& nz) { nx = s[0], ny = s[1], nz = s[2]; }, x, y, z);
    store_begun(state, points, T, i, x, y, z, radius2);
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

// one round for V consecutive rays.  Unbounded: ray i has direction row i / dir_div.  BOUNDED (rays that end at a light): direction row i
// of ray i, read as the points are written, and bounds [2][T] = t_end, tan_half (nsky_light_trace_begin)
template <int V, bool BOUNDED>
__global__ __launch_bounds__(256) void step_kernel(float* __restrict__ state, const float* __restrict__ sdf, const float* __restrict__ dirs,
                                                   const float* __restrict__ bounds, int64_t T, int64_t dir_div,
                                                   const float* __restrict__ params, int it, int steps, int grace,
                                                   float* __restrict__ points) {
  const Params P = load_params(params);
  const int64_t groups = T / V;  // (V == 4: T % 4 == 0)
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t i = g * V;
    Rays<V> r;
    alignas(16) float f[V], p[3 * V];
    load_rays<V>(state, T, i, r);
    load_v<V>(f, sdf + i);
    if constexpr (BOUNDED) {
      alignas(16) float te[V], th[V], s[3 * V];
      load_v<V>(te, bounds + i);
      load_v<V>(th, bounds + T + i);
      load_rows<V>(s, dirs + i * 3);
#pragma unroll
      for (int v = 0; v < V; ++v)
        march_ray<true>(P, f[v], r.x[v], r.y[v], r.z[v], s[3 * v], s[3 * v + 1], s[3 * v + 2], it, steps, grace, r.t[v], r.m[v], r.flags[v],
                        p[3 * v], p[3 * v + 1], p[3 * v + 2], te[v], th[v]);
    } else {
      int64_t row = i / dir_div, left = dir_div - (i - row * dir_div);  // one division for the V rays: `left` of them still share `row`
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int64_t k = row * 3;
        if (--left == 0) ++row, left = dir_div;
        march_ray(P, f[v], r.x[v], r.y[v], r.z[v], dirs[k], dirs[k + 1], dirs[k + 2], it, steps, grace, r.t[v], r.m[v], r.flags[v], p[3 * v],
                  p[3 * v + 1], p[3 * v + 2]);
      }
    }
    store_marching<V>(state, T, i, r);
    store_rows<V>(points + i * 3, p);
  }
}

template <int V>
__global__ __launch_bounds__(256) void finish_kernel(const float* __restrict__ state, int64_t T, float* __restrict__ vis,
                                                     int8_t* __restrict__ status, float* __restrict__ t_out) {
  const int64_t groups = T / V;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t i = g * V;
    Rays<V> r;
    load_marching<V>(state, T, i, r);
    store_v<V>(vis + i, r.m);
    store_v<V>(t_out + i, r.t);
    uint32_t packed = 0;  // V statuses, one byte each
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int s = r.flags[v] & kStatusMask;
      packed |= (uint32_t)(s == NSKY_TRACE_ALIVE ? NSKY_TRACE_EXHAUSTED : s) << (8 * v);
    }
    if constexpr (V == 4)
      *reinterpret_cast<uint32_t*>(status + i) = packed;
    else
      status[i] = (int8_t)packed;
  }
}

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

extern "C" int nsky_sphere_trace_step(float* state, const float* sdf, const float* directions, const float* bounds, int64_t T, int64_t dir_div,
                                      const float* params, int32_t iteration, int32_t steps, int32_t grace, float* points,
                                      nsky_stream_t stream) {
  NSKY_CHECK_ARG(T >= 0 && dir_div >= 1 && iteration >= 0 && iteration < steps && grace >= 0,
                 "nsky_sphere_trace_step: T %ld, dir_div %ld, iteration %d of %d, grace %d", (long)T, (long)dir_div, (int)iteration, (int)steps,
                 (int)grace);
  NSKY_CHECK_ARG(!bounds || dir_div == 1, "nsky_sphere_trace_step: bounds go with a direction of each ray's own, got dir_div %ld", (long)dir_div);
  if (T == 0) return NSKY_OK;
  NSKY_CHECK_ARG(state && sdf && directions && params && points, "nsky_sphere_trace_step: NULL state / sdf / directions / params / points");
  const bool wide = T % 4 == 0 && aligned16(state) && aligned16(sdf) && aligned16(points) && (!bounds || (aligned16(directions) && aligned16(bounds)));
  const auto kernel = bounds ? (wide ? step_kernel<4, true> : step_kernel<1, true>) : (wide ? step_kernel<4, false> : step_kernel<1, false>);
  hipLaunchKernelGGL(kernel, dim3(grid_for(wide ? T / 4 : T)), dim3(256), 0, (hipStream_t)stream, state, sdf, directions, bounds, T, dir_div,
                     params, (int)iteration, (int)steps, (int)grace, points);
  NSKY_CHECK_LAUNCH("nsky_sphere_trace_step");
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
