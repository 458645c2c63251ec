// Point and spot lights inside the scene (neusky_amd/relight/lights.py).  Definitions: include/neusky_hip.h.
//
// A sun is one direction for all samples of all rays; a lamp has a direction and a distance of its own at every sample:
//   t[l,r,c]   = sum_s w[r,s] alb[r,s,c] clamp(n[r,s].u, 0, 1) spot(-u.a_l) / max(|p_l - x[r,s]|^2, min_distance_l^2),  u = (p_l - x) / |p_l - x|
//   lin[k,r,c] = base[k,r,c] + sum_l I[l,c] V[l,r] t[l,r,c]
//   lights     fp32 [L][16] in device memory: p (0..2), a (3..5), cos_inner, cos_outer, rho, clearance, min_distance, -, I (12..14), -
//   transfer   nsky_sun_transfer's kernel (ray_transfer_kernel, csrc/light_pass.h): a sample (40 bytes) is read once per pass and meets
//              up to 8 lights; the factor cosine spot / max(q, min_distance^2) is formed in fp64 (a square root and two divisions per
//              sample and light) and rounded once.
//   begin      one thread per shadow ray i = l R + r: the start point as nsky_sphere_trace_begin forms it, then the ray's own direction,
//              end and penumbra width in fp64, rounded once (the start point and the store of the begun ray: csrc/trace.h).  The march
//              itself is nsky_sphere_trace_step with these bounds (csrc/sphere_trace.hip).
//   composite  one thread per (ray, channel): the L terms in fp64, l ascending, added to each of the Kb base images with one rounding.
// No atomics, a fixed reduction order: two runs agree bit for bit.  Flat indices are 64-bit.  Nothing here synchronises with the host.
#include "light_pass.h"
#include "numerics.h"
#include "trace.h"

namespace {

constexpr int kLightStride = NSKY_LIGHT_FLOATS;
enum { L_P = 0, L_A = 3, L_COS_INNER = 6, L_COS_OUTER = 7, L_RHO = 8, L_CLEARANCE = 9, L_MIN_DISTANCE = 10, L_I = 12 };

// a lamp of the per-ray transfer sum (csrc/light_pass.h): cosine spot / max(q, min_distance^2) towards the lamp from the sample at x
struct Lamp {
  static constexpr int kFloats = kLightStride;
  static constexpr bool kPositions = true;
  double px, py, pz, ax, ay, az, ci, co, md2;
  __device__ __forceinline__ void load(const float* q) {
    px = q[L_P], py = q[L_P + 1], pz = q[L_P + 2];
    ax = q[L_A], ay = q[L_A + 1], az = q[L_A + 2];
    ci = q[L_COS_INNER], co = q[L_COS_OUTER];
    md2 = (double)q[L_MIN_DISTANCE] * (double)q[L_MIN_DISTANCE];
  }
  __device__ __forceinline__ float factor(double nx, double ny, double nz, double x, double y, double z) const {
    const double vx = px - x, vy = py - y, vz = pz - z;
    const double q = fma(vz, vz, fma(vy, vy, vx * vx));
    float factor = 0.0f;
    if (q > 0.0) {
      const double inv = 1.0 / sqrt(q);
      const double ux = vx * inv, uy = vy * inv, uz = vz * inv;
      const double cosine = fmin(fmax(fma(nz, uz, fma(ny, uy, nx * ux)), 0.0), 1.0);
      const double c = -fma(uz, az, fma(uy, ay, ux * ax));
      double spot = 1.0;
      if (!(c >= ci)) {
        if (c <= co) {
          spot = 0.0;
        } else {
          const double h = (c - co) / (ci - co);
          spot = h * h * (3.0 - 2.0 * h);
        }
      }
      factor = (float)(cosine * spot / fmax(q, md2));
    }
    return factor;
  }
};

// o, d, n [R][3] and depth [R] (d, depth, n all NULL: o holds the start points); ray i = l R + r
__global__ __launch_bounds__(256) void light_begin_kernel(const float* __restrict__ o, const float* __restrict__ d,
                                                          const float* __restrict__ depth, const float* __restrict__ n,
                                                          const float* __restrict__ lights, int64_t R, int64_t T,
                                                          const float* __restrict__ params, float* __restrict__ state,
                                                          float* __restrict__ points, float* __restrict__ ray_dirs,
                                                          float* __restrict__ bounds) {
  const float radius2 = params[P_RADIUS] * params[P_RADIUS], bias = params[P_BIAS];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
    const int64_t l = i / R, r = (i - l * R) * 3;
    const float* q = lights + l * kLightStride;
    const double lx = q[L_P], ly = q[L_P + 1], lz = q[L_P + 2];
    float x = o[r], y = o[r + 1], z = o[r + 2];
    if (d)  // (no rendered normal: the point is lifted towards the lamp)
      lifted_start(o + r, d + r, depth[i - l * R], n + r, bias, [=](float ux, float uy, float uz, float& nx, float& ny, float& nz) {
        const double wx = lx - ux, wy = ly - uy, wz = lz - uz;
        const double ww = wx * wx + wy * wy + wz * wz;
        if (ww > 0.0) {
          const double inv = 1.0 / sqrt(ww);
          nx = (float)(wx * inv), ny = (float)(wy * inv), nz = (float)(wz * inv);
        } else {
          nx = 0.0f, ny = 0.0f, nz = 1.0f;
        }
      }, x, y, z);
    const double vx = lx - x, vy = ly - y, vz = lz - z;
    const double len = sqrt(vx * vx + vy * vy + vz * vz);
    float sx = 0.0f, sy = 0.0f, sz = 1.0f, t_end = 0.0f, tan_half = 0.0f;
    if (len > 0.0) {
      sx = (float)(vx / len), sy = (float)(vy / len), sz = (float)(vz / len);
      t_end = (float)(len - (double)q[L_CLEARANCE]);
      tan_half = (float)((double)q[L_RHO] / len);
    }
    // rule step 1 of iteration 0, t = 0: the ray is at its light already, or starts beyond the radius
    store_begun(state, points, T, i, x, y, z, radius2, !(0.0f < t_end));
    ray_dirs[i * 3] = sx, ray_dirs[i * 3 + 1] = sy, ray_dirs[i * 3 + 2] = sz;
    bounds[i] = t_end;
    bounds[T + i] = tan_half;
  }
}

// element j of [R][3]; base_stride: floats between two base images: 0 for one base [R][3] under all Kb outputs, R 3 for [Kb][R][3]
__global__ __launch_bounds__(256) void lights_composite_kernel(const float* __restrict__ base, int64_t base_stride, const float* __restrict__ t,
                                                               const float* __restrict__ vis, const float* __restrict__ acc,
                                                               const float* __restrict__ acc_threshold, const float* __restrict__ lights,
                                                               int64_t R, int L, int Kb, float* __restrict__ rgb, float* __restrict__ lin,
                                                               float* __restrict__ light_lin, float* __restrict__ visibility) {
  const int64_t n = R * 3;
  const float thr = acc_threshold[0];
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const int64_t r = j / 3;
    const int c = (int)(j - r * 3);
    const bool on = acc[r] > thr;
    double e = 0.0;
    for (int l = 0; l < L; ++l) {
      const int64_t lr = (int64_t)l * R + r;
      const float v = on ? (vis ? vis[lr] : 1.0f) : 0.0f;
      e += (double)lights[l * kLightStride + L_I + c] * (double)v * (double)t[lr * 3 + c];
      if (visibility && c == 0) visibility[lr] = v;
    }
    if (light_lin) light_lin[j] = (float)e;
    for (int k = 0; k < Kb; ++k) {
      const float b = base[(int64_t)k * base_stride + j];
      const float x = e == 0.0 ? b : (float)((double)b + e);  // (no light: the base's bits, a -0 included)
      const int64_t i = (int64_t)k * n + j;
      if (lin) lin[i] = x;
      rgb[i] = srgb_fwd(x);
    }
  }
}

int launch_begin(const char* name, const float* o, const float* d, const float* depth, const float* n, const float* lights, int64_t R, int32_t L,
                 const float* params, float* state, float* points, float* ray_dirs, float* bounds, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && L >= 0, "%s: R %ld, L %d", name, (long)R, (int)L);
  const int64_t T = (int64_t)L * R;
  if (T == 0) return NSKY_OK;
  NSKY_CHECK_ARG(o && lights && params && state && points && ray_dirs && bounds,
                 "%s: NULL origins / lights / params / state / points / ray_dirs / bounds", name);
  hipLaunchKernelGGL(light_begin_kernel, dim3(grid_for(T)), dim3(256), 0, (hipStream_t)stream, o, d, depth, n, lights, R, T, params, state, points,
                     ray_dirs, bounds);
  NSKY_CHECK_LAUNCH(name);
  return NSKY_OK;
}

}  // namespace

extern "C" int nsky_light_transfer(const float* positions, const float* albedo, const float* normals, const float* weights,
                                   const float* lights, int64_t R, int32_t S, int32_t L, float* out, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && S >= 1 && L >= 0, "nsky_light_transfer: R %ld, S %d, L %d", (long)R, (int)S, (int)L);
  if (R == 0 || L == 0) return NSKY_OK;
  NSKY_CHECK_ARG(positions && albedo && normals && weights && lights && out,
                 "nsky_light_transfer: NULL positions / albedo / normals / weights / lights / out");
  return launch_ray_transfer<Lamp>("nsky_light_transfer", positions, albedo, normals, weights, lights, R, S, L, out, (hipStream_t)stream);
}

extern "C" int nsky_light_trace_begin(const float* origins, const float* directions, const float* depth, const float* normals,
                                      const float* lights, int64_t R, int32_t L, const float* params, float* state, float* points,
                                      float* ray_dirs, float* bounds, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R == 0 || L <= 0 || (directions && depth && normals), "nsky_light_trace_begin: NULL directions / depth / normals");
  return launch_begin("nsky_light_trace_begin", origins, directions, depth, normals, lights, R, L, params, state, points, ray_dirs, bounds,
                      stream);
}

extern "C" int nsky_light_trace_begin_points(const float* starts, const float* lights, int64_t M, int32_t L, const float* params, float* state,
                                             float* points, float* ray_dirs, float* bounds, nsky_stream_t stream) {
  return launch_begin("nsky_light_trace_begin_points", starts, nullptr, nullptr, nullptr, lights, M, L, params, state, points, ray_dirs, bounds,
                      stream);
}

extern "C" int nsky_lights_composite(const float* base, int64_t base_stride, const float* t, const float* vis, const float* acc,
                                     const float* acc_threshold, const float* lights, int64_t R, int32_t L, int32_t Kb, float* rgb, float* lin,
                                     float* light_lin, float* visibility, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && L >= 0 && Kb >= 0 && (base_stride == 0 || base_stride == R * 3), "nsky_lights_composite: R %ld, L %d, Kb %d, stride %ld",
                 (long)R, (int)L, (int)Kb, (long)base_stride);
  if (R == 0 || Kb == 0) return NSKY_OK;
  NSKY_CHECK_ARG(base && acc && acc_threshold && rgb && (L == 0 || (t && lights)),
                 "nsky_lights_composite: NULL base / t / acc / acc_threshold / lights / rgb");
  hipLaunchKernelGGL(lights_composite_kernel, dim3(grid_for(R * 3)), dim3(256), 0, (hipStream_t)stream, base, base_stride, t, vis, acc,
                     acc_threshold, lights, R, (int)L, (int)Kb, rgb, lin, light_lin, visibility);
  NSKY_CHECK_LAUNCH("nsky_lights_composite");
  return NSKY_OK;
}
