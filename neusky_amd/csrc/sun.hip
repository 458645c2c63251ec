// A directional sun on top of the hemisphere render (neusky_amd/relight/sun.py).  Definitions: include/neusky_hip.h.
//
// The frame render sees light as its D directions (one cell ~ 4 pi / D sr); a sun is one direction of its own:
//   t[k,r,c]   = sum_s w[r,s] alb[r,s,c] clamp(n[r,s].s_k, 0, 1)
//   lin[k,r,c] = lin_sky[r,c] + C[k,c] V[k,r] t[k,r,c]
//   transfer   ray_transfer_kernel (csrc/light_pass.h): a sample (28 bytes) is read once per pass and meets up to 8 suns; the cosine
//              itself is taken in fp64 (one rounding instead of three: a term is then within 3 2^-24 of its definition).
//   composite  one thread per output element: mask, set-sun rule, the sum in fp64 rounded once, the sRGB curve of numerics.h.
//              sky_stride = 3 R: lin_sky[k,r,c], a sky of each sun's own (relight/daylight.py).
// No atomics, a fixed reduction order: two runs agree bit for bit.  Flat indices are 64-bit.  Nothing here synchronises with the host.
#include "light_pass.h"
#include "numerics.h"
#include "../../include/neusky_hip.h"

namespace {

// a sun of the per-ray transfer sum (csrc/light_pass.h): its direction; the factor is the clamped cosine
struct Sun {
  static constexpr int kFloats = 3;
  static constexpr bool kPositions = false;
  double sx, sy, sz;
  __device__ __forceinline__ void load(const float* q) { sx = q[0], sy = q[1], sz = q[2]; }
  __device__ __forceinline__ float factor(double nx, double ny, double nz, double, double, double) const {
    const double d = fma(nz, sz, fma(ny, sy, nx * sx));
    const float c = (float)fmin(fmax(d, 0.0), 1.0);
    return c;
  }
};

// element i of [K][R][3]: a sun that has set (s_z <= 0) and a ray under the accumulation threshold have V = 0 whatever `vis` holds.
// sky_stride: floats between the skies of two suns: 0 for one sky [R][3] under all K, R 3 for a sky of each sun's own [K][R][3]
__global__ __launch_bounds__(256) void sun_composite_kernel(const float* __restrict__ lin_sky, int64_t sky_stride, const float* __restrict__ t,
                                                            const float* __restrict__ vis, const float* __restrict__ acc,
                                                            const float* __restrict__ acc_threshold, const float* __restrict__ suns,
                                                            const float* __restrict__ colours, int64_t R, int K, float* __restrict__ rgb,
                                                            float* __restrict__ lin, float* __restrict__ shadow) {
  const int64_t n = (int64_t)K * R * 3;
  const float thr = acc_threshold[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t kr = i / 3;
    const int c = (int)(i - kr * 3);
    const int k = (int)(kr / R);
    const int64_t r = kr - (int64_t)k * R;
    const bool on = suns[3 * k + 2] > 0.0f && acc[r] > thr;
    const float v = on ? (vis ? vis[kr] : 1.0f) : 0.0f;
    const float sky = lin_sky[(int64_t)k * sky_stride + r * 3 + c];
    const float x = on ? (float)((double)sky + (double)colours[3 * k + c] * (double)v * (double)t[i]) : sky;
    if (lin) lin[i] = x;
    rgb[i] = srgb_fwd(x);
    if (shadow && c == 0) shadow[kr] = v;
  }
}

}  // namespace

extern "C" int nsky_sun_transfer(const float* albedo, const float* normals, const float* weights, const float* suns, int64_t R, int32_t S,
                                 int32_t K, float* out, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && S >= 1 && K >= 0, "nsky_sun_transfer: R %ld, S %d, K %d", (long)R, (int)S, (int)K);
  if (R == 0 || K == 0) return NSKY_OK;
  NSKY_CHECK_ARG(albedo && normals && weights && suns && out, "nsky_sun_transfer: NULL albedo / normals / weights / suns / out");
  return launch_ray_transfer<Sun>("nsky_sun_transfer", nullptr, albedo, normals, weights, suns, R, S, K, out, (hipStream_t)stream);
}

extern "C" int nsky_sun_composite(const float* lin_sky, int64_t sky_stride, const float* t, const float* vis, const float* acc,
                                  const float* acc_threshold, const float* suns, const float* colours, int64_t R, int32_t K, float* rgb,
                                  float* lin, float* shadow, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && K >= 0 && (sky_stride == 0 || sky_stride == R * 3), "nsky_sun_composite: R %ld, K %d, stride %ld", (long)R, (int)K,
                 (long)sky_stride);
  if (R == 0 || K == 0) return NSKY_OK;
  NSKY_CHECK_ARG(lin_sky && t && acc && acc_threshold && suns && colours && rgb,
                 "nsky_sun_composite: NULL lin_sky / t / acc / acc_threshold / suns / colours / rgb");
  hipLaunchKernelGGL(sun_composite_kernel, dim3(capped_grid(((int64_t)K * R * 3 + 255) / 256, 16)), dim3(256), 0, (hipStream_t)stream, lin_sky,
                     sky_stride, t, vis, acc, acc_threshold, suns, colours, R, (int)K, rgb, lin, shadow);
  NSKY_CHECK_LAUNCH("nsky_sun_composite");
  return NSKY_OK;
}
