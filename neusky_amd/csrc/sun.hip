// A directional sun on top of the hemisphere render (neusky_amd/relight/sun.py).  Definitions: include/neusky_hip.h.
//
// The frame render sees light as its D directions (one cell ~ 4 pi / D sr); a sun is one direction of its own:
//   t[k,r,c]   = sum_s w[r,s] alb[r,s,c] clamp(n[r,s].s_k, 0, 1)
//   lin[k,r,c] = lin_sky[r,c] + C[k,c] V[k,r] t[k,r,c]
//   transfer   one wave per ray, lanes stride the samples: a sample (28 bytes) is read once per pass and meets up to 8 suns held in
//              scalar registers; a lane keeps 24 fp32 sums; the cosine itself is taken in fp64 (one rounding instead of three: a term
//              is then within 3 2^-24 of its definition), the 24 sums of the wave are finished with wave_sum.
//   composite  one thread per output element: mask, set-sun rule, the sum in fp64 rounded once, the sRGB curve of numerics.h.
//              nsky_sun_composite_skies: the same kernel, lin_sky[k,r,c] a sky of each sun's own (relight/daylight.py).
// No atomics, a fixed reduction order: two runs agree bit for bit.  Flat indices are 64-bit.  Nothing here synchronises with the host.
#include <algorithm>

#include "numerics.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr int kMaxSunsPerPass = 8;

template <int KB>
__global__ __launch_bounds__(256) void sun_transfer_kernel(const float* __restrict__ albedo, const float* __restrict__ normals,
                                                           const float* __restrict__ weights, const float* __restrict__ suns, int64_t R,
                                                           int S, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double sx[KB], sy[KB], sz[KB];  // (uniform: scalar registers)
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    sx[k] = suns[3 * k];
    sy[k] = suns[3 * k + 1];
    sz[k] = suns[3 * k + 2];
  }
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < R; r += (int64_t)gridDim.x * 4) {
    float a[KB][3];
#pragma unroll
    for (int k = 0; k < KB; ++k) a[k][0] = a[k][1] = a[k][2] = 0.0f;
    for (int s = lane; s < S; s += 64) {
      const int64_t i = r * S + s, o = i * 3;
      const float w = weights[i];
      const float g0 = w * albedo[o], g1 = w * albedo[o + 1], g2 = w * albedo[o + 2];
      const double nx = normals[o], ny = normals[o + 1], nz = normals[o + 2];
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const double d = fma(nz, sz[k], fma(ny, sy[k], nx * sx[k]));
        const float c = (float)fmin(fmax(d, 0.0), 1.0);
        a[k][0] = fmaf(g0, c, a[k][0]);
        a[k][1] = fmaf(g1, c, a[k][1]);
        a[k][2] = fmaf(g2, c, a[k][2]);
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

template <int KB>
void launch_transfer(hipStream_t st, const float* albedo, const float* normals, const float* weights, const float* suns, int64_t R, int S,
                     float* out) {
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((R + 3) / 4, 256 * 8));
  hipLaunchKernelGGL((sun_transfer_kernel<KB>), dim3(grid), dim3(256), 0, st, albedo, normals, weights, suns, R, S, out);
}

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
  hipStream_t st = (hipStream_t)stream;
  for (int k0 = 0; k0 < K; k0 += kMaxSunsPerPass) {
    const float* s = suns + 3 * k0;
    float* o = out + (int64_t)k0 * R * 3;
    switch (std::min(kMaxSunsPerPass, K - k0)) {
      case 1: launch_transfer<1>(st, albedo, normals, weights, s, R, S, o); break;
      case 2: launch_transfer<2>(st, albedo, normals, weights, s, R, S, o); break;
      case 3: launch_transfer<3>(st, albedo, normals, weights, s, R, S, o); break;
      case 4: launch_transfer<4>(st, albedo, normals, weights, s, R, S, o); break;
      case 5: launch_transfer<5>(st, albedo, normals, weights, s, R, S, o); break;
      case 6: launch_transfer<6>(st, albedo, normals, weights, s, R, S, o); break;
      case 7: launch_transfer<7>(st, albedo, normals, weights, s, R, S, o); break;
      default: launch_transfer<8>(st, albedo, normals, weights, s, R, S, o); break;
    }
    NSKY_CHECK_LAUNCH("nsky_sun_transfer");
  }
  return NSKY_OK;
}

// both composites: one sky under all K suns (sky_stride 0) or a sky of each sun's own
static int launch_composite(const char* name, const float* lin_sky, int64_t sky_stride, const float* t, const float* vis, const float* acc,
                            const float* acc_threshold, const float* suns, const float* colours, int64_t R, int32_t K, float* rgb,
                            float* lin, float* shadow, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && K >= 0, "%s: R %ld, K %d", name, (long)R, (int)K);
  if (R == 0 || K == 0) return NSKY_OK;
  NSKY_CHECK_ARG(lin_sky && t && acc && acc_threshold && suns && colours && rgb,
                 "%s: NULL lin_sky / t / acc / acc_threshold / suns / colours / rgb", name);
  const int64_t n = (int64_t)K * R * 3;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 16));
  hipLaunchKernelGGL(sun_composite_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, lin_sky, sky_stride, t, vis, acc, acc_threshold, suns,
                     colours, R, (int)K, rgb, lin, shadow);
  NSKY_CHECK_LAUNCH(name);
  return NSKY_OK;
}

extern "C" int nsky_sun_composite(const float* lin_sky, const float* t, const float* vis, const float* acc, const float* acc_threshold,
                                  const float* suns, const float* colours, int64_t R, int32_t K, float* rgb, float* lin, float* shadow,
                                  nsky_stream_t stream) {
  return launch_composite("nsky_sun_composite", lin_sky, 0, t, vis, acc, acc_threshold, suns, colours, R, K, rgb, lin, shadow, stream);
}

extern "C" int nsky_sun_composite_skies(const float* lin_skies, const float* t, const float* vis, const float* acc, const float* acc_threshold,
                                        const float* suns, const float* colours, int64_t R, int32_t K, float* rgb, float* lin, float* shadow,
                                        nsky_stream_t stream) {
  return launch_composite("nsky_sun_composite_skies", lin_skies, R * 3, t, vis, acc, acc_threshold, suns, colours, R, K, rgb, lin, shadow, stream);
}
