// Height fog and haze with shadowed sun shafts (neusky_amd/relight/atmosphere.py).  Definitions: include/neusky_hip.h.
//
//   params     fp32 [12] in device memory: density (0..2), albedo (3..5), H (0: homogeneous), base_height, g, far, background (1 or 0), -
//   rows       one thread per row i = m R + r of the shaft queries: the ray's origin and direction copied, the depth of the midpoint of
//              segment m, (m + 0.5) (far / M), formed in fp64 and rounded once.
//   apply      one thread per ray, bases and channels looped.  The ray's own factors (E, d_z, t_s, A, the transmittances to t_s and to
//              far) are formed once; per base the source's two terms; per segment one phi and three exponentials, shared by up to 8
//              bases, whose sums sit in registers (more bases: further passes over the segments).  Everything is fp64 from the fp32
//              inputs and every output is rounded once: a float64 restatement differs by that rounding and by the last bits of the
//              device's exp and expm1.  At a chunk's 4096 rays (64 workgroups) it is bound by its chain of fp64 exponentials, not by
//              its launch or its bytes: a few microseconds without shafts (README: measured).
// No atomics, a fixed summation order (m ascending): two runs agree bit for bit.  Flat indices are 64-bit.  Nothing here synchronises
// with the host.
#include <algorithm>

#include "numerics.h"
#include "../../include/neusky_hip.h"

namespace {

enum { A_DENSITY = 0, A_ALBEDO = 3, A_H = 6, A_BASE = 7, A_G = 8, A_FAR = 9, A_BACKGROUND = 10 };
constexpr double kPi = 3.14159265358979323846;

__global__ __launch_bounds__(256) void atmosphere_rows_kernel(const float* __restrict__ o, const float* __restrict__ d,
                                                              const float* __restrict__ params, int64_t R, int M,
                                                              float* __restrict__ row_o, float* __restrict__ row_d,
                                                              float* __restrict__ row_depth) {
  const int64_t T = R * M;
  const double step = (double)params[A_FAR] / (double)M;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / R, r = (i - m * R) * 3, j = i * 3;
    row_o[j] = o[r], row_o[j + 1] = o[r + 1], row_o[j + 2] = o[r + 2];
    row_d[j] = d[r], row_d[j + 1] = d[r + 1], row_d[j + 2] = d[r + 2];
    row_depth[i] = (float)(((double)m + 0.5) * step);
  }
}

// phi(u) = (1 - exp(-u)) / u
__device__ __forceinline__ double phi(double u) {
  if (fabs(u) < 1e-4) return 1.0 - u / 2.0 + u * u / 6.0;
  return -expm1(-u) / u;
}

// the path factor of tau: E t phi(d_z t / H); t for a homogeneous medium (H == 0)
__device__ __forceinline__ double path(double t, double E, double dz, double H) {
  return H > 0.0 ? E * t * phi(dz * t / H) : t;
}

// lin_in [Kb][R][3] through (ls_k, ls_r); the [Kb][R][3] outputs through (os_k, os_r); vis [M][K][R] through (vs_m, vs_k, vs_r).
// KB: the bases whose in-scatter sums a thread keeps in registers while it walks the segments once (1 for a frame of one base, else 8)
template <int KB>
__global__ __launch_bounds__(64) void atmosphere_apply_kernel(
    const float* __restrict__ o, const float* __restrict__ d, const float* __restrict__ depth, const float* __restrict__ acc,
    const float* __restrict__ lin_in, int64_t ls_k, int64_t ls_r, const float* __restrict__ background, int64_t bg_stride,
    const float* __restrict__ abar, const float* __restrict__ sun_dirs, const float* __restrict__ sun_colours,
    const float* __restrict__ vis, int64_t vs_m, int64_t vs_k, int64_t vs_r, const float* __restrict__ params, int64_t R, int M, int Kb,
    float* __restrict__ lin, float* __restrict__ rgb, float* __restrict__ inscatter, int64_t os_k, int64_t os_r,
    float* __restrict__ transmittance, float* __restrict__ light_lin) {
  const double H = params[A_H], base = params[A_BASE], g = params[A_G], far = params[A_FAR];
  const bool fog_background = params[A_BACKGROUND] != 0.0f;
  const double dens[3] = {params[A_DENSITY], params[A_DENSITY + 1], params[A_DENSITY + 2]};
  const double alb[3] = {params[A_ALBEDO], params[A_ALBEDO + 1], params[A_ALBEDO + 2]};
  const int Mseg = M > 1 ? M : 1;
  for (int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x; r < R; r += (int64_t)gridDim.x * 64) {
    const double dx = d[r * 3], dy = d[r * 3 + 1], dz = d[r * 3 + 2];
    const double E = H > 0.0 ? exp(fmin(fmax(-((double)o[r * 3 + 2] - base) / H, -80.0), 80.0)) : 1.0;
    const double ts = fmin(fmax((double)depth[r], 0.0), far);
    const double A = fmin(fmax((double)acc[r], 0.0), 1.0);
    const double ps = path(ts, E, dz, H), pf = path(far, E, dz, H);
    double Ts[3], Tf[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Ts[c] = exp(-(dens[c] * ps));
      Tf[c] = exp(-(dens[c] * pf));
      transmittance[r * 3 + c] = (float)Ts[c];
      if (light_lin) light_lin[r * 3 + c] = (float)((double)light_lin[r * 3 + c] * Ts[c]);
    }
    // the segments' transmittances do not depend on the base image: segments outside, up to KB bases inside, their sums in registers
    // (every loop over j is unrolled: no array is indexed by a variable)
    for (int k0 = 0; k0 < Kb; k0 += KB) {
      double sun[KB][3];  // 2 pi p_g(<d, s_k>) C_k up_k
      double Ss[KB][3], Sf[KB][3];  // S_b(t_s), S_b(far)
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const int k = k0 + j;
#pragma unroll
        for (int c = 0; c < 3; ++c) sun[j][c] = Ss[j][c] = Sf[j][c] = 0.0;
        if (k < Kb && sun_dirs && sun_dirs[k * 3 + 2] > 0.0f) {
          const double mu = dx * (double)sun_dirs[k * 3] + dy * (double)sun_dirs[k * 3 + 1] + dz * (double)sun_dirs[k * 3 + 2];
          const double q = 1.0 + g * g - 2.0 * g * mu;
          const double p = (1.0 / (4.0 * kPi)) * (1.0 - g * g) / (q * sqrt(q));
#pragma unroll
          for (int c = 0; c < 3; ++c) sun[j][c] = 2.0 * kPi * p * (double)sun_colours[k * 3 + c];
        }
      }
      double Ps[3] = {1.0, 1.0, 1.0}, Pf[3] = {1.0, 1.0, 1.0};  // T(min(t_m, t_e)) of the segment's near bound
      for (int m = 0; m < Mseg; ++m) {
        const double t1 = (double)(m + 1) * far / (double)Mseg;
        const bool last = m + 1 == Mseg;  // t1 is far: T(far) is at hand
        const double p1 = last ? pf : path(t1, E, dz, H);
        double ds[3], df[3];  // T(min(t_m, t_e)) - T(min(t_{m+1}, t_e)) for t_e = t_s and far
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double T1f = last ? Tf[c] : exp(-(dens[c] * p1));
          const double T1s = t1 < ts ? T1f : Ts[c];  // (t1 < ts <= far: never the last bound)
          ds[c] = Ps[c] - T1s, df[c] = Pf[c] - T1f;
          Ps[c] = T1s, Pf[c] = T1f;
        }
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          const int k = k0 + j;
          if (k < Kb) {
            const double v = (vis && M > 0) ? (double)vis[(int64_t)m * vs_m + (int64_t)k * vs_k + r * vs_r] : 1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const double J = alb[c] * ((double)abar[k * 3 + c] + sun[j][c] * v);
              Ss[j][c] += J * ds[c];
              Sf[j][c] += J * df[c];
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const int k = k0 + j;
        if (k < Kb) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double B = background[(int64_t)k * bg_stride + r * 3 + c];
            const double L = lin_in[(int64_t)k * ls_k + r * ls_r + c];
            const double behind = fog_background ? Sf[j][c] : 0.0;  // X - B, without the background's own attenuation
            const double X = fog_background ? Tf[c] * B + Sf[j][c] : B;
            const double in = A * Ss[j][c] + (1.0 - A) * behind;
            const double out = Ts[c] * (L - (1.0 - A) * B) + A * Ss[j][c] + (1.0 - A) * X;
            const int64_t i = (int64_t)k * os_k + r * os_r + c;
            const float x = (float)out;
            lin[i] = x;
            rgb[i] = srgb_fwd(x);
            inscatter[i] = (float)in;
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" int nsky_atmosphere_rows(const float* origins, const float* directions, const float* params, int64_t R, int32_t M,
                                    float* row_origins, float* row_directions, float* row_depth, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && M >= 0 && M <= NSKY_ATMOSPHERE_MAX_SHAFTS, "nsky_atmosphere_rows: R %ld, M %d", (long)R, (int)M);
  const int64_t T = R * M;
  if (T == 0) return NSKY_OK;
  NSKY_CHECK_ARG(origins && directions && params && row_origins && row_directions && row_depth,
                 "nsky_atmosphere_rows: NULL origins / directions / params / row_origins / row_directions / row_depth");
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((T + 255) / 256, 256 * 8));
  hipLaunchKernelGGL(atmosphere_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, origins, directions, params, R, (int)M, row_origins,
                     row_directions, row_depth);
  NSKY_CHECK_LAUNCH("nsky_atmosphere_rows");
  return NSKY_OK;
}

extern "C" int nsky_atmosphere_apply(const float* origins, const float* directions, const float* depth, const float* accumulation,
                                     const float* lin_in, int64_t lin_stride_k, int64_t lin_stride_r, const float* background,
                                     int64_t background_stride, const float* abar, const float* sun_dirs, const float* sun_colours,
                                     const float* vis, int64_t vis_stride_m, int64_t vis_stride_k, int64_t vis_stride_r, const float* params,
                                     int64_t R, int32_t M, int32_t Kb, float* lin, float* rgb, float* inscatter, int64_t out_stride_k,
                                     int64_t out_stride_r, float* transmittance, float* light_lin, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && Kb >= 0 && M >= 0 && M <= NSKY_ATMOSPHERE_MAX_SHAFTS && (background_stride == 0 || background_stride == R * 3),
                 "nsky_atmosphere_apply: R %ld, Kb %d, M %d, background stride %ld", (long)R, (int)Kb, (int)M, (long)background_stride);
  if (R == 0 || Kb == 0) return NSKY_OK;
  NSKY_CHECK_ARG(origins && directions && depth && accumulation && lin_in && background && abar && params && lin && rgb && inscatter &&
                     transmittance,
                 "nsky_atmosphere_apply: NULL origins / directions / depth / accumulation / lin_in / background / abar / params / outputs");
  NSKY_CHECK_ARG((sun_dirs == nullptr) == (sun_colours == nullptr), "nsky_atmosphere_apply: sun directions and colours go together");
  NSKY_CHECK_ARG(vis == nullptr || (sun_dirs && M > 0), "nsky_atmosphere_apply: shaft visibilities need suns and M > 0");
  NSKY_CHECK_ARG(lin_stride_k >= 0 && lin_stride_r >= 3 && out_stride_k >= 0 && out_stride_r >= 3 &&
                     (vis == nullptr || (vis_stride_m >= 0 && vis_stride_k >= 0 && vis_stride_r >= 1)),
                 "nsky_atmosphere_apply: strides lin (%ld, %ld), out (%ld, %ld), vis (%ld, %ld, %ld)", (long)lin_stride_k, (long)lin_stride_r,
                 (long)out_stride_k, (long)out_stride_r, (long)vis_stride_m, (long)vis_stride_k, (long)vis_stride_r);
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((R + 63) / 64, 256 * 32));
  auto kernel = Kb == 1 ? atmosphere_apply_kernel<1> : atmosphere_apply_kernel<8>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, origins, directions, depth, accumulation, lin_in, lin_stride_k,
                     lin_stride_r, background, background_stride, abar, sun_dirs, sun_colours, vis, vis_stride_m, vis_stride_k, vis_stride_r,
                     params, R, (int)M, (int)Kb, lin, rgb, inscatter, out_stride_k, out_stride_r, transmittance, light_lin);
  NSKY_CHECK_LAUNCH("nsky_atmosphere_apply");
  return NSKY_OK;
}
