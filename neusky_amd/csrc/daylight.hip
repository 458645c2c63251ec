// A clear-sky daylight model whose sky follows the sun (neusky_amd/relight/daylight.py).  Definitions: include/neusky_hip.h.
//
// Preetham, Shirley, Smits 1999: the sky's luminance Y and chromaticity (x, y) towards d are their zenith values times F(ct, g) / F(1, ts),
//   F(ct, g) = (1 + A exp(B / ct)) (1 + C exp(D g) + E cos^2 g),   ct = d.z,  g = the angle between d and the sun,  ts = the sun's zenith angle
// The first factor depends on the direction only, the zenith values and F(1, ts) on the sun only:
//   setup    the first lanes of a workgroup take one sun each and leave (s, Yz / F0_Y, xz / F0_x, yz / F0_y) in LDS, worked out in fp64
//            (1 + A exp(B) cancels to 0.17 at T = 2: in fp32 the whole sky of a sun would carry that error); lane 0 leaves the 9 constants
//            C, D, E the stream needs.
//   stream   a thread owns a direction: it is read once, normalised and its gradient factors 1 + A exp(B / ct) formed in fp64 (three
//            exponentials per direction, whatever K), rounded once.  It then walks the suns: per (direction, sun) fp32 only -- a cross and
//            a dot product, one atan2f, three v_exp_f32, one division, the colour matrix: ~140 instructions for 12 bytes written.
//   store    a wave's 64 x 3 floats of one sun are contiguous in out[k]: they cross a wave-private LDS tile so that lane l stores dwords
//            l, l + 64, l + 128 of the 768 bytes (three fully coalesced stores) instead of three stride-12 ones.
// No atomics, no reductions: every output is bitwise repeatable.  Flat indices are 64-bit.  Nothing here synchronises with the host.
#include <algorithm>

#include "numerics.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr int kMaxSunsPerLaunch = 256;  // LDS table rows (8 KiB); more suns take another launch
constexpr int kSunRow = 8;              // s.x, s.y, s.z, Yz / F0_Y, xz / F0_x, yz / F0_y, on (s.z > 0), pad
constexpr double kPi = 3.14159265358979323846;

// A, B, C, D, E of Y, x, y: value = slope T + offset
__constant__ double kPerez[3][5][2] = {
    {{0.1787, -1.4630}, {-0.3554, 0.4275}, {-0.0227, 5.3251}, {0.1206, -2.5771}, {-0.0670, 0.3703}},
    {{-0.0193, -0.2592}, {-0.0665, 0.0008}, {-0.0004, 0.2125}, {-0.0641, -0.8989}, {-0.0033, 0.0452}},
    {{-0.0167, -0.2608}, {-0.0950, 0.0092}, {-0.0079, 0.2102}, {-0.0441, -1.6537}, {-0.0109, 0.0529}}};
__constant__ double kZenithX[3][4] = {{0.00166, -0.00375, 0.00209, 0.0}, {-0.02903, 0.06377, -0.03202, 0.00394}, {0.11693, -0.21196, 0.06052, 0.25886}};
__constant__ double kZenithY[3][4] = {{0.00275, -0.00610, 0.00317, 0.0}, {-0.04214, 0.08970, -0.04153, 0.00516}, {0.15346, -0.26756, 0.06670, 0.26688}};

__device__ __forceinline__ double perez(double T, int q, int j) { return fma(kPerez[q][j][0], T, kPerez[q][j][1]); }

__device__ __forceinline__ double zenith_chroma(const double (&M)[3][4], double T, double ts) {
  double v = 0.0;
  const double tp[3] = {T * T, T, 1.0};
#pragma unroll
  for (int i = 0; i < 3; ++i) v += tp[i] * (((M[i][0] * ts + M[i][1]) * ts + M[i][2]) * ts + M[i][3]);
  return v;
}

// what sun k contributes to every direction: its direction, and zenith value / F(1, ts) of Y, x, y
__device__ void sun_row(const float* __restrict__ sun, double T, float* __restrict__ row) {
  const double sz = sun[2];
  const bool on = sz > 0.0;
  double ratio[3] = {0.0, 0.0, 0.0};
  if (on) {
    const double ts = acos(fmin(sz, 1.0));
    const double chi = (4.0 / 9.0 - T / 120.0) * (kPi - 2.0 * ts);
    const double zen[3] = {(4.0453 * T - 4.9710) * tan(chi) - 0.2155 * T + 2.4192, zenith_chroma(kZenithX, T, ts), zenith_chroma(kZenithY, T, ts)};
    const double c = fmin(sz, 1.0);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double f0 = (1.0 + perez(T, q, 0) * exp(perez(T, q, 1))) * (1.0 + perez(T, q, 2) * exp(perez(T, q, 3) * ts) + perez(T, q, 4) * c * c);
      ratio[q] = zen[q] / f0;
    }
  }
  row[0] = sun[0];
  row[1] = sun[1];
  row[2] = sun[2];
  row[3] = (float)ratio[0];
  row[4] = (float)ratio[1];
  row[5] = (float)ratio[2];
  row[6] = on ? 1.0f : 0.0f;
  row[7] = 0.0f;
}

__global__ __launch_bounds__(256) void daylight_eval_kernel(const float* __restrict__ directions, const float* __restrict__ suns,
                                                            const float* __restrict__ turbidity, const float* __restrict__ exposure,
                                                            const float* __restrict__ ground, int64_t N, int K,
                                                            float* __restrict__ out) {
  __shared__ float table[kMaxSunsPerLaunch * kSunRow];
  __shared__ float cde[9];         // C, D, E of Y, x, y
  __shared__ float tile[4][192];   // a wave's 64 x 3 outputs of one sun
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double T = (double)turbidity[0];
  for (int k = threadIdx.x; k < K; k += 256) sun_row(suns + 3 * k, T, table + kSunRow * k);
  if (threadIdx.x < 9) cde[threadIdx.x] = (float)perez(T, threadIdx.x / 3, 2 + threadIdx.x % 3);
  __syncthreads();
  const float cY = cde[0], dY = cde[1], eY = cde[2], cx = cde[3], dx = cde[4], ex = cde[5], cy = cde[6], dy = cde[7], ey = cde[8];
  const float gain = exposure[0];
  const float gr0 = ground[0], gr1 = ground[1], gr2 = ground[2];
  double pa[3], pb[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    pa[q] = perez(T, q, 0);
    pb[q] = perez(T, q, 1);
  }
  const int64_t tiles = (N + 63) / 64;
  for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < tiles; t += (int64_t)gridDim.x * 4) {  // (uniform over the wave)
    const int64_t i = t * 64 + lane;
    const bool live = i < N;
    float ux = 0.0f, uy = 0.0f, uz = 1.0f, grad[3] = {0.0f, 0.0f, 0.0f}, m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
    if (live) {
      double x = directions[i * 3], y = directions[i * 3 + 1], z = directions[i * 3 + 2];
      const bool below = z < 0.0;
      if (below) {  // its horizon point; straight down: the zenith
        const bool down = x == 0.0 && y == 0.0;
        z = down ? 1.0 : 0.0;
      }
      const double n2 = x * x + y * y + z * z;
      const bool none = !(n2 > 0.0 && n2 < 1.0e300);  // no direction (zero, infinite or NaN): no sky, 0
      if (none) {
        x = y = 0.0;
        z = 1.0;
      }
      const double inv = none ? 1.0 : 1.0 / sqrt(n2);
      x *= inv;
      y *= inv;
      z *= inv;
#pragma unroll
      for (int q = 0; q < 3; ++q) grad[q] = (float)(z > 0.0 ? 1.0 + pa[q] * exp(pb[q] / z) : 1.0);
      ux = (float)x;
      uy = (float)y;
      uz = (float)z;
      m0 = none ? 0.0f : below ? gr0 * gain : gain;
      m1 = none ? 0.0f : below ? gr1 * gain : gain;
      m2 = none ? 0.0f : below ? gr2 * gain : gain;
    }
    for (int k = 0; k < K; ++k) {
      const float* row = table + kSunRow * k;  // (one address for the wave: broadcast reads)
      const float sx = row[0], sy = row[1], sz = row[2];
      const float c0 = uy * sz - uz * sy, c1 = uz * sx - ux * sz, c2 = ux * sy - uy * sx;
      const float cr = sqrtf(c0 * c0 + c1 * c1 + c2 * c2), dt = ux * sx + uy * sy + uz * sz;
      const float g = atan2f(cr, dt);
      const float h2 = cr * cr + dt * dt;
      const float cos2 = h2 > 0.0f ? dt * dt * __builtin_amdgcn_rcpf(h2) : 1.0f;  // (E <= 0.37: an ulp of the reciprocal is nothing here)
      const float fY = grad[0] * (1.0f + cY * __expf(dY * g) + eY * cos2);
      const float fx = grad[1] * (1.0f + cx * __expf(dx * g) + ex * cos2);
      const float fy = grad[2] * (1.0f + cy * __expf(dy * g) + ey * cos2);
      const float Y = row[3] * fY, cxv = row[4] * fx, cyv = row[5] * fy;
      const float s = Y / cyv;
      const float X = cxv * s, Z = (1.0f - cxv - cyv) * s;
      const bool on = row[6] != 0.0f;
      const float r = 3.2404542f * X - 1.5371385f * Y - 0.4985314f * Z;
      const float gch = -0.9692660f * X + 1.8760108f * Y + 0.0415560f * Z;
      const float b = 0.0556434f * X - 0.2040259f * Y + 1.0572252f * Z;
      float* tl = tile[wave];
      tl[lane * 3] = on ? fmaxf(r, 0.0f) * m0 : 0.0f;
      tl[lane * 3 + 1] = on ? fmaxf(gch, 0.0f) * m1 : 0.0f;
      tl[lane * 3 + 2] = on ? fmaxf(b, 0.0f) * m2 : 0.0f;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int64_t base = ((int64_t)k * N + t * 64) * 3;
      const int64_t left = std::min<int64_t>(192, (N - t * 64) * 3);  // floats of this tile inside out[k]
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int e = lane + 64 * j;
        if (e < left) out[base + e] = tl[e];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // the tile is read before the next sun overwrites it
    }
  }
}

}  // namespace

extern "C" int nsky_daylight_eval(const float* directions, const float* suns, const float* turbidity, const float* exposure,
                                  const float* ground, int64_t N, int32_t K, float* out, nsky_stream_t stream) {
  NSKY_CHECK_ARG(N >= 0 && K >= 0, "nsky_daylight_eval: N %ld, K %d", (long)N, (int)K);
  if (N == 0 || K == 0) return NSKY_OK;
  NSKY_CHECK_ARG(directions && suns && turbidity && exposure && ground && out,
                 "nsky_daylight_eval: NULL directions / suns / turbidity / exposure / ground / out");
  // every workgroup repeats the per-sun setup: no more of them than the device holds at once (256 CUs x 3 at this kernel's registers)
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((N + 255) / 256, 256 * 3));
  for (int k0 = 0; k0 < K; k0 += kMaxSunsPerLaunch) {
    hipLaunchKernelGGL(daylight_eval_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, directions, suns + 3 * (int64_t)k0, turbidity,
                       exposure, ground, N, std::min(kMaxSunsPerLaunch, (int)K - k0), out + (int64_t)k0 * N * 3);
    NSKY_CHECK_LAUNCH("nsky_daylight_eval");
  }
  return NSKY_OK;
}
