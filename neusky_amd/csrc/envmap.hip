// Relighting under an equirectangular HDR environment map (neusky_amd/relight): the projection of a map onto the renderer's D light
// directions and the bilinear sky lookup of the camera rays.  Definitions: include/neusky_hip.h.
//
// The renderer treats its D light directions as point samples of radiance, so a map is projected first: every texel goes to the
// direction nearest to it (its cell), and each direction gets the solid-angle-weighted mean of its cell.  Three passes:
//   label   one thread per 4 texels: the arg-max of <t, R d_k> over the D rotated directions, held in LDS (int16 labels)
//   (sort)  the caller groups texels by label with a stable sort (ascending texel index inside a cell)
//   reduce  one workgroup per direction: finds its segment of the sorted labels (a 64-way search by one wave), sums omega L and
//           omega in fp64 in a fixed order (strided per-thread partials, then a fixed tree), or falls back to the lookup
//   lookup  one thread per ray: bilinear at R d, coordinates in fp64
// No atomics: every output is a pure function of the inputs, so two runs agree bit for bit.  Flat texel indices are 64-bit.
// R and the exposure are read from device memory, and nothing here synchronises with the host: graph-capture safe.
#include "common.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr int kMaxDirs = NSKY_ENVMAP_MAX_DIRECTIONS;
constexpr int kLabelThreads = 256;
constexpr int kLabelPerThread = 4;
constexpr int kReduceThreads = 512;
constexpr int kLookupThreads = 256;

struct MapView {
  const float* map;
  int64_t H, W;
  int conv;
};

// R (row-major, NULL = identity) into registers
__device__ __forceinline__ void load_rotation(const float* __restrict__ rot, float r[9]) {
#pragma unroll
  for (int q = 0; q < 9; ++q) r[q] = rot ? rot[q] : (q % 4 == 0 ? 1.0f : 0.0f);
}

// the direction of texel (i, j), computed in fp64 and rounded once
__device__ __forceinline__ float3 texel_direction(int64_t i, int64_t j, int64_t H, int64_t W, int conv) {
  const double th = kPi * ((double)i + 0.5) / (double)H;
  const double u = ((double)j + 0.5) / (double)W;
  const double ph = conv == NSKY_ENVMAP_BLENDER ? kPi - 2.0 * kPi * u : 2.0 * kPi * u;
  double st, ct, sp, cp;
  sincos(th, &st, &ct);
  sincos(ph, &sp, &cp);
  return make_float3((float)(st * cp), (float)(st * sp), (float)ct);
}

// bilinear lookup at direction v (any length); exposure applied.  A non-finite v reads nothing and gives NaN.
__device__ void lookup(const MapView& m, double vx, double vy, double vz, double ex, float* __restrict__ out) {
  const double theta = atan2(sqrt(vx * vx + vy * vy), vz);
  const double phi = atan2(vy, vx);
  double u = phi * (0.5 / kPi);
  if (m.conv == NSKY_ENVMAP_BLENDER) u = 0.5 - u;
  const double x = u * (double)m.W - 0.5, y = theta * (1.0 / kPi) * (double)m.H - 0.5;
  if (!isfinite(x) || !isfinite(y)) {
    out[0] = out[1] = out[2] = __builtin_nanf("");
    return;
  }
  const double x0 = floor(x), y0 = floor(y);
  const double fx = x - x0, fy = y - y0;
  int64_t j0 = (int64_t)x0 % m.W;
  if (j0 < 0) j0 += m.W;
  const int64_t j1 = j0 + 1 == m.W ? 0 : j0 + 1;
  const int64_t iy = (int64_t)y0;
  const int64_t i0 = iy < 0 ? 0 : (iy > m.H - 1 ? m.H - 1 : iy);
  const int64_t i1 = iy + 1 < 0 ? 0 : (iy + 1 > m.H - 1 ? m.H - 1 : iy + 1);
  const float* a = m.map + (i0 * m.W + j0) * 3;
  const float* b = m.map + (i0 * m.W + j1) * 3;
  const float* c = m.map + (i1 * m.W + j0) * 3;
  const float* d = m.map + (i1 * m.W + j1) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double top = (1.0 - fx) * (double)a[ch] + fx * (double)b[ch];
    const double bot = (1.0 - fx) * (double)c[ch] + fx * (double)d[ch];
    out[ch] = (float)(ex * ((1.0 - fy) * top + fy * bot));
  }
}

__global__ __launch_bounds__(kLabelThreads) void envmap_label_kernel(const float* __restrict__ dirs, int D, const float* __restrict__ rot,
                                                                      int64_t H, int64_t W, int conv, int16_t* __restrict__ labels) {
  __shared__ float4 sd[kMaxDirs];
  float r[9];
  load_rotation(rot, r);
  for (int k = threadIdx.x; k < D; k += kLabelThreads) {
    const float dx = dirs[3 * k], dy = dirs[3 * k + 1], dz = dirs[3 * k + 2];
    sd[k] = make_float4(fmaf(r[2], dz, fmaf(r[1], dy, r[0] * dx)), fmaf(r[5], dz, fmaf(r[4], dy, r[3] * dx)),
                        fmaf(r[8], dz, fmaf(r[7], dy, r[6] * dx)), 0.0f);
  }
  __syncthreads();
  const int64_t n = H * W;
  const int64_t base = (int64_t)blockIdx.x * (kLabelThreads * kLabelPerThread) + threadIdx.x;
  float tx[kLabelPerThread], ty[kLabelPerThread], tz[kLabelPerThread], best[kLabelPerThread];
  int arg[kLabelPerThread];
#pragma unroll
  for (int q = 0; q < kLabelPerThread; ++q) {
    const int64_t p = base + (int64_t)q * kLabelThreads;
    float3 t = make_float3(0.0f, 0.0f, 0.0f);
    if (p < n) {
      const int64_t i = p / W;
      t = texel_direction(i, p - i * W, H, W, conv);
    }
    tx[q] = t.x; ty[q] = t.y; tz[q] = t.z;
    best[q] = -INFINITY;
    arg[q] = 0;
  }
#pragma unroll 4
  for (int k = 0; k < D; ++k) {
    const float4 e = sd[k];
#pragma unroll
    for (int q = 0; q < kLabelPerThread; ++q) {
      const float dot = fmaf(tz[q], e.z, fmaf(ty[q], e.y, tx[q] * e.x));
      if (dot > best[q]) {  // strict: ties keep the lower k
        best[q] = dot;
        arg[q] = k;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kLabelPerThread; ++q) {
    const int64_t p = base + (int64_t)q * kLabelThreads;
    if (p < n) labels[p] = (int16_t)arg[q];
  }
}

// first index of sorted[0, n) holding a value >= key (n when none), by the calling wave: 64 probes per round, so a round shrinks
// the range 64-fold.  Every lane returns the same value.
__device__ int64_t wave_lower_bound(const int16_t* __restrict__ sorted, int64_t n, int key) {
  const int lane = threadIdx.x & 63;
  int64_t lo = 0, hi = n;  // the answer lies in [lo, hi]
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) / 64;
    const int64_t p = lo + lane * step;
    const uint64_t m = __ballot(p < hi && (int)sorted[p] >= key);
    if (m == 0) {
      lo += step * ((hi - 1 - lo) / step) + 1;  // past the last probe below hi
    } else {
      const int f = __ffsll((unsigned long long)m) - 1;
      hi = lo + f * step;
      if (f > 0) lo += (int64_t)(f - 1) * step + 1;
    }
  }
  return lo;
}

__global__ __launch_bounds__(kReduceThreads) void envmap_reduce_kernel(MapView m, const float* __restrict__ dirs, const float* __restrict__ rot,
                                                                        const float* __restrict__ exposure,
                                                                        const int16_t* __restrict__ sorted, const int64_t* __restrict__ order,
                                                                        float* __restrict__ colours, float* __restrict__ cell_weight) {
  __shared__ int64_t seg[2];
  __shared__ double acc[4][kReduceThreads];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int64_t n = m.H * m.W;
  if (tid < 128) {  // wave 0: the segment's start, wave 1: its end
    const int64_t b = wave_lower_bound(sorted, n, k + (tid >> 6));
    if ((tid & 63) == 0) seg[tid >> 6] = b;
  }
  __syncthreads();
  const int64_t s = seg[0], e = seg[1];
  const double th_scale = kPi / (double)m.H;
  double ar = 0.0, ag = 0.0, ab = 0.0, aw = 0.0;
  int64_t idx = s + tid;
  for (; idx + 3 * kReduceThreads < e; idx += 4 * kReduceThreads) {  // four gathers in flight, summed in the plain loop's order
    int64_t p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = order[idx + q * kReduceThreads];
    float L[4][3];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ok[q] = p[q] >= 0 && p[q] < n;
      L[q][0] = ok[q] ? m.map[3 * p[q]] : 0.0f;
      L[q][1] = ok[q] ? m.map[3 * p[q] + 1] : 0.0f;
      L[q][2] = ok[q] ? m.map[3 * p[q] + 2] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double w = ok[q] ? sin(th_scale * ((double)(p[q] / m.W) + 0.5)) : 0.0;
      ar += w * (double)L[q][0];
      ag += w * (double)L[q][1];
      ab += w * (double)L[q][2];
      aw += w;
    }
  }
  for (; idx < e; idx += kReduceThreads) {
    const int64_t p = order[idx];
    if (p < 0 || p >= n) continue;
    const double w = sin(th_scale * ((double)(p / m.W) + 0.5));
    ar += w * (double)m.map[3 * p];
    ag += w * (double)m.map[3 * p + 1];
    ab += w * (double)m.map[3 * p + 2];
    aw += w;
  }
  acc[0][tid] = ar; acc[1][tid] = ag; acc[2][tid] = ab; acc[3][tid] = aw;
  __syncthreads();
  for (int h = kReduceThreads / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c][tid] += acc[c][tid + h];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double ex = exposure ? (double)exposure[0] : 1.0;
  if (e > s) {
    const double wsum = acc[3][0];
#pragma unroll
    for (int c = 0; c < 3; ++c) colours[3 * k + c] = (float)(ex * (acc[c][0] / wsum));
    cell_weight[k] = (float)(wsum * (2.0 * kPi / (double)m.W) * 2.0 * sin(kPi / (2.0 * (double)m.H)));
  } else {  // no texel centre in this cell: the lookup at R d_k
    float r[9];
    load_rotation(rot, r);
    const double dx = dirs[3 * k], dy = dirs[3 * k + 1], dz = dirs[3 * k + 2];
    lookup(m, r[0] * dx + r[1] * dy + r[2] * dz, r[3] * dx + r[4] * dy + r[5] * dz, r[6] * dx + r[7] * dy + r[8] * dz, ex, colours + 3 * k);
    cell_weight[k] = 0.0f;
  }
}

__global__ __launch_bounds__(kLookupThreads) void envmap_lookup_kernel(MapView m, const float* __restrict__ dirs, int64_t N,
                                                                        const float* __restrict__ rot, const float* __restrict__ exposure,
                                                                        float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kLookupThreads + threadIdx.x;
  if (t >= N) return;
  float r[9];
  load_rotation(rot, r);
  const double dx = dirs[3 * t], dy = dirs[3 * t + 1], dz = dirs[3 * t + 2];
  const double ex = exposure ? (double)exposure[0] : 1.0;
  lookup(m, r[0] * dx + r[1] * dy + r[2] * dz, r[3] * dx + r[4] * dy + r[5] * dz, r[6] * dx + r[7] * dy + r[8] * dz, ex, out + 3 * t);
}

constexpr int64_t kMaxTexels = (int64_t)1 << 31;  // a sort of 2^31 int16 keys with int64 values; also the int32 grid limit below

bool valid_map(int64_t H, int64_t W, int convention) {
  return H >= 1 && W >= 1 && H <= kMaxTexels && W <= kMaxTexels && H * W <= kMaxTexels &&
         (convention == NSKY_ENVMAP_NEUSKY || convention == NSKY_ENVMAP_BLENDER);
}

}  // namespace

extern "C" int nsky_envmap_label(const float* directions, int32_t D, const float* rotation, int64_t H, int64_t W, int32_t convention,
                                 int16_t* labels, nsky_stream_t stream) {
  NSKY_CHECK_ARG(valid_map(H, W, convention), "nsky_envmap_label: map [%ld, %ld] convention %d", (long)H, (long)W, (int)convention);
  NSKY_CHECK_ARG(directions && labels && D >= 1 && D <= kMaxDirs, "nsky_envmap_label: directions %p [%d] (1..%d), labels %p", directions,
                 (int)D, kMaxDirs, labels);
  const int64_t per_block = kLabelThreads * kLabelPerThread;
  const int64_t blocks = (H * W + per_block - 1) / per_block;
  hipLaunchKernelGGL(envmap_label_kernel, dim3((unsigned)blocks), dim3(kLabelThreads), 0, (hipStream_t)stream, directions, (int)D, rotation,
                     H, W, (int)convention, labels);
  NSKY_CHECK_LAUNCH("nsky_envmap_label");
  return NSKY_OK;
}

extern "C" int nsky_envmap_reduce(const float* map, int64_t H, int64_t W, int32_t convention, const float* directions, int32_t D,
                                  const float* rotation, const float* exposure, const int16_t* sorted_labels, const int64_t* order,
                                  float* colours, float* cell_weight, nsky_stream_t stream) {
  NSKY_CHECK_ARG(map && valid_map(H, W, convention), "nsky_envmap_reduce: map %p [%ld, %ld] convention %d", map, (long)H, (long)W,
                 (int)convention);
  NSKY_CHECK_ARG(directions && D >= 1 && D <= kMaxDirs, "nsky_envmap_reduce: directions %p [%d] (1..%d)", directions, (int)D, kMaxDirs);
  NSKY_CHECK_ARG(sorted_labels && order && colours && cell_weight, "nsky_envmap_reduce: NULL sorted_labels / order / colours / cell_weight");
  const MapView m{map, H, W, (int)convention};
  hipLaunchKernelGGL(envmap_reduce_kernel, dim3(D), dim3(kReduceThreads), 0, (hipStream_t)stream, m, directions, rotation, exposure,
                     sorted_labels, order, colours, cell_weight);
  NSKY_CHECK_LAUNCH("nsky_envmap_reduce");
  return NSKY_OK;
}

extern "C" int nsky_envmap_lookup(const float* map, int64_t H, int64_t W, int32_t convention, const float* directions, int64_t N,
                                  const float* rotation, const float* exposure, float* out, nsky_stream_t stream) {
  NSKY_CHECK_ARG(map && valid_map(H, W, convention), "nsky_envmap_lookup: map %p [%ld, %ld] convention %d", map, (long)H, (long)W,
                 (int)convention);
  NSKY_CHECK_ARG(N >= 0 && N <= kMaxTexels && (N == 0 || (directions && out)), "nsky_envmap_lookup: directions %p [%ld], out %p",
                 directions, (long)N, out);
  if (N == 0) return NSKY_OK;
  const MapView m{map, H, W, (int)convention};
  hipLaunchKernelGGL(envmap_lookup_kernel, dim3((unsigned)((N + kLookupThreads - 1) / kLookupThreads)), dim3(kLookupThreads), 0,
                     (hipStream_t)stream, m, directions, N, rotation, exposure, out);
  NSKY_CHECK_LAUNCH("nsky_envmap_lookup");
  return NSKY_OK;
}
