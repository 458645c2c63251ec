// The display transform of a linear image (neusky_amd/relight/display.py).  Definitions: include/neusky_hip.h, "A display transform".
//
//   histogram  a workgroup keeps 3072 32-bit counts in LDS (12 KB), walks its share of one image in a grid-stride loop (16-byte loads of
//              4 pixels when the image allows it), and adds its non-zero counts to the 64-bit histogram with integer atomics: the result
//              is an integer-exact function of the input, whatever the order of arrival.
//   exposure   one workgroup per histogram row; a thread owns 12 consecutive bins.  Every sum is an integer (the log2 of a bin's centre
//              is a multiple of 1/128), so the mean is exact before its one division.
//   blur       two passes over rows of 3 W floats.  The row pass keeps a tile of 256 floats and a halo of 3 r on each side in LDS and
//              forms the bloom source on the way in; the column pass keeps 32 + 2 r rows of 64 floats.  A position outside the frame is
//              a zero in LDS, so an image smaller than the radius needs no other rule.
//   map        one pass: exposure, bloom, curve, sRGB, 8-bit rounding; 4 pixels per thread when the image allows it.
// Flat indices are 64-bit.  Nothing here synchronises with the host.
#include <algorithm>

#include "numerics.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr int kBins = NSKY_DISPLAY_BINS;
constexpr int kMaxRadius = NSKY_DISPLAY_MAX_RADIUS;
constexpr int kRowTile = 256;   // floats of a row per workgroup (row pass)
constexpr int kColTile = 32;    // rows per workgroup (column pass), 64 floats wide
enum { P_KEY = 0, P_EV, P_LO, P_HI, P_WHITE, P_THRESHOLD, P_STRENGTH, P_MASK };

// ------------------------------------------------------------------------------------------ histogram
// every product and sum rounded once: a float32 restatement has the same bits
__device__ __forceinline__ float luminance(float r, float g, float b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, r), __fmul_rn(0.7152f, g)), __fmul_rn(0.0722f, b));
}

// the bin of a luminance, or -1: not finite, below 2^-24 (zero, negative and NaN among them).  2^-24 has the bit pattern 0x33800000,
// and the patterns of the positive finite floats ascend with their values.
__device__ __forceinline__ int bin_of(float y) {
  const unsigned u = __float_as_uint(y);
  if (u < 0x33800000u || u >= 0x7f800000u) return -1;
  return min((int)(u >> 17) - 6592, kBins - 1);
}

__device__ __forceinline__ void count(unsigned* sH, float r, float g, float b, bool masked) {
  const int bin = bin_of(luminance(r, g, b));
  if (bin >= 0 && !masked) atomicAdd(&sH[bin], 1u);
}

template <bool VEC>
__global__ __launch_bounds__(256) void display_histogram_kernel(const float* __restrict__ lin, const float* __restrict__ mask,
                                                                const float* __restrict__ params, int64_t P, int row_stride,
                                                                unsigned long long* __restrict__ hist) {
  __shared__ unsigned sH[kBins];
  for (int i = threadIdx.x; i < kBins; i += 256) sH[i] = 0u;
  __syncthreads();
  const int k = blockIdx.y;
  const float* img = lin + (int64_t)k * P * 3;
  const float* msk = mask ? mask + (int64_t)k * P : nullptr;
  const float thr = mask ? params[P_MASK] : 0.0f;
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  if (VEC) {  // P % 4 == 0 and 16-byte aligned images: 4 pixels = 3 float4
    for (int64_t g = first; g < P / 4; g += step) {
      const float4 a = ldg4(img + g * 12), b = ldg4(img + g * 12 + 4), c = ldg4(img + g * 12 + 8);
      float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (msk) m = ldg4(msk + g * 4);
      count(sH, a.x, a.y, a.z, msk && !(m.x > thr));
      count(sH, a.w, b.x, b.y, msk && !(m.y > thr));
      count(sH, b.z, b.w, c.x, msk && !(m.z > thr));
      count(sH, c.y, c.z, c.w, msk && !(m.w > thr));
    }
  } else {
    for (int64_t p = first; p < P; p += step) count(sH, img[p * 3], img[p * 3 + 1], img[p * 3 + 2], msk && !(msk[p] > thr));
  }
  __syncthreads();
  unsigned long long* out = hist + (int64_t)k * row_stride;
  for (int i = threadIdx.x; i < kBins; i += 256) {
    const unsigned c = sH[i];
    if (c) atomicAdd(&out[i], (unsigned long long)c);
  }
}

// ------------------------------------------------------------------------------------------ exposure
__global__ __launch_bounds__(256) void display_exposure_kernel(const long long* __restrict__ hist, const float* __restrict__ params,
                                                               float* __restrict__ E) {
  constexpr int kPer = kBins / 256;  // 12 bins per thread
  __shared__ long long sScan[256];
  __shared__ long long sSum[256];
  const int k = blockIdx.x, t = threadIdx.x;
  const long long* h = hist + (int64_t)k * kBins;
  long long c[kPer], mine = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    c[i] = h[t * kPer + i];
    mine += c[i];
  }
  // inclusive scan of the 256 partial counts (integers: exact in any order)
  sScan[t] = mine;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const long long add = t >= off ? sScan[t - off] : 0;
    __syncthreads();
    sScan[t] += add;
    __syncthreads();
  }
  const long long n = sScan[255];
  long long pos = sScan[t] - mine;  // sorted position of this thread's first pixel
  const double lo = (double)params[P_LO], hi = (double)params[P_HI];
  const long long a = (long long)floor(lo * (double)n);
  const long long b = n - (long long)floor((1.0 - hi) * (double)n);
  // sum_j c_j (2 j + 1 - 3072) = 128 sum_j c_j ((j + 0.5) / 64 - 24), an integer
  long long s = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const long long from = max(pos, a), to = min(pos + c[i], b);
    if (to > from) s += (to - from) * (long long)(2 * (t * kPer + i) + 1 - kBins);
    pos += c[i];
  }
  sSum[t] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) sSum[t] += sSum[t + off];
    __syncthreads();
  }
  if (t == 0) {
    float e = 1.0f;
    if (b > a) {
      const double m = (double)sSum[0] / 128.0 / (double)(b - a);
      e = (float)((double)params[P_KEY] * exp2((double)params[P_EV] - m));
    }
    E[k] = e;
  }
}

// ------------------------------------------------------------------------------------------ blur
// rows pass: out[row, i] = sum_t w[t] s[row, i + 3 (t - r)], i a float of the row's 3 W, s = max(E lin - threshold, 0), 0 outside
__global__ __launch_bounds__(256) void display_blur_rows_kernel(const float* __restrict__ lin, const float* __restrict__ E, int KE,
                                                                const float* __restrict__ params, const float* __restrict__ weights, int r,
                                                                int64_t rows, int H, int N, float* __restrict__ out) {
  __shared__ float sS[kRowTile + 6 * kMaxRadius];
  __shared__ float sW[2 * kMaxRadius + 1];
  for (int i = threadIdx.x; i < 2 * r + 1; i += 256) sW[i] = weights[i];
  const float thr = params[P_THRESHOLD];
  const int tiles = (N + kRowTile - 1) / kRowTile;
  const int64_t units = rows * tiles;
  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t row = unit / tiles;
    const int i0 = (int)(unit - row * tiles) * kRowTile;
    const float e = E[KE == 1 ? 0 : row / H];
    const float* src = lin + row * N;
    __syncthreads();  // (the previous unit's reads of sS, and sW on the first)
    for (int i = threadIdx.x; i < kRowTile + 6 * r; i += 256) {
      const int j = i0 - 3 * r + i;
      sS[i] = (j >= 0 && j < N) ? fmaxf(__fsub_rn(__fmul_rn(e, src[j]), thr), 0.0f) : 0.0f;
    }
    __syncthreads();
    const int i = i0 + threadIdx.x;
    if (i < N) {
      float acc = 0.0f;
      for (int t = 0; t <= 2 * r; ++t) acc = fmaf(sW[t], sS[threadIdx.x + 3 * t], acc);
      out[row * N + i] = acc;
    }
  }
}

// columns pass: out[k, y, i] = sum_t w[t] in[k, y + t - r, i], 0 outside the image's own rows
__global__ __launch_bounds__(256) void display_blur_cols_kernel(const float* __restrict__ in, const float* __restrict__ weights, int r, int K,
                                                                int H, int N, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float sT[];  // [kColTile + 2 r][64]
  __shared__ float sW[2 * kMaxRadius + 1];
  for (int i = threadIdx.x; i < 2 * r + 1; i += 256) sW[i] = weights[i];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int xt = (N + 63) / 64, yt = (H + kColTile - 1) / kColTile;
  const int64_t units = (int64_t)K * yt * xt;
  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int k = (int)(unit / ((int64_t)yt * xt));
    const int rem = (int)(unit - (int64_t)k * yt * xt);
    const int y0 = (rem / xt) * kColTile, i = (rem % xt) * 64 + tx;
    const float* img = in + (int64_t)k * H * N;
    __syncthreads();
    for (int q = ty; q < kColTile + 2 * r; q += 4) {
      const int y = y0 - r + q;
      sT[q * 64 + tx] = (y >= 0 && y < H && i < N) ? img[(int64_t)y * N + i] : 0.0f;
    }
    __syncthreads();
    if (i < N) {
      for (int q = ty; q < kColTile; q += 4) {
        const int y = y0 + q;
        if (y >= H) break;
        float acc = 0.0f;
        for (int t = 0; t <= 2 * r; ++t) acc = fmaf(sW[t], sT[(q + t) * 64 + tx], acc);
        out[((int64_t)k * H + y) * N + i] = acc;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ map
// Hable's operator with the constant terms cancelled on paper, so that its value at 0 is exactly 0:
//   h(v) = (v (A v + C B) + D E) / (v (A v + B) + D F) - E / F = v (A (F - E) v + B (F C - E)) / (F (v (A v + B) + D F))
constexpr double kHableWhite = 11.2;
constexpr double hable_d(double v) { return v * (0.042 * v + 0.005) / (0.3 * (v * (0.15 * v + 0.5) + 0.06)); }
__device__ __forceinline__ float hable(float v) { return v * (0.042f * v + 0.005f) / (0.3f * (v * (0.15f * v + 0.5f) + 0.06f)); }

template <int CURVE>
__device__ __forceinline__ float curve(float x, float inv_w2) {
  if (CURVE == NSKY_DISPLAY_REINHARD) return x * (1.0f + x * inv_w2) / (1.0f + x);
  if (CURVE == NSKY_DISPLAY_ACES) return x * (2.51f * x + 0.03f) / (x * (2.43f * x + 0.59f) + 0.14f);
  if (CURVE == NSKY_DISPLAY_HABLE) return hable(2.0f * x) * (float)(1.0 / hable_d(kHableWhite));
  return x;
}

template <int CURVE>
__device__ __forceinline__ float shade(float l, float b, float e, float strength, bool bloom, float inv_w2) {
  const float v = bloom ? fmaf(strength, b, __fmul_rn(e, l)) : __fmul_rn(e, l);
  const float x = fminf(fmaxf(v, 0.0f), 0x1p60f);  // (fmaxf: a NaN becomes 0)
  return srgb_fwd(curve<CURVE>(x, inv_w2));
}

__device__ __forceinline__ unsigned to8(float v) { return (unsigned)rintf(__fmul_rn(255.0f, v)); }

template <int CURVE, bool VEC>
__global__ __launch_bounds__(256) void display_map_kernel(const float* __restrict__ lin, const float* __restrict__ B,
                                                          const float* __restrict__ E, int KE, const float* __restrict__ params, int64_t P,
                                                          int64_t total, uint8_t* __restrict__ rgb8, float* __restrict__ rgb) {
  const float strength = params[P_STRENGTH], w = params[P_WHITE];
  const float inv_w2 = 1.0f / (w * w);
  const bool bloom = B != nullptr;
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  if (VEC) {  // P % 4 == 0: the 4 pixels of a group lie in one image
    for (int64_t g = first; g < total / 4; g += step) {
      const float e = E[KE == 1 ? 0 : (g * 4) / P];
      float l[12], b[12], o[12];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float4 v = ldg4(lin + g * 12 + 4 * q);
        l[4 * q] = v.x; l[4 * q + 1] = v.y; l[4 * q + 2] = v.z; l[4 * q + 3] = v.w;
        float4 u = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (bloom) u = ldg4(B + g * 12 + 4 * q);
        b[4 * q] = u.x; b[4 * q + 1] = u.y; b[4 * q + 2] = u.z; b[4 * q + 3] = u.w;
      }
#pragma unroll
      for (int j = 0; j < 12; ++j) o[j] = shade<CURVE>(l[j], b[j], e, strength, bloom, inv_w2);
      unsigned* o8 = (unsigned*)(rgb8 + g * 12);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        o8[q] = to8(o[4 * q]) | (to8(o[4 * q + 1]) << 8) | (to8(o[4 * q + 2]) << 16) | (to8(o[4 * q + 3]) << 24);
        if (rgb) stg4(rgb + g * 12 + 4 * q, make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]));
      }
    }
  } else {
    for (int64_t i = first; i < total * 3; i += step) {
      const float e = E[KE == 1 ? 0 : (i / 3) / P];
      const float o = shade<CURVE>(lin[i], bloom ? B[i] : 0.0f, e, strength, bloom, inv_w2);
      rgb8[i] = (uint8_t)to8(o);
      if (rgb) rgb[i] = o;
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int CURVE>
void launch_map(hipStream_t st, const float* lin, const float* B, const float* E, int KE, const float* params, int64_t P, int64_t total,
                uint8_t* rgb8, float* rgb) {
  const bool vec = P % 4 == 0 && aligned16(lin) && aligned16(B) && aligned16(rgb) && ((uintptr_t)rgb8 & 3) == 0;
  const int64_t items = vec ? total / 4 : total * 3;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 256 * 16));
  if (vec)
    hipLaunchKernelGGL((display_map_kernel<CURVE, true>), dim3(grid), dim3(256), 0, st, lin, B, E, KE, params, P, total, rgb8, rgb);
  else
    hipLaunchKernelGGL((display_map_kernel<CURVE, false>), dim3(grid), dim3(256), 0, st, lin, B, E, KE, params, P, total, rgb8, rgb);
}

}  // namespace

extern "C" int nsky_display_histogram(const float* lin, const float* mask, const float* params, int64_t P, int32_t K, int32_t shared,
                                      int64_t* hist, nsky_stream_t stream) {
  NSKY_CHECK_ARG(P >= 0 && K >= 0 && K <= 65535, "nsky_display_histogram: P %ld, K %d (0..65535)", (long)P, (int)K);
  if (P == 0 || K == 0) return NSKY_OK;
  NSKY_CHECK_ARG(lin && params && hist, "nsky_display_histogram: NULL lin / params / hist");
  const bool vec = P % 4 == 0 && aligned16(lin) && aligned16(mask);
  const int64_t items = vec ? P / 4 : P;
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 256)), (unsigned)K);
  const int row_stride = shared ? 0 : kBins;
  if (vec)
    hipLaunchKernelGGL(display_histogram_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, lin, mask, params, P, row_stride,
                       (unsigned long long*)hist);
  else
    hipLaunchKernelGGL(display_histogram_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, lin, mask, params, P, row_stride,
                       (unsigned long long*)hist);
  NSKY_CHECK_LAUNCH("nsky_display_histogram");
  return NSKY_OK;
}

extern "C" int nsky_display_exposure(const int64_t* hist, const float* params, int32_t K, float* E, nsky_stream_t stream) {
  NSKY_CHECK_ARG(K >= 0, "nsky_display_exposure: K %d", (int)K);
  if (K == 0) return NSKY_OK;
  NSKY_CHECK_ARG(hist && params && E, "nsky_display_exposure: NULL hist / params / E");
  hipLaunchKernelGGL(display_exposure_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, (const long long*)hist, params, E);
  NSKY_CHECK_LAUNCH("nsky_display_exposure");
  return NSKY_OK;
}

extern "C" int nsky_display_blur(const float* lin, const float* E, int32_t KE, const float* params, const float* weights, int32_t radius,
                                 int32_t K, int32_t H, int32_t W, float* scratch, float* B, nsky_stream_t stream) {
  NSKY_CHECK_ARG(K >= 0 && H >= 0 && W >= 0 && W <= (1 << 29), "nsky_display_blur: K %d, H %d, W %d", (int)K, (int)H, (int)W);
  NSKY_CHECK_ARG(radius >= 1 && radius <= kMaxRadius, "nsky_display_blur: radius %d (1..%d)", (int)radius, kMaxRadius);
  NSKY_CHECK_ARG(KE == 1 || KE == K, "nsky_display_blur: %d exposures for %d images", (int)KE, (int)K);
  if (K == 0 || H == 0 || W == 0) return NSKY_OK;
  NSKY_CHECK_ARG(lin && E && params && weights && scratch && B, "nsky_display_blur: NULL lin / E / params / weights / scratch / B");
  hipStream_t st = (hipStream_t)stream;
  const int N = 3 * W;
  const int64_t rows = (int64_t)K * H;
  const int64_t row_units = rows * ((N + kRowTile - 1) / kRowTile);
  hipLaunchKernelGGL(display_blur_rows_kernel, dim3((unsigned)std::min<int64_t>(row_units, 256 * 16)), dim3(256), 0, st, lin, E, (int)KE,
                     params, weights, (int)radius, rows, (int)H, N, scratch);
  NSKY_CHECK_LAUNCH("nsky_display_blur (rows)");
  const int64_t col_units = (int64_t)K * ((H + kColTile - 1) / kColTile) * ((N + 63) / 64);
  const size_t lds = (size_t)(kColTile + 2 * radius) * 64 * sizeof(float);  // 57 344 bytes at radius 96
  hipLaunchKernelGGL(display_blur_cols_kernel, dim3((unsigned)std::min<int64_t>(col_units, 256 * 8)), dim3(256), lds, st, scratch, weights,
                     (int)radius, (int)K, (int)H, N, B);
  NSKY_CHECK_LAUNCH("nsky_display_blur (columns)");
  return NSKY_OK;
}

extern "C" int nsky_display_map(const float* lin, const float* B, const float* E, int32_t KE, const float* params, int32_t curve, int64_t P,
                                int32_t K, uint8_t* rgb8, float* rgb, nsky_stream_t stream) {
  NSKY_CHECK_ARG(P >= 0 && K >= 0, "nsky_display_map: P %ld, K %d", (long)P, (int)K);
  NSKY_CHECK_ARG(curve >= NSKY_DISPLAY_CLAMP && curve <= NSKY_DISPLAY_HABLE, "nsky_display_map: curve %d", (int)curve);
  NSKY_CHECK_ARG(KE == 1 || KE == K, "nsky_display_map: %d exposures for %d images", (int)KE, (int)K);
  if (P == 0 || K == 0) return NSKY_OK;
  NSKY_CHECK_ARG(lin && E && params && rgb8, "nsky_display_map: NULL lin / E / params / rgb8");
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = P * K;
  switch (curve) {
    case NSKY_DISPLAY_REINHARD: launch_map<NSKY_DISPLAY_REINHARD>(st, lin, B, E, KE, params, P, total, rgb8, rgb); break;
    case NSKY_DISPLAY_ACES: launch_map<NSKY_DISPLAY_ACES>(st, lin, B, E, KE, params, P, total, rgb8, rgb); break;
    case NSKY_DISPLAY_HABLE: launch_map<NSKY_DISPLAY_HABLE>(st, lin, B, E, KE, params, P, total, rgb8, rgb); break;
    default: launch_map<NSKY_DISPLAY_CLAMP>(st, lin, B, E, KE, params, P, total, rgb8, rgb); break;
  }
  NSKY_CHECK_LAUNCH("nsky_display_map");
  return NSKY_OK;
}
