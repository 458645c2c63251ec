// Precomputed radiance transfer of one frame (neusky_amd/relight/transfer.py).  Definitions: include/neusky_hip.h.
//
// The hemisphere renderer (render.hip, hemi_fwd_kernel) is linear in the light colours.  With the order of its two sums swapped,
//   T[r,d,c] = vis[r,d] sum_s w[r,s] alb[r,s,c] clamp(n[r,s].dir[d], 0, 1) / cnt[r,s]
//   lin[r,c] = sum_d T[r,d,c] L[d,c] + bg[r,c] (1 - acc[r])
// and T, acc depend on the camera and the scene only.
//   bake     one workgroup (4 waves) per ray, the work of hemi_fwd_kernel: wave w takes samples w, w+4, ...; a lane keeps its directions
//            and its slice of the row (fp64) in registers; the four partial rows meet in LDS in wave order, the row maximum is reduced
//            there, and the row is rounded and stored once (fp32, or fp16 scaled by a per-row power of two).
//   relight  a wave takes 4 rows and up to 8 lights: 16 bytes of T per lane per load (1 KB contiguous per wave), the lights in LDS,
//            each LDS read of a light shared by the 4 rows; fp32 accumulation; one fixed butterfly reduces every sum of the wave.
// No atomics: every output is a pure function of the inputs, so two runs agree bit for bit.  Flat indices are 64-bit.  Nothing
// here synchronises with the host.
#include <algorithm>

#include "light_pass.h"
#include "numerics.h"
#include "transfer_rows.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr int kMaxDirs = NSKY_TRANSFER_MAX_DIRECTIONS;
constexpr int kMaxLightsPerPass = 8;
constexpr int kRowsPerWave = 4;
constexpr int kLdsBudget = 64 * 1024;  // bytes of light colours per workgroup

// ------------------------------------------------------------------------------------------ bake
// NQ = ceil(D / 64) rounded up to a power of two: the directions a lane owns are j = lane + 64 q, q < NQ.
// The row is accumulated in fp64 and rounded once on the way out (an element is then within half an ulp of the definition evaluated on
// the fp32 inputs, whatever S is); the count of a sample comes from the fp32 cosine of hemi_fwd_kernel, so that a frame relit from its
// transfer counts the directions the frame render counts.
template <int NQ, bool HALF>
__global__ __launch_bounds__(256) void transfer_bake_kernel(const float* __restrict__ albedo, const float* __restrict__ normals,
                                                            const float* __restrict__ weights, const float* __restrict__ dirs,
                                                            const float* __restrict__ vis, int R, int S, int D, void* __restrict__ T,
                                                            int64_t row0, int* __restrict__ exps, float* __restrict__ acc) {
  constexpr int NE = NQ * 192;                // padded row length (elements)
  constexpr int NG = (NE / 4 + 255) / 256;    // groups of 4 elements per thread
  __shared__ __attribute__((aligned(16))) double sA[NE];
  __shared__ double red[4], redw[4];
  const int r = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float dx[NQ], dy[NQ], dz[NQ];
  double A[NQ][3];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int j = lane + 64 * q;
    const bool in = j < D;
    dx[q] = in ? dirs[3 * j] : 0.0f;
    dy[q] = in ? dirs[3 * j + 1] : 0.0f;
    dz[q] = in ? dirs[3 * j + 2] : 0.0f;
    A[q][0] = A[q][1] = A[q][2] = 0.0;
  }
  double wsum = 0.0;
  for (int s = wave; s < S; s += 4) {
    const int64_t o = ((int64_t)r * S + s) * 3;
    const float nx = normals[o], ny = normals[o + 1], nz = normals[o + 2];
    float cnt = 0.0f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float v = nx * dx[q] + ny * dy[q] + nz * dz[q];  // the expression of hemi_fwd_kernel
      v = fminf(fmaxf(v, 0.0f), 1.0f);
      cnt += v > 0.0f ? 1.0f : 0.0f;  // (a padded direction is zero: never counted)
    }
    cnt = wave_sum(cnt);  // an exact integer <= D in every order
    const double w = weights[(int64_t)r * S + s];
    const double inv = 1.0 / (double)(cnt > 0.0f ? cnt : 1.0f);
    const double g0 = w * (double)albedo[o] * inv, g1 = w * (double)albedo[o + 1] * inv, g2 = w * (double)albedo[o + 2] * inv;
    const double mx_ = nx, my_ = ny, mz_ = nz;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      double d = mx_ * (double)dx[q] + my_ * (double)dy[q] + mz_ * (double)dz[q];
      d = fmin(fmax(d, 0.0), 1.0);
      A[q][0] = fma(g0, d, A[q][0]);
      A[q][1] = fma(g1, d, A[q][1]);
      A[q][2] = fma(g2, d, A[q][2]);
    }
    wsum += w;
  }
  // the four partial rows meet in one LDS row, in wave order
  if (lane == 0) redw[wave] = wsum;
  for (int turn = 0; turn < 4; ++turn) {
    if (wave == turn) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = lane + 64 * q;
#pragma unroll
        for (int c = 0; c < 3; ++c) sA[3 * j + c] = turn == 0 ? A[q][c] : sA[3 * j + c] + A[q][c];
      }
    }
    __syncthreads();
  }
  const int N = 3 * D;
  double v[NG][4], mx = 0.0;
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const int i0 = 4 * (threadIdx.x + 256 * k);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = i0 + e;
      v[k][e] = 0.0;
      if (i < N) {
        const double vj = vis ? (double)vis[(int64_t)r * D + i / 3] : 1.0;
        v[k][e] = vj * sA[i];
        mx = fmax(mx, fabs(v[k][e]));
      }
    }
  }
  int ex = 0;
  if (HALF) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    ex = row_exponent(mx);
  }
  if (threadIdx.x == 0) {
    acc[r] = (float)(((redw[0] + redw[1]) + redw[2]) + redw[3]);
    if (HALF) exps[r] = ex;
  }
  const int64_t base = (row0 + r) * (int64_t)N;
  const bool vec = (D & 3) == 0;  // rows start on a 16-byte (fp32) / 8-byte (fp16) boundary and hold whole groups
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const int i0 = 4 * (threadIdx.x + 256 * k);
    if (i0 >= N) continue;
    if (HALF) {
      __half* out = (__half*)T + base + i0;
      __half h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = __float2half_rn((float)ldexp(v[k][e], ex));
      if (vec) {
        *(uint2*)out = *(const uint2*)h;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i0 + e < N) out[e] = h[e];
      }
    } else {
      float* out = (float*)T + base + i0;
      if (vec) {
        *(float4*)out = make_float4((float)v[k][0], (float)v[k][1], (float)v[k][2], (float)v[k][3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i0 + e < N) out[e] = (float)v[k][e];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ relight
// Sum each of the NV values of a lane over the 64 lanes with the fewest exchanges: while the count is even, a lane hands half of its
// values to its partner and keeps the other half (so the count halves with the stride doubling); the rest is a plain butterfly.
// Afterwards lane l < 2^h holds, in slot i, the total of value i + first(l), where h is the number of halvings.
template <int NV, int BIT>
struct WaveReduce {
  static constexpr bool kHalve = NV % 2 == 0;
  static constexpr int kNext = kHalve ? NV / 2 : NV;
  using Next = WaveReduce<kNext, BIT + 1>;
  static constexpr int kHalvings = kHalve ? 1 + Next::kHalvings : 0;
  static constexpr int kFinal = Next::kFinal;
  __device__ __forceinline__ static int run(float* v, int lane) {
    if constexpr (kHalve) {
      const bool up = (lane >> BIT) & 1;
#pragma unroll
      for (int i = 0; i < NV / 2; ++i) {
        const float keep = up ? v[i + NV / 2] : v[i];
        const float send = up ? v[i] : v[i + NV / 2];
        v[i] = keep + __shfl_xor(send, 1 << BIT, 64);
      }
      return (up ? NV / 2 : 0) + Next::run(v, lane);
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] += __shfl_xor(v[i], 1 << BIT, 64);
      return Next::run(v, lane);
    }
  }
};
template <int NV>
struct WaveReduce<NV, 6> {
  static constexpr int kHalvings = 0;
  static constexpr int kFinal = NV;
  __device__ __forceinline__ static int run(float*, int) { return 0; }
};

// rows are [D*3] with D a multiple of 4 (fp32) / 8 (fp16): every 16-byte load lies inside one row and is aligned
template <int KB, bool HALF>
__global__ __launch_bounds__(256) void transfer_relight_kernel(const void* __restrict__ T, const int* __restrict__ exps,
                                                               const float* __restrict__ acc, const float* __restrict__ lights,
                                                               const float* __restrict__ bg, int64_t R, int D, float* __restrict__ rgb,
                                                               float* __restrict__ lin) {
  using Vec = RowVec<HALF>;
  constexpr int VE = Vec::kElems;
  constexpr int P = kRowsPerWave;
  extern __shared__ __attribute__((aligned(16))) float sL[];  // [KB][N]
  const int N = 3 * D;
  for (int i = threadIdx.x * 4; i < KB * N; i += 256 * 4) *(float4*)&sL[i] = *(const float4*)&lights[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nv = N / VE;             // 16-byte vectors per row
  const int nit = (nv + 63) / 64;
  // vector `v` of a row starts at element VE v, whose channel is (VE v) mod 3 = (VE mod 3)(lane + it) mod 3 as 64 mod 3 = 1; with
  // it = 3 m + t element e of it has channel (lb + u) mod 3, lb = (VE mod 3) lane mod 3, u = ((VE mod 3) t + e) mod 3: u is a constant
  const int lb = ((VE % 3) * lane) % 3;
  const int64_t units = (R + P - 1) / P;
  for (int64_t unit = (int64_t)blockIdx.x * 4 + wave; unit < units; unit += (int64_t)gridDim.x * 4) {
    int64_t row[P];
#pragma unroll
    for (int p = 0; p < P; ++p) row[p] = unit * P + p < R ? unit * P + p : R - 1;  // (a row past the end re-reads the last one; never written)
    float a[P][KB][3];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int k = 0; k < KB; ++k) a[p][k][0] = a[p][k][1] = a[p][k][2] = 0.0f;
    for (int it0 = 0; it0 < nit; it0 += 3) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int v = lane + 64 * (it0 + t);
        if (v < nv) {
          Vec tv[P];
#pragma unroll
          for (int p = 0; p < P; ++p) tv[p].load(T, row[p] * (int64_t)N + (int64_t)v * VE);
#pragma unroll
          for (int k = 0; k < KB; ++k) {
            float l[VE];
#pragma unroll
            for (int h = 0; h < VE / 4; ++h) {
              const float4 q = *(const float4*)&sL[k * N + v * VE + 4 * h];
              l[4 * h] = q.x; l[4 * h + 1] = q.y; l[4 * h + 2] = q.z; l[4 * h + 3] = q.w;
            }
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
              for (int e = 0; e < VE; ++e) {
                constexpr int m = VE % 3;
                const int u = (m * t + e) % 3;
                a[p][k][u] = fmaf(tv[p].get(e), l[e], a[p][k][u]);
              }
          }
        }
      }
    }
    // slot u of a lane is channel (lb + u) mod 3: channel c is slot (c - lb) mod 3
    constexpr int NV = P * KB * 3;
    float val[NV];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const float a0 = a[p][k][0], a1 = a[p][k][1], a2 = a[p][k][2];
        val[(p * KB + k) * 3 + 0] = lb == 0 ? a0 : (lb == 1 ? a2 : a1);
        val[(p * KB + k) * 3 + 1] = lb == 0 ? a1 : (lb == 1 ? a0 : a2);
        val[(p * KB + k) * 3 + 2] = lb == 0 ? a2 : (lb == 1 ? a1 : a0);
      }
    using Red = WaveReduce<NV, 0>;
    const int first = Red::run(val, lane);
    if (lane < (1 << Red::kHalvings)) {
#pragma unroll
      for (int i = 0; i < Red::kFinal; ++i) {
        const int id = first + i;
        const int c = id % 3, k = (id / 3) % KB, p = id / (3 * KB);
        const int64_t rr = unit * P + p;
        if (rr < R) {
          float s = val[i];
          if (HALF) s = ldexpf(s, -exps[rr]);
          const int64_t o = ((int64_t)k * R + rr) * 3 + c;
          const float x = s + bg[o] * (1.0f - acc[rr]);
          if (lin) lin[o] = x;
          rgb[o] = srgb_fwd(x);
        }
      }
    }
  }
}

// any D: one wave per row, one light at a time (the row is re-read from cache), scalar loads
template <bool HALF>
__global__ __launch_bounds__(256) void transfer_relight_any_kernel(const void* __restrict__ T, const int* __restrict__ exps,
                                                                   const float* __restrict__ acc, const float* __restrict__ lights,
                                                                   const float* __restrict__ bg, int64_t R, int D, int K,
                                                                   float* __restrict__ rgb, float* __restrict__ lin) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = 3 * D;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < R; r += (int64_t)gridDim.x * 4) {
    for (int k = 0; k < K; ++k) {
      float a[3] = {0.0f, 0.0f, 0.0f};
      // 192 = 3 * 64: lane l always meets channel l mod 3
      for (int i = lane; i < N; i += 192) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int j = i + 64 * q;
          if (j < N) {
            const float t = row_element<HALF>(T, r * N + j);
            a[q] = fmaf(t, lights[(int64_t)k * N + j], a[q]);
          }
        }
      }
      // slot q of lane l is channel (l + q) mod 3, as 64 mod 3 = 1
      const int lb = lane % 3;
      float c[3] = {lb == 0 ? a[0] : (lb == 1 ? a[2] : a[1]), lb == 0 ? a[1] : (lb == 1 ? a[0] : a[2]),
                    lb == 0 ? a[2] : (lb == 1 ? a[1] : a[0])};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) c[ch] = wave_sum(c[ch]);
      if (lane < 3) {
        float s = lane == 0 ? c[0] : (lane == 1 ? c[1] : c[2]);
        if (HALF) s = ldexpf(s, -exps[r]);
        const int64_t o = ((int64_t)k * R + r) * 3 + lane;
        const float x = s + bg[o] * (1.0f - acc[r]);
        if (lin) lin[o] = x;
        rgb[o] = srgb_fwd(x);
      }
    }
  }
}

int workgroups_per_cu(size_t lds) { return lds == 0 ? 4 : (int)std::min<size_t>(4, (160 * 1024) / lds); }

}  // namespace

extern "C" int nsky_transfer_bake(const float* albedo, const float* normals, const float* weights, const float* dirs, const float* vis,
                                  int32_t R, int32_t S, int32_t D, int32_t storage, void* T, int64_t row0, int32_t* exponents, float* acc,
                                  nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && S >= 1 && D >= 1 && D <= kMaxDirs && row0 >= 0, "nsky_transfer_bake: R %d, S %d, D %d (1..%d), row0 %ld", (int)R,
                 (int)S, (int)D, kMaxDirs, (long)row0);
  NSKY_CHECK_ARG(storage == NSKY_TRANSFER_FP32 || storage == NSKY_TRANSFER_FP16, "nsky_transfer_bake: storage %d", (int)storage);
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(albedo && normals && weights && dirs && T && acc, "nsky_transfer_bake: NULL albedo / normals / weights / dirs / T / acc");
  const bool half = storage == NSKY_TRANSFER_FP16;
  NSKY_CHECK_ARG(!half || exponents, "nsky_transfer_bake: fp16 storage needs the row exponents");
  hipStream_t st = (hipStream_t)stream;
  return with_count<1, 2, 4, 8, 16>((D + 63) / 64, [&](auto nq) {
    return with_storage(half, [&](auto h) {
      hipLaunchKernelGGL((transfer_bake_kernel<decltype(nq)::value, decltype(h)::value>), dim3(R), dim3(256), 0, st, albedo, normals, weights,
                         dirs, vis, R, S, D, T, row0, exponents, acc);
      NSKY_CHECK_LAUNCH("nsky_transfer_bake");
      return NSKY_OK;
    });
  });
}

extern "C" int nsky_transfer_relight(const void* T, int32_t storage, const int32_t* exponents, const float* acc, const float* lights,
                                     const float* bg, int64_t R, int32_t D, int32_t K, float* rgb, float* lin, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && D >= 1 && D <= kMaxDirs && K >= 0, "nsky_transfer_relight: R %ld, D %d (1..%d), K %d", (long)R, (int)D, kMaxDirs,
                 (int)K);
  NSKY_CHECK_ARG(storage == NSKY_TRANSFER_FP32 || storage == NSKY_TRANSFER_FP16, "nsky_transfer_relight: storage %d", (int)storage);
  if (R == 0 || K == 0) return NSKY_OK;
  NSKY_CHECK_ARG(T && acc && lights && bg && rgb, "nsky_transfer_relight: NULL T / acc / lights / bg / rgb");
  const bool half = storage == NSKY_TRANSFER_FP16;
  NSKY_CHECK_ARG(!half || exponents, "nsky_transfer_relight: fp16 storage needs the row exponents");
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = (int64_t)D * 3;
  if (D % (half ? 8 : 4) != 0)
    return with_storage(half, [&](auto h) {
      hipLaunchKernelGGL((transfer_relight_any_kernel<decltype(h)::value>), dim3(capped_grid((R + 3) / 4, 8)), dim3(256), 0, st, T, exponents, acc,
                         lights, bg, R, (int)D, (int)K, rgb, lin);
      NSKY_CHECK_LAUNCH("nsky_transfer_relight");
      return NSKY_OK;
    });
  // the lights of one pass share the workgroup's LDS: up to 8, fewer when D is large; T is read once per pass
  const int per_pass = (int)std::min<int64_t>(kMaxLightsPerPass, kLdsBudget / (N * (int64_t)sizeof(float)));
  const int64_t units = (R + kRowsPerWave - 1) / kRowsPerWave;
  return for_each_pass<kMaxLightsPerPass>(K, [&](int k0, auto kb) {
    const size_t lds = (size_t)kb * D * 3 * sizeof(float);
    const int64_t o = (int64_t)k0 * R * 3;
    return with_storage(half, [&](auto h) {
      hipLaunchKernelGGL((transfer_relight_kernel<decltype(kb)::value, decltype(h)::value>), dim3(capped_grid((units + 3) / 4, workgroups_per_cu(lds))),
                         dim3(256), lds, st, T, exponents, acc, lights + k0 * N, bg + o, R, D, rgb + o, lin ? lin + o : nullptr);
      NSKY_CHECK_LAUNCH("nsky_transfer_relight");
      return NSKY_OK;
    });
  }, per_pass);
}
