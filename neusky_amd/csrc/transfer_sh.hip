// A baked radiance transfer in a basis of the light directions (neusky_amd/relight/transfer_sh.py).  Definitions: include/neusky_hip.h.
//
// The relight of transfer.hip is linear in the light: with a basis B [D, J] of the directions,
//   sum_d T[r,d,c] L[d,c] = sum_j C[r,j,c] l[j,c],   C = T B,   l = B^T L   (for L in the span of an orthonormal B)
// and a row of C holds 3 J numbers where a row of T holds 3 D.  Both kernels take any B: nothing here knows what the basis is.
//   project        a workgroup takes 64 (4 / NJW) rows and walks the directions in blocks of 16: the block of T goes to LDS as fp32 (8- or
//                  16-byte loads where the rows allow them), the block of B beside it, zero-padded; a lane owns ONE row and JT coefficients
//                  of it in registers (the NJW waves of a row group split J), reads its row 16 bytes at a time (the row stride is 4 x 13
//                  dwords: conflict-free) and B as 16-byte broadcasts; fp32 FMAs in the order of d.  A row's sums depend on that row
//                  alone, so a chunk of a frame projects to the bits the whole frame projects to.
//   relight_short  a workgroup takes 64 (or, for long rows, 32) whole rows of C, which are contiguous: 16-byte loads of the flat tile
//                  into LDS rows padded with zeros to a multiple of 12 (4 coefficients x 3 channels: the channel of a slot is then a
//                  constant); 4 (or 8) lanes share a row, each takes every 4th (8th) group of 12; the lights of the pass sit in LDS as
//                  doubles.  The sums are fp64 (the products are exact), folded over the lanes of the row, and leave through LDS: a
//                  light's rows of the tile are consecutive in bg, lin and rgb, read and written as whole lines, rounded once.
// No atomics and a fixed order everywhere: two runs agree bit for bit.  Flat indices are 64-bit.  Nothing synchronises with the host.
#include <algorithm>

#include "light_pass.h"
#include "numerics.h"
#include "transfer_rows.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr int kMaxDirs = NSKY_TRANSFER_MAX_DIRECTIONS;
constexpr int kMaxCoeffs = NSKY_TRANSFER_MAX_COEFFICIENTS;
constexpr int kMaxLightsPerPass = 8;

// ------------------------------------------------------------------------------------------ project
constexpr int kDirBlock = 16;                // directions per block: 48 floats of a row
constexpr int kBlockElems = kDirBlock * 3;   // 12 groups of 4
constexpr int kTileStride = 52;              // dwords between the rows of the LDS tile: 4 x an odd number, so that the 16 lanes a 16-byte
                                             // read serves together (16 rows, all different mod 16) meet 64 different banks

template <int JT, bool HALF>
__global__ __launch_bounds__(256) void transfer_project_kernel(const void* __restrict__ T, const int* __restrict__ exps,
                                                               const float* __restrict__ B, int64_t R, int D, int J, int njw,
                                                               void* __restrict__ C, int64_t row0, int* __restrict__ cexps, int out_half) {
  static_assert(JT % 4 == 0, "a lane reads B four coefficients at a time");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int rows = 64 * (4 / njw);   // rows of the tile
  const int jpad = JT * njw;         // coefficients of the padded B block
  float* sT = lds;                   // [rows][kTileStride]
  float* sB = lds + rows * kTileStride;  // [kDirBlock][jpad]
  float* sM = sB + kDirBlock * jpad;     // [njw][rows]: the partial row maxima (fp16 output)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jw = wave % njw, rg = wave / njw;
  const int lrow = rg * 64 + lane;   // this lane's row of the tile
  const int j0 = jw * JT;
  const int N = 3 * D;
  // rows start on a 16-byte (fp32) / 8-byte (fp16) boundary and hold whole groups of 4
  const bool vec = (D & 3) == 0 && ((uintptr_t)T & (HALF ? 7 : 15)) == 0;
  const int64_t tiles = (R + rows - 1) / rows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * rows;
    float acc[JT][3];
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.0f;
    for (int d0 = 0; d0 < D; d0 += kDirBlock) {
      __syncthreads();  // the block before this one has been read
      const int k0 = 3 * d0;
      if (vec) {
        // six loads in flight per thread, then their stores: one at a time, a block would wait out a memory latency per load.  A
        // group outside the frame reads element 0 (always there) and stores zeros
        constexpr int G = kBlockElems / 4, kInFlight = 6;
        const int items = rows * G;
        for (int i0 = threadIdx.x; i0 < items; i0 += 256 * kInFlight) {
          float4 v[kInFlight];
#pragma unroll
          for (int u = 0; u < kInFlight; ++u) {
            const int i = i0 + 256 * u;
            const int rr = i / G, k = k0 + 4 * (i % G);
            const bool in = i < items && r0 + rr < R && k < N;
            const int64_t e = in ? (r0 + rr) * (int64_t)N + k : 0;
            v[u] = row_load4<HALF>(T, e);
            if (!in) v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          }
#pragma unroll
          for (int u = 0; u < kInFlight; ++u) {
            const int i = i0 + 256 * u;
            if (i < items) *(float4*)&sT[(i / G) * kTileStride + 4 * (i % G)] = v[u];
          }
        }
      } else {
        for (int i = threadIdx.x; i < rows * kBlockElems; i += 256) {
          const int rr = i / kBlockElems, kk = i % kBlockElems;
          float v = 0.0f;
          if (r0 + rr < R && k0 + kk < N) v = row_element<HALF>(T, (r0 + rr) * (int64_t)N + k0 + kk);
          sT[rr * kTileStride + kk] = v;
        }
      }
      for (int i = threadIdx.x; i < kDirBlock * jpad; i += 256) {
        const int dd = i / jpad, j = i % jpad;
        sB[i] = (d0 + dd < D && j < J) ? B[(int64_t)(d0 + dd) * J + j] : 0.0f;
      }
      __syncthreads();
#pragma unroll 1  // (unrolled, the compiler hoists every read of the block: 350 registers at JT = 36, one wave per SIMD)
      for (int g = 0; g < kDirBlock / 4; ++g) {  // 4 directions: 12 floats of the row, 3 reads
        float t[12];
#pragma unroll
        for (int h = 0; h < 3; ++h) {
          const float4 q = *(const float4*)&sT[lrow * kTileStride + 12 * g + 4 * h];
          t[4 * h] = q.x; t[4 * h + 1] = q.y; t[4 * h + 2] = q.z; t[4 * h + 3] = q.w;
        }
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) {
#pragma unroll
          for (int jq = 0; jq < JT / 4; ++jq) {
            const float4 b4 = *(const float4*)&sB[(4 * g + dd) * jpad + j0 + 4 * jq];
            const float b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int c = 0; c < 3; ++c) acc[4 * jq + e][c] = fmaf(t[3 * dd + c], b[e], acc[4 * jq + e][c]);
          }
          __builtin_amdgcn_sched_barrier(0);  // one direction's reads of B in flight, not four
        }
      }
    }
    const int64_t r = r0 + lrow;
    const bool live = r < R;
    if (HALF) {  // the input row's own power of two: exact
      const int ein = live ? exps[r] : 0;
#pragma unroll
      for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[j][c] = ldexpf(acc[j][c], -ein);
    }
    int ex = 0;
    if (out_half) {  // (uniform) the row maximum over the waves that share the row, in wave order
      float mx = 0.0f;
#pragma unroll
      for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) mx = fmaxf(mx, fabsf(acc[j][c]));  // (a padded coefficient is zero)
      sM[jw * rows + lrow] = mx;
      __syncthreads();
      mx = sM[lrow];
      for (int w = 1; w < njw; ++w) mx = fmaxf(mx, sM[w * rows + lrow]);
      ex = row_exponent(mx);
      if (live && jw == 0) cexps[row0 + r] = ex;
    }
    if (live) {
      const int64_t base = (row0 + r) * (int64_t)J * 3;
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        if (j0 + j < J) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int64_t o = base + (int64_t)(j0 + j) * 3 + c;
            if (out_half) ((__half*)C)[o] = __float2half_rn(ldexpf(acc[j][c], ex));
            else ((float*)C)[o] = acc[j][c];
          }
        }
      }
    }
  }
}

// the smallest (JT, njw) of the instantiations below whose JT njw coefficients hold J
struct ProjectShape {
  int jt, njw;
};
ProjectShape project_shape(int J, int64_t R) {
  const int jts[] = {4, 12, 16, 24, 28, 36};
  ProjectShape best{36, 4};
  // a chunk of a bake is a few thousand rows: tiles of 64 rows (4 waves per row group) spread it over more CUs.  The shape does not
  // reach the bits: a coefficient is summed in the order of d by whichever lane holds it
  const int min_njw = R <= 64 * 256 ? 4 : 1;
  for (int njw = 4; njw >= min_njw; njw /= 2)
    for (int jt : jts)
      if (jt * njw >= J && jt * njw <= best.jt * best.njw) best = ProjectShape{jt, njw};  // on a tie the fewer waves per row: more rows per tile
  return best;
}

template <int JT>
int launch_project(bool half, hipStream_t st, const void* T, const int* exps, const float* B, int64_t R, int D, int J, int njw, void* C,
                   int64_t row0, int* cexps, int out_half) {
  const int rows = 64 * (4 / njw);
  const size_t lds = ((size_t)rows * kTileStride + (size_t)kDirBlock * JT * njw + (size_t)njw * rows) * sizeof(float);
  const int64_t tiles = (R + rows - 1) / rows;
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / lds));
  return with_storage(half, [&](auto h) {
    hipLaunchKernelGGL((transfer_project_kernel<JT, decltype(h)::value>), dim3(capped_grid(tiles, per_cu)), dim3(256), lds, st, T, exps, B, R, D,
                       J, njw, C, row0, cexps, out_half);
    NSKY_CHECK_LAUNCH("nsky_transfer_project");
    return NSKY_OK;
  });
}

// ------------------------------------------------------------------------------------------ relight of short rows
// the dwords between the rows of the LDS tile: the row padded to whole groups of 12, then up to 16 mod 32 -- the 16 lanes that a 16-byte
// read serves together are, at 4 lanes per row, 4 rows (one of each residue mod 4) x 4 consecutive groups, and then meet 64 different banks
inline int short_stride(int J) {
  const int n12 = (3 * J + 11) / 12 * 12;
  return n12 + ((16 - n12 % 32) + 32) % 32;
}

template <int KB, bool HALF>
__global__ __launch_bounds__(256) void transfer_relight_short_kernel(const void* __restrict__ Cm, const int* __restrict__ exps,
                                                                     const float* __restrict__ acc, const float* __restrict__ lights,
                                                                     const float* __restrict__ bg, int64_t R, int J, int stride, int lsh,
                                                                     float* __restrict__ rgb, float* __restrict__ lin) {
  constexpr int VE = RowVec<HALF>::kElems;  // elements of a 16-byte load
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = 3 * J;
  const int units = (N + 11) / 12;
  const int n12 = units * 12;
  const int lpr = 1 << lsh;                   // lanes per row: 4 or 8
  const int rows = 256 >> lsh;                // rows of a tile: 64 or 32
  double* sL = (double*)lds;                  // [KB][n12], zero past N
  float* sC = lds + 2 * KB * n12;             // [rows][stride], zero past N
  double* sO = (double*)(sC + rows * stride); // [KB][rows][3]: the sums on their way out
  for (int i = threadIdx.x; i < KB * n12; i += 256) {
    const int k = i / n12, e = i % n12;
    sL[i] = e < N ? (double)lights[(int64_t)k * N + e] : 0.0;
  }
  for (int i = threadIdx.x; i < rows * stride; i += 256) sC[i] = 0.0f;  // (the pads stay zero: a tile writes elements below N only)
  const int row = threadIdx.x >> lsh, q = threadIdx.x & (lpr - 1);
  const int64_t total = R * (int64_t)N;
  const int64_t tiles = (R + rows - 1) / rows;
  const int tile_elems = rows * N;  // a multiple of 32: every tile starts on a 16-byte boundary
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();  // the tile before this one has been read (and, the first time, the zeros are in place)
    const int64_t e0 = tile * (int64_t)tile_elems;
    for (int v = threadIdx.x * VE; v < tile_elems; v += 256 * VE) {
      float x[VE];
      const int64_t e = e0 + v;
      if (e + VE <= total) {
        RowVec<HALF> raw;
        raw.load(Cm, e);
#pragma unroll
        for (int i = 0; i < VE; ++i) x[i] = raw.get(i);
      } else {
#pragma unroll
        for (int i = 0; i < VE; ++i) x[i] = e + i < total ? row_element<HALF>(Cm, e + i) : 0.0f;
      }
      int rr = v / N, k = v % N;
#pragma unroll
      for (int i = 0; i < VE; ++i) {
        if (rr < rows) sC[rr * stride + k] = x[i];
        if (++k == N) {
          k = 0;
          ++rr;
        }
      }
    }
    __syncthreads();
    double a[KB][3];
#pragma unroll
    for (int k = 0; k < KB; ++k) a[k][0] = a[k][1] = a[k][2] = 0.0;
    for (int u = q; u < units; u += lpr) {
      double t[12];
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const float4 c4 = *(const float4*)&sC[row * stride + 12 * u + 4 * h];
        t[4 * h] = c4.x; t[4 * h + 1] = c4.y; t[4 * h + 2] = c4.z; t[4 * h + 3] = c4.w;
      }
#pragma unroll
      for (int k = 0; k < KB; ++k)
#pragma unroll
        for (int e = 0; e < 12; e += 2) {
          const double2 l2 = *(const double2*)&sL[k * n12 + 12 * u + e];
          a[k][e % 3] = fma(t[e], l2.x, a[k][e % 3]);
          a[k][(e + 1) % 3] = fma(t[e + 1], l2.y, a[k][(e + 1) % 3]);
        }
    }
    // the lanes of a row, in one fixed order
#pragma unroll
    for (int k = 0; k < KB; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        a[k][c] += __shfl_xor(a[k][c], 1, 64);
        a[k][c] += __shfl_xor(a[k][c], 2, 64);
        if (lsh == 3) a[k][c] += __shfl_xor(a[k][c], 4, 64);  // (uniform)
      }
    const int64_t r0 = tile * rows;
    const double scale = HALF && r0 + row < R ? ldexp(1.0, -exps[r0 + row]) : 1.0;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      if ((k & (lpr - 1)) == q) {  // lane q hands over lights q, q + lpr, ...
#pragma unroll
        for (int c = 0; c < 3; ++c) sO[(k * rows + row) * 3 + c] = a[k][c] * scale;
      }
    }
    __syncthreads();
    // a light's rows of the tile are 3 `rows` consecutive floats of bg, lin and rgb: whole cache lines per wave
    for (int i = threadIdx.x; i < KB * rows * 3; i += 256) {
      const int k = i / (rows * 3), e = i % (rows * 3);
      const int64_t r = r0 + e / 3;
      if (r < R) {
        const int64_t o = ((int64_t)k * R + r0) * 3 + e;
        const float x = (float)fma((double)bg[o], 1.0 - (double)acc[r], sO[i]);
        if (lin) lin[o] = x;
        rgb[o] = srgb_fwd(x);
      }
    }
  }
}

template <int KB>
int launch_relight_short(bool half, hipStream_t st, const void* C, const int* exps, const float* acc, const float* lights, const float* bg,
                         int64_t R, int J, float* rgb, float* lin) {
  const int stride = short_stride(J);
  const int n12 = (3 * J + 11) / 12 * 12;
  auto bytes = [&](int rows) { return ((size_t)2 * KB * n12 + (size_t)rows * stride + (size_t)2 * KB * rows * 3) * sizeof(float); };
  // 64 rows at 4 lanes each while 3 workgroups of them fit a CU, else 32 rows at 8 lanes: a tile is loaded, then summed, so it takes
  // several workgroups per CU to keep loads in flight
  const int lsh = bytes(64) <= 48 * 1024 ? 2 : 3;
  const int rows = 256 >> lsh;
  const size_t lds = bytes(rows);
  const int64_t tiles = (R + rows - 1) / rows;
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds));
  return with_storage(half, [&](auto h) {
    const auto kernel = &transfer_relight_short_kernel<KB, decltype(h)::value>;
    if (lds > 64 * 1024)  // (above the default limit of dynamic LDS)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(kernel, dim3(capped_grid(tiles, per_cu)), dim3(256), lds, st, C, exps, acc, lights, bg, R, J, stride, lsh, rgb, lin);
    NSKY_CHECK_LAUNCH("nsky_transfer_relight_short");
    return NSKY_OK;
  });
}

}  // namespace

extern "C" int nsky_transfer_project(const void* T, int32_t storage, const int32_t* exponents, const float* B, int64_t R, int32_t D, int32_t J,
                                     int32_t out_storage, void* C, int64_t row0, int32_t* out_exponents, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && D >= 1 && D <= kMaxDirs && J >= 1 && J <= kMaxCoeffs && row0 >= 0,
                 "nsky_transfer_project: R %ld, D %d (1..%d), J %d (1..%d), row0 %ld", (long)R, (int)D, kMaxDirs, (int)J, kMaxCoeffs, (long)row0);
  NSKY_CHECK_ARG((storage == NSKY_TRANSFER_FP32 || storage == NSKY_TRANSFER_FP16) &&
                     (out_storage == NSKY_TRANSFER_FP32 || out_storage == NSKY_TRANSFER_FP16),
                 "nsky_transfer_project: storage %d -> %d", (int)storage, (int)out_storage);
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(T && B && C, "nsky_transfer_project: NULL T / B / C");
  const bool half = storage == NSKY_TRANSFER_FP16;
  const int out_half = out_storage == NSKY_TRANSFER_FP16;
  NSKY_CHECK_ARG((!half || exponents) && (!out_half || out_exponents), "nsky_transfer_project: fp16 storage needs the row exponents");
  hipStream_t st = (hipStream_t)stream;
  const ProjectShape s = project_shape(J, R);
  return with_count<4, 12, 16, 24, 28, 36>(s.jt, [&](auto jt) {  // (the values of project_shape)
    return launch_project<decltype(jt)::value>(half, st, T, exponents, B, R, D, J, s.njw, C, row0, out_exponents, out_half);
  });
}

extern "C" int nsky_transfer_relight_short(const void* C, int32_t storage, const int32_t* exponents, const float* acc, const float* lights,
                                           const float* bg, int64_t R, int32_t J, int32_t K, float* rgb, float* lin, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && J >= 1 && J <= kMaxCoeffs && K >= 0, "nsky_transfer_relight_short: R %ld, J %d (1..%d), K %d", (long)R, (int)J,
                 kMaxCoeffs, (int)K);
  NSKY_CHECK_ARG(storage == NSKY_TRANSFER_FP32 || storage == NSKY_TRANSFER_FP16, "nsky_transfer_relight_short: storage %d", (int)storage);
  if (R == 0 || K == 0) return NSKY_OK;
  NSKY_CHECK_ARG(C && acc && lights && bg && rgb, "nsky_transfer_relight_short: NULL C / acc / lights / bg / rgb");
  const bool half = storage == NSKY_TRANSFER_FP16;
  NSKY_CHECK_ARG(!half || exponents, "nsky_transfer_relight_short: fp16 storage needs the row exponents");
  NSKY_CHECK_ARG(((uintptr_t)C & 15) == 0, "nsky_transfer_relight_short: C must start on a 16-byte boundary");
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = (int64_t)J * 3;
  return for_each_pass<kMaxLightsPerPass>(K, [&](int k0, auto kb) {  // C is read once per pass
    const int64_t o = (int64_t)k0 * R * 3;
    return launch_relight_short<decltype(kb)::value>(half, st, C, exponents, acc, lights + k0 * N, bg + o, R, J, rgb + o, lin ? lin + o : nullptr);
  });
}
