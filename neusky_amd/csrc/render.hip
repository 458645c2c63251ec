// Bandwidth-shaped stages of the NeuSky step:
//   * hemisphere integral + alpha composite + sRGB  (renderers.py:60-130)           fwd + bwd
//   * NeuS alpha -> transmittance -> weights (+ accumulation, expected depth)        fwd + bwd
//   * DDF visibility ray set-up (surface point, sphere hit, local frame, encoding)   fwd
//   * visibility sigmoid + scatter into the D illumination directions                fwd + bwd
// None of the broadcast tensors of the reference ([R*S,D,3] directions / colours, [R*S,D,1] visibility)
// is ever materialised: directions [D,3], per-camera colours [U,D,3] and visibility [R,D] are read once
// per ray into LDS and reduced over the hemisphere with wavefront shuffles.
#include "numerics.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr int MAXD = 1024;  // max illumination directions

// The three-term products of these kernels, in the one form their results have always had: (x0 y0 + rn(x1 y1)) + rn(x2 y2), the first
// product fused, the other two rounded on their own.  Written out with contraction off so that no rearrangement of the loops around
// them changes which products the compiler fuses: the rendered colours and their gradients stay bit for bit what they were.
__device__ __forceinline__ float dot3(float x0, float y0, float x1, float y1, float x2, float y2) {
#pragma clang fp contract(off)
  const float p1 = x1 * y1, p2 = x2 * y2;
  return fmaf(x0, y0, p1) + p2;
}

// sum_c gcomp_c (albedo_c I_c - bg_c) with the roundings it has always had: channels 0 and 1 round their product before the background
// is taken off, channel 2 fuses it; the sum starts from channel 1's term
__device__ __forceinline__ float weight_gradient(const float (&gcomp)[3], const float (&bgc)[3], float al0, float I0, float al1, float I1, float al2,
                                                 float I2) {
#pragma clang fp contract(off)
  const float r0 = al0 * I0, r1 = al1 * I1;
  const float t0 = r0 - bgc[0], t1 = r1 - bgc[1], t2 = fmaf(I2, al2, -bgc[2]);
  const float g1 = gcomp[1] * t1;
  return fmaf(gcomp[2], t2, fmaf(gcomp[0], t0, g1));
}

// Four wave sums for the price of seven exchanges instead of twenty-four: at the xor-32 level a lane keeps one value of a pair and hands
// the other to its partner, at the xor-16 level likewise for the two pairs, and the last four levels carry one value per 16-lane group.
// Every value is added in exactly the tree wave_sum() uses ((l, l^32), then ^16, ^8, ...; float addition commutes), so the totals are
// bit-equal to four wave_sum() calls.  They come back to all lanes through SGPRs.
__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__device__ __forceinline__ void wave_sum4(float& v0, float& v1, float& v2, float& v3, int lane) {
  const bool h32 = (lane & 32) != 0, h16 = (lane & 16) != 0;
  const float a = (h32 ? v1 : v0) + __shfl_xor(h32 ? v0 : v1, 32, 64);
  const float b = (h32 ? v3 : v2) + __shfl_xor(h32 ? v2 : v3, 32, 64);
  float x = (h16 ? b : a) + __shfl_xor(h16 ? a : b, 16, 64);
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  v0 = lane_value(x, 0); v2 = lane_value(x, 16); v1 = lane_value(x, 32); v3 = lane_value(x, 48);
}

// One workgroup (4 waves) per ray; wave w takes samples w, w+4, ...; lanes stride the D directions.  A lane's directions j = lane + 64 q
// never change, so their (direction, visibility x colour) rows are read into registers once (NQ = ceil(D / 64) rounded up to 4, 8 or 16;
// rows past D are zero and add nothing), and a wave reads the normals / albedo / weights of up to 64 of its samples with one load per
// lane and hands them round by readlane: the sample loop touches no memory.
template <int NQ>
__global__ __launch_bounds__(256) void hemi_fwd_kernel(const float* __restrict__ albedo, const float* __restrict__ normals,
                                                       const float* __restrict__ weights, const float* __restrict__ dirs,
                                                       const float* __restrict__ cam_colours, const int* __restrict__ cam_of_ray,
                                                       const float* __restrict__ vis, const float* __restrict__ bg, int R, int S,
                                                       int D, float* __restrict__ rgb, float* __restrict__ lin) {
  __shared__ float sdir[NQ * 64 * 3];
  __shared__ float svl[NQ * 64 * 3];
  __shared__ float red[4][4];
  const int r = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float* col = cam_colours + (long)cam_of_ray[r] * D * 3;
  for (int i = threadIdx.x; i < D * 3; i += 256) {
    sdir[i] = dirs[i];
    const float v = vis ? vis[(long)r * D + i / 3] : 1.0f;
    svl[i] = v * col[i];
  }
  __syncthreads();
  float lx[NQ], ly[NQ], lz[NQ], v0[NQ], v1[NQ], v2[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int j = lane + 64 * q;
    const bool in = j < D;
    lx[q] = in ? sdir[3 * j] : 0.0f; ly[q] = in ? sdir[3 * j + 1] : 0.0f; lz[q] = in ? sdir[3 * j + 2] : 0.0f;
    v0[q] = in ? svl[3 * j] : 0.0f; v1[q] = in ? svl[3 * j + 1] : 0.0f; v2[q] = in ? svl[3 * j + 2] : 0.0f;
  }
  float c0 = 0.f, c1 = 0.f, c2 = 0.f, wsum = 0.f;
  const int mine = S > wave ? (S - wave + 3) / 4 : 0;  // samples of this wave
  for (int base = 0; base < mine; base += 64) {
    const int sl = wave + 4 * (base + lane);  // lane l holds the inputs of the wave's sample base + l
    float pn0 = 0.f, pn1 = 0.f, pn2 = 0.f, pa0 = 0.f, pa1 = 0.f, pa2 = 0.f, pw = 0.f;
    if (sl < S) {
      const long o = ((long)r * S + sl) * 3;
      pn0 = normals[o]; pn1 = normals[o + 1]; pn2 = normals[o + 2];
      pa0 = albedo[o]; pa1 = albedo[o + 1]; pa2 = albedo[o + 2];
      pw = weights[(long)r * S + sl];
    }
    const int here = min(64, mine - base);
    for (int k = 0; k < here; ++k) {
      const float nx = lane_value(pn0, k), ny = lane_value(pn1, k), nz = lane_value(pn2, k);
      float cnt = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float d = fminf(fmaxf(dot3(nx, lx[q], ny, ly[q], nz, lz[q]), 0.0f), 1.0f);
        cnt += d > 0.0f ? 1.0f : 0.0f;
        a0 = fmaf(d, v0[q], a0); a1 = fmaf(d, v1[q], a1); a2 = fmaf(d, v2[q], a2);
      }
      wave_sum4(cnt, a0, a1, a2, lane);
      const float inv = 1.0f / (cnt > 0.0f ? cnt : 1.0f);
      const float w = lane_value(pw, k);
      c0 = fmaf(w, lane_value(pa0, k) * a0 * inv, c0);
      c1 = fmaf(w, lane_value(pa1, k) * a1 * inv, c1);
      c2 = fmaf(w, lane_value(pa2, k) * a2 * inv, c2);
      wsum += w;
    }
  }
  if (lane == 0) { red[wave][0] = c0; red[wave][1] = c1; red[wave][2] = c2; red[wave][3] = wsum; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    const float acc = red[0][3] + red[1][3] + red[2][3] + red[3][3];
    const float v = red[0][c] + red[1][c] + red[2][c] + red[3][c] + bg[(long)r * 3 + c] * (1.0f - acc);
    if (lin) lin[(long)r * 3 + c] = v;
    rgb[(long)r * 3 + c] = srgb_fwd(v);
  }
}

// the backward recomputes the forward's sums with the same registers and keeps A[q][c] = sum_s gI_c clamp(n.l_j) beside them
template <int NQ>
__global__ __launch_bounds__(256, NQ <= 8 ? 4 : 1) void hemi_bwd_kernel(const float* __restrict__ albedo, const float* __restrict__ normals,
                                                       const float* __restrict__ weights, const float* __restrict__ dirs,
                                                       const float* __restrict__ cam_colours, const int* __restrict__ cam_of_ray,
                                                       const float* __restrict__ vis, const float* __restrict__ bg,
                                                       const float* __restrict__ lin, const float* __restrict__ d_rgb, int R,
                                                       int S, int D, float* __restrict__ d_albedo, float* __restrict__ d_normals,
                                                       float* __restrict__ d_weights, float* __restrict__ d_cam_colours,
                                                       float* __restrict__ d_vis, float* __restrict__ d_bg) {
  __shared__ float sdir[NQ * 64 * 3];
  __shared__ float svl[NQ * 64 * 3];
  __shared__ float sA[4][NQ * 64 * 3];  // per-wave sum_s gI_c * clamp(n.l_j)
  __shared__ float red[4];
  const int r = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cam = cam_of_ray[r];
  const float* col = cam_colours + (long)cam * D * 3;
  for (int i = threadIdx.x; i < D * 3; i += 256) {
    sdir[i] = dirs[i];
    const float v = vis ? vis[(long)r * D + i / 3] : 1.0f;
    svl[i] = v * col[i];
  }
  __syncthreads();
  float gcomp[3], bgc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    gcomp[c] = d_rgb[(long)r * 3 + c] * srgb_bwd(lin[(long)r * 3 + c]);
    bgc[c] = bg[(long)r * 3 + c];
  }
  float lx[NQ], ly[NQ], lz[NQ], v0[NQ], v1[NQ], v2[NQ];
  float A[NQ][3];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int j = lane + 64 * q;
    const bool in = j < D;
    lx[q] = in ? sdir[3 * j] : 0.0f; ly[q] = in ? sdir[3 * j + 1] : 0.0f; lz[q] = in ? sdir[3 * j + 2] : 0.0f;
    v0[q] = in ? svl[3 * j] : 0.0f; v1[q] = in ? svl[3 * j + 1] : 0.0f; v2[q] = in ? svl[3 * j + 2] : 0.0f;
    A[q][0] = A[q][1] = A[q][2] = 0.0f;
  }
  float wsum = 0.f;
  const int mine = S > wave ? (S - wave + 3) / 4 : 0;  // samples of this wave
  for (int base = 0; base < mine; base += 64) {
    const int sl = wave + 4 * (base + lane);  // lane l holds the inputs of the wave's sample base + l
    float pn0 = 0.f, pn1 = 0.f, pn2 = 0.f, pa0 = 0.f, pa1 = 0.f, pa2 = 0.f, pw = 0.f;
    if (sl < S) {
      const long o = ((long)r * S + sl) * 3;
      pn0 = normals[o]; pn1 = normals[o + 1]; pn2 = normals[o + 2];
      pa0 = albedo[o]; pa1 = albedo[o + 1]; pa2 = albedo[o + 2];
      pw = weights[(long)r * S + sl];
    }
    const int here = min(64, mine - base);
    for (int k = 0; k < here; ++k) {
      const float nx = lane_value(pn0, k), ny = lane_value(pn1, k), nz = lane_value(pn2, k);
      float cnt = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float d = fminf(fmaxf(dot3(nx, lx[q], ny, ly[q], nz, lz[q]), 0.0f), 1.0f);
        cnt += d > 0.0f ? 1.0f : 0.0f;
        a0 = fmaf(d, v0[q], a0); a1 = fmaf(d, v1[q], a1); a2 = fmaf(d, v2[q], a2);
      }
      wave_sum4(cnt, a0, a1, a2, lane);
      const float inv = 1.0f / (cnt > 0.0f ? cnt : 1.0f);
      const float w = lane_value(pw, k);
      const float al0 = lane_value(pa0, k), al1 = lane_value(pa1, k), al2 = lane_value(pa2, k);
      const float I0 = a0 * inv, I1 = a1 * inv, I2 = a2 * inv;
      // d comp / d w_s = rad_c - bg_c ; d comp / d albedo = w I ; d comp / d I = w albedo
      const float gw = weight_gradient(gcomp, bgc, al0, I0, al1, I1, al2, I2);
      const float gI0 = gcomp[0] * w * al0 * inv, gI1 = gcomp[1] * w * al1 * inv, gI2 = gcomp[2] * w * al2 * inv;
      float gn0 = 0.f, gn1 = 0.f, gn2 = 0.f, unused = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float draw = dot3(nx, lx[q], ny, ly[q], nz, lz[q]);
        const float dc = fminf(fmaxf(draw, 0.0f), 1.0f);
        // torch.clamp_ passes gradient on the closed interval [0, 1]
        if (draw >= 0.0f && draw <= 1.0f) {
          const float qj = dot3(gI0, v0[q], gI1, v1[q], gI2, v2[q]);
          gn0 = fmaf(qj, lx[q], gn0); gn1 = fmaf(qj, ly[q], gn1); gn2 = fmaf(qj, lz[q], gn2);
        }
        A[q][0] = fmaf(gI0, dc, A[q][0]); A[q][1] = fmaf(gI1, dc, A[q][1]); A[q][2] = fmaf(gI2, dc, A[q][2]);
      }
      wave_sum4(gn0, gn1, gn2, unused, lane);
      if (lane == 0) {
        const long o = ((long)r * S + wave + 4 * (base + k)) * 3;
        d_albedo[o] = gcomp[0] * w * I0; d_albedo[o + 1] = gcomp[1] * w * I1; d_albedo[o + 2] = gcomp[2] * w * I2;
        d_normals[o] = gn0; d_normals[o + 1] = gn1; d_normals[o + 2] = gn2;
        d_weights[(long)r * S + wave + 4 * (base + k)] = gw;
      }
      wsum += w;
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int j = lane + 64 * q;
    if (j < D) { sA[wave][3 * j] = A[q][0]; sA[wave][3 * j + 1] = A[q][1]; sA[wave][3 * j + 2] = A[q][2]; }
  }
  if (lane == 0) red[wave] = wsum;
  __syncthreads();
  // the waves' sums meet in sA[0]; a thread walks the camera's row of [D, 3] linearly, so a wave's atomics are 256 contiguous bytes
  for (int i = threadIdx.x; i < D * 3; i += 256) {
    const float a = sA[0][i] + sA[1][i] + sA[2][i] + sA[3][i];
    sA[0][i] = a;
    if (d_cam_colours) {
      const float v = vis ? vis[(long)r * D + i / 3] : 1.0f;
      atomicAdd(d_cam_colours + (long)cam * D * 3 + i, a * v);
    }
  }
  if (d_vis) {
    __syncthreads();
    for (int j = threadIdx.x; j < D; j += 256) {
      float gv = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) gv = fmaf(sA[0][3 * j + c], col[3 * j + c], gv);
      d_vis[(long)r * D + j] = gv;
    }
  }
  if (threadIdx.x < 3) {
    const float acc = red[0] + red[1] + red[2] + red[3];
    d_bg[(long)r * 3 + threadIdx.x] = gcomp[threadIdx.x] * (1.0f - acc);
  }
}

// ------------------------------------------------------------------------------------------------
// NeuS alpha / transmittance / weights.  One wave per ray, lane l owns samples [l*CH, (l+1)*CH).
// ------------------------------------------------------------------------------------------------
constexpr int MAXCH = 4;  // S <= 256

__device__ __forceinline__ float wave_excl_prod_scan(float v, int lane) {
  // inclusive multiplicative scan, then shift
  float x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    float y = __shfl_up(x, off, 64);
    if (lane >= off) x *= y;
  }
  float e = __shfl_up(x, 1, 64);
  return lane == 0 ? 1.0f : e;
}
__device__ __forceinline__ float wave_excl_sum_scan_rev(float v, int lane) {
  // exclusive suffix sum: result[l] = sum_{m>l} v[m]
  float x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    float y = __shfl_down(x, off, 64);
    if (lane + off < 64) x += y;
  }
  float e = __shfl_down(x, 1, 64);
  return lane == 63 ? 0.0f : e;
}

struct AlphaTerms {
  float alpha, prev_cdf, next_cdf, cosv, ic, inv_s;
  bool clip_pass;
};

// cosv = d . grad(sdf), formed by the caller (neus_alpha_terms) or handed in as one precomputed column (the directional field pass)
__device__ __forceinline__ AlphaTerms neus_alpha_terms_cos(float sdf, float cosv, float delta, float inv_s, float anneal) {
  AlphaTerms t;
  t.inv_s = inv_s;
  t.cosv = cosv;
  t.ic = -(fmaxf(-t.cosv * 0.5f + 0.5f, 0.0f) * (1.0f - anneal) + fmaxf(-t.cosv, 0.0f) * anneal);
  const float nxt = sdf + t.ic * delta * 0.5f, prv = sdf - t.ic * delta * 0.5f;
  t.prev_cdf = sigmoidf_(prv * inv_s);
  t.next_cdf = sigmoidf_(nxt * inv_s);
  const float a = (t.prev_cdf - t.next_cdf + 1e-5f) / (t.prev_cdf + 1e-5f);
  t.clip_pass = (a >= 0.0f && a <= 1.0f);
  t.alpha = fminf(fmaxf(a, 0.0f), 1.0f);
  return t;
}

__device__ __forceinline__ AlphaTerms neus_alpha_terms(float sdf, const float g[3], const float d[3], float delta, float inv_s,
                                                      float anneal) {
  return neus_alpha_terms_cos(sdf, d[0] * g[0] + d[1] * g[1] + d[2] * g[2], delta, inv_s, anneal);
}

__global__ __launch_bounds__(256) void neus_weights_fwd_kernel(const float* __restrict__ sdf, const float* __restrict__ grad,
                                                               const float* __restrict__ ray_dirs, const float* __restrict__ starts,
                                                               const float* __restrict__ ends, const float* __restrict__ variance,
                                                               float anneal, int R, int S, float* __restrict__ alpha_out,
                                                               float* __restrict__ weights, float* __restrict__ trans_bg,
                                                               float* __restrict__ acc_out, float* __restrict__ depth_out, int gcols) {
  // gcols = 3: grad [R S, 3], cos = ray_dirs . grad; gcols = 1: grad [R S] is that cosine already (ray_dirs unused, may be null)
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int CH = (S + 63) / 64;
  const float inv_s = fminf(fmaxf(expf(variance[0] * 10.0f), 1e-6f), 1e6f);
  float d[3] = {0.f, 0.f, 0.f};
  if (gcols == 3) { d[0] = ray_dirs[(long)r * 3]; d[1] = ray_dirs[(long)r * 3 + 1]; d[2] = ray_dirs[(long)r * 3 + 2]; }
  float al[MAXCH], mid[MAXCH];
  float prod = 1.0f;
#pragma unroll
  for (int q = 0; q < MAXCH; ++q) {
    const int s = lane * CH + q;
    al[q] = 0.0f; mid[q] = 0.0f;
    if (q < CH && s < S) {
      const long o = (long)r * S + s;
      const float st = starts[o], en = ends[o];
      AlphaTerms t;
      if (gcols == 3) {
        const float g[3] = {grad[o * 3], grad[o * 3 + 1], grad[o * 3 + 2]};
        t = neus_alpha_terms(sdf[o], g, d, en - st, inv_s, anneal);
      } else {
        t = neus_alpha_terms_cos(sdf[o], grad[o], en - st, inv_s, anneal);
      }
      al[q] = t.alpha; mid[q] = 0.5f * (st + en);
      if (alpha_out) alpha_out[o] = t.alpha;
      prod *= (1.0f - t.alpha + 1e-7f);
    }
  }
  float T = wave_excl_prod_scan(prod, lane);
  float wsum = 0.f, dsum = 0.f;
#pragma unroll
  for (int q = 0; q < MAXCH; ++q) {
    const int s = lane * CH + q;
    if (q < CH && s < S) {
      const float w = al[q] * T;
      weights[(long)r * S + s] = w;
      wsum += w; dsum = fmaf(w, mid[q], dsum);
      T *= (1.0f - al[q] + 1e-7f);
    }
  }
  // T of the last active lane == transmittance past the last sample
  const int last_lane = (S - 1) / CH;
  const float Tbg = __shfl(T, last_lane, 64);
  wsum = wave_sum(wsum); dsum = wave_sum(dsum);
  if (lane == 0) {
    if (trans_bg) trans_bg[r] = Tbg;
    if (acc_out) acc_out[r] = wsum;
    if (depth_out) depth_out[r] = dsum / (wsum + 1e-10f);
  }
}

__global__ __launch_bounds__(256) void neus_weights_bwd_kernel(const float* __restrict__ sdf, const float* __restrict__ grad,
                                                               const float* __restrict__ ray_dirs, const float* __restrict__ starts,
                                                               const float* __restrict__ ends, const float* __restrict__ variance,
                                                               float anneal, int R, int S, const float* __restrict__ d_weights,
                                                               const float* __restrict__ d_trans_bg, float* __restrict__ d_sdf,
                                                               float* __restrict__ d_grad, float* __restrict__ d_variance, int gcols) {
  // gcols as in the forward; gcols = 1: d_grad [R S] is the gradient of the cosine column
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int CH = (S + 63) / 64;
  const float e10 = expf(variance[0] * 10.0f);
  const float inv_s = fminf(fmaxf(e10, 1e-6f), 1e6f);
  const bool invs_pass = (e10 >= 1e-6f && e10 <= 1e6f);
  float d[3] = {0.f, 0.f, 0.f};
  if (gcols == 3) { d[0] = ray_dirs[(long)r * 3]; d[1] = ray_dirs[(long)r * 3 + 1]; d[2] = ray_dirs[(long)r * 3 + 2]; }
  AlphaTerms tt[MAXCH];
  float sd[MAXCH], dl[MAXCH];
  float prod = 1.0f;
#pragma unroll
  for (int q = 0; q < MAXCH; ++q) {
    const int s = lane * CH + q;
    tt[q].alpha = 0.f;
    if (q < CH && s < S) {
      const long o = (long)r * S + s;
      sd[q] = sdf[o]; dl[q] = ends[o] - starts[o];
      if (gcols == 3) {
        const float g[3] = {grad[o * 3], grad[o * 3 + 1], grad[o * 3 + 2]};
        tt[q] = neus_alpha_terms(sd[q], g, d, dl[q], inv_s, anneal);
      } else {
        tt[q] = neus_alpha_terms_cos(sd[q], grad[o], dl[q], inv_s, anneal);
      }
      prod *= (1.0f - tt[q].alpha + 1e-7f);
    }
  }
  float T0 = wave_excl_prod_scan(prod, lane);
  // per-sample w and T; suffix sums of gw_i * w_i
  float w[MAXCH], Tq[MAXCH], gw[MAXCH];
  float local = 0.f, T = T0;
#pragma unroll
  for (int q = 0; q < MAXCH; ++q) {
    const int s = lane * CH + q;
    w[q] = 0.f; Tq[q] = T; gw[q] = 0.f;
    if (q < CH && s < S) {
      gw[q] = d_weights[(long)r * S + s];
      w[q] = tt[q].alpha * T;
      local = fmaf(gw[q], w[q], local);
      T *= (1.0f - tt[q].alpha + 1e-7f);
    }
  }
  const int last_lane = (S - 1) / CH;
  const float Tbg = __shfl(T, last_lane, 64);
  const float gT = d_trans_bg ? d_trans_bg[r] : 0.0f;
  float suffix = wave_excl_sum_scan_rev(local, lane) + gT * Tbg;  // sum over later lanes (+ background term)
  float gvar = 0.f;
#pragma unroll
  for (int q = MAXCH - 1; q >= 0; --q) {
    const int s = lane * CH + q;
    if (q < CH && s < S) {
      const AlphaTerms& t = tt[q];
      float galpha = gw[q] * Tq[q] - suffix / (1.0f - t.alpha + 1e-7f);
      suffix = fmaf(gw[q], w[q], suffix);
      float gs = 0.f, gg[3] = {0.f, 0.f, 0.f}, gcos = 0.f;
      if (t.clip_pass) {
        // a = (p + e)/(c + e), p = c - n, c = prev_cdf, n = next_cdf
        const float den = t.prev_cdf + 1e-5f;
        const float a = (t.prev_cdf - t.next_cdf + 1e-5f) / den;
        const float ga_c = (1.0f - a) / den, ga_n = -1.0f / den;
        const float gc = galpha * ga_c * t.prev_cdf * (1.0f - t.prev_cdf);  // d/d(prv*inv_s)
        const float gn = galpha * ga_n * t.next_cdf * (1.0f - t.next_cdf);  // d/d(nxt*inv_s)
        const float prv = sd[q] - t.ic * dl[q] * 0.5f, nxt = sd[q] + t.ic * dl[q] * 0.5f;
        gs = (gc + gn) * t.inv_s;
        gvar += gc * prv + gn * nxt;  // d/d inv_s
        const float gic = (gn - gc) * t.inv_s * dl[q] * 0.5f;
        // ic = -(relu(-cos/2+1/2)(1-an) + relu(-cos) an)
        float dic = 0.f;
        if (-t.cosv * 0.5f + 0.5f > 0.0f) dic += 0.5f * (1.0f - anneal);
        if (-t.cosv > 0.0f) dic += anneal;
        gcos = gic * dic;
        gg[0] = gcos * d[0]; gg[1] = gcos * d[1]; gg[2] = gcos * d[2];
      }
      const long o = (long)r * S + s;
      d_sdf[o] = gs;
      if (gcols == 3) { d_grad[o * 3] = gg[0]; d_grad[o * 3 + 1] = gg[1]; d_grad[o * 3 + 2] = gg[2]; }
      else d_grad[o] = gcos;
    }
  }
  gvar = wave_sum(gvar);
  if (lane == 0 && d_variance && invs_pass) atomicAdd(d_variance, gvar * inv_s * 10.0f);
}

// NeuS alphas of isolated samples for three interval lengths each (the hash-grid density probe: SDFField.get_alpha with `deltas` = the
// three axis gaps broadcast against [P,1], neusky_model.py:715-732): alphas[p][a] for gap a, and the backward to sdf, gradients, variance.
__global__ void point_alphas_fwd_kernel(const float* __restrict__ sdf, const float* __restrict__ grad, const float* __restrict__ dirs,
                                        float g0, float g1, float g2, const float* __restrict__ variance, float anneal, int P,
                                        float* __restrict__ alphas) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float inv_s = fminf(fmaxf(expf(variance[0] * 10.0f), 1e-6f), 1e6f);
  const float g[3] = {grad[3 * p], grad[3 * p + 1], grad[3 * p + 2]}, d[3] = {dirs[3 * p], dirs[3 * p + 1], dirs[3 * p + 2]};
  const float gaps[3] = {g0, g1, g2};
#pragma unroll
  for (int a = 0; a < 3; ++a) alphas[3 * p + a] = neus_alpha_terms(sdf[p], g, d, gaps[a], inv_s, anneal).alpha;
}

__global__ void point_alphas_bwd_kernel(const float* __restrict__ sdf, const float* __restrict__ grad, const float* __restrict__ dirs,
                                        float g0, float g1, float g2, const float* __restrict__ variance, float anneal, int P,
                                        const float* __restrict__ d_alphas, float* __restrict__ d_sdf, float* __restrict__ d_grad,
                                        float* __restrict__ d_variance) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const float e10 = expf(variance[0] * 10.0f);
  const float inv_s = fminf(fmaxf(e10, 1e-6f), 1e6f);
  const bool invs_pass = (e10 >= 1e-6f && e10 <= 1e6f);
  float gvar = 0.0f;
  if (p < P) {
    const float sd = sdf[p];
    const float g[3] = {grad[3 * p], grad[3 * p + 1], grad[3 * p + 2]}, d[3] = {dirs[3 * p], dirs[3 * p + 1], dirs[3 * p + 2]};
    const float gaps[3] = {g0, g1, g2};
    float gs = 0.0f, gg[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const AlphaTerms t = neus_alpha_terms(sd, g, d, gaps[a], inv_s, anneal);
      if (!t.clip_pass) continue;
      const float galpha = d_alphas[3 * p + a];
      const float den = t.prev_cdf + 1e-5f;
      const float av = (t.prev_cdf - t.next_cdf + 1e-5f) / den;
      const float gc = galpha * ((1.0f - av) / den) * t.prev_cdf * (1.0f - t.prev_cdf);
      const float gn = galpha * (-1.0f / den) * t.next_cdf * (1.0f - t.next_cdf);
      const float prv = sd - t.ic * gaps[a] * 0.5f, nxt = sd + t.ic * gaps[a] * 0.5f;
      gs += (gc + gn) * inv_s;
      gvar += gc * prv + gn * nxt;
      const float gic = (gn - gc) * inv_s * gaps[a] * 0.5f;
      float dic = 0.0f;
      if (-t.cosv * 0.5f + 0.5f > 0.0f) dic += 0.5f * (1.0f - anneal);
      if (-t.cosv > 0.0f) dic += anneal;
      const float gcos = gic * dic;
      gg[0] += gcos * d[0]; gg[1] += gcos * d[1]; gg[2] += gcos * d[2];
    }
    d_sdf[p] = gs;
    d_grad[3 * p] = gg[0]; d_grad[3 * p + 1] = gg[1]; d_grad[3 * p + 2] = gg[2];
  }
  gvar = wave_sum(gvar);
  if ((threadIdx.x & 63) == 0 && d_variance && invs_pass && gvar != 0.0f) atomicAdd(d_variance, gvar * inv_s * 10.0f);
}

// ------------------------------------------------------------------------------------------------
// DDF visibility ray set-up: thread per (ray, selected direction)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sphere_hit_clamped(const float p[3], const float dir[3], float radius, float out[3]) {
  // neusky_model.py:1590-1622: normalise dir, clamp discriminant, far root
  const float n = sqrtf(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
  const float d[3] = {dir[0] / n, dir[1] / n, dir[2] / n};
  const float b = 2.0f * (d[0] * p[0] + d[1] * p[1] + d[2] * p[2]);
  const float c = p[0] * p[0] + p[1] * p[1] + p[2] * p[2] - radius * radius;
  const float disc = fmaxf(b * b - 4.0f * c, 0.0f);
  const float sq = sqrtf(disc);
  const float t = fmaxf((-b - sq) * 0.5f, (-b + sq) * 0.5f);
  out[0] = p[0] + t * d[0]; out[1] = p[1] + t * d[1]; out[2] = p[2] + t * d[2];
}

__global__ void visibility_rays_kernel(const float* __restrict__ origins, const float* __restrict__ ray_dirs,
                                       const float* __restrict__ depth, const float* __restrict__ sel_dirs, int R, int Dv,
                                       float radius, float* __restrict__ sphere_pts, float* __restrict__ xrow, int ldx,
                                       float* __restrict__ surf_dist, float* __restrict__ term_dist) {
  const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= (long)R * Dv) return;
  const int r = (int)(m / Dv), j = (int)(m % Dv);
  const float o[3] = {origins[r * 3], origins[r * 3 + 1], origins[r * 3 + 2]};
  const float rd[3] = {ray_dirs[r * 3], ray_dirs[r * 3 + 1], ray_dirs[r * 3 + 2]};
  const float t = depth[r];
  float pos[3] = {o[0] + rd[0] * t, o[1] + rd[1] * t, o[2] + rd[2] * t};  // :1671
  const float nrm = sqrtf(pos[0] * pos[0] + pos[1] * pos[1] + pos[2] * pos[2]);
  if (!(nrm < radius)) {  // :1674-1683 (sic: elementwise product with -dir)
    float hit[3];
    sphere_hit_clamped(o, rd, radius, hit);
    pos[0] = hit[0] * 0.01f * -rd[0]; pos[1] = hit[1] * 0.01f * -rd[1]; pos[2] = hit[2] * 0.01f * -rd[2];
  }
  const float l[3] = {sel_dirs[j * 3], sel_dirs[j * 3 + 1], sel_dirs[j * 3 + 2]};
  float sp[3];
  sphere_hit_clamped(pos, l, radius, sp);  // :1693
  const float dx = sp[0] - pos[0], dy = sp[1] - pos[1], dz = sp[2] - pos[2];
  const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
  if (term_dist) term_dist[m] = dist;                        // :1697
  surf_dist[m] = fminf(dist, 2.0f * radius);                 // :1724-1727
  sphere_pts[m * 3] = sp[0]; sphere_pts[m * 3 + 1] = sp[1]; sphere_pts[m * 3 + 2] = sp[2];
  // local frame (ddf_model.py:158-181) applied to the DDF query direction -l (:1702, ddf_model.py:200)
  const float y[3] = {-sp[0], -sp[1], -sp[2]};
  float xl[3] = {-y[1], y[0], 0.0f};  // cross(up=(0,0,1), y)
  const float xn = sqrtf(xl[0] * xl[0] + xl[1] * xl[1] + xl[2] * xl[2]);
  if (xn > 0.0f) { xl[0] /= xn; xl[1] /= xn; xl[2] /= xn; }
  else { xl[0] = 1.0f; xl[1] = 0.0f; xl[2] = 0.0f; }  // sphere hit ON the pole (0 / 0 in the reference): any unit vector across the axis
  float zl[3] = {y[1] * xl[2] - y[2] * xl[1], y[2] * xl[0] - y[0] * xl[2], y[0] * xl[1] - y[1] * xl[0]};  // cross(y, x)
  const float zn = sqrtf(zl[0] * zl[0] + zl[1] * zl[1] + zl[2] * zl[2]);
  zl[0] /= zn; zl[1] /= zn; zl[2] /= zn;
  const float q[3] = {-l[0], -l[1], -l[2]};
  const float dl[3] = {xl[0] * q[0] + xl[1] * q[1] + xl[2] * q[2], y[0] * q[0] + y[1] * q[1] + y[2] * q[2],
                       zl[0] * q[0] + zl[1] * q[1] + zl[2] * q[2]};
  float* row = xrow + m * ldx;
  // [d_loc (3) | sin(2 pi d_i {1,4}) (6) | sin(.. + pi/2) (6) | 0]   NeRFEncoding(2 freqs, 0..2) :188-191
  row[0] = dl[0]; row[1] = dl[1]; row[2] = dl[2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float arg = 6.283185307179586f * dl[i] * (f == 0 ? 1.0f : 4.0f);
      row[3 + i * 2 + f] = sinf(arg);
      row[9 + i * 2 + f] = sinf(arg + 1.5707963267948966f);
    }
  for (int c = 15; c < ldx; ++c) row[c] = 0.0f;
}

__global__ void visibility_finish_fwd_kernel(const float* __restrict__ t_hat, const float* __restrict__ surf_dist,
                                             const float* __restrict__ threshold, float scale, const int* __restrict__ sel_index,
                                             int R, int Dv, int D, float* __restrict__ vis) {
  const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= (long)R * Dv) return;
  const int r = (int)(m / Dv), j = (int)(m % Dv);
  const float u = scale * (surf_dist[m] - t_hat[m] - threshold[0]);  // :1730-1739
  vis[(long)r * D + sel_index[j]] = 1.0f - sigmoidf_(u);
}

// The per-row term and the wave's share of the threshold's gradient are formed in double: scale (25) multiplies the float rounding
// of surf_dist - t_hat - threshold into the sigmoid's argument, and where few rows are off saturation those roundings do not average
// out of their sum.  One exp per row of a kernel that streams four floats per row.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ void visibility_finish_bwd_kernel(const float* __restrict__ t_hat, const float* __restrict__ surf_dist,
                                             const float* __restrict__ threshold, float scale, const int* __restrict__ sel_index,
                                             int R, int Dv, int D, const float* __restrict__ d_vis, float* __restrict__ d_t_hat,
                                             float* __restrict__ d_threshold) {
  // grid-stride over the rows; the workgroup's share of the threshold's gradient leaves as ONE atomic (the word is a single address:
  // its atomics serialise at the memory side, so their count, not the rows' bytes, used to set this kernel's time)
  __shared__ double red[4];
  const long n = (long)R * Dv;
  const double thr = (double)threshold[0];
  double gthr = 0.0;
  for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < n; m += (long)gridDim.x * blockDim.x) {
    const int r = (int)(m / Dv), j = (int)(m % Dv);
    const double s = 1.0 / (1.0 + exp(-(double)scale * ((double)surf_dist[m] - (double)t_hat[m] - thr)));
    const double g = (double)d_vis[(long)r * D + sel_index[j]] * s * (1.0 - s) * (double)scale;  // d vis / d t_hat = + s' * scale
    d_t_hat[m] = (float)g;
    gthr += g;
  }
  if (!d_threshold) return;
  gthr = wave_sum_f64(gthr);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = gthr;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t = (red[0] + red[1]) + (red[2] + red[3]);
    if (t != 0.0) atomicAdd(d_threshold, (float)t);
  }
}


// ------------------------------------------------------------------------------------------------
// Proposal-network weights: raw density head -> density = exp(raw) -> volumetric weights of one ray.
//   dd_i = delta_i exp(raw_i),  w_i = nan_to_num((1 - exp(-dd_i)) exp(-sum_{j<i} dd_j))
// One wave per ray, lane l owns bins [l*CH, (l+1)*CH).  Backward recomputes the forward terms:
//   dL/ddd_j = g_j exp(-dd_j) T_j - sum_{i>j} g_i w_i,   d raw_j = dL/ddd_j delta_j exp(clamp(raw_j, -15, 15))
// (the density activation is nerfstudio's trunc_exp: forward exp, backward exp of the clamped input).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_excl_sum_scan(float v, int lane) {
  float x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    float y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  float e = __shfl_up(x, 1, 64);
  return lane == 0 ? 0.0f : e;
}
__device__ __forceinline__ float nan_to_num_f(float v) {
  if (v != v) return 0.0f;
  return fminf(fmaxf(v, -3.402823466e38f), 3.402823466e38f);
}

__global__ __launch_bounds__(256) void density_weights_fwd_kernel(const float* __restrict__ raw, int ld_raw,
                                                                  const float* __restrict__ ebins, int R, int n,
                                                                  float* __restrict__ weights) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int CH = (n + 63) / 64;
  float dd[MAXCH];
  float local = 0.0f;
#pragma unroll
  for (int q = 0; q < MAXCH; ++q) {
    const int i = lane * CH + q;
    dd[q] = 0.0f;
    if (q < CH && i < n) {
      const float delta = ebins[(long)r * (n + 1) + i + 1] - ebins[(long)r * (n + 1) + i];
      dd[q] = delta * expf(raw[((long)r * n + i) * ld_raw]);
      local += dd[q];
    }
  }
  float C = wave_excl_sum_scan(local, lane);
#pragma unroll
  for (int q = 0; q < MAXCH; ++q) {
    const int i = lane * CH + q;
    if (q < CH && i < n) {
      weights[(long)r * n + i] = nan_to_num_f((1.0f - expf(-dd[q])) * expf(-C));
      C += dd[q];
    }
  }
}

__global__ __launch_bounds__(256) void density_weights_bwd_kernel(const float* __restrict__ raw, int ld_raw,
                                                                  const float* __restrict__ ebins, const float* __restrict__ d_w,
                                                                  int R, int n, float* __restrict__ d_raw) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int CH = (n + 63) / 64;
  float dd[MAXCH], gw[MAXCH], gdirect[MAXCH], dens_b[MAXCH];
  float local = 0.0f;
#pragma unroll
  for (int q = 0; q < MAXCH; ++q) {
    const int i = lane * CH + q;
    dd[q] = 0.0f;
    if (q < CH && i < n) {
      const float delta = ebins[(long)r * (n + 1) + i + 1] - ebins[(long)r * (n + 1) + i];
      const float rv = raw[((long)r * n + i) * ld_raw];
      dd[q] = delta * expf(rv);
      dens_b[q] = delta * expf(fminf(fmaxf(rv, -15.0f), 15.0f));
      local += dd[q];
    }
  }
  float C = wave_excl_sum_scan(local, lane);
  float gsum = 0.0f;
#pragma unroll
  for (int q = 0; q < MAXCH; ++q) {
    const int i = lane * CH + q;
    gw[q] = 0.0f; gdirect[q] = 0.0f;
    if (q < CH && i < n) {
      const float T = expf(-C), e = expf(-dd[q]);
      const float w = (1.0f - e) * T;
      const bool pass = (w == w) && fabsf(w) <= 3.402823466e38f;  // nan_to_num passes gradients of finite values only
      const float g = pass ? d_w[(long)r * n + i] : 0.0f;
      gw[q] = g * w;
      gdirect[q] = g * e * T;
      gsum += gw[q];
      C += dd[q];
    }
  }
  float suffix = wave_excl_sum_scan_rev(gsum, lane);  // sum of g w over later lanes
#pragma unroll
  for (int q = MAXCH - 1; q >= 0; --q) {
    const int i = lane * CH + q;
    if (q < CH && i < n) {
      float* o = d_raw + ((long)r * n + i) * ld_raw;
      o[0] = (gdirect[q] - suffix) * dens_b[q];
      for (int c = 1; c < ld_raw; ++c) o[c] = 0.0f;
      suffix += gw[q];
    }
  }
}


// ------------------------------------------------------------------------------------------------
// Interlevel (proposal) loss of mip-NeRF 360 as nerfstudio states it: for every final-level interval [c_s, c_{s+1}] with
// weight w_s, the proposal histogram's outer measure  w_outer = sum_{j = lo..hi} wp_j,
//   lo = clamp(searchsorted_right(starts, c_s) - 1, 0, n-1),  hi = clamp(searchsorted_right(ends, c_{s+1}), 0, n-1),
// and the per-ray sum of max(w_s - w_outer, 0)^2 / (w_s + 1e-7).  One wave per ray; the proposal bins and the prefix
// sums of wp live in LDS.  Backward: d wp_j = sum over the s whose [lo, hi] contains j of  -2 g max(.)/(w_s + 1e-7),
// scattered as a difference array and prefix-summed.  A bin no active interval covers has a gradient of EXACTLY zero in the reference's
// autograd; the float prefix sum of +g / -g pairs leaves a residue of ~1e-9 g there, and Adam with eps = 1e-15 turns any nonzero
// gradient into a step of ~lr (a trajectory test found hash-table rows moving that the oracle never touches): an integer difference
// array of the coverage count decides which bins receive a gradient at all.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int upper_bound_f(const float* a, int n, float v) {  // first index with a[idx] > v
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <bool BWD>
__global__ __launch_bounds__(256) void interlevel_kernel(const float* __restrict__ c, const float* __restrict__ w,
                                                         const float* __restrict__ sb, const float* __restrict__ wp,
                                                         const float* __restrict__ g_ray, int R, int S, int n,
                                                         float* __restrict__ per_ray, float* __restrict__ d_wp) {
  extern __shared__ float sm[];  // per wave: bins[n+1], cy[n+1] (exclusive prefix sums), diff[n+1], cover[n+1] (int)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= R) return;
  float* bins = sm + wave * 4 * (n + 1);
  float* cy = bins + (n + 1);
  float* diff = cy + (n + 1);
  int* cover = reinterpret_cast<int*>(diff + (n + 1));
  for (int i = lane; i <= n; i += 64) {
    bins[i] = sb[(long)r * (n + 1) + i];
    cy[i] = i == 0 ? 0.0f : wp[(long)r * n + i - 1];  // the whole wave brings wp in; lane 0 then sums it in place
    if (BWD) { diff[i] = 0.0f; cover[i] = 0; }
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  if (lane == 0) {  // sequential prefix sums (n <= 1023, the host's LDS limit), the order torch.cumsum uses on one row
    float acc = 0.0f;
#pragma unroll 8
    for (int i = 1; i <= n; ++i) {
      acc += cy[i];
      cy[i] = acc;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  const float g = BWD ? g_ray[r] : 0.0f;
  float sum = 0.0f;
  for (int s_ = lane; s_ < S; s_ += 64) {
    const float c0 = c[(long)r * (S + 1) + s_], c1 = c[(long)r * (S + 1) + s_ + 1];
    const int lo = min(max(upper_bound_f(bins, n, c0) - 1, 0), n - 1);      // starts = bins[0..n)
    const int hi = min(max(upper_bound_f(bins + 1, n, c1), 0), n - 1);      // ends   = bins[1..n]
    const float w_outer = cy[hi + 1] - cy[lo];
    const float ws = w[(long)r * S + s_];
    const float dlt = fmaxf(ws - w_outer, 0.0f);
    if (!BWD) {
      sum += dlt * dlt / (ws + 1e-7f);
    } else if (dlt > 0.0f && hi >= lo) {
      const float gj = -2.0f * g * dlt / (ws + 1e-7f);
      atomicAdd(diff + lo, gj);
      atomicAdd(diff + hi + 1, -gj);
      atomicAdd(cover + lo, 1);
      atomicAdd(cover + hi + 1, -1);
    }
  }
  if (!BWD) {
    sum = wave_sum(sum);
    if (lane == 0) per_ray[r] = sum;
    return;
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  if (lane == 0) {  // the same sequential order as before, in place; the row then leaves with all lanes
    float acc = 0.0f;
    int cnt = 0;
#pragma unroll 8
    for (int i = 0; i < n; ++i) {
      acc += diff[i];
      cnt += cover[i];
      diff[i] = cnt > 0 ? acc : 0.0f;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  for (int i = lane; i < n; i += 64) d_wp[(long)r * n + i] = diff[i];
}

// ------------------------------------------------------------------------------------------------
// Per-ray reductions of the renderers: expected depth (nerfstudio DepthRenderer('expected'), neusky_model.py:591,1342: clipped
// to the global [min, max] of the sample mid points), accumulation (:595), weighted normal (:812) and albedo on a white
// background (:813).  One wave per ray; the clip bounds are two float atomics into a [2] buffer the caller initialises to
// (+inf, -inf); a finishing kernel applies them.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void atomic_min_float(float* addr, float v) {
  int* ia = reinterpret_cast<int*>(addr);
  int old = *ia;
  while (__int_as_float(old) > v) {
    const int prev = atomicCAS(ia, old, __float_as_int(v));
    if (prev == old) break;
    old = prev;
  }
}
__device__ __forceinline__ void atomic_max_float(float* addr, float v) {
  int* ia = reinterpret_cast<int*>(addr);
  int old = *ia;
  while (__int_as_float(old) < v) {
    const int prev = atomicCAS(ia, old, __float_as_int(v));
    if (prev == old) break;
    old = prev;
  }
}

constexpr int RR_WAVES = 16, RR_MAX_BLOCKS = 32;

__global__ __launch_bounds__(RR_WAVES * 64) void ray_reduce_fwd_kernel(const float* __restrict__ w, const float* __restrict__ starts,
                                                                       const float* __restrict__ ends, const float* __restrict__ normals,
                                                                       const float* __restrict__ albedo, int R, int S,
                                                                       float* __restrict__ sums, float* __restrict__ bounds) {
  // RR_WAVES waves per workgroup, a wave per ray, grid-stride over the rays; the clip bounds of all the workgroup's rays meet in LDS
  // and leave as one CAS loop each (the two words are single addresses: every update of them serialises)
  __shared__ float smn[RR_WAVES], smx[RR_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float mn = 3.0e38f, mx = -3.0e38f;
  for (int r = blockIdx.x * RR_WAVES + wave; r < R; r += gridDim.x * RR_WAVES) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = lane; k < S; k += 64) {
      const long i = (long)r * S + k;
      const float wk = w[i], mid = (starts[i] + ends[i]) * 0.5f;
      mn = fminf(mn, mid); mx = fmaxf(mx, mid);
      acc[0] = fmaf(wk, mid, acc[0]);
      acc[1] += wk;
      if (normals)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[2 + c] = fmaf(wk, normals[i * 3 + c], acc[2 + c]);
      if (albedo)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[5 + c] = fmaf(wk, albedo[i * 3 + c], acc[5 + c]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sums[(long)r * 8 + j] = acc[j];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off, 64)); mx = fmaxf(mx, __shfl_xor(mx, off, 64)); }
  if (lane == 0) { smn[wave] = mn; smx[wave] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 1; v < RR_WAVES; ++v) { mn = fminf(mn, smn[v]); mx = fmaxf(mx, smx[v]); }
    atomic_min_float(bounds, mn);
    atomic_max_float(bounds + 1, mx);
  }
}

__global__ void ray_reduce_finish_kernel(const float* __restrict__ sums, const float* __restrict__ bounds, int R, float max_clamp,
                                         float* __restrict__ p2p, float* __restrict__ accum, float* __restrict__ normal,
                                         float* __restrict__ albedo_acc) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float* s = sums + (long)r * 8;
  float d = s[0] / (s[1] + 1e-10f);
  d = fminf(fmaxf(d, bounds[0]), bounds[1]);
  if (max_clamp > 0.0f) d = fminf(d, max_clamp);
  p2p[r] = d;
  accum[r] = s[1];
  if (normal)
    for (int c = 0; c < 3; ++c) normal[r * 3 + c] = s[2 + c];
  if (albedo_acc)
    for (int c = 0; c < 3; ++c) albedo_acc[r * 3 + c] = s[5 + c] + (1.0f - s[1]);
}

__global__ __launch_bounds__(256) void ray_reduce_bwd_kernel(const float* __restrict__ w, const float* __restrict__ starts,
                                                             const float* __restrict__ ends, const float* __restrict__ normals,
                                                             const float* __restrict__ albedo, const float* __restrict__ sums,
                                                             const float* __restrict__ bounds, int R, int S, float max_clamp,
                                                             const float* __restrict__ d_p2p, const float* __restrict__ d_accum,
                                                             const float* __restrict__ d_normal, const float* __restrict__ d_albedo_acc,
                                                             float* __restrict__ d_w, float* __restrict__ d_normals,
                                                             float* __restrict__ d_albedo) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float A = sums[(long)r * 8], B = sums[(long)r * 8 + 1];
  const float depth = A / (B + 1e-10f);
  // torch.clamp's backward passes the gradient where min <= x <= max
  float gd = d_p2p ? d_p2p[r] : 0.0f;
  if (!(depth >= bounds[0] && depth <= bounds[1])) gd = 0.0f;
  if (max_clamp > 0.0f && !(fminf(fmaxf(depth, bounds[0]), bounds[1]) <= max_clamp)) gd = 0.0f;
  const float ga = d_accum ? d_accum[r] : 0.0f;
  float gn[3] = {0.f, 0.f, 0.f}, gb[3] = {0.f, 0.f, 0.f};
  if (d_normal) for (int c = 0; c < 3; ++c) gn[c] = d_normal[r * 3 + c];
  if (d_albedo_acc) for (int c = 0; c < 3; ++c) gb[c] = d_albedo_acc[r * 3 + c];
  const float gbs = gb[0] + gb[1] + gb[2];
  const float inv = 1.0f / (B + 1e-10f);
  for (int k = lane; k < S; k += 64) {
    const long i = (long)r * S + k;
    const float wk = w[i], mid = (starts[i] + ends[i]) * 0.5f;
    float g = gd * (mid - depth) * inv + ga - gbs;
    if (normals) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        g = fmaf(normals[i * 3 + c], gn[c], g);
        if (d_normals) d_normals[i * 3 + c] = wk * gn[c];
      }
    }
    if (albedo) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        g = fmaf(albedo[i * 3 + c], gb[c], g);
        if (d_albedo) d_albedo[i * 3 + c] = wk * gb[c];
      }
    }
    d_w[i] = g;
  }
}

// rows of g [P,3] -> unit rows (torch.nn.functional.normalize, eps = 1e-12; sdf_albedo_field.py:256) and the backward
__global__ void normalize3_fwd_kernel(const float* __restrict__ g, long P, float* __restrict__ n) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float x = g[p * 3], y = g[p * 3 + 1], z = g[p * 3 + 2];
  const float inv = 1.0f / fmaxf(sqrtf(x * x + y * y + z * z), 1e-12f);
  n[p * 3] = x * inv; n[p * 3 + 1] = y * inv; n[p * 3 + 2] = z * inv;
}
__global__ void normalize3_bwd_kernel(const float* __restrict__ g, const float* __restrict__ d_n, long P, float* __restrict__ d_g) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float x = g[p * 3], y = g[p * 3 + 1], z = g[p * 3 + 2];
  const float len = sqrtf(x * x + y * y + z * z);
  const float a = d_n[p * 3], b = d_n[p * 3 + 1], c = d_n[p * 3 + 2];
  if (len > 1e-12f) {
    const float inv = 1.0f / len;
    const float nx = x * inv, ny = y * inv, nz = z * inv;
    const float dot = nx * a + ny * b + nz * c;
    d_g[p * 3] = (a - nx * dot) * inv; d_g[p * 3 + 1] = (b - ny * dot) * inv; d_g[p * 3 + 2] = (c - nz * dot) * inv;
  } else {  // the clamped branch: n = g / eps
    d_g[p * 3] = a * 1e12f; d_g[p * 3 + 1] = b * 1e12f; d_g[p * 3 + 2] = c * 1e12f;
  }
}

// the DDF's output activation (directional_distance_field.py:297-299): t = scale sigmoid(raw[:, 0]) on the chain's padded [M, 4] head
// output, and its backward as one [M, 4] matrix (columns 1..3 zero)
__global__ void sigmoid_column_fwd_kernel(const float* __restrict__ raw, int ld, long n, float scale, float* __restrict__ t) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  t[i] = scale * sigmoidf_(raw[i * ld]);
}
__global__ void sigmoid_column_bwd_kernel(const float* __restrict__ raw, int ld, long n, float scale, const float* __restrict__ d_t,
                                          float* __restrict__ d_raw) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float sg = sigmoidf_(raw[i * ld]);
  d_raw[i * ld] = d_t[i] * scale * sg * (1.0f - sg);
  for (int c = 1; c < ld; ++c) d_raw[i * ld + c] = 0.0f;
}

// points along rays: out[i] = o[i] + sign t[i] d[i % n_dirs] (the DDF's predicted termination points, ddf_model.py:243 and
// neusky_model.py:1716-1724: sphere point minus the direction to the sun-side sample times the predicted distance), and d t
__global__ void ray_points_fwd_kernel(const float* __restrict__ o, const float* __restrict__ d, int n_dirs, float sign,
                                      const float* __restrict__ t, long n, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* dd = d + 3 * (i % n_dirs);
  const float tt = sign * t[i];
  out[3 * i] = fmaf(dd[0], tt, o[3 * i]); out[3 * i + 1] = fmaf(dd[1], tt, o[3 * i + 1]); out[3 * i + 2] = fmaf(dd[2], tt, o[3 * i + 2]);
}
__global__ void ray_points_bwd_kernel(const float* __restrict__ d, int n_dirs, float sign, const float* __restrict__ d_out, long n,
                                      float* __restrict__ d_t) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* dd = d + 3 * (i % n_dirs);
  d_t[i] = sign * (d_out[3 * i] * dd[0] + d_out[3 * i + 1] * dd[1] + d_out[3 * i + 2] * dd[2]);
}

}  // namespace

extern "C" int nsky_hemi_composite_fwd(const float* albedo, const float* normals, const float* weights, const float* dirs,
                                       const float* cam_colours, const int32_t* cam_of_ray, const float* vis, const float* bg,
                                       int32_t R, int32_t S, int32_t D, float* rgb, float* lin, nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(albedo && normals && weights && dirs && cam_colours && cam_of_ray && bg && rgb, "nsky_hemi_composite_fwd: null argument");
  NSKY_CHECK_ARG(R > 0 && S > 0 && D > 0 && D <= MAXD, "nsky_hemi_composite_fwd: bad sizes R=%d S=%d D=%d (D <= %d)", R, S, D, MAXD);
  auto kernel = D <= 256 ? hemi_fwd_kernel<4> : D <= 512 ? hemi_fwd_kernel<8> : hemi_fwd_kernel<MAXD / 64>;
  hipLaunchKernelGGL(kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, albedo, normals, weights, dirs, cam_colours, cam_of_ray, vis, bg,
                     R, S, D, rgb, lin);
  NSKY_CHECK_LAUNCH("nsky_hemi_composite_fwd");
  return NSKY_OK;
}

extern "C" int nsky_hemi_composite_bwd(const float* albedo, const float* normals, const float* weights, const float* dirs,
                                       const float* cam_colours, const int32_t* cam_of_ray, const float* vis, const float* bg,
                                       const float* lin, const float* d_rgb, int32_t R, int32_t S, int32_t D, float* d_albedo,
                                       float* d_normals, float* d_weights, float* d_cam_colours, float* d_vis, float* d_bg,
                                       nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(albedo && normals && weights && dirs && cam_colours && cam_of_ray && bg && lin && d_rgb && d_albedo && d_normals &&
                     d_weights && d_bg, "nsky_hemi_composite_bwd: null argument");
  NSKY_CHECK_ARG(R > 0 && S > 0 && D > 0 && D <= MAXD, "nsky_hemi_composite_bwd: bad sizes R=%d S=%d D=%d (D <= %d)", R, S, D, MAXD);
  auto kernel = D <= 256 ? hemi_bwd_kernel<4> : D <= 512 ? hemi_bwd_kernel<8> : hemi_bwd_kernel<MAXD / 64>;
  hipLaunchKernelGGL(kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, albedo, normals, weights, dirs, cam_colours, cam_of_ray, vis, bg,
                     lin, d_rgb, R, S, D, d_albedo, d_normals, d_weights, d_cam_colours, d_vis, d_bg);
  NSKY_CHECK_LAUNCH("nsky_hemi_composite_bwd");
  return NSKY_OK;
}

extern "C" int nsky_neus_weights_fwd(const float* sdf, const float* grad, const float* ray_dirs, const float* starts,
                                     const float* ends, const float* variance, float cos_anneal, int32_t R, int32_t S,
                                     float* alpha, float* weights, float* trans_bg, float* accumulation, float* depth,
                                     nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(sdf && grad && ray_dirs && starts && ends && variance && weights, "nsky_neus_weights_fwd: null argument");
  NSKY_CHECK_ARG(R > 0 && S > 0 && S <= 64 * MAXCH, "nsky_neus_weights_fwd: S=%d out of range (<= %d)", S, 64 * MAXCH);
  hipLaunchKernelGGL(neus_weights_fwd_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, sdf, grad, ray_dirs, starts,
                     ends, variance, cos_anneal, R, S, alpha, weights, trans_bg, accumulation, depth, 3);
  NSKY_CHECK_LAUNCH("nsky_neus_weights_fwd");
  return NSKY_OK;
}

extern "C" int nsky_neus_weights_cos_fwd(const float* sdf, const float* cosv, const float* starts, const float* ends, const float* variance,
                                         float cos_anneal, int32_t R, int32_t S, float* alpha, float* weights, float* trans_bg,
                                         float* accumulation, float* depth, nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(sdf && cosv && starts && ends && variance && weights, "nsky_neus_weights_cos_fwd: null argument");
  NSKY_CHECK_ARG(R > 0 && S > 0 && S <= 64 * MAXCH, "nsky_neus_weights_cos_fwd: S=%d out of range (<= %d)", S, 64 * MAXCH);
  hipLaunchKernelGGL(neus_weights_fwd_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, sdf, cosv, (const float*)nullptr, starts,
                     ends, variance, cos_anneal, R, S, alpha, weights, trans_bg, accumulation, depth, 1);
  NSKY_CHECK_LAUNCH("nsky_neus_weights_cos_fwd");
  return NSKY_OK;
}

extern "C" int nsky_neus_weights_bwd(const float* sdf, const float* grad, const float* ray_dirs, const float* starts,
                                     const float* ends, const float* variance, float cos_anneal, int32_t R, int32_t S,
                                     const float* d_weights, const float* d_trans_bg, float* d_sdf, float* d_grad,
                                     float* d_variance, nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(sdf && grad && ray_dirs && starts && ends && variance && d_weights && d_sdf && d_grad, "nsky_neus_weights_bwd: null argument");
  NSKY_CHECK_ARG(R > 0 && S > 0 && S <= 64 * MAXCH, "nsky_neus_weights_bwd: S=%d out of range (<= %d)", S, 64 * MAXCH);
  hipLaunchKernelGGL(neus_weights_bwd_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, sdf, grad, ray_dirs, starts,
                     ends, variance, cos_anneal, R, S, d_weights, d_trans_bg, d_sdf, d_grad, d_variance, 3);
  NSKY_CHECK_LAUNCH("nsky_neus_weights_bwd");
  return NSKY_OK;
}

extern "C" int nsky_neus_weights_cos_bwd(const float* sdf, const float* cosv, const float* starts, const float* ends, const float* variance,
                                         float cos_anneal, int32_t R, int32_t S, const float* d_weights, const float* d_trans_bg, float* d_sdf,
                                         float* d_cos, float* d_variance, nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(sdf && cosv && starts && ends && variance && d_weights && d_sdf && d_cos, "nsky_neus_weights_cos_bwd: null argument");
  NSKY_CHECK_ARG(R > 0 && S > 0 && S <= 64 * MAXCH, "nsky_neus_weights_cos_bwd: S=%d out of range (<= %d)", S, 64 * MAXCH);
  hipLaunchKernelGGL(neus_weights_bwd_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, sdf, cosv, (const float*)nullptr, starts,
                     ends, variance, cos_anneal, R, S, d_weights, d_trans_bg, d_sdf, d_cos, d_variance, 1);
  NSKY_CHECK_LAUNCH("nsky_neus_weights_cos_bwd");
  return NSKY_OK;
}

extern "C" int nsky_visibility_rays(const float* origins, const float* ray_dirs, const float* depth, const float* sel_dirs,
                                    int32_t R, int32_t Dv, float radius, float* sphere_pts, float* xrow, int32_t ldx,
                                    float* surf_dist, float* term_dist, nsky_stream_t stream) {
  if ((long)R * Dv == 0) return NSKY_OK;
  NSKY_CHECK_ARG(origins && ray_dirs && depth && sel_dirs && sphere_pts && xrow && surf_dist, "nsky_visibility_rays: null argument");
  NSKY_CHECK_ARG(R > 0 && Dv > 0 && ldx >= 15 && radius > 0.0f, "nsky_visibility_rays: bad sizes");
  const long n = (long)R * Dv;
  hipLaunchKernelGGL(visibility_rays_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, origins, ray_dirs, depth,
                     sel_dirs, R, Dv, radius, sphere_pts, xrow, ldx, surf_dist, term_dist);
  NSKY_CHECK_LAUNCH("nsky_visibility_rays");
  return NSKY_OK;
}

extern "C" int nsky_visibility_finish_fwd(const float* t_hat, const float* surf_dist, const float* threshold, float scale,
                                          const int32_t* sel_index, int32_t R, int32_t Dv, int32_t D, float* vis,
                                          nsky_stream_t stream) {
  if ((long)R * Dv == 0) return NSKY_OK;
  NSKY_CHECK_ARG(t_hat && surf_dist && threshold && sel_index && vis && R > 0 && Dv > 0 && D >= Dv, "nsky_visibility_finish_fwd: bad argument");
  const long n = (long)R * Dv;
  hipLaunchKernelGGL(visibility_finish_fwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, t_hat, surf_dist,
                     threshold, scale, sel_index, R, Dv, D, vis);
  NSKY_CHECK_LAUNCH("nsky_visibility_finish_fwd");
  return NSKY_OK;
}

extern "C" int nsky_visibility_finish_bwd(const float* t_hat, const float* surf_dist, const float* threshold, float scale,
                                          const int32_t* sel_index, int32_t R, int32_t Dv, int32_t D, const float* d_vis,
                                          float* d_t_hat, float* d_threshold, nsky_stream_t stream) {
  if ((long)R * Dv == 0) return NSKY_OK;
  NSKY_CHECK_ARG(t_hat && surf_dist && threshold && sel_index && d_vis && d_t_hat && R > 0 && Dv > 0 && D >= Dv,
                 "nsky_visibility_finish_bwd: bad argument");
  const long n = (long)R * Dv;
  const long blocks = ceil_div(n, 256);  // at most 256 workgroups: one atomic each into d_threshold
  hipLaunchKernelGGL(visibility_finish_bwd_kernel, dim3(blocks < 256 ? blocks : 256), dim3(256), 0, (hipStream_t)stream, t_hat, surf_dist,
                     threshold, scale, sel_index, R, Dv, D, d_vis, d_t_hat, d_threshold);
  NSKY_CHECK_LAUNCH("nsky_visibility_finish_bwd");
  return NSKY_OK;
}

extern "C" int nsky_density_weights_fwd(const float* raw, int32_t ld_raw, const float* ebins, int32_t R, int32_t n, float* weights,
                                        nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(raw && ebins && weights && ld_raw >= 1, "nsky_density_weights_fwd: bad argument");
  NSKY_CHECK_ARG(R > 0 && n > 0 && n <= 64 * MAXCH, "nsky_density_weights_fwd: n=%d out of range (<= %d)", n, 64 * MAXCH);
  hipLaunchKernelGGL(density_weights_fwd_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, raw, ld_raw, ebins, R, n,
                     weights);
  NSKY_CHECK_LAUNCH("nsky_density_weights_fwd");
  return NSKY_OK;
}

extern "C" int nsky_density_weights_bwd(const float* raw, int32_t ld_raw, const float* ebins, const float* d_weights, int32_t R,
                                        int32_t n, float* d_raw, nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(raw && ebins && d_weights && d_raw && ld_raw >= 1, "nsky_density_weights_bwd: bad argument");
  NSKY_CHECK_ARG(R > 0 && n > 0 && n <= 64 * MAXCH, "nsky_density_weights_bwd: n=%d out of range (<= %d)", n, 64 * MAXCH);
  hipLaunchKernelGGL(density_weights_bwd_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, raw, ld_raw, ebins,
                     d_weights, R, n, d_raw);
  NSKY_CHECK_LAUNCH("nsky_density_weights_bwd");
  return NSKY_OK;
}

extern "C" int nsky_interlevel_fwd(const float* c, const float* w, const float* sb, const float* wp, int32_t R, int32_t S, int32_t n,
                                   float* per_ray, nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(c && w && sb && wp && per_ray && R > 0 && S > 0 && n > 0, "nsky_interlevel_fwd: bad argument");
  NSKY_CHECK_ARG(n <= 1023, "nsky_interlevel_fwd: %d proposal samples per ray: at most 1023 (four rays x four (n + 1)-float arrays = 64 (n + 1) bytes of LDS per workgroup, 64 KB)", n);
  const size_t smem = 4 * 4 * (size_t)(n + 1) * sizeof(float);
  hipLaunchKernelGGL((interlevel_kernel<false>), dim3(ceil_div(R, 4)), dim3(256), smem, (hipStream_t)stream, c, w, sb, wp, nullptr, R,
                     S, n, per_ray, nullptr);
  NSKY_CHECK_LAUNCH("nsky_interlevel_fwd");
  return NSKY_OK;
}

extern "C" int nsky_interlevel_bwd(const float* c, const float* w, const float* sb, const float* wp, const float* d_per_ray,
                                   int32_t R, int32_t S, int32_t n, float* d_wp, nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(c && w && sb && wp && d_per_ray && d_wp && R > 0 && S > 0 && n > 0, "nsky_interlevel_bwd: bad argument");
  NSKY_CHECK_ARG(n <= 1023, "nsky_interlevel_bwd: %d proposal samples per ray: at most 1023 (four rays x four (n + 1)-float arrays = 64 (n + 1) bytes of LDS per workgroup, 64 KB)", n);
  const size_t smem = 4 * 4 * (size_t)(n + 1) * sizeof(float);
  hipLaunchKernelGGL((interlevel_kernel<true>), dim3(ceil_div(R, 4)), dim3(256), smem, (hipStream_t)stream, c, w, sb, wp, d_per_ray, R,
                     S, n, nullptr, d_wp);
  NSKY_CHECK_LAUNCH("nsky_interlevel_bwd");
  return NSKY_OK;
}

extern "C" int nsky_ray_reduce_fwd(const float* weights, const float* starts, const float* ends, const float* normals, const float* albedo,
                                   int32_t R, int32_t S, float max_clamp, float* sums, float* bounds, float* p2p, float* accumulation,
                                   float* normal, float* albedo_acc, nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(weights && starts && ends && sums && bounds && p2p && accumulation && R > 0 && S > 0, "nsky_ray_reduce_fwd: bad argument");
  NSKY_CHECK_ARG((normals != nullptr) == (normal != nullptr) && (albedo != nullptr) == (albedo_acc != nullptr),
                 "nsky_ray_reduce_fwd: normals / albedo inputs and outputs go together");
  // every workgroup has a ray; RR_MAX_BLOCKS updates reach each clip bound at the train step's ray counts, and a frame chunk's larger
  // ray sets keep at most eight rays per wave
  const int blocks = ceil_div(R, RR_WAVES), cap = ceil_div(R, RR_WAVES * 8) > RR_MAX_BLOCKS ? ceil_div(R, RR_WAVES * 8) : RR_MAX_BLOCKS;
  hipLaunchKernelGGL(ray_reduce_fwd_kernel, dim3(blocks < cap ? blocks : cap), dim3(RR_WAVES * 64), 0, (hipStream_t)stream, weights, starts,
                     ends, normals, albedo, R, S, sums, bounds);
  hipLaunchKernelGGL(ray_reduce_finish_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, (hipStream_t)stream, sums, bounds, R, max_clamp, p2p,
                     accumulation, normal, albedo_acc);
  NSKY_CHECK_LAUNCH("nsky_ray_reduce_fwd");
  return NSKY_OK;
}

extern "C" int nsky_ray_reduce_bwd(const float* weights, const float* starts, const float* ends, const float* normals, const float* albedo,
                                   const float* sums, const float* bounds, int32_t R, int32_t S, float max_clamp, const float* d_p2p,
                                   const float* d_accumulation, const float* d_normal, const float* d_albedo_acc, float* d_weights,
                                   float* d_normals, float* d_albedo, nsky_stream_t stream) {
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(weights && starts && ends && sums && bounds && d_weights && R > 0 && S > 0, "nsky_ray_reduce_bwd: bad argument");
  hipLaunchKernelGGL(ray_reduce_bwd_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, weights, starts, ends, normals, albedo,
                     sums, bounds, R, S, max_clamp, d_p2p, d_accumulation, d_normal, d_albedo_acc, d_weights, d_normals, d_albedo);
  NSKY_CHECK_LAUNCH("nsky_ray_reduce_bwd");
  return NSKY_OK;
}

extern "C" int nsky_normalize3_fwd(const float* g, int64_t P, float* n, nsky_stream_t stream) {
  if (P == 0) return NSKY_OK;
  NSKY_CHECK_ARG(g && n && P > 0, "nsky_normalize3_fwd: bad argument");
  hipLaunchKernelGGL(normalize3_fwd_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, (hipStream_t)stream, g, (long)P, n);
  NSKY_CHECK_LAUNCH("nsky_normalize3_fwd");
  return NSKY_OK;
}

extern "C" int nsky_normalize3_bwd(const float* g, const float* d_n, int64_t P, float* d_g, nsky_stream_t stream) {
  if (P == 0) return NSKY_OK;
  NSKY_CHECK_ARG(g && d_n && d_g && P > 0, "nsky_normalize3_bwd: bad argument");
  hipLaunchKernelGGL(normalize3_bwd_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, (hipStream_t)stream, g, d_n, (long)P, d_g);
  NSKY_CHECK_LAUNCH("nsky_normalize3_bwd");
  return NSKY_OK;
}

extern "C" int nsky_ray_points_fwd(const float* origins, const float* dirs, int32_t n_dirs, float sign, const float* t, int64_t n, float* out,
                                   nsky_stream_t stream) {
  if (n == 0) return NSKY_OK;
  NSKY_CHECK_ARG(origins && dirs && t && out && n > 0 && n_dirs > 0, "nsky_ray_points_fwd: bad argument");
  hipLaunchKernelGGL(ray_points_fwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, origins, dirs, n_dirs, sign, t, (long)n, out);
  NSKY_CHECK_LAUNCH("nsky_ray_points_fwd");
  return NSKY_OK;
}

extern "C" int nsky_ray_points_bwd(const float* dirs, int32_t n_dirs, float sign, const float* d_out, int64_t n, float* d_t, nsky_stream_t stream) {
  if (n == 0) return NSKY_OK;
  NSKY_CHECK_ARG(dirs && d_out && d_t && n > 0 && n_dirs > 0, "nsky_ray_points_bwd: bad argument");
  hipLaunchKernelGGL(ray_points_bwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, dirs, n_dirs, sign, d_out, (long)n, d_t);
  NSKY_CHECK_LAUNCH("nsky_ray_points_bwd");
  return NSKY_OK;
}

extern "C" int nsky_point_alphas_fwd(const float* sdf, const float* grad, const float* dirs, const float* gap3_host, const float* variance,
                                     float anneal, int32_t P, float* alphas, nsky_stream_t stream) {
  if (P == 0) return NSKY_OK;
  NSKY_CHECK_ARG(sdf && grad && dirs && gap3_host && variance && alphas && P > 0, "nsky_point_alphas_fwd: bad argument");
  hipLaunchKernelGGL(point_alphas_fwd_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, (hipStream_t)stream, sdf, grad, dirs, gap3_host[0], gap3_host[1],
                     gap3_host[2], variance, anneal, P, alphas);
  NSKY_CHECK_LAUNCH("nsky_point_alphas_fwd");
  return NSKY_OK;
}

extern "C" int nsky_point_alphas_bwd(const float* sdf, const float* grad, const float* dirs, const float* gap3_host, const float* variance,
                                     float anneal, int32_t P, const float* d_alphas, float* d_sdf, float* d_grad, float* d_variance,
                                     nsky_stream_t stream) {
  if (P == 0) return NSKY_OK;
  NSKY_CHECK_ARG(sdf && grad && dirs && gap3_host && variance && d_alphas && d_sdf && d_grad && P > 0, "nsky_point_alphas_bwd: bad argument");
  hipLaunchKernelGGL(point_alphas_bwd_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, (hipStream_t)stream, sdf, grad, dirs, gap3_host[0], gap3_host[1],
                     gap3_host[2], variance, anneal, P, d_alphas, d_sdf, d_grad, d_variance);
  NSKY_CHECK_LAUNCH("nsky_point_alphas_bwd");
  return NSKY_OK;
}

extern "C" int nsky_sigmoid_column_fwd(const float* raw, int32_t ld, int64_t n, float scale, float* t, nsky_stream_t stream) {
  if (n == 0) return NSKY_OK;
  NSKY_CHECK_ARG(raw && t && ld >= 1 && n > 0, "nsky_sigmoid_column_fwd: bad argument");
  hipLaunchKernelGGL(sigmoid_column_fwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, raw, ld, (long)n, scale, t);
  NSKY_CHECK_LAUNCH("nsky_sigmoid_column_fwd");
  return NSKY_OK;
}

extern "C" int nsky_sigmoid_column_bwd(const float* raw, int32_t ld, int64_t n, float scale, const float* d_t, float* d_raw, nsky_stream_t stream) {
  if (n == 0) return NSKY_OK;
  NSKY_CHECK_ARG(raw && d_t && d_raw && ld >= 1 && ld <= 8 && n > 0, "nsky_sigmoid_column_bwd: bad argument");
  hipLaunchKernelGGL(sigmoid_column_bwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, raw, ld, (long)n, scale, d_t, d_raw);
  NSKY_CHECK_LAUNCH("nsky_sigmoid_column_bwd");
  return NSKY_OK;
}
