// Adaptive antialiasing of a frame (neusky_amd/relight/antialias.py).  Definitions: include/neusky_hip.h, "Adaptive antialiasing of a frame".
//
//   edge mask  one thread per pixel: its own G-buffer values and those of its up to 4 neighbours, then the K luminances; the first test
//              that fires ends the thread.  The neighbours' reads are the wave's own lines or the rows next to them: they come from L2.
//   rays       one thread per (marked pixel, offset): three pixels of the bundle (itself, one along each axis), a normalisation.
//   resolve    one thread per (marked pixel, image, channel): S1 reads of the second pass's output through its strides, an fp64 sum, one
//              read-modify-write of the frame.
// Every rule is written with __fmul_rn / __fadd_rn / __fsub_rn: nothing contracts into a fused multiply-add, so a float32 restatement in
// the same order has the same bits.  Flat indices are 64-bit.  Nothing here synchronises with the host.
#include <algorithm>

#include "numerics.h"
#include "../../include/neusky_hip.h"

namespace {

// the display transform's luminance (display.hip): every product and sum rounded once
__device__ __forceinline__ float luminance(const float* p) {
  return __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, p[0]), __fmul_rn(0.7152f, p[1])), __fmul_rn(0.0722f, p[2]));
}

__device__ __forceinline__ float dot3(const float* a, const float* b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2]));
}

struct EdgeThresholds {
  float accumulation, depth, cos2, colour, covered;
};

// the three tests that read the G-buffer, of the pair (p, q)
__device__ __forceinline__ bool geometry_differs(const float* __restrict__ depth, const float* __restrict__ normal,
                                                 const float* __restrict__ acc, int64_t p, int64_t q, float ap, float dp, float pp,
                                                 const EdgeThresholds& t) {
  const float aq = acc[q];
  if (fabsf(__fsub_rn(ap, aq)) > t.accumulation) return true;
  if (!(ap > t.covered && aq > t.covered)) return false;
  const float dq = depth[q];
  if (fabsf(__fsub_rn(dp, dq)) > __fmul_rn(t.depth, fminf(dp, dq))) return true;
  const float qq = dot3(normal + q * 3, normal + q * 3);
  if (!(pp >= 1e-12f && qq >= 1e-12f)) return false;
  const float d = dot3(normal + p * 3, normal + q * 3);
  return d <= 0.0f || __fmul_rn(d, d) < __fmul_rn(t.cos2, __fmul_rn(pp, qq));
}

__global__ __launch_bounds__(256) void aa_edge_mask_kernel(const float* __restrict__ depth, const float* __restrict__ normal,
                                                           const float* __restrict__ acc, const float* __restrict__ lin, int64_t ls_k,
                                                           int64_t ls_p, int K, int H, int W, EdgeThresholds t,
                                                           uint8_t* __restrict__ mask) {
  const int64_t P = (int64_t)H * W;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    int64_t nb[4];
    int n = 0;
    if (x > 0) nb[n++] = p - 1;
    if (x + 1 < W) nb[n++] = p + 1;
    if (y > 0) nb[n++] = p - W;
    if (y + 1 < H) nb[n++] = p + W;
    const float ap = acc[p], dp = depth[p], pp = dot3(normal + p * 3, normal + p * 3);
    bool marked = false;
    for (int j = 0; j < n && !marked; ++j) marked = geometry_differs(depth, normal, acc, p, nb[j], ap, dp, pp, t);
    for (int k = 0; k < K && !marked; ++k) {
      const float* img = lin + (int64_t)k * ls_k;
      const float yp = luminance(img + p * ls_p);
      for (int j = 0; j < n && !marked; ++j) {
        const float yq = luminance(img + nb[j] * ls_p);
        marked = fabsf(__fsub_rn(yp, yq)) > __fmul_rn(t.colour, fmaxf(fmaxf(yp, yq), 1e-4f));
      }
    }
    mask[p] = marked ? 1 : 0;
  }
}

// D = directions * norm of pixel p
__device__ __forceinline__ void unnormalised(const float* __restrict__ directions, const float* __restrict__ norm, int64_t p, float (&D)[3]) {
  const float n = norm ? norm[p] : 1.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) D[c] = __fmul_rn(directions[p * 3 + c], n);
}

__global__ __launch_bounds__(256) void aa_subpixel_rays_kernel(const float* __restrict__ origins, const float* __restrict__ directions,
                                                               const float* __restrict__ norm, const float* __restrict__ pixel_area,
                                                               const int64_t* __restrict__ camera_indices, const int64_t* __restrict__ pixels,
                                                               const float* __restrict__ offsets, int H, int W, int64_t E, int S1,
                                                               float* __restrict__ out_origins, float* __restrict__ out_directions,
                                                               float* __restrict__ out_norm, float* __restrict__ out_pixel_area,
                                                               int64_t* __restrict__ out_camera_indices) {
  const int64_t P = (int64_t)H * W, N = E * S1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const int64_t e = i / S1;
    const int s = (int)(i - e * S1);
    const int64_t p = min(max(pixels[e], (int64_t)0), P - 1);  // (no access leaves the frame)
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const float dx = offsets[2 * s], dy = offsets[2 * s + 1];
    float D[3], A[3], B[3], gx[3] = {0.0f, 0.0f, 0.0f}, gy[3] = {0.0f, 0.0f, 0.0f};
    unnormalised(directions, norm, p, D);
    if (W > 1) {  // forward difference; backward in the last column
      const int64_t a = x + 1 < W ? p : p - 1;
      unnormalised(directions, norm, a, A);
      unnormalised(directions, norm, a + 1, B);
#pragma unroll
      for (int c = 0; c < 3; ++c) gx[c] = __fsub_rn(B[c], A[c]);
    }
    if (H > 1) {
      const int64_t a = y + 1 < H ? p : p - W;
      unnormalised(directions, norm, a, A);
      unnormalised(directions, norm, a + W, B);
#pragma unroll
      for (int c = 0; c < 3; ++c) gy[c] = __fsub_rn(B[c], A[c]);
    }
    float d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = __fadd_rn(__fadd_rn(D[c], __fmul_rn(dx, gx[c])), __fmul_rn(dy, gy[c]));
    const float len = __fsqrt_rn(dot3(d, d));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      out_directions[i * 3 + c] = __fdiv_rn(d[c], len);
      out_origins[i * 3 + c] = origins[p * 3 + c];
    }
    out_norm[i] = len;
    if (pixel_area) out_pixel_area[i] = pixel_area[p];
    if (camera_indices) out_camera_indices[i] = camera_indices[p];
  }
}

__global__ __launch_bounds__(256) void aa_resolve_kernel(float* __restrict__ F, int64_t fs_k, int64_t fs_p, const float* __restrict__ X,
                                                         int64_t xs_k, int64_t xs_e, int64_t xs_s, const int64_t* __restrict__ pixels, int K,
                                                         int64_t P, int64_t E, int S1, int C, float* __restrict__ rgb, int64_t rs_k,
                                                         int64_t rs_p) {
  const int64_t n = E * K * C;
  const double count = (double)(S1 + 1);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t ek = i / C;
    const int c = (int)(i - ek * C);
    const int64_t e = ek / K;
    const int k = (int)(ek - e * K);
    const int64_t p = pixels[e];
    if (p < 0 || p >= P) continue;
    const int64_t o = (int64_t)k * fs_k + p * fs_p + c;
    const float* x = X + (int64_t)k * xs_k + e * xs_e + c;
    double sum = (double)F[o];
    for (int s = 0; s < S1; ++s) sum += (double)x[s * xs_s];
    const float v = (float)(sum / count);
    F[o] = v;
    if (rgb) rgb[(int64_t)k * rs_k + p * rs_p + c] = srgb_fwd(v);
  }
}

unsigned grid_of(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 256 * 16)); }

}  // namespace

extern "C" int nsky_aa_edge_mask(const float* depth, const float* normal, const float* accumulation, const float* lin, int64_t ls_k,
                                 int64_t ls_p, int32_t K, int32_t H, int32_t W, float t_accumulation, float t_depth, float cos2,
                                 float t_colour, float covered, uint8_t* mask, nsky_stream_t stream) {
  NSKY_CHECK_ARG(K >= 0 && H >= 0 && W >= 0, "nsky_aa_edge_mask: K %d, H %d, W %d", (int)K, (int)H, (int)W);
  NSKY_CHECK_ARG(K == 0 || (ls_k >= 0 && ls_p >= 3), "nsky_aa_edge_mask: strides %ld, %ld of lin", (long)ls_k, (long)ls_p);
  if (H == 0 || W == 0) return NSKY_OK;
  NSKY_CHECK_ARG(depth && normal && accumulation && mask && (lin || K == 0), "nsky_aa_edge_mask: NULL depth / normal / accumulation / lin / mask");
  const EdgeThresholds t = {t_accumulation, t_depth, cos2, t_colour, covered};
  hipLaunchKernelGGL(aa_edge_mask_kernel, dim3(grid_of((int64_t)H * W)), dim3(256), 0, (hipStream_t)stream, depth, normal, accumulation, lin,
                     ls_k, ls_p, (int)K, (int)H, (int)W, t, mask);
  NSKY_CHECK_LAUNCH("nsky_aa_edge_mask");
  return NSKY_OK;
}

extern "C" int nsky_aa_subpixel_rays(const float* origins, const float* directions, const float* norm, const float* pixel_area,
                                     const int64_t* camera_indices, const int64_t* pixels, const float* offsets, int32_t H, int32_t W, int64_t E,
                                     int32_t S1, float* out_origins, float* out_directions, float* out_norm, float* out_pixel_area,
                                     int64_t* out_camera_indices, nsky_stream_t stream) {
  NSKY_CHECK_ARG(H >= 0 && W >= 0 && E >= 0 && S1 >= 0, "nsky_aa_subpixel_rays: H %d, W %d, E %ld, S1 %d", (int)H, (int)W, (long)E, (int)S1);
  if (E == 0 || S1 == 0) return NSKY_OK;
  NSKY_CHECK_ARG(H >= 1 && W >= 1, "nsky_aa_subpixel_rays: %ld pixels of an empty frame (H %d, W %d)", (long)E, (int)H, (int)W);
  NSKY_CHECK_ARG(origins && directions && pixels && offsets && out_origins && out_directions && out_norm,
                 "nsky_aa_subpixel_rays: NULL origins / directions / pixels / offsets / out_origins / out_directions / out_norm");
  NSKY_CHECK_ARG((!pixel_area || out_pixel_area) && (!camera_indices || out_camera_indices),
                 "nsky_aa_subpixel_rays: pixel_area / camera_indices given without their outputs");
  hipLaunchKernelGGL(aa_subpixel_rays_kernel, dim3(grid_of(E * S1)), dim3(256), 0, (hipStream_t)stream, origins, directions, norm, pixel_area,
                     camera_indices, pixels, offsets, (int)H, (int)W, E, (int)S1, out_origins, out_directions, out_norm, out_pixel_area,
                     out_camera_indices);
  NSKY_CHECK_LAUNCH("nsky_aa_subpixel_rays");
  return NSKY_OK;
}

extern "C" int nsky_aa_resolve(float* F, int64_t fs_k, int64_t fs_p, const float* X, int64_t xs_k, int64_t xs_e, int64_t xs_s,
                               const int64_t* pixels, int32_t K, int64_t P, int64_t E, int32_t S1, int32_t C, float* rgb, int64_t rs_k,
                               int64_t rs_p, nsky_stream_t stream) {
  NSKY_CHECK_ARG(K >= 0 && P >= 0 && E >= 0 && S1 >= 0 && C >= 0, "nsky_aa_resolve: K %d, P %ld, E %ld, S1 %d, C %d", (int)K, (long)P, (long)E,
                 (int)S1, (int)C);
  NSKY_CHECK_ARG(xs_k >= 0 && xs_e >= 0 && xs_s >= 0, "nsky_aa_resolve: strides %ld, %ld, %ld of X", (long)xs_k, (long)xs_e, (long)xs_s);
  NSKY_CHECK_ARG(fs_k >= 0 && fs_p >= 0 && rs_k >= 0 && rs_p >= 0, "nsky_aa_resolve: strides %ld, %ld of F, %ld, %ld of rgb", (long)fs_k,
                 (long)fs_p, (long)rs_k, (long)rs_p);
  if (K == 0 || P == 0 || E == 0 || C == 0) return NSKY_OK;
  NSKY_CHECK_ARG(F && pixels && (X || S1 == 0), "nsky_aa_resolve: NULL F / X / pixels");
  hipLaunchKernelGGL(aa_resolve_kernel, dim3(grid_of(E * K * C)), dim3(256), 0, (hipStream_t)stream, F, fs_k, fs_p, X, xs_k, xs_e, xs_s,
                     pixels, (int)K, P, E, (int)S1, (int)C, rgb, rs_k, rs_p);
  NSKY_CHECK_LAUNCH("nsky_aa_resolve");
  return NSKY_OK;
}
