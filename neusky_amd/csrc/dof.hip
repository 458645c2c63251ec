// Thin-lens depth of field of a frame (neusky_amd/relight/depth_of_field.py).  Definitions: include/neusky_hip.h, "Depth of field of a frame".
//
//   coc        one thread per pixel: depth and accumulation in, the blur radius in pixels out; the focus, where it is a pixel's, is read
//              by every thread from that pixel (one broadcast line) and written back into the lens block by one thread.
//   mark       a gather of every blurred pixel's square: pixel p is marked when a pixel q within `reach` of it has a radius that covers
//              their Chebyshev distance.  max(|dx|, |dy|) <= r_q holds for some q of row y' exactly when |dy| <= m(x, y'), m the largest
//              radius among the pixels of row y' whose span covers column x: the (2 reach + 1)^2 window folds into a row pass and a column
//              pass of 2 reach + 1 reads each.  A block owns a 64 x 64 tile: it loads the integer radii of the tile and its halo of
//              `reach` into LDS as bytes ((64 + 2 reach)^2, 36 KiB at reach 64), writes m for the tile's columns and the halo's rows into
//              LDS ((64 + 2 reach) x 64 bytes), and reads a column of it per pixel.  Neighbouring threads read neighbouring bytes: the
//              LDS serves a wave's read from 16 dwords, no bank is asked twice.  256 threads, 16 pixels each; 48 KiB of LDS at the most,
//              so three blocks share a CU at reach 64 and every tile of a 1080p frame (510) is resident at once.
//   lens rays  one thread per (marked pixel, lens sample): three pixels of the bundle, one hash, one sincos, two normalisations.
// Every rule is written with __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn: nothing contracts into a fused multiply-add, so a float32
// restatement in the same order has the same bits for the blur radius and the same mask.  Flat indices are 64-bit.  No atomics.
// Nothing here synchronises with the host.
#include <algorithm>

#include "numerics.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr int TILE = 64;       // a block's pixels: TILE x TILE
constexpr int MAX_REACH = 64;  // (the radii are bytes, and the halo is sized by it)

__device__ __forceinline__ float dot3(const float* a, const float* b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2]));
}

__global__ __launch_bounds__(256) void dof_coc_kernel(const float* __restrict__ depth, const float* __restrict__ acc, float* lens, int64_t P,
                                                      int64_t focus_pixel, float covered, float* __restrict__ coc) {
  float izf;
  if (focus_pixel >= 0) {  // (lens[10] is only written in this case, by one thread, and read by none)
    const float df = depth[focus_pixel];
    izf = (acc[focus_pixel] > covered && df > 0.0f) ? __fdiv_rn(1.0f, df) : 0.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) lens[10] = izf;
  } else {
    izf = lens[10];
  }
  const float afpx = lens[11];
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const float d = depth[p];
    const float iz = (acc[p] > covered && !(d <= 0.0f)) ? __fdiv_rn(1.0f, d) : 0.0f;  // (a NaN depth of a covered pixel stays a NaN)
    coc[p] = __fmul_rn(afpx, fabsf(__fsub_rn(iz, izf)));
  }
}

// the largest integer d <= reach with c + 0.5f >= (float)d, for a pixel with c >= threshold; -1 for every other (a NaN among them)
__device__ __forceinline__ int radius_of(float c, float threshold, int reach) {
  if (!(c >= threshold)) return -1;
  const float s = floorf(__fadd_rn(c, 0.5f));
  if (!(s >= 0.0f)) return -1;
  return (int)fminf(s, (float)reach);
}

__global__ __launch_bounds__(256) void dof_mark_kernel(const float* __restrict__ coc, int H, int W, float threshold, int reach,
                                                       uint8_t* __restrict__ mask) {
  extern __shared__ int8_t lds[];
  const int side = TILE + 2 * reach;  // the tile and its halo
  int8_t* rad = lds;                  // [side][side]: radii, -1 outside the image
  int8_t* cover = lds + side * side;  // [side][TILE]: m(x, y') for the tile's columns and the halo's rows
  const int x0 = (int)blockIdx.x * TILE, y0 = (int)blockIdx.y * TILE;
  for (int i = threadIdx.x; i < side * side; i += 256) {
    const int ly = i / side, lx = i - ly * side;
    const int y = y0 - reach + ly, x = x0 - reach + lx;
    int r = -1;
    if (y >= 0 && y < H && x >= 0 && x < W) r = radius_of(coc[(int64_t)y * W + x], threshold, reach);
    rad[i] = (int8_t)r;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < side * TILE; i += 256) {
    const int ly = i / TILE, lx = i - ly * TILE;  // column x0 + lx is at lx + reach of the halo row
    const int8_t* row = rad + ly * side + lx;     // row[j]: the pixel at dx = j - reach
    int m = -1;
    for (int j = 0; j <= 2 * reach; ++j) {
      const int r = row[j], dx = j < reach ? reach - j : j - reach;
      if (r >= dx && r > m) m = r;
    }
    cover[i] = (int8_t)m;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TILE * TILE; i += 256) {
    const int ly = i / TILE, lx = i - ly * TILE;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const int8_t* col = cover + ly * TILE + lx;  // col[j * TILE]: row y + j - reach
    bool marked = false;
    for (int j = 0; j <= 2 * reach; ++j) {
      const int dy = j < reach ? reach - j : j - reach;
      marked = marked || col[j * TILE] >= dy;
    }
    mask[(int64_t)y * W + x] = marked ? 1 : 0;
  }
}

// D = directions * norm of pixel p
__device__ __forceinline__ void unnormalised(const float* __restrict__ directions, const float* __restrict__ norm, int64_t p, float (&D)[3]) {
  const float n = norm ? norm[p] : 1.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) D[c] = __fmul_rn(directions[p * 3 + c], n);
}

// the 32-bit integer hash of the header
__device__ __forceinline__ uint32_t hash32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__global__ __launch_bounds__(256) void dof_lens_rays_kernel(const float* __restrict__ origins, const float* __restrict__ directions,
                                                            const float* __restrict__ norm, const float* __restrict__ pixel_area,
                                                            const int64_t* __restrict__ camera_indices, const int64_t* __restrict__ pixels,
                                                            const float* __restrict__ table, const float* __restrict__ lens, int H, int W,
                                                            int64_t E, int S1, int rotate, float* __restrict__ out_origins,
                                                            float* __restrict__ out_directions, float* __restrict__ out_norm,
                                                            float* __restrict__ out_pixel_area, int64_t* __restrict__ out_camera_indices) {
  const int64_t P = (int64_t)H * W, N = E * S1;
  float rh[3], sh[3], wh[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) rh[c] = lens[c], sh[c] = lens[3 + c], wh[c] = lens[6 + c];
  const float a = lens[9], izf = lens[10];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const int64_t e = i / S1;
    const int s = (int)(i - e * S1);
    const int64_t p = min(max(pixels[e], (int64_t)0), P - 1);  // (no access leaves the frame)
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const float dx = table[4 * s], dy = table[4 * s + 1];
    float u = table[4 * s + 2], v = table[4 * s + 3];
    float D[3], A[3], B[3], gx[3] = {0.0f, 0.0f, 0.0f}, gy[3] = {0.0f, 0.0f, 0.0f};
    unnormalised(directions, norm, p, D);
    if (W > 1) {  // forward difference; backward in the last column
      const int64_t q = x + 1 < W ? p : p - 1;
      unnormalised(directions, norm, q, A);
      unnormalised(directions, norm, q + 1, B);
#pragma unroll
      for (int c = 0; c < 3; ++c) gx[c] = __fsub_rn(B[c], A[c]);
    }
    if (H > 1) {
      const int64_t q = y + 1 < H ? p : p - W;
      unnormalised(directions, norm, q, A);
      unnormalised(directions, norm, q + W, B);
#pragma unroll
      for (int c = 0; c < 3; ++c) gy[c] = __fsub_rn(B[c], A[c]);
    }
    float d[3], l[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = __fadd_rn(__fadd_rn(D[c], __fmul_rn(dx, gx[c])), __fmul_rn(dy, gy[c]));
    if (rotate) {
      const float theta = __fmul_rn((float)(hash32((uint32_t)p) >> 8), 3.7450702829239286e-07f);  // 2 pi 2^-24
      float sn, cs;
      sincosf(theta, &sn, &cs);
      const float ur = __fsub_rn(__fmul_rn(u, cs), __fmul_rn(v, sn)), vr = __fadd_rn(__fmul_rn(u, sn), __fmul_rn(v, cs));
      u = ur, v = vr;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) l[c] = __fmul_rn(a, __fadd_rn(__fmul_rn(u, rh[c]), __fmul_rn(v, sh[c])));
    const float k = dot3(d, wh), t = __fmul_rn(k, izf);
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = __fsub_rn(d[c], __fmul_rn(t, l[c]));
    const float len = __fsqrt_rn(dot3(d, d));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      out_directions[i * 3 + c] = __fdiv_rn(d[c], len);
      out_origins[i * 3 + c] = __fadd_rn(origins[p * 3 + c], l[c]);
    }
    out_norm[i] = __fdiv_rn(len, k);
    if (pixel_area) out_pixel_area[i] = pixel_area[p];
    if (camera_indices) out_camera_indices[i] = camera_indices[p];
  }
}

unsigned grid_of(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 256 * 16)); }

}  // namespace

extern "C" int nsky_dof_coc(const float* depth, const float* accumulation, float* lens, int32_t H, int32_t W, int64_t focus_pixel,
                            float covered, float* coc, nsky_stream_t stream) {
  NSKY_CHECK_ARG(H >= 0 && W >= 0, "nsky_dof_coc: H %d, W %d", (int)H, (int)W);
  const int64_t P = (int64_t)H * W;
  NSKY_CHECK_ARG(focus_pixel < P, "nsky_dof_coc: focus pixel %ld of %ld pixels", (long)focus_pixel, (long)P);
  if (P == 0) return NSKY_OK;
  NSKY_CHECK_ARG(depth && accumulation && lens && coc, "nsky_dof_coc: NULL depth / accumulation / lens / coc");
  hipLaunchKernelGGL(dof_coc_kernel, dim3(grid_of(P)), dim3(256), 0, (hipStream_t)stream, depth, accumulation, lens, P, focus_pixel, covered,
                     coc);
  NSKY_CHECK_LAUNCH("nsky_dof_coc");
  return NSKY_OK;
}

extern "C" int nsky_dof_mark(const float* coc, int32_t H, int32_t W, float threshold, int32_t reach, uint8_t* mask, nsky_stream_t stream) {
  NSKY_CHECK_ARG(H >= 0 && W >= 0, "nsky_dof_mark: H %d, W %d", (int)H, (int)W);
  NSKY_CHECK_ARG(reach >= 1 && reach <= MAX_REACH, "nsky_dof_mark: reach %d outside 1..%d", (int)reach, MAX_REACH);
  if (H == 0 || W == 0) return NSKY_OK;
  NSKY_CHECK_ARG(coc && mask, "nsky_dof_mark: NULL coc / mask");
  const int64_t tx = ((int64_t)W + TILE - 1) / TILE, ty = ((int64_t)H + TILE - 1) / TILE;
  NSKY_CHECK_ARG(ty <= 65535, "nsky_dof_mark: %d rows are more than 65535 tiles of %d", (int)H, TILE);
  const int side = TILE + 2 * reach;
  const size_t lds = (size_t)side * side + (size_t)side * TILE;  // 48 KiB at reach 64
  hipLaunchKernelGGL(dof_mark_kernel, dim3((unsigned)tx, (unsigned)ty), dim3(256), lds, (hipStream_t)stream, coc, (int)H, (int)W, threshold,
                     (int)reach, mask);
  NSKY_CHECK_LAUNCH("nsky_dof_mark");
  return NSKY_OK;
}

extern "C" int nsky_dof_lens_rays(const float* origins, const float* directions, const float* norm, const float* pixel_area,
                                  const int64_t* camera_indices, const int64_t* pixels, const float* table, const float* lens, int32_t H,
                                  int32_t W, int64_t E, int32_t S1, int32_t rotate, float* out_origins, float* out_directions, float* out_norm,
                                  float* out_pixel_area, int64_t* out_camera_indices, nsky_stream_t stream) {
  NSKY_CHECK_ARG(H >= 0 && W >= 0 && E >= 0 && S1 >= 0, "nsky_dof_lens_rays: H %d, W %d, E %ld, S1 %d", (int)H, (int)W, (long)E, (int)S1);
  if (E == 0 || S1 == 0) return NSKY_OK;
  NSKY_CHECK_ARG(H >= 1 && W >= 1, "nsky_dof_lens_rays: %ld pixels of an empty frame (H %d, W %d)", (long)E, (int)H, (int)W);
  NSKY_CHECK_ARG(origins && directions && pixels && table && lens && out_origins && out_directions && out_norm,
                 "nsky_dof_lens_rays: NULL origins / directions / pixels / table / lens / out_origins / out_directions / out_norm");
  NSKY_CHECK_ARG((!pixel_area || out_pixel_area) && (!camera_indices || out_camera_indices),
                 "nsky_dof_lens_rays: pixel_area / camera_indices given without their outputs");
  hipLaunchKernelGGL(dof_lens_rays_kernel, dim3(grid_of(E * S1)), dim3(256), 0, (hipStream_t)stream, origins, directions, norm, pixel_area,
                     camera_indices, pixels, table, lens, (int)H, (int)W, E, (int)S1, (int)rotate, out_origins, out_directions, out_norm,
                     out_pixel_area, out_camera_indices);
  NSKY_CHECK_LAUNCH("nsky_dof_lens_rays");
  return NSKY_OK;
}
