// Mesh simplification by vertex clustering with quadric-error placement (Lindstrom 2000): the exporter's step after marching
// cubes (neusky_amd/exporter/simplify.py).  Definitions: include/neusky_hip.h (nsky_mesh_*).
//
//   cell_keys        key of every vertex's cell (float64 floor of (p - lo) / h, three 21-bit fields)
//   cluster_count    faces whose corners lie in three different cells, straight from vertices and faces: no sort, one integer
//   vertex_cells     rank of every vertex's cell, scattered back from the sorted order
//   remap_faces      corner cells of every face and the sort key (smallest cell << 32 | its successor) of a surviving face
//   cluster_reduce   per cell: the plane quadrics of the faces touching it (computed on the fly from the face's corners: the 3 F
//                    records of 10 doubles are never stored) and the sums of its vertices' positions, normals and colours
//   cluster_solve    one thread per cell: cyclic Jacobi on the 3x3 quadric matrix, pseudo-inverse step, box test, fp32 result
//   flag_duplicates  faces with the same (rotated) triple: the first in input order stays
//   compact_faces    surviving faces, rotated so that the smallest index leads, to their scanned slots
// No floating-point atomics: a cell's sums run over the records a stable sort brought together, strided over the lanes of a
// fixed-width group, then an xor butterfly (the same bits in every lane).  The only atomic is cluster_count's integer counter.
// All geometry is float64 on the fp32 inputs, without contraction into fmas, so that floor() sees what the restatement sees.
#include "common.h"
#include "../../include/neusky_hip.h"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGrid = 1 << 16;
constexpr double kCellMax = (double)((1 << NSKY_MESH_KEY_BITS) - 1);
constexpr int kSums = NSKY_MESH_CELL_SUMS;
constexpr int kSweeps = 12;  // cyclic Jacobi converges quadratically: a 3x3 matrix is diagonal to the last bit after 5 or 6

struct Grid {
  double lx, ly, lz, h;
};

__device__ __forceinline__ int64_t axis_cell(double p, double lo, double h) {
  double t = floor((p - lo) / h);
  t = fmin(fmax(t, 0.0), kCellMax);  // fmax(NaN, 0) = 0
  return (int64_t)t;
}

__device__ __forceinline__ int64_t cell_key(const float* __restrict__ verts, int64_t v, const Grid& g) {
  const int64_t i = axis_cell((double)verts[3 * v], g.lx, g.h), j = axis_cell((double)verts[3 * v + 1], g.ly, g.h),
                k = axis_cell((double)verts[3 * v + 2], g.lz, g.h);
  return (i << (2 * NSKY_MESH_KEY_BITS)) | (j << NSKY_MESH_KEY_BITS) | k;
}

__device__ __forceinline__ bool in_range(int32_t a, int32_t b, int32_t c, int64_t V) {
  return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
}

__global__ __launch_bounds__(kThreads) void cell_keys_kernel(const float* __restrict__ verts, int64_t V, Grid g, int64_t* __restrict__ keys) {
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += (int64_t)gridDim.x * kThreads) keys[v] = cell_key(verts, v, g);
}

__global__ __launch_bounds__(kThreads) void cluster_count_kernel(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                                  int64_t F, Grid g, unsigned long long* __restrict__ count) {
  __shared__ int wsum[kThreads / 64];
  int local = 0;
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += (int64_t)gridDim.x * kThreads) {
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!in_range(a, b, c, V)) continue;
    const int64_t ka = cell_key(verts, a, g), kb = cell_key(verts, b, g), kc = cell_key(verts, c, g);
    local += (ka != kb && kb != kc && ka != kc);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) t += wsum[w];
    if (t) atomicAdd(count, (unsigned long long)t);
  }
}

__global__ __launch_bounds__(kThreads) void vertex_cells_kernel(const int64_t* __restrict__ order, const int64_t* __restrict__ rank_sorted,
                                                                 int64_t V, int32_t* __restrict__ vertex_cell) {
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < V; p += (int64_t)gridDim.x * kThreads) {
    const int64_t v = order[p];
    if (v >= 0 && v < V) vertex_cell[v] = (int32_t)rank_sorted[p];
  }
}

// the face's corner cells rotated (orientation kept) so that the smallest comes first; the three differ
__device__ __forceinline__ void rotate_smallest_first(int32_t a, int32_t b, int32_t c, int32_t& i, int32_t& j, int32_t& k) {
  i = a; j = b; k = c;
  if (b < a && b < c) {
    i = b; j = c; k = a;
  } else if (c < a && c < b) {
    i = c; j = a; k = b;
  }
}

__global__ __launch_bounds__(kThreads) void remap_faces_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                                const int32_t* __restrict__ vertex_cell, int64_t V,
                                                                int32_t* __restrict__ corner_cells, int64_t* __restrict__ face_keys) {
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += (int64_t)gridDim.x * kThreads) {
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const bool ok = in_range(a, b, c, V);
    const int32_t ca = ok ? vertex_cell[a] : -1, cb = ok ? vertex_cell[b] : -1, cc = ok ? vertex_cell[c] : -1;
    corner_cells[3 * f] = ca;
    corner_cells[3 * f + 1] = cb;
    corner_cells[3 * f + 2] = cc;
    int64_t key = -1;
    if (ok && ca != cb && cb != cc && ca != cc) {
      int32_t i, j, k;
      rotate_smallest_first(ca, cb, cc, i, j, k);
      key = ((int64_t)i << 32) | (int64_t)j;
    }
    face_keys[f] = key;
  }
}

__device__ __forceinline__ int32_t last_of_rotated(const int32_t* __restrict__ corner_cells, int64_t f) {
  int32_t i, j, k;
  rotate_smallest_first(corner_cells[3 * f], corner_cells[3 * f + 1], corner_cells[3 * f + 2], i, j, k);
  return k;
}

// sorted position p holds face order[p]; equal keys (same first two indices) are adjacent and, the sort being stable, in input order:
// a face is a duplicate when an earlier face of its run has the same third index.  Runs are a few faces long (the faces that cross
// one directed cell-to-cell edge).
__global__ __launch_bounds__(kThreads) void flag_duplicates_kernel(const int32_t* __restrict__ corner_cells, int64_t F,
                                                                    const int64_t* __restrict__ sorted_keys, const int64_t* __restrict__ order,
                                                                    int32_t* __restrict__ keep) {
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < F; p += (int64_t)gridDim.x * kThreads) {
    const int64_t f = order[p];
    if (f < 0 || f >= F) continue;
    const int64_t key = sorted_keys[p];
    int32_t flag = key >= 0;
    if (flag) {
      const int32_t k = last_of_rotated(corner_cells, f);
      for (int64_t q = p - 1; q >= 0 && sorted_keys[q] == key; --q) {
        const int64_t e = order[q];
        if (e >= 0 && e < F && last_of_rotated(corner_cells, e) == k) {
          flag = 0;
          break;
        }
      }
    }
    keep[f] = flag;
  }
}

__global__ __launch_bounds__(kThreads) void compact_faces_kernel(const int32_t* __restrict__ corner_cells, int64_t F,
                                                                  const int32_t* __restrict__ keep, const int64_t* __restrict__ ends,
                                                                  int64_t F_out, int32_t* __restrict__ out) {
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += (int64_t)gridDim.x * kThreads) {
    if (!keep[f]) continue;
    const int64_t o = ends[f] - 1;
    if (o < 0 || o >= F_out) continue;
    int32_t i, j, k;
    rotate_smallest_first(corner_cells[3 * f], corner_cells[3 * f + 1], corner_cells[3 * f + 2], i, j, k);
    out[3 * o] = i;
    out[3 * o + 1] = j;
    out[3 * o + 2] = k;
  }
}

__device__ __forceinline__ int64_t lower_bound(const int32_t* __restrict__ sorted, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)sorted[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// A group of G lanes per cell (G = 8 for the handful of records of a fine grid, G = 64 for the hundreds of a coarse one): lane l
// takes records l, l + G, ... of the cell's two segments in order, then the group's xor butterfly adds the G partials.
template <int G>
__global__ __launch_bounds__(kThreads) void cluster_reduce_kernel(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                                   int64_t F, const float* __restrict__ normals,
                                                                   const uint8_t* __restrict__ colours, Grid g,
                                                                   const int64_t* __restrict__ vertex_order, const int64_t* __restrict__ cell_start,
                                                                   int64_t C, const int32_t* __restrict__ sorted_corner_cells,
                                                                   const int64_t* __restrict__ corner_order, double* __restrict__ sums) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t n_groups = (int64_t)gridDim.x * (kThreads / G);
  for (int64_t c = (int64_t)blockIdx.x * (kThreads / G) + threadIdx.x / G; c < C; c += n_groups) {
    double s[kSums];
#pragma unroll
    for (int u = 0; u < kSums; ++u) s[u] = 0.0;
    const int64_t n_rec = 3 * F;
    const int64_t rs = lower_bound(sorted_corner_cells, n_rec, c), re = lower_bound(sorted_corner_cells, n_rec, c + 1);
    for (int64_t p = rs + lane; p < re; p += G) {
      const int64_t r = corner_order[p];
      if (r < 0 || r >= n_rec) continue;
      const int64_t f = r / 3;
      const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
      if (!in_range(ia, ib, ic, V)) continue;
      const double ax = (double)verts[3 * (int64_t)ia] - g.lx, ay = (double)verts[3 * (int64_t)ia + 1] - g.ly, az = (double)verts[3 * (int64_t)ia + 2] - g.lz;
      const double bx = (double)verts[3 * (int64_t)ib] - g.lx, by = (double)verts[3 * (int64_t)ib + 1] - g.ly, bz = (double)verts[3 * (int64_t)ib + 2] - g.lz;
      const double cx = (double)verts[3 * (int64_t)ic] - g.lx, cy = (double)verts[3 * (int64_t)ic + 1] - g.ly, cz = (double)verts[3 * (int64_t)ic + 2] - g.lz;
      const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
      const double mx = uy * vz - uz * vy, my = uz * vx - ux * vz, mz = ux * vy - uy * vx;
      const double len = sqrt(mx * mx + my * my + mz * mz);
      if (!(len > 0.0) || !(len < INFINITY)) continue;
      const double nx = mx / len, ny = my / len, nz = mz / len, w = 0.5 * len;
      const double d = nx * ax + ny * ay + nz * az;
      const double wx = w * nx, wy = w * ny, wz = w * nz, wd = w * d;
      s[0] += wx * nx; s[1] += wx * ny; s[2] += wx * nz;
      s[3] += wy * ny; s[4] += wy * nz; s[5] += wz * nz;
      s[6] += wd * nx; s[7] += wd * ny; s[8] += wd * nz;
      s[9] += wd * d;
    }
    for (int64_t p = cell_start[c] + lane; p < cell_start[c + 1]; p += G) {
      const int64_t v = vertex_order[p];
      if (v < 0 || v >= V) continue;
      s[10] += (double)verts[3 * v] - g.lx;
      s[11] += (double)verts[3 * v + 1] - g.ly;
      s[12] += (double)verts[3 * v + 2] - g.lz;
      if (normals) {
        s[13] += (double)normals[3 * v];
        s[14] += (double)normals[3 * v + 1];
        s[15] += (double)normals[3 * v + 2];
      }
      if (colours) {
        s[16] += (double)colours[3 * v];
        s[17] += (double)colours[3 * v + 1];
        s[18] += (double)colours[3 * v + 2];
      }
      s[19] += 1.0;
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
#pragma unroll
      for (int u = 0; u < kSums; ++u) s[u] += __shfl_xor(s[u], off, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < kSums; ++u) sums[c * kSums + u] = s[u];
    }
  }
}

// one Jacobi rotation that zeroes A[P][Q] (P < Q; R is the third index); E accumulates the eigenvectors as columns
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&A)[3][3], double (&E)[3][3]) {
  constexpr int R = 3 - P - Q;
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  A[P][P] -= t * apq;
  A[Q][Q] += t * apq;
  A[P][Q] = A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = arp - s * (arq + tau * arp);
  A[R][Q] = A[Q][R] = arq + s * (arp - tau * arq);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double ekp = E[k][P], ekq = E[k][Q];
    E[k][P] = ekp - s * (ekq + tau * ekp);
    E[k][Q] = ekq + s * (ekp - tau * ekq);
  }
}

__global__ __launch_bounds__(kThreads) void cluster_solve_kernel(const double* __restrict__ sums, const int64_t* __restrict__ cell_keys, int64_t C,
                                                                  Grid g, float* __restrict__ verts_out, float* __restrict__ normals_out,
                                                                  uint8_t* __restrict__ colours_out) {
  for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < C; c += (int64_t)gridDim.x * kThreads) {
    const double* s = sums + c * kSums;
    const double cnt = s[19] > 0.0 ? s[19] : 1.0;
    const double xbar[3] = {s[10] / cnt, s[11] / cnt, s[12] / cnt};
    const double A0[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    double A[3][3], E[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        A[a][b] = A0[a][b];
        E[a][b] = a == b ? 1.0 : 0.0;
      }
    }
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
      jacobi_rotate<0, 1>(A, E);
      jacobi_rotate<0, 2>(A, E);
      jacobi_rotate<1, 2>(A, E);
    }
    const double lmax = fmax(A[0][0], fmax(A[1][1], A[2][2]));
    double x[3] = {xbar[0], xbar[1], xbar[2]};
    if (lmax > 0.0) {
      double r[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) r[a] = s[6 + a] - (A0[a][0] * xbar[0] + A0[a][1] * xbar[1] + A0[a][2] * xbar[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double lam = A[i][i];
        if (lam > NSKY_MESH_TAU * lmax) {
          const double co = (E[0][i] * r[0] + E[1][i] * r[1] + E[2][i] * r[2]) / lam;
#pragma unroll
          for (int a = 0; a < 3; ++a) x[a] += E[a][i] * co;
        }
      }
      const int64_t key = cell_keys[c];
      const int64_t mask = ((int64_t)1 << NSKY_MESH_KEY_BITS) - 1;
      const double idx[3] = {(double)((key >> (2 * NSKY_MESH_KEY_BITS)) & mask), (double)((key >> NSKY_MESH_KEY_BITS) & mask), (double)(key & mask)};
      bool inside = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) inside = inside && x[a] >= idx[a] * g.h && x[a] <= (idx[a] + 1.0) * g.h;
      if (!inside) {
#pragma unroll
        for (int a = 0; a < 3; ++a) x[a] = xbar[a];
      }
    }
    verts_out[3 * c] = (float)(x[0] + g.lx);
    verts_out[3 * c + 1] = (float)(x[1] + g.ly);
    verts_out[3 * c + 2] = (float)(x[2] + g.lz);
    if (normals_out) {
      const double len = sqrt(s[13] * s[13] + s[14] * s[14] + s[15] * s[15]);
      const bool ok = len > 0.0 && len < INFINITY;
      normals_out[3 * c] = ok ? (float)(s[13] / len) : 0.0f;
      normals_out[3 * c + 1] = ok ? (float)(s[14] / len) : 0.0f;
      normals_out[3 * c + 2] = ok ? (float)(s[15] / len) : 1.0f;
    }
    if (colours_out) {
#pragma unroll
      for (int a = 0; a < 3; ++a) colours_out[3 * c + a] = (uint8_t)fmin(fmax(rint(s[16 + a] / cnt), 0.0), 255.0);
    }
  }
}

int grid_of(int64_t n, int per_block = kThreads) {
  const int64_t b = (n + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : b < kMaxGrid ? b : kMaxGrid);
}

bool make_grid(double lx, double ly, double lz, double h, Grid& g) {
  g = Grid{lx, ly, lz, h};
  return lx == lx && ly == ly && lz == lz && h > 0.0 && h < (double)INFINITY && lx - lx == 0.0 && ly - ly == 0.0 && lz - lz == 0.0;
}

}  // namespace

#define NSKY_MESH_GRID(name)                                                                                                       \
  Grid g;                                                                                                                          \
  NSKY_CHECK_ARG(make_grid(lo_x, lo_y, lo_z, h, g), name ": origin (%g, %g, %g) must be finite and the cell edge %g positive", lo_x, \
                 lo_y, lo_z, h)

extern "C" int nsky_mesh_cell_keys(const float* vertices, int64_t V, double lo_x, double lo_y, double lo_z, double h, int64_t* keys,
                                   nsky_stream_t stream) {
  NSKY_MESH_GRID("nsky_mesh_cell_keys");
  NSKY_CHECK_ARG(V >= 0 && V <= INT32_MAX, "nsky_mesh_cell_keys: V %ld", (long)V);
  if (V == 0) return NSKY_OK;
  NSKY_CHECK_ARG(vertices && keys, "nsky_mesh_cell_keys: NULL vertices / keys");
  hipLaunchKernelGGL(cell_keys_kernel, dim3(grid_of(V)), dim3(kThreads), 0, (hipStream_t)stream, vertices, V, g, keys);
  NSKY_CHECK_LAUNCH("nsky_mesh_cell_keys");
  return NSKY_OK;
}

extern "C" int nsky_mesh_cluster_count(const float* vertices, int64_t V, const int32_t* faces, int64_t F, double lo_x, double lo_y,
                                       double lo_z, double h, int64_t* count, nsky_stream_t stream) {
  NSKY_MESH_GRID("nsky_mesh_cluster_count");
  NSKY_CHECK_ARG(V >= 0 && V <= INT32_MAX && F >= 0 && F <= INT32_MAX, "nsky_mesh_cluster_count: V %ld F %ld", (long)V, (long)F);
  NSKY_CHECK_ARG(count, "nsky_mesh_cluster_count: count is NULL");
  if (F == 0 || V == 0) return NSKY_OK;
  NSKY_CHECK_ARG(vertices && faces, "nsky_mesh_cluster_count: NULL vertices / faces");
  hipLaunchKernelGGL(cluster_count_kernel, dim3(grid_of(F)), dim3(kThreads), 0, (hipStream_t)stream, vertices, V, faces, F, g,
                     (unsigned long long*)count);
  NSKY_CHECK_LAUNCH("nsky_mesh_cluster_count");
  return NSKY_OK;
}

extern "C" int nsky_mesh_vertex_cells(const int64_t* vertex_order, const int64_t* rank_sorted, int64_t V, int32_t* vertex_cell,
                                      nsky_stream_t stream) {
  NSKY_CHECK_ARG(V >= 0 && V <= INT32_MAX, "nsky_mesh_vertex_cells: V %ld", (long)V);
  if (V == 0) return NSKY_OK;
  NSKY_CHECK_ARG(vertex_order && rank_sorted && vertex_cell, "nsky_mesh_vertex_cells: NULL argument");
  hipLaunchKernelGGL(vertex_cells_kernel, dim3(grid_of(V)), dim3(kThreads), 0, (hipStream_t)stream, vertex_order, rank_sorted, V, vertex_cell);
  NSKY_CHECK_LAUNCH("nsky_mesh_vertex_cells");
  return NSKY_OK;
}

extern "C" int nsky_mesh_remap_faces(const int32_t* faces, int64_t F, const int32_t* vertex_cell, int64_t V, int32_t* corner_cells,
                                     int64_t* face_keys, nsky_stream_t stream) {
  NSKY_CHECK_ARG(V >= 0 && V <= INT32_MAX && F >= 0 && F <= INT32_MAX, "nsky_mesh_remap_faces: V %ld F %ld", (long)V, (long)F);
  if (F == 0) return NSKY_OK;
  NSKY_CHECK_ARG(faces && vertex_cell && corner_cells && face_keys, "nsky_mesh_remap_faces: NULL argument");
  hipLaunchKernelGGL(remap_faces_kernel, dim3(grid_of(F)), dim3(kThreads), 0, (hipStream_t)stream, faces, F, vertex_cell, V, corner_cells,
                     face_keys);
  NSKY_CHECK_LAUNCH("nsky_mesh_remap_faces");
  return NSKY_OK;
}

extern "C" int nsky_mesh_cluster_reduce(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* normals,
                                        const uint8_t* colours, double lo_x, double lo_y, double lo_z, double h, const int64_t* vertex_order,
                                        const int64_t* cell_start, int64_t C, const int32_t* sorted_corner_cells, const int64_t* corner_order,
                                        int32_t group, double* cell_sums, nsky_stream_t stream) {
  NSKY_MESH_GRID("nsky_mesh_cluster_reduce");
  NSKY_CHECK_ARG(V >= 0 && V <= INT32_MAX && F >= 0 && F <= INT32_MAX && C >= 0 && C <= V, "nsky_mesh_cluster_reduce: V %ld F %ld C %ld", (long)V,
                 (long)F, (long)C);
  NSKY_CHECK_ARG(group == 0 || group == 8 || group == 64, "nsky_mesh_cluster_reduce: group %d (0 = by the mean cell size, 8 or 64)", group);
  if (C == 0) return NSKY_OK;
  NSKY_CHECK_ARG(vertices && vertex_order && cell_start && cell_sums, "nsky_mesh_cluster_reduce: NULL argument");
  NSKY_CHECK_ARG(F == 0 || (faces && sorted_corner_cells && corner_order), "nsky_mesh_cluster_reduce: NULL faces / corner records");
  if (group == 0) group = (3 * F + V) / C > NSKY_MESH_WIDE_GROUP_RECORDS ? 64 : 8;
  hipStream_t s = (hipStream_t)stream;
  if (group == 8)
    hipLaunchKernelGGL(cluster_reduce_kernel<8>, dim3(grid_of(C, kThreads / 8)), dim3(kThreads), 0, s, vertices, V, faces, F, normals, colours, g,
                       vertex_order, cell_start, C, sorted_corner_cells, corner_order, cell_sums);
  else
    hipLaunchKernelGGL(cluster_reduce_kernel<64>, dim3(grid_of(C, kThreads / 64)), dim3(kThreads), 0, s, vertices, V, faces, F, normals, colours,
                       g, vertex_order, cell_start, C, sorted_corner_cells, corner_order, cell_sums);
  NSKY_CHECK_LAUNCH("nsky_mesh_cluster_reduce");
  return NSKY_OK;
}

extern "C" int nsky_mesh_cluster_solve(const double* cell_sums, const int64_t* cell_keys, int64_t C, double lo_x, double lo_y, double lo_z,
                                       double h, float* vertices_out, float* normals_out, uint8_t* colours_out, nsky_stream_t stream) {
  NSKY_MESH_GRID("nsky_mesh_cluster_solve");
  NSKY_CHECK_ARG(C >= 0 && C <= INT32_MAX, "nsky_mesh_cluster_solve: C %ld", (long)C);
  if (C == 0) return NSKY_OK;
  NSKY_CHECK_ARG(cell_sums && cell_keys && vertices_out, "nsky_mesh_cluster_solve: NULL argument");
  hipLaunchKernelGGL(cluster_solve_kernel, dim3(grid_of(C)), dim3(kThreads), 0, (hipStream_t)stream, cell_sums, cell_keys, C, g, vertices_out,
                     normals_out, colours_out);
  NSKY_CHECK_LAUNCH("nsky_mesh_cluster_solve");
  return NSKY_OK;
}

extern "C" int nsky_mesh_flag_duplicates(const int32_t* corner_cells, int64_t F, const int64_t* sorted_keys, const int64_t* face_order,
                                         int32_t* keep, nsky_stream_t stream) {
  NSKY_CHECK_ARG(F >= 0 && F <= INT32_MAX, "nsky_mesh_flag_duplicates: F %ld", (long)F);
  if (F == 0) return NSKY_OK;
  NSKY_CHECK_ARG(corner_cells && sorted_keys && face_order && keep, "nsky_mesh_flag_duplicates: NULL argument");
  hipLaunchKernelGGL(flag_duplicates_kernel, dim3(grid_of(F)), dim3(kThreads), 0, (hipStream_t)stream, corner_cells, F, sorted_keys, face_order,
                     keep);
  NSKY_CHECK_LAUNCH("nsky_mesh_flag_duplicates");
  return NSKY_OK;
}

extern "C" int nsky_mesh_compact_faces(const int32_t* corner_cells, int64_t F, const int32_t* keep, const int64_t* ends, int64_t F_out,
                                       int32_t* faces_out, nsky_stream_t stream) {
  NSKY_CHECK_ARG(F >= 0 && F <= INT32_MAX && F_out >= 0 && F_out <= F, "nsky_mesh_compact_faces: F %ld F_out %ld", (long)F, (long)F_out);
  if (F == 0 || F_out == 0) return NSKY_OK;
  NSKY_CHECK_ARG(corner_cells && keep && ends && faces_out, "nsky_mesh_compact_faces: NULL argument");
  hipLaunchKernelGGL(compact_faces_kernel, dim3(grid_of(F)), dim3(kThreads), 0, (hipStream_t)stream, corner_cells, F, keep, ends, F_out,
                     faces_out);
  NSKY_CHECK_LAUNCH("nsky_mesh_compact_faces");
  return NSKY_OK;
}
