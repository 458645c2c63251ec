// Connected components of a triangle mesh and the removal of small ones ("floaters"): the exporter's step between marching cubes and
// simplification (neusky_amd/exporter/components.py).  Definitions: include/neusky_hip.h (nsky_cc_*).
//
//   link      one pass over the faces: a lock-free union-find over parent[V] (smaller index wins, so parent[x] <= x always)
//   flatten   vertex_root[V] and face_root[F] by read-only finds, in a launch of its own
//   select    keep[F] from the faces' component ranks and a per-component flag; marks the vertices that kept faces use
//   compact   kept vertices (with their attributes) and kept faces, re-indexed, to their scanned slots
//
// Inside link every access to parent is an agent-scope relaxed atomic: the eight L2s do not see each other's plain stores.  Nothing
// in link depends on a load being fresh: a stale parent value is an ancestor in an older forest (same component, an index no smaller
// than today's), and the hook is a compare-and-swap on a root, decided at the memory side.  Every loop descends strictly, no thread
// waits for another, and every loop is capped by the bound that argument gives: a thread that reaches the cap (a broken invariant:
// parent not the identity on entry, or a defect here) sets *status and leaves.
#include "common.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGrid = 1 << 16;

#define CC_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ bool in_range(int32_t a, int32_t b, int32_t c, int64_t V) {
  return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
}

__device__ __forceinline__ void fail(int32_t* status, int32_t what) {
  __hip_atomic_fetch_or(status, what, CC_RELAXED);
}

// parent[x] of a node x in [0, V): in [0, x] while the invariant holds.  Anything else would send the next access out of bounds.
__device__ __forceinline__ bool load_parent(int32_t* parent, int32_t x, int32_t& p) {
  p = __hip_atomic_load(parent + x, CC_RELAXED);
  return p >= 0 && p <= x;
}

// A root candidate of x, halving the path on the way: prev -> curr -> next becomes prev -> next (an ancestor of prev in whichever
// forest the two loads saw; only a pointer of a non-root moves, and a non-root never becomes a root again).  The walk descends
// strictly, so it takes fewer than V steps.
__device__ __forceinline__ bool find_halving(int32_t* parent, int32_t x, int64_t cap, int32_t& root) {
  int32_t prev = x, curr, next;
  if (!load_parent(parent, prev, curr)) return false;
  for (int64_t it = 0; it < cap; ++it) {
    if (!load_parent(parent, curr, next)) return false;
    if (next == curr) {
      root = curr;
      return true;
    }
    __hip_atomic_store(parent + prev, next, CC_RELAXED);
    prev = curr;
    curr = next;
  }
  return false;
}

// ECL-CC's hook: the larger of two root candidates is linked below the smaller by a compare-and-swap that succeeds only on a root.  A
// failed compare-and-swap returns what memory holds, which is smaller than the node it was tried on: the walk continues from that
// value, with no re-read.  One of the two candidates falls in every round, so there are at most ra + rb < 2 V rounds.
__device__ __forceinline__ bool link(int32_t* parent, int32_t a, int32_t b, int64_t V) {
  int32_t ra, rb;
  if (!find_halving(parent, a, V, ra) || !find_halving(parent, b, V, rb)) return false;
  for (int64_t it = 0; it < 2 * V; ++it) {
    if (ra == rb) return true;
    const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    int32_t old = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &old, lo, __ATOMIC_RELAXED, CC_RELAXED)) return true;
    if (old < 0 || old >= hi) return false;
    ra = old;
    rb = lo;
  }
  return ra == rb;
}

__global__ __launch_bounds__(kThreads) void link_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V, int32_t* parent,
                                                         int32_t* status) {
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += (int64_t)gridDim.x * kThreads) {
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!in_range(a, b, c, V)) {
      fail(status, NSKY_CC_STATUS_INDEX);
      continue;
    }
    if (!link(parent, a, b, V) || !link(parent, b, c, V)) {
      fail(status, NSKY_CC_STATUS_LINK);
      return;
    }
  }
}

// The link launch is complete and visible here, and nothing writes parent any more: plain loads.
__device__ __forceinline__ int32_t find_readonly(const int32_t* __restrict__ parent, int32_t x, int64_t cap) {
  for (int64_t it = 0; it <= cap; ++it) {
    const int32_t p = parent[x];
    if (p == x) return x;
    if (p < 0 || p > x) return -1;
    x = p;
  }
  return -1;
}

__global__ __launch_bounds__(kThreads) void flatten_kernel(const int32_t* __restrict__ parent, int64_t V, const int32_t* __restrict__ faces,
                                                            int64_t F, int32_t* __restrict__ vertex_root, int32_t* __restrict__ face_root,
                                                            int32_t* status) {
  const int64_t start = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  for (int64_t v = start; v < V; v += step) {
    const int32_t r = find_readonly(parent, (int32_t)v, V);
    if (r < 0) fail(status, NSKY_CC_STATUS_FLATTEN);
    vertex_root[v] = r < 0 ? (int32_t)v : r;
  }
  for (int64_t f = start; f < F; f += step) {
    const int32_t a = faces[3 * f];
    int32_t r = -1;
    if (a >= 0 && a < V) {
      r = find_readonly(parent, a, V);
      if (r < 0) fail(status, NSKY_CC_STATUS_FLATTEN);
    } else {
      fail(status, NSKY_CC_STATUS_INDEX);
    }
    face_root[f] = r < 0 ? 0 : r;
  }
}

__global__ __launch_bounds__(kThreads) void select_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V,
                                                           const int32_t* __restrict__ face_labels,
                                                           const uint8_t* __restrict__ keep_component, int64_t C,
                                                           uint8_t* __restrict__ keep, uint8_t* vertex_used) {
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += (int64_t)gridDim.x * kThreads) {
    const int32_t l = face_labels[f];
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const bool k = l >= 0 && l < C && keep_component[l] != 0 && in_range(a, b, c, V);
    keep[f] = k ? 1 : 0;
    if (k) {  // every writer stores the same byte: the race has one outcome
      vertex_used[a] = 1;
      vertex_used[b] = 1;
      vertex_used[c] = 1;
    }
  }
}

__global__ __launch_bounds__(kThreads) void compact_kernel(const float* __restrict__ verts, const float* __restrict__ normals,
                                                            const uint8_t* __restrict__ colours, int64_t V,
                                                            const int32_t* __restrict__ faces, int64_t F, const uint8_t* __restrict__ keep,
                                                            const int64_t* __restrict__ face_ends, const uint8_t* __restrict__ vertex_used,
                                                            const int64_t* __restrict__ vertex_ends, int64_t V_out, int64_t F_out,
                                                            float* __restrict__ verts_out, float* __restrict__ normals_out,
                                                            uint8_t* __restrict__ colours_out, int32_t* __restrict__ faces_out) {
  const int64_t start = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  for (int64_t v = start; v < V; v += step) {
    if (!vertex_used[v]) continue;
    const int64_t o = vertex_ends[v] - 1;
    if (o < 0 || o >= V_out) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      verts_out[3 * o + a] = verts[3 * v + a];
      if (normals) normals_out[3 * o + a] = normals[3 * v + a];
      if (colours) colours_out[3 * o + a] = colours[3 * v + a];
    }
  }
  for (int64_t f = start; f < F; f += step) {
    if (!keep[f]) continue;
    const int64_t o = face_ends[f] - 1;
    if (o < 0 || o >= F_out) continue;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!in_range(a, b, c, V)) continue;
    faces_out[3 * o] = (int32_t)(vertex_ends[a] - 1);
    faces_out[3 * o + 1] = (int32_t)(vertex_ends[b] - 1);
    faces_out[3 * o + 2] = (int32_t)(vertex_ends[c] - 1);
  }
}

int grid_of(int64_t n) {
  const int64_t b = (n + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : b < kMaxGrid ? b : kMaxGrid);
}

}  // namespace

extern "C" int nsky_cc_link(const int32_t* faces, int64_t F, int64_t V, int32_t* parent, int32_t* status, nsky_stream_t stream) {
  NSKY_CHECK_ARG(V >= 0 && V <= INT32_MAX && F >= 0 && F <= INT32_MAX, "nsky_cc_link: V %ld F %ld", (long)V, (long)F);
  if (F == 0 || V == 0) return NSKY_OK;
  NSKY_CHECK_ARG(faces && parent && status, "nsky_cc_link: NULL argument");
  hipLaunchKernelGGL(link_kernel, dim3(grid_of(F)), dim3(kThreads), 0, (hipStream_t)stream, faces, F, V, parent, status);
  NSKY_CHECK_LAUNCH("nsky_cc_link");
  return NSKY_OK;
}

extern "C" int nsky_cc_flatten(const int32_t* parent, int64_t V, const int32_t* faces, int64_t F, int32_t* vertex_root, int32_t* face_root,
                               int32_t* status, nsky_stream_t stream) {
  NSKY_CHECK_ARG(V >= 0 && V <= INT32_MAX && F >= 0 && F <= INT32_MAX, "nsky_cc_flatten: V %ld F %ld", (long)V, (long)F);
  NSKY_CHECK_ARG(V > 0 || F == 0, "nsky_cc_flatten: %ld faces without a vertex", (long)F);
  if (V == 0) return NSKY_OK;
  NSKY_CHECK_ARG(parent && vertex_root && status && (F == 0 || (faces && face_root)), "nsky_cc_flatten: NULL argument");
  hipLaunchKernelGGL(flatten_kernel, dim3(grid_of(V > F ? V : F)), dim3(kThreads), 0, (hipStream_t)stream, parent, V, faces, F, vertex_root,
                     face_root, status);
  NSKY_CHECK_LAUNCH("nsky_cc_flatten");
  return NSKY_OK;
}

extern "C" int nsky_cc_select(const int32_t* faces, int64_t F, int64_t V, const int32_t* face_labels, const uint8_t* keep_component, int64_t C,
                              uint8_t* keep, uint8_t* vertex_used, nsky_stream_t stream) {
  NSKY_CHECK_ARG(V >= 0 && V <= INT32_MAX && F >= 0 && F <= INT32_MAX && C >= 0 && C <= F, "nsky_cc_select: V %ld F %ld C %ld", (long)V,
                 (long)F, (long)C);
  if (F == 0) return NSKY_OK;
  NSKY_CHECK_ARG(faces && face_labels && keep_component && keep && vertex_used, "nsky_cc_select: NULL argument");
  hipLaunchKernelGGL(select_kernel, dim3(grid_of(F)), dim3(kThreads), 0, (hipStream_t)stream, faces, F, V, face_labels, keep_component, C, keep,
                     vertex_used);
  NSKY_CHECK_LAUNCH("nsky_cc_select");
  return NSKY_OK;
}

extern "C" int nsky_cc_compact(const float* vertices, const float* normals, const uint8_t* colours, int64_t V, const int32_t* faces, int64_t F,
                               const uint8_t* keep, const int64_t* face_ends, const uint8_t* vertex_used, const int64_t* vertex_ends,
                               int64_t V_out, int64_t F_out, float* vertices_out, float* normals_out, uint8_t* colours_out,
                               int32_t* faces_out, nsky_stream_t stream) {
  NSKY_CHECK_ARG(V >= 0 && V <= INT32_MAX && F >= 0 && F <= INT32_MAX && V_out >= 0 && V_out <= V && F_out >= 0 && F_out <= F,
                 "nsky_cc_compact: V %ld F %ld V_out %ld F_out %ld", (long)V, (long)F, (long)V_out, (long)F_out);
  if (V == 0 || V_out == 0) return NSKY_OK;
  NSKY_CHECK_ARG(vertices && vertex_used && vertex_ends && vertices_out, "nsky_cc_compact: NULL vertices / scan");
  NSKY_CHECK_ARG((!normals || normals_out) && (!colours || colours_out), "nsky_cc_compact: attributes without an output");
  NSKY_CHECK_ARG(F_out == 0 || (faces && keep && face_ends && faces_out), "nsky_cc_compact: NULL faces / scan");
  if (F_out == 0) F = 0;
  hipLaunchKernelGGL(compact_kernel, dim3(grid_of(V > F ? V : F)), dim3(kThreads), 0, (hipStream_t)stream, vertices, normals, colours, V, faces,
                     F, keep, face_ends, vertex_used, vertex_ends, V_out, F_out, vertices_out, normals_out, colours_out, faces_out);
  NSKY_CHECK_LAUNCH("nsky_cc_compact");
  return NSKY_OK;
}
