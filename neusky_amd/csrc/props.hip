// Solid props placed in a frame (neusky_amd/relight/props.py).  Definitions and rules: include/neusky_hip.h.
//
// A prop is a sphere or a yawed box.  It enters a frame through two seams and no shading kernel knows of it:
//   intersect  one thread per camera ray, the block [P][16] staged once per workgroup in LDS: the nearest visible prop the ray enters.
//   insert     one wave per ray: the ray's S samples copied into S + 1, those behind the hit without their weight, and the hit as sample
//              S with the transmittance left in front of it.  The sum of the weights in front is fp64 in sample order: every lane adds
//              the 64 masked weights of a tile lane by lane, so all lanes hold the same sum and no LDS is needed.
//   occlude    one thread per entry (m, n) of a visibility tensor, the block in LDS (all lanes read one prop: a broadcast, no bank
//              conflict), the flat index split so that consecutive threads walk the tensor's fast stride.  The frame's shapes at
//              R = 4096 decide the form: [R, D] has 2^20 entries, but [K, R] and [L, R] with K = L = 1 have one direction per point, and
//              a wave per point walking N directions would then keep one lane of 64 busy.  An entry that is not occluded is neither
//              read nor written.  The start point's lift is formed again by each of the N threads of a point: one square root and three
//              divisions beside the P interval tests.
// Every interval is formed in fp64 from the fp32 inputs without fused multiply-adds (a float64 restatement rounds where this does).
// No atomics, no reduction across threads: two runs agree bit for bit.  Flat indices are 64-bit.  Nothing here synchronises with the host.
#include "common.h"
#include "../../include/neusky_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPropStride = NSKY_PROP_FLOATS;
enum { Q_KIND = 0, Q_C = 1, Q_H = 4, Q_COS = 7, Q_SIN = 8, Q_ALBEDO = 9, Q_VISIBLE = 12, Q_CASTS = 13 };

static inline unsigned prop_grid(int64_t threads) { return capped_grid((threads + 255) / 256, 8); }

// the block into LDS: P kPropStride floats, P <= NSKY_MAX_PROPS
__device__ __forceinline__ void stage_props(const float* __restrict__ props, int P, float* __restrict__ lds) {
  for (int i = threadIdx.x; i < P * kPropStride; i += blockDim.x) lds[i] = props[i];
  __syncthreads();
}

struct Interval {
  double t_in, t_out;
  int axis;  // a box's entry axis
};

// the interval of the line o + t d inside prop q (oc = o - c), or false
__device__ __forceinline__ bool prop_interval(const float* __restrict__ q, double ox, double oy, double oz, double dx, double dy, double dz,
                                              Interval& iv) {
  const double ocx = ox - (double)q[Q_C], ocy = oy - (double)q[Q_C + 1], ocz = oz - (double)q[Q_C + 2];
  if (q[Q_KIND] == 0.0f) {
    const double r = q[Q_H];
    const double a = dx * dx + dy * dy + dz * dz;
    const double b = ocx * dx + ocy * dy + ocz * dz;
    const double c = ocx * ocx + ocy * ocy + ocz * ocz - r * r;
    const double disc = b * b - a * c;
    if (!(disc > 0.0)) return false;
    const double s = sqrt(disc);
    iv.t_in = (-b - s) / a;
    iv.t_out = (-b + s) / a;
    iv.axis = -1;
    return true;
  }
  const double cy = q[Q_COS], sy = q[Q_SIN];
  const double o[3] = {cy * ocx + sy * ocy, cy * ocy - sy * ocx, ocz};
  const double d[3] = {cy * dx + sy * dy, cy * dy - sy * dx, dz};
  double t_in = -(double)INFINITY, t_out = (double)INFINITY;
  int axis = -1;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double h = q[Q_H + i];
    if (d[i] != 0.0) {
      const double t0 = (-h - o[i]) / d[i], t1 = (h - o[i]) / d[i];
      const double lo = fmin(t0, t1), hi = fmax(t0, t1);
      if (lo > t_in) t_in = lo, axis = i;
      if (hi < t_out) t_out = hi;
    } else if (!(fabs(o[i]) < h)) {
      return false;
    }
  }
  if (!(t_in < t_out)) return false;
  iv.t_in = t_in, iv.t_out = t_out, iv.axis = axis;
  return true;
}

__global__ __launch_bounds__(256) void props_intersect_kernel(const float* __restrict__ origins, const float* __restrict__ directions,
                                                              const float* __restrict__ props, int64_t R, int P, float* __restrict__ t_hit,
                                                              int32_t* __restrict__ id, float* __restrict__ normal,
                                                              float* __restrict__ albedo) {
  __shared__ float lds[NSKY_MAX_PROPS * kPropStride];
  stage_props(props, P, lds);
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
    const double ox = origins[r * 3], oy = origins[r * 3 + 1], oz = origins[r * 3 + 2];
    const double dx = directions[r * 3], dy = directions[r * 3 + 1], dz = directions[r * 3 + 2];
    double best = (double)INFINITY;
    int who = -1, axis = -1;
    for (int p = 0; p < P; ++p) {
      const float* q = lds + p * kPropStride;
      if (q[Q_VISIBLE] == 0.0f) continue;
      Interval iv;
      if (prop_interval(q, ox, oy, oz, dx, dy, dz, iv) && iv.t_in > 0.0 && iv.t_in < best) best = iv.t_in, who = p, axis = iv.axis;
    }
    float n[3] = {0.0f, 0.0f, 0.0f}, a[3] = {0.0f, 0.0f, 0.0f};
    if (who >= 0) {
      const float* q = lds + who * kPropStride;
      if (q[Q_KIND] == 0.0f) {
        const double rad = q[Q_H];
        const double vx = (ox - (double)q[Q_C] + best * dx) / rad, vy = (oy - (double)q[Q_C + 1] + best * dy) / rad,
                     vz = (oz - (double)q[Q_C + 2] + best * dz) / rad;
        const double len = sqrt(vx * vx + vy * vy + vz * vz);
        n[0] = (float)(vx / len), n[1] = (float)(vy / len), n[2] = (float)(vz / len);
      } else {
        const float cy = q[Q_COS], sy = q[Q_SIN];
        const double dl[3] = {(double)cy * dx + (double)sy * dy, (double)cy * dy - (double)sy * dx, dz};
        const float sign = dl[axis] > 0.0 ? -1.0f : 1.0f;  // against the direction, in the box's frame
        if (axis == 0) n[0] = sign * cy, n[1] = sign * sy;
        else if (axis == 1) n[0] = -sign * sy, n[1] = sign * cy;
        else n[2] = sign;
      }
      a[0] = q[Q_ALBEDO], a[1] = q[Q_ALBEDO + 1], a[2] = q[Q_ALBEDO + 2];
    }
    t_hit[r] = (float)best;
    id[r] = who;
#pragma unroll
    for (int c = 0; c < 3; ++c) normal[r * 3 + c] = n[c], albedo[r * 3 + c] = a[c];
  }
}

// one wave per ray; blocks of 4 waves
__global__ __launch_bounds__(256) void props_insert_kernel(const float* __restrict__ weights, const float* __restrict__ starts,
                                                           const float* __restrict__ ends, const float* __restrict__ albedo,
                                                           const float* __restrict__ normals, const float* __restrict__ t_hit,
                                                           const int32_t* __restrict__ id, const float* __restrict__ hit_normal,
                                                           const float* __restrict__ hit_albedo, int64_t R, int S,
                                                           float* __restrict__ weights_out, float* __restrict__ starts_out,
                                                           float* __restrict__ ends_out, float* __restrict__ albedo_out,
                                                           float* __restrict__ normals_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < R; r += (int64_t)gridDim.x * 4) {
    const int64_t in = r * S, out = r * ((int64_t)S + 1);
    const float t = t_hit[r];
    const bool entered = id[r] >= 0;
    double sum = 0.0;
    for (int s0 = 0; s0 < S; s0 += 64) {  // (uniform per wave)
      const int s = s0 + lane;
      float w = 0.0f;
      if (s < S) {
        const float a = starts[in + s], b = ends[in + s];
        w = (a + b) / 2.0f < t ? weights[in + s] : 0.0f;
        weights_out[out + s] = w, starts_out[out + s] = a, ends_out[out + s] = b;
      }
#pragma unroll
      for (int j = 0; j < 64; ++j) sum += (double)__shfl(w, j);  // sample order; a lane past S adds +0
    }
    for (int j = lane; j < S * 3; j += 64) albedo_out[out * 3 + j] = albedo[in * 3 + j], normals_out[out * 3 + j] = normals[in * 3 + j];
    if (lane < 3) {
      albedo_out[(out + S) * 3 + lane] = entered ? hit_albedo[r * 3 + lane] : 0.0f;
      normals_out[(out + S) * 3 + lane] = entered ? hit_normal[r * 3 + lane] : 0.0f;
    }
    if (lane == 0) {
      const float at = entered ? t : ends[in + S - 1];
      weights_out[out + S] = entered ? (float)fmin(fmax(1.0 - sum, 0.0), 1.0) : 0.0f;
      starts_out[out + S] = at, ends_out[out + S] = at;
    }
  }
}

// entry i of M N: consecutive threads along the tensor's fast stride.  lamps: `towards` holds lamp positions and `clearance` their
// clearances; otherwise directions towards lights at infinity
__global__ __launch_bounds__(256) void props_occlude_kernel(const float* __restrict__ x, const float* __restrict__ normals,
                                                            const float* __restrict__ towards, const float* __restrict__ clearance,
                                                            const float* __restrict__ bias, const float* __restrict__ props, int64_t M,
                                                            int64_t N, int P, float* __restrict__ vis, int64_t stride_m, int64_t stride_n) {
  __shared__ float lds[NSKY_MAX_PROPS * kPropStride];
  stage_props(props, P, lds);
  const int64_t T = M * N;
  const bool n_fast = stride_n <= stride_m;
  const double lift = bias[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
    const int64_t m = n_fast ? i / N : i % M, n = n_fast ? i % N : i / M;
    double ox = x[m * 3], oy = x[m * 3 + 1], oz = x[m * 3 + 2];
    if (normals) {
      const double nx = normals[m * 3], ny = normals[m * 3 + 1], nz = normals[m * 3 + 2];
      const double nn = nx * nx + ny * ny + nz * nz;
      if (nn > 0.0 && nn < (double)INFINITY) {
        const double len = sqrt(nn);
        ox = ox + lift * (nx / len), oy = oy + lift * (ny / len), oz = oz + lift * (nz / len);
      }
    }
    double dx = towards[n * 3], dy = towards[n * 3 + 1], dz = towards[n * 3 + 2];
    double t_max = (double)INFINITY;
    if (clearance) {
      dx = dx - ox, dy = dy - oy, dz = dz - oz;
      const double len = sqrt(dx * dx + dy * dy + dz * dz);
      if (!(len > 0.0)) continue;  // the point is at its lamp: no direction, nothing between them
      dx = dx / len, dy = dy / len, dz = dz / len;
      t_max = len - (double)clearance[n];
    }
    bool occluded = false;
    for (int p = 0; p < P && !occluded; ++p) {
      const float* q = lds + p * kPropStride;
      if (q[Q_CASTS] == 0.0f) continue;
      Interval iv;
      occluded = prop_interval(q, ox, oy, oz, dx, dy, dz, iv) && iv.t_out > 0.0 && iv.t_in < t_max;
    }
    if (occluded) {
      float* v = vis + m * stride_m + n * stride_n;
      *v = *v * 0.0f;
    }
  }
}

}  // namespace

extern "C" int nsky_props_intersect(const float* origins, const float* directions, const float* props, int64_t R, int32_t P, float* t_hit,
                                    int32_t* id, float* normal, float* albedo, nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && P >= 1 && P <= NSKY_MAX_PROPS, "nsky_props_intersect: R %ld, P %d (1..%d)", (long)R, (int)P, NSKY_MAX_PROPS);
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(origins && directions && props && t_hit && id && normal && albedo,
                 "nsky_props_intersect: NULL origins / directions / props / t_hit / id / normal / albedo");
  hipLaunchKernelGGL(props_intersect_kernel, dim3(prop_grid(R)), dim3(256), 0, (hipStream_t)stream, origins, directions, props, R, (int)P, t_hit,
                     id, normal, albedo);
  NSKY_CHECK_LAUNCH("nsky_props_intersect");
  return NSKY_OK;
}

extern "C" int nsky_props_insert(const float* weights, const float* starts, const float* ends, const float* albedo, const float* normals,
                                 const float* t_hit, const int32_t* id, const float* hit_normal, const float* hit_albedo, int64_t R, int32_t S,
                                 float* weights_out, float* starts_out, float* ends_out, float* albedo_out, float* normals_out,
                                 nsky_stream_t stream) {
  NSKY_CHECK_ARG(R >= 0 && S >= 1, "nsky_props_insert: R %ld, S %d", (long)R, (int)S);
  if (R == 0) return NSKY_OK;
  NSKY_CHECK_ARG(weights && starts && ends && albedo && normals && t_hit && id && hit_normal && hit_albedo,
                 "nsky_props_insert: NULL weights / starts / ends / albedo / normals / t_hit / id / hit_normal / hit_albedo");
  NSKY_CHECK_ARG(weights_out && starts_out && ends_out && albedo_out && normals_out, "nsky_props_insert: NULL output");
  hipLaunchKernelGGL(props_insert_kernel, dim3(capped_grid((R + 3) / 4, 8)), dim3(256), 0, (hipStream_t)stream, weights, starts, ends, albedo,
                     normals, t_hit, id, hit_normal, hit_albedo, R, (int)S, weights_out, starts_out, ends_out, albedo_out, normals_out);
  NSKY_CHECK_LAUNCH("nsky_props_insert");
  return NSKY_OK;
}

extern "C" int nsky_props_occlude(const float* x, const float* normals, const float* directions, const float* targets, const float* clearance,
                                  const float* bias, const float* props, int64_t M, int64_t N, int32_t P, float* vis, int64_t stride_m,
                                  int64_t stride_n, nsky_stream_t stream) {
  NSKY_CHECK_ARG(M >= 0 && N >= 0 && P >= 1 && P <= NSKY_MAX_PROPS && stride_m >= 0 && stride_n >= 0,
                 "nsky_props_occlude: M %ld, N %ld, P %d (1..%d), strides %ld, %ld", (long)M, (long)N, (int)P, NSKY_MAX_PROPS, (long)stride_m,
                 (long)stride_n);
  if (M == 0 || N == 0) return NSKY_OK;
  NSKY_CHECK_ARG((directions != nullptr) != (targets != nullptr) && (targets != nullptr) == (clearance != nullptr),
                 "nsky_props_occlude: either directions, or targets with their clearances");
  NSKY_CHECK_ARG(x && bias && props && vis, "nsky_props_occlude: NULL x / bias / props / vis");
  hipLaunchKernelGGL(props_occlude_kernel, dim3(prop_grid(M * N)), dim3(256), 0, (hipStream_t)stream, x, normals,
                     directions ? directions : targets, clearance, bias, props, M, N, (int)P, vis, stride_m, stride_n);
  NSKY_CHECK_LAUNCH("nsky_props_occlude");
  return NSKY_OK;
}
