// Shared machinery of the chain kernels (film_chain.hip: FiLM-SIREN; sdf_chain.hip: the sdf value chain; field_chain.hip: the
// SDF / albedo field): packed weight stream (one tile = 32 output features x K as fp16 hi + residual planes in MFMA-fragment order),
// the LDS ring it is streamed through by global_load_lds_dwordx4 (common.h glds16), the register-resident product and the movers of
// tile-native activations.  The arithmetic itself -- power-of-two scales, the fp16 hi / residual split, the sine / cosine and softplus
// forms, the layout's definition -- is numerics.h, shared with the per-layer kernels.  Everything here is device-inline code in an
// anonymous namespace: each translation unit gets its own copy (so does the host side: device_cus() caches the CU count once per
// translation unit).
#pragma once
#include "numerics.h"
#include "../../include/neusky_hip.h"

namespace {

constexpr int SLAB = 2048;
constexpr int GSLABS = 8;
constexpr int GROUP = SLAB * GSLABS;  // 16 KB
constexpr int RING_GROUPS = 8;
constexpr int RING_BYTES = GROUP * RING_GROUPS;  // 128 KB
constexpr int BIAS_FLOATS = 6144;                // 24 KB: every bias of the network
constexpr int SCALE_FLOATS = 512;                // reciprocal tile scales, stream order
constexpr int MAXL = NSKY_FILM_MAX_LAYERS;
constexpr float Y_SCALE = 16384.0f;              // sine outputs live in [-1, 1]: fixed power-of-two scale
constexpr int PACK_KMAX = 320;

__host__ __device__ inline int ksteps_of(int K) { return (K + 15) / 16; }
__host__ __device__ inline int groups_of(int K) { return (ksteps_of(K) + GSLABS - 1) / GSLABS; }

struct TileDesc {
  const float* W;
  int ld, row0, nrows, K, transposed, k0;
  long group;
  int slab0 = 0;  // first slab inside the group (tiles of K <= 64 may share a group: product_pair)
};

// one block per tile: absmax -> power-of-two scale -> fp16 hi / residual planes in fragment order (tile = blockIdx.x)
__device__ __forceinline__ void pack_tile(const TileDesc& d, unsigned char* __restrict__ stream, float* __restrict__ scales,
                                          float (*w)[PACK_KMAX + 1], float* red) {
  const int tid = threadIdx.x;
  const int Kp = ksteps_of(d.K) * 16;
  float m = 0.0f;
  for (int idx = tid; idx < 32 * Kp; idx += 256) {
    const int r = idx / Kp, k = idx % Kp;
    float v = 0.0f;
    if (r < d.nrows && k < d.K) v = d.transposed ? d.W[(long)(d.k0 + k) * d.ld + d.row0 + r] : d.W[(long)(d.row0 + r) * d.ld + k];
    w[r][k] = v;
    m = fmaxf(m, fabsf(v));
  }
  red[tid] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  m = red[0];
  float inv;
  const float sc = pow2_scale(m, inv);
  if (tid == 0) scales[blockIdx.x] = 1.0f / sc;  // == inv (a power of two); the division is what the pack kernels have always run
  unsigned char* base = stream + d.group * GROUP + (long)d.slab0 * SLAB;
  const int KS = ksteps_of(d.K);
  for (int idx = tid; idx < KS * 64; idx += 256) {
    const int ks = idx >> 6, lane = idx & 63;
    const int r = lane & 31, h = lane >> 5;
    f16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = w[r][16 * ks + 8 * (j >> 2) + 4 * h + (j & 3)] * sc;
      const _Float16 xh = (_Float16)x;
      hi[j] = xh;
      lo[j] = (_Float16)(x - (float)xh);
    }
    *reinterpret_cast<f16x8*>(base + (long)ks * SLAB + lane * 16) = hi;
    *reinterpret_cast<f16x8*>(base + (long)ks * SLAB + 1024 + lane * 16) = lo;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight stream consumer.  Invariant while slabs of group g are being consumed: every piece of groups <= g + 1 has landed and
// all four waves know it (barrier).  Fragment reads run TWO k-steps ahead of the MFMAs (three register buffers, rotated at
// compile time inside a product) and one k-step ahead across a tile boundary, so an LDS round trip (~150-200 cycles under
// load) hides behind 6 MFMAs; the waits are counted (lgkmcnt(2): only the youngest pair may still be in flight; LDS returns
// in order, so a scalar load the compiler slips in can only make the wait stricter).
// Transition g -> g + 1 (after this wave's last fragment of group g has arrived): wait for the wave's own pieces of group g + 2
// (at most RING_GROUPS - 3 younger groups x 4 pieces outstanding; every other vector-memory operation of the wave only makes the
// wait longer), barrier (all pieces of g + 2 landed; nobody reads group g any more), refill the slot of g with group g + 8.
// LDS reads in flight across the barrier belong to group g + 1: never the slot being refilled.
struct WStream {
  const unsigned char* src;  // this lane's source address inside group 0 (stream + wave * 4096 + lane * 16)
  uint32_t dst;              // this wave's destination inside ring slot 0 (lds0 + wave * 4096)
  uint32_t lds_lane;         // lds0 + lane * 16
  int g;                     // group of the slab whose fragments are carried in (ch, cl): slab 0 of the next tile
  f16x8 ch, cl;              // fragments requested ahead of the next product (landed: every product settles them at its end)
  int total, sg;             // WRAP streams (persistent workgroups walk the stream again for every row tile): groups in the
                             // stream, and the source group the next DMA issue reads (wraps to 0 after total - 1)
};

// PW = 1 KB pieces of a 16 KB group this wave moves: 4 with four waves per workgroup, 2 with eight
// WRAP: the stream is walked cyclically: the ring slot follows the running group count, the source wraps
// RG: groups in the LDS ring (a power of two; 8 = 128 KB with one workgroup per CU, 4 = 64 KB with two)
template <int PW = 4, bool WRAP = false, int RG = RING_GROUPS>
__device__ __forceinline__ void ws_issue(WStream& w, int group) {
  const unsigned char* s = w.src + (long)(WRAP ? w.sg : group) * GROUP;
  const uint32_t d = w.dst + (uint32_t)(group & (RG - 1)) * GROUP;
#pragma unroll
  for (int p = 0; p < PW; ++p) {
    glds16(s + p * 1024, d + p * 1024);
  }
  if (WRAP) w.sg = w.sg + 1 == w.total ? 0 : w.sg + 1;
}

// The two fragment registers are read-write operands of BOTH the request and the wait: the compiler sees one value that is
// modified in place, so it neither renames it nor copies it while the LDS read is still in flight (a copy of a register whose
// load has not landed would capture stale data; cdna_hip_programming.md section 5.7 item 1).
__device__ __forceinline__ void frag_read(f16x8& h, f16x8& l, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024" : "+v"(h), "+v"(l) : "v"(addr) : "memory");
}
template <int N>
__device__ __forceinline__ void frag_wait(f16x8& h, f16x8& l) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(h), "+v"(l) : "n"(N) : "memory");
}
// The LAST wait of a product and the hand-over of the landed fragments to the registers that carry them into the next product, as
// ONE statement.  A tied ("+v") operand lets the register allocator satisfy the tie with a copy IN FRONT of the statement when the
// value has to change registers anyway (here it does: three buffers rotate over KS k-steps, the carried pair must end where the
// next product expects buffer 0), and a copy in front of the wait captures whatever the destination of the in-flight ds_read held:
// the field kernels of round 3 were built that way (v_mov_b64 x 4, then s_waitcnt lgkmcnt(0)) and gave one wave a stale first
// k-step of its next tile in about one launch of six (tools/isa_lint.py checks every kernel for the pattern).
// Here the moves are the statement's own, behind the wait; sources and destinations are separate (early-clobber) operands.
__device__ __forceinline__ void frag_settle(f16x8& ch, f16x8& cl, const f16x8& h, const f16x8& l) {
  typedef unsigned long u64x2 __attribute__((ext_vector_type(2)));
  const u64x2 sh = __builtin_bit_cast(u64x2, h), sl = __builtin_bit_cast(u64x2, l);
  unsigned long h0, h1, l0, l1;
  asm volatile("s_waitcnt lgkmcnt(0)\n\tv_mov_b64 %0, %4\n\tv_mov_b64 %1, %5\n\tv_mov_b64 %2, %6\n\tv_mov_b64 %3, %7"
               : "=&v"(h0), "=&v"(h1), "=&v"(l0), "=&v"(l1) : "v"(sh[0]), "v"(sh[1]), "v"(sl[0]), "v"(sl[1]) : "memory");
  ch = __builtin_bit_cast(f16x8, u64x2{h0, h1});
  cl = __builtin_bit_cast(f16x8, u64x2{l0, l1});
}

template <int RG = RING_GROUPS>
__device__ __forceinline__ uint32_t ws_addr(const WStream& w, int group, int slab) {
  return w.lds_lane + (uint32_t)(group & (RG - 1)) * GROUP + slab * SLAB;
}

template <int PW = 4, bool WRAP = false, int RG = RING_GROUPS>
__device__ __forceinline__ void ws_begin(WStream& w, int total_groups) {  // total_groups: read by WRAP streams only
  w.total = total_groups;
  w.sg = 0;
#pragma unroll
  for (int g = 0; g < RG; ++g) ws_issue<PW, WRAP, RG>(w, g);
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(PW * (RG - 2)) : "memory");  // groups 0 and 1 landed
  w.g = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { w.ch[j] = (_Float16)0.0f; w.cl[j] = (_Float16)0.0f; }
  frag_read(w.ch, w.cl, ws_addr<RG>(w, 0, 0));
  frag_wait<0>(w.ch, w.cl);
}

// A kernel's stream from its first DMA issue to its last: ws_open behind the __syncthreads() that publishes the kernel's LDS tables,
// ws_close as its last statement.  ws_open first waits until every memory operation the compiler knows about is done: the DMA pieces
// are hidden from its bookkeeping and counted by hand on the one in-order vector-memory counter, so the counted waits of the stream
// hold only if nothing but pieces (and hidden loads counted with them) is in flight from the first issue on.
// stream: the packed groups; smem: the ring (RG groups, first in the kernel's LDS); total_groups: length of a WRAP stream -- a WRAP
// caller MUST pass it (the default serves the streams that are walked once and never read it; with 0 the source would never wrap).
// DRAINED: the caller vouches that nothing is pending and the wait is left out (film_fwd_kernel: the table copy, its only loads, has
// been consumed by the LDS stores in front of the barrier; with the wait its time fell outside the spread of two parent runs).
template <int PW = 4, bool WRAP = false, int RG = RING_GROUPS, bool DRAINED = false>
__device__ __forceinline__ void ws_open(WStream& w, const unsigned char* stream, unsigned char* smem, int wave, int lane, int total_groups = 0) {
  if (!DRAINED) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  w.src = stream + wave * (PW * 1024) + lane * 16;
  w.dst = (uint32_t)(uintptr_t)smem + wave * (PW * 1024);
  w.lds_lane = (uint32_t)(uintptr_t)smem + lane * 16;
  ws_begin<PW, WRAP, RG>(w, total_groups);
}
__device__ __forceinline__ void ws_close() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the tail groups of the ring are still landing
}

template <int PW = 4, bool WRAP = false, int RG = RING_GROUPS>
__device__ __forceinline__ void ws_transition(WStream& w, int from_group) {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(PW * (RG - 3)) : "memory");
  ws_issue<PW, WRAP, RG>(w, from_group + RG);
}

// what a wave WITHOUT a row tile does in place of a product (the last round of a persistent workgroup): its share of the group
// hand-shakes (counted wait, barrier, DMA pieces of the refill) and nothing else -- the same number of barriers as product<KS>
template <int KS, int PW, bool WRAP, int RG = RING_GROUPS>
__device__ __forceinline__ void product_skip(WStream& w) {
  constexpr int NG = (KS + GSLABS - 1) / GSLABS;
  const int g0 = w.g;
#pragma unroll
  for (int i = 0; i < NG; ++i) ws_transition<PW, WRAP, RG>(w, g0 + i);
  w.g = g0 + NG;
}

// acc += W_tile X over KS k-steps, B planes in registers.  One wave per SIMD issues in order, so everything that is not an
// MFMA is placed in the shadow of one: the LDS requests of k-step ks + NB - 1 (and a group transition: barrier + 4 DMA pieces) right
// behind the first MFMA of k-step ks, the counted wait for the fragments of ks + 1 behind the third.
// NB fragment buffers rotate: reads run NB - 1 k-steps ahead of the MFMAs (NB = 4 where a wave has the registers: the last wait of a
// product, for slab 0 of the next tile, then has had 9 MFMAs to be satisfied instead of 6).
template <int KS, int PW = 4, bool WRAP = false, int RG = RING_GROUPS, int NB = 3>
__device__ __forceinline__ void product(WStream& w, const f16x8 (&bh)[KS], const f16x8 (&bl)[KS], f32x16& acc) {
  constexpr int NG = (KS + GSLABS - 1) / GSLABS;  // groups of this tile; slab index KS stands for slab 0 of the next tile
  constexpr int AHEAD = NB - 1;
  f16x8 fh[NB], fl[NB];
  fh[0] = w.ch;
  fl[0] = w.cl;
#pragma unroll
  for (int b = 1; b < NB; ++b)
#pragma unroll
    for (int j = 0; j < 8; ++j) { fh[b][j] = (_Float16)0.0f; fl[b][j] = (_Float16)0.0f; }
  const int g0 = w.g;
  auto request = [&](int s) {  // s static
    if (s < KS) frag_read(fh[s % NB], fl[s % NB], ws_addr<RG>(w, g0 + s / GSLABS, s % GSLABS));
    else frag_read(fh[s % NB], fl[s % NB], ws_addr<RG>(w, g0 + NG, 0));
  };
#pragma unroll
  for (int s = 1; s < AHEAD; ++s)
    if (s <= KS) request(s);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[ks % NB], bl[ks], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (ks + AHEAD <= KS) request(ks + AHEAD);  // into the buffer of k-step ks - 1, whose MFMAs have been issued
    if ((ks & (GSLABS - 1)) == GSLABS - 1 || ks == KS - 1) ws_transition<PW, WRAP, RG>(w, g0 + ks / GSLABS);
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fl[ks % NB], bh[ks], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[ks % NB], bh[ks], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    // fragments of k-step ks + 1 (slab KS = first slab of the next tile): the younger pairs (slabs ks + 2 .. min(ks + AHEAD, KS)) may
    // still be in flight
    static_assert(AHEAD == 2 || AHEAD == 3, "two or three k-steps of read-ahead");
    if (ks < KS - 1) {  // (ks is a constant after unrolling: one of the two waits survives)
      if (AHEAD == 3 && ks + 3 <= KS) frag_wait<4>(fh[(ks + 1) % NB], fl[(ks + 1) % NB]);
      else frag_wait<2>(fh[(ks + 1) % NB], fl[(ks + 1) % NB]);
    }
  }
  // the last wait (lgkmcnt(0)) and the carry in one statement: nothing is in flight behind it, no load crosses a loop back-edge or
  // a branch join.  (Even when the carried slab sits in buffer 0 -- NB = 4, KS a multiple of 4 -- the register allocator does not
  // keep buffer 0 in the carry's registers and would copy in front of a tied wait: tools/isa_lint.py caught exactly that.)
  frag_settle(w.ch, w.cl, fh[KS % NB], fl[KS % NB]);
  w.g = g0 + NG;
}

// Two tiles of K = 64 (four k-steps each) sharing one group and one set of B planes: slabs 0..3 accumulate into a0, slabs 4..7 into
// a1.  The accumulators are NOT zeroed: the mapping backward's head product adds k-block after k-block into them.
template <int PW = 4, int RG = RING_GROUPS>
__device__ __forceinline__ void product_pair(WStream& w, const f16x8 (&bh)[4], const f16x8 (&bl)[4], f32x16& a0, f32x16& a1) {
  constexpr int KS = 8;
  f16x8 fh[3], fl[3];
  fh[0] = w.ch;
  fl[0] = w.cl;
#pragma unroll
  for (int j = 0; j < 8; ++j) { fh[1][j] = fh[2][j] = fl[1][j] = fl[2][j] = (_Float16)0.0f; }
  const int g0 = w.g;
  auto request = [&](int s) {  // s static
    if (s < KS) frag_read(fh[s % 3], fl[s % 3], ws_addr<RG>(w, g0, s));
    else frag_read(fh[s % 3], fl[s % 3], ws_addr<RG>(w, g0 + 1, 0));
  };
  auto step = [&](int ks, f32x16& acc) {  // ks static
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[ks % 3], bl[ks & 3], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (ks + 2 <= KS) request(ks + 2);
    if (ks == KS - 1) ws_transition<PW, false, RG>(w, g0);
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fl[ks % 3], bh[ks & 3], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[ks % 3], bh[ks & 3], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (ks + 2 <= KS) frag_wait<2>(fh[(ks + 1) % 3], fl[(ks + 1) % 3]);
  };
  request(1);
  step(0, a0); step(1, a0); step(2, a0); step(3, a0);
  step(4, a1); step(5, a1); step(6, a1); step(7, a1);
  frag_settle(w.ch, w.cl, fh[KS % 3], fl[KS % 3]);
  w.g = g0 + 1;
}

// A tile's product for a wave WITH a row tile, or (active false) its share of the ring's hand-shakes: a wave that runs one barrier
// fewer than its workgroup hangs the CU, so the two are paired here and nowhere else.  active is wave-uniform: a constant (the
// ACTIVE instantiations of the tile functions) or a run-time value (the sdf chain's tail workgroups).  ZERO: the accumulator starts
// at zero (false: the product adds to what it holds).
template <int KS, int PW = 4, bool WRAP = false, int RG = RING_GROUPS, bool ZERO = true>
__device__ __forceinline__ void prod(WStream& w, bool active, const f16x8 (&bh)[KS], const f16x8 (&bl)[KS], f32x16& acc) {
  if (ZERO) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  }
  if (active) product<KS, PW, WRAP, RG>(w, bh, bl, acc);
  else product_skip<KS, PW, WRAP, RG>(w);
}

// the same over the first ksn (wave-uniform, run time; >= 1) of KS k-steps: the mapping network's first layer.  No read-ahead
// inside the tile (every step sits in its own branch); 8 short tiles per row tile.
template <int KS>
__device__ __forceinline__ void product_dyn(WStream& w, int ksn, const f16x8 (&bh)[KS], const f16x8 (&bl)[KS], f32x16& acc) {
  const int g0 = w.g;
  const int ng = (ksn + GSLABS - 1) / GSLABS;
  f16x8 ah = w.ch, al = w.cl;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    if (ks < ksn) {
      const bool last = ks == ksn - 1;
      if ((ks & (GSLABS - 1)) == GSLABS - 1 || last) ws_transition(w, g0 + ks / GSLABS);
      f16x8 nh = ah, nl = al;
      frag_read(nh, nl, last ? ws_addr(w, g0 + ng, 0) : ws_addr(w, g0 + (ks + 1) / GSLABS, (ks + 1) % GSLABS));
      __builtin_amdgcn_sched_barrier(0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[ks], acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      frag_settle(ah, al, nh, nl);
    }
  }
  w.ch = ah;
  w.cl = al;
  w.g = g0 + ng;
}

// pow2_scale of a batch row's largest magnitude (lanes l and l ^ 32 hold the two halves of the row)
__device__ __forceinline__ float row_scale(float m, float& inv) {
  return pow2_scale(fmaxf(m, __shfl_xor(m, 32, 64)), inv);
}

__device__ __forceinline__ float4 ldg4_nt(const float* p) {  // bypasses this CU's vector L1 (served by the XCD's L2)
  const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}

// B planes of KS k-steps from an fp32 row [dim] (dim % 4 == 0, columns >= dim read as 0): returns 1 / scale
template <int KS>
__device__ __forceinline__ float load_planes(const float* __restrict__ rowp, int dim, int ksn, int h, f16x8 (&ph)[KS], f16x8 (&pl)[KS]) {
  float v[KS][8];
  float m = 0.0f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int feat = 16 * ks + 8 * u + 4 * h;
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ks < ksn && feat < dim) q = ldg4(rowp + feat);
      v[ks][4 * u] = q.x; v[ks][4 * u + 1] = q.y; v[ks][4 * u + 2] = q.z; v[ks][4 * u + 3] = q.w;
      m = fmaxf(fmaxf(m, fmaxf(fabsf(q.x), fabsf(q.y))), fmaxf(fabsf(q.z), fabsf(q.w)));
    }
  float inv;
  const float s = row_scale(m, inv);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = v[ks][j] * s;
    split8(x, ph[ks], pl[ks]);
  }
  return inv;
}

// a wave's 32 x 32 tile of a tile-native matrix (numerics.h) <-> its accumulator registers: four 1 KB-contiguous float4 instructions
__device__ __forceinline__ void store_tile(float* blk, int lane, const float (&v)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) stg4(blk + g * 256 + lane * 4, make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]));
}
// a tile nothing reads again before the backward (saved h / z): non-temporal, it need not displace the weight stream in L2
__device__ __forceinline__ void store_tile_nt(float* blk, int lane, const float (&v)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    __builtin_nontemporal_store(f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]}, reinterpret_cast<f32x4*>(blk + g * 256 + lane * 4));
}
__device__ __forceinline__ void load_tile(const float* blk, int lane, float (&v)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 q = ldg4(blk + g * 256 + lane * 4);
    v[4 * g] = q.x; v[4 * g + 1] = q.y; v[4 * g + 2] = q.z; v[4 * g + 3] = q.w;
  }
}

// largest magnitude of a gradient matrix -> device scalar (the weight-gradient GEMM pre-scales its fp16 split with it)
__device__ __forceinline__ void publish_max(float* slot, float v, bool live_row, bool wave_live, int lane) {
  v = wave_max(live_row ? v : 0.0f);
  if (wave_live && lane == 0 && v > 0.0f) atomicMax(reinterpret_cast<unsigned int*>(slot), __float_as_uint(v));
}

__device__ __forceinline__ void hidden_load4(f32x4& q, const float* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(q) : "v"(p) : "memory");
}
template <int N>
__device__ __forceinline__ void hidden_wait(f32x4 (&q)[4]) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]) : "n"(N) : "memory");
}

template <int N>
__device__ __forceinline__ void hidden_wait8(f32x4 (&p)[4], f32x4 (&q)[4]) {
  asm volatile("s_waitcnt vmcnt(%8)" : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3]), "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]) : "n"(N) : "memory");
}
// a load of data THIS lane stored earlier in the launch: bypass the CU's vector L1 (nt), served by the XCD's L2
__device__ __forceinline__ void hidden_load4_nt(f32x4& q, const float* p) {
  asm volatile("global_load_dwordx4 %0, %1, off nt" : "+v"(q) : "v"(p) : "memory");
}

// planes of 2 NT k-steps from NT tiles this wave stored (the lane that stored a piece loads it).  x is the row maximum: the tiles are
// scaled by the power of two that suits it (row_scale) and 1 / scale is returned.  SCALED (planes_scaled below, the only user of the
// flag): x is the scale itself, a power of two the caller formed, and the return value (1) means nothing.  One body with a flag, not
// row_scale followed by a call of planes_scaled: that form schedules the loads of every caller differently.
template <int NT, bool SCALED = false>
__device__ __forceinline__ float planes_from_tiles(const float* blk, int lane, float x, f16x8 (&ph)[2 * NT], f16x8 (&pl)[2 * NT]) {
  float inv = 1.0f;
  const float s = SCALED ? x : row_scale(x, inv);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float v[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 q = ldg4_nt(blk + t * 1024 + g * 256 + lane * 4);
      v[4 * g] = q.x; v[4 * g + 1] = q.y; v[4 * g + 2] = q.z; v[4 * g + 3] = q.w;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float x8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x8[j] = v[8 * u + j] * s;
      split8(x8, ph[2 * t + u], pl[2 * t + u]);
    }
  }
  return inv;
}
template <int NT>
__device__ __forceinline__ void planes_scaled(const float* blk, int lane, float s, f16x8 (&ph)[2 * NT], f16x8 (&pl)[2 * NT]) {
  planes_from_tiles<NT, true>(blk, lane, s, ph, pl);
}

// A kernel's table of N4 float4 (film_pack_kernel's biases + tile scales) -> LDS by THREADS threads, all loads in flight at once.
// A macro, not a function: through a function's parameters (the two pointers, a reference to the kernel argument, the LDS offset as
// a template parameter: all tried) the first loads lose their scalar-base + 32-bit-offset form to 64-bit adds per lane.
#define NSKY_STAGE_TABLE(N4, THREADS, table, lds, tid)                                                                  \
  {                                                                                                                    \
    float4 q[((N4) + (THREADS) - 1) / (THREADS)];                                                                      \
    _Pragma("unroll") for (int i = 0; i < ((N4) + (THREADS) - 1) / (THREADS); ++i)                                     \
      if (i * (THREADS) + (tid) < (N4)) q[i] = ldg4((table) + 4 * (i * (THREADS) + (tid)));                             \
    _Pragma("unroll") for (int i = 0; i < ((N4) + (THREADS) - 1) / (THREADS); ++i)                                     \
      if (i * (THREADS) + (tid) < (N4)) *reinterpret_cast<float4*>((lds) + 4 * (i * (THREADS) + (tid))) = q[i];         \
  }

// Tail workgroups of the EIGHT-wave kernels (the mapping backward, the sdf chain: two waves per SIMD, 256 batch rows share one weight
// stream).  A launch of n wave tiles (32 rows each) on C CUs runs F = floor(n / (8 C)) C full workgroups of eight tiles; the
// remaining R = n - 8 F tiles (less than one workgroup round) do not get a round of full workgroups on a few CUs: they are dealt k =
// ceil(R / C) to a workgroup (T = ceil(R / k) "tail" workgroups, FIRST in the grid), whose other waves only take part in the ring's
// hand-shakes (product_skip).  A tail workgroup is done sooner than a full one and the dispatcher hands its CU the next workgroup, so
// the remainder costs its share of a round instead of a whole one (263 456 DDF rows = 8233 tiles: 1024 full + 41 one-tile workgroups
// instead of 1030 full ones = five rounds of time for 4.02 of work).
struct TailPlan { int full_wgs, tail_wgs, tail_k; };
inline TailPlan tail_plan(long n_tiles, int cus) {
  TailPlan p;
  p.full_wgs = (int)(n_tiles / (8L * cus)) * cus;
  const long rem = n_tiles - 8L * p.full_wgs;
  if (rem >= 8L * cus - cus) {  // nearly a whole round: full workgroups
    p.full_wgs += (int)((rem + 7) / 8); p.tail_wgs = 0; p.tail_k = 0;
    return p;
  }
  p.tail_k = (int)((rem + cus - 1) / cus);
  p.tail_wgs = p.tail_k ? (int)((rem + p.tail_k - 1) / p.tail_k) : 0;
  return p;
}
// wave tile of this wave, or -1 (a wave of a tail workgroup without one)
__device__ __forceinline__ long tail_tile(int full_wgs, int tail_wgs, int tail_k, long n_tiles, int wave) {
  const int b = blockIdx.x;
  if (b >= tail_wgs) return (long)(b - tail_wgs) * 8 + wave;
  const long t = 8L * full_wgs + (long)b * tail_k + wave;
  return (wave < tail_k && t < n_tiles) ? t : -1;
}

inline int device_cus() {
  static int cus = [] {
    hipDeviceProp_t p;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return 256;
    return p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
  }();
  return cus;
}

}  // namespace
