/* neusky_hip.h - C ABI of libneusky_hip.so (MI355X / gfx950 HIP kernels for the NeuSky hot path).
 *
 * The reference (JADGardner/neusky) is 100% Python and has NO native boundary of its own
 * (SURVEY.md F1): every native kernel it runs belongs to tiny-cuda-nn / torch / nerfacc.  This
 * header is therefore the drop-in seam SURVEY.md 8(b) defines: each entry point replaces the
 * external kernel (or the chain of torch ops) the reference reaches at the cited call site.
 *
 * Conventions (all entry points)
 *   - extern "C", plain device pointers + sizes + scalars + a hipStream_t; no torch types.
 *   - ownership: the caller allocates every buffer (device memory); the callee never allocates,
 *     frees or retains a pointer.  All matrices are row-major float32 unless stated; leading
 *     dimensions (ld*) are in elements.
 *   - errors: return 0 on success, <0 on error (never throws); nsky_last_error() returns the text
 *     of the calling thread's last error.
 *   - threading: re-entrant, no global mutable state except the thread-local error string;
 *     stream-ordered; no host synchronisation and no allocation inside (hipGraph-capturable).
 */
#ifndef NEUSKY_HIP_H
#define NEUSKY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nsky_stream_t; /* hipStream_t */

const char* nsky_last_error(void);
int nsky_abi_version(void); /* 18 (bumped when a struct layout or an entry point's signature changes) */

/* ------------------------------------------------------------------------------------------
 * Dense layer on the matrix cores: C[M,N] = epilogue( sum_k A(m,k) * B(n,k) + bias[n] )
 * exact fp32 (v_mfma_f32_32x32x2_f32).  Replaces torch nn.Linear / F.linear + activation at
 *   neusky/fields/sdf_albedo_field.py:172,199-207,233 (geo + colour nets),
 *   neusky/utils/siren.py:114-119,138-144,207 (mapping net, FiLM sine layers, head),
 * and the autograd-generated backward GEMMs of the same layers.
 *   a_kcontig: 1 -> A stored [M][lda] (k contiguous); 0 -> A stored [K][lda] (m contiguous, i.e. A^T view)
 *   b_kcontig: 1 -> B stored [N][ldb] (k contiguous, torch Linear weight); 0 -> B stored [K][ldb]
 *   k-contiguous operands need K % 4 == 0 (zero padded); every ld % 4 == 0, bases 16-byte aligned.
 *   k_splits > 1: split the K range over grid.z and atomically add into C (C pre-zeroed by the
 *                 caller, epilogue must be NSKY_EPI_NONE, bias NULL) - used for weight gradients.
 */
enum {
  NSKY_EPI_NONE = 0,
  NSKY_EPI_RELU = 1,
  NSKY_EPI_LEAKY = 2,      /* slope p0 */
  NSKY_EPI_SIGMOID = 3,    /* C = p0 * sigmoid(v) */
  NSKY_EPI_SOFTPLUS = 4,   /* beta p0 (threshold 20); out1 (optional) = sigmoid(beta v) = d softplus/dv */
  NSKY_EPI_FILM = 5,       /* C = sin((p0*aux0+p1) * v + aux1); out1 (optional) = v */
  NSKY_EPI_MUL_AUX = 6,    /* C = v * aux0[row % row_mod] */
  NSKY_EPI_BWD_RELU = 7,   /* C = v * (aux0 > 0) */
  NSKY_EPI_BWD_LEAKY = 8,  /* C = v * (aux0 > 0 ? 1 : p0) */
  NSKY_EPI_BWD_FILM = 9,   /* z=aux0, F=aux1, P=aux2: u=(p0 F+p1) z+P; C=v cos(u)(p0 F+p1); out1=v cos(u) z p0; out2=v cos(u) */
  NSKY_EPI_EXP = 10        /* C = exp(min(v, p0)) */
};

/* contraction arithmetic: exact fp32 MFMA (default); or operands split on the fly into 2 / 3 bf16 terms and
 * rebuilt from 3 / 6 bf16 MFMAs with fp32 accumulation (relative product error ~2^-16 / ~2^-22); or F16X2: split into
 * fp16 hi + fp16 residual scaled by 2^11, rebuilt from 3 fp16 MFMAs in two fp32 accumulators (~2^-21, fp32-grade) --
 * for operands within fp16's range only (|x| <= 65504, larger magnitudes saturate): forward layers, not gradients.
 * N <= 64 always runs the fp32 kernel. */
enum { NSKY_PREC_F32 = 0, NSKY_PREC_BF16X2 = 2, NSKY_PREC_BF16X3 = 3, NSKY_PREC_F16X2 = 4 };

typedef struct nsky_gemm_desc {
  const float* A; const float* B; float* C;
  int32_t M, N, K;
  int32_t lda, ldb, ldc;
  int32_t a_kcontig, b_kcontig;
  const float* bias;
  int32_t epi;
  float p0, p1;
  const float* aux0; int32_t ldaux0;
  const float* aux1; int32_t ldaux1;
  const float* aux2; int32_t ldaux2;
  float* out1; int32_t ldout1;
  float* out2; int32_t ldout2;
  int32_t row_mod;   /* 0 = M */
  int32_t k_splits;  /* 0/1 = none */
  float beta;        /* C = result + beta * C_old (non-split only; 0 or 1) */
  float* a_rowsum;   /* optional [M]: ACCUMULATES sum_k A(m,k) (bias gradient when A = dZ^T); atomics */
  int32_t precision; /* NSKY_PREC_*: arithmetic of the contraction (operands and result stay fp32 in memory) */
  int32_t rowsum_k_limit; /* a_rowsum sums only k < rowsum_k_limit (multiple of 32; 0 = all of K): the value rows of a stacked
                             [value; tangent] gradient matrix carry the bias, the tangent rows do not */
  int32_t a_native_nt, b_native_nt; /* > 0: that operand (a_kcontig / b_kcontig must be 0) is a TILE-NATIVE matrix with this many
                             32-feature tiles per row, as the FiLM chain kernels store activations and gradients (below) */
  const float* a_scale_max; /* optional device scalar = largest |A| (NSKY_PREC_F16X2, N > 64): A is staged times the power of two
                             that brings it to ~2^14, so the fp16 split keeps fp32-grade products for gradients of any
                             magnitude; C and a_rowsum are scaled back */
} nsky_gemm_desc;

int nsky_gemm_f32(const nsky_gemm_desc* d, nsky_stream_t stream);

/* Same contraction against a PRE-SPLIT B operand (a weight matrix, re-read by every row tile of A): the two 16-bit
 * planes of B -- fp16 hi + 2^11-scaled fp16 residual (NSKY_PREC_F16X2) or bf16 hi + bf16 residual (NSKY_PREC_BF16X2) --
 * are produced once per optimisation step by nsky_split_planes and streamed into LDS by LDS-DMA, as is the raw fp32 A,
 * which is split in place there (no register staging; same MFMA sequence and results as nsky_gemm_f32 with that precision).
 *   nsky_split_planes: planes(n, k) = W[n][k] (transpose = 0: forward layers, W = torch Linear weight [out, in]) or
 *                      W[k][n] (transpose = 1: input gradients dX = dZ W); hi / lo are [rows_pad][ldp] uint16, zero padded,
 *                      rows_pad % 256 == 0, ldp % 32 == 0.
 *   nsky_gemm_f32_planes: d->B, ldb, b_kcontig are ignored; A must be k-contiguous; K % 4 == 0 (finite A); no split-K, no a_rowsum;
 *                      d->precision selects the plane format (must match the split); epilogues as nsky_gemm_f32. */
int nsky_split_planes(const float* W, int32_t n_rows, int32_t n_k, int32_t ldw, int32_t transpose, int32_t precision,
                      uint16_t* hi, uint16_t* lo, int32_t rows_pad, int32_t ldp, nsky_stream_t stream);
int nsky_gemm_f32_planes(const nsky_gemm_desc* d, const uint16_t* B_hi, const uint16_t* B_lo, int32_t ldp, nsky_stream_t stream);

/* column sums: out[n] (+)= sum_m X[m,n]  (bias gradients) */
int nsky_colsum_f32(const float* X, int32_t M, int32_t N, int32_t ldx, float* out, nsky_stream_t stream);
/* out[c] += sum_r w[r * w_stride] X[r][c]: the weight gradient of a ONE-output dense layer (the sdf head of the geo net,
 * sdf_albedo_field.py:169-174 and :233-238) -- a matrix-vector product streamed at HBM rate instead of a 1-row GEMM. */
int nsky_weighted_colsum_f32(const float* X, int32_t M, int32_t N, int32_t ldx, const float* w, int32_t w_stride, float* out,
                             nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * FiLM-SIREN chain as ONE kernel per row tile (no per-layer launches, no [M, 2 n_film H] frequency / phase matrix, no
 * layer-to-layer activation round trip through HBM).  Replaces the whole module neusky/utils/siren.py:108-208
 * (CustomMappingNetwork :108-131, FiLMLayer :133-145, DDFFiLMSiren.forward :189-208; frequencies = raw * 15 + 30 :200) at
 * its call sites neusky/fields/directional_distance_field.py:233-243,275-276 (DDF) and the RENI-shaped illumination
 * decode driven from neusky/models/neusky_model.py:488-506,535-549.
 *   net: geometry + the fp32 parameter pointers in torch nn.Linear layout ([out, in], rows contiguous, leading dimensions
 *        in elements).  hidden = width of the FiLM layers AND of the mapping layers (128 or 256); cond_dim <= 320,
 *        x_dim <= 16, out_dim <= 4, at most NSKY_FILM_MAX_LAYERS layers each.
 *   nsky_film_stream_layout: bytes of the packed weight stream and number of 32-feature weight tiles.
 *   nsky_film_pack: once per optimisation step: every weight tile -> power-of-two scaled fp16 hi + fp16 residual planes in
 *        MFMA-fragment order (direction 0 = forward stream, 1 = FiLM backward, 2 = mapping backward, 3 = FiLM backward on saved operands), plus `table` (NSKY_FILM_TABLE_FLOATS
 *        floats, 16-byte aligned): every bias of the network followed by one reciprocal scale per tile.
 *   nsky_film_chain_fwd: cond [M, ldcond] (first cond_dim columns), x [M, ldx] -> res [M, ldres] (first out_dim columns,
 *        raw head output; columns out_dim..3 are written too).  Side outputs, each a TILE-NATIVE [ceil32(M), hidden] matrix
 *        (below): y_save[i] (FiLM layer outputs, also the hand-off to the next layer), z_save[i] (FiLM pre-activations
 *        W y + b; optional), h_save[l] (mapping activations after LeakyReLU(0.2); optional).
 *        Only the weight gradients read the kept y_save[i].  A caller that does not need them (frozen weights, no gradient)
 *        passes, at hidden 128, y_save = NULL or every entry NULL: the hand-off stays in registers and no output is written;
 *        at hidden 256 (no registers to spare) two ping-pong buffers, y_save[i] = buffer i % 2 (entries may alias: a wave
 *        reads a layer's tiles back before it stores the next layer's).  A mix of NULL and non-NULL entries is an error.
 *        Products are fp32-grade (three fp16 MFMAs on power-of-two pre-scaled hi / residual planes, fp32 accumulate).
 *   Tile-native layout of a [rows, width] fp32 matrix (rows padded to a multiple of 32, width % 32 == 0): 32 x 32 blocks of
 *        4 KB in the accumulator order of v_mfma_f32_32x32x16; the element offsets are defined in
 *        neusky_amd/csrc/numerics.h (native_offset).  nsky_gemm_f32 reads such operands with
 *        a_native_nt / b_native_nt = width / 32 (weight gradients).
 */
#define NSKY_FILM_MAX_LAYERS 12
#define NSKY_FILM_TABLE_FLOATS 6656
typedef struct nsky_film_net {
  int32_t hidden, n_map, n_film;
  int32_t cond_dim, x_dim, out_dim;
  const float* map_w[NSKY_FILM_MAX_LAYERS]; const float* map_b[NSKY_FILM_MAX_LAYERS]; int32_t map_ld[NSKY_FILM_MAX_LAYERS];
  const float* mo_w; const float* mo_b; int32_t mo_ld;     /* mapping head [2 n_film hidden, hidden]: frequencies, then phases */
  const float* film_w[NSKY_FILM_MAX_LAYERS]; const float* film_b[NSKY_FILM_MAX_LAYERS]; int32_t film_ld[NSKY_FILM_MAX_LAYERS];
  const float* out_w; const float* out_b; int32_t out_ld;  /* head [out_dim, hidden] */
} nsky_film_net;
int nsky_film_stream_layout(const nsky_film_net* net, int32_t direction, int64_t* stream_bytes, int32_t* n_tiles);
int nsky_film_pack(const nsky_film_net* net, int32_t direction, void* stream_buf, float* table, nsky_stream_t stream);
int nsky_film_chain_fwd(const nsky_film_net* net, const void* stream_buf, const float* table, const float* cond,
                        int32_t ldcond, const float* x, int32_t ldx, int32_t M, float* const* h_save, float* const* z_save,
                        float* const* y_save, float* res, int32_t ldres, nsky_stream_t stream);
/* Backward of the chain (replaces the autograd-generated backward of siren.py:108-208; parameters' gradients are then plain
 * weight-gradient GEMMs, nsky_gemm_f32 with a_native_nt / b_native_nt, over the tile-native matrices written here).
 *   nsky_film_chain_bwd_film (stream / table packed with direction 1): d_res [M, ldres] -> for every FiLM layer i
 *        dz_save[i] = dL/d(W y + b) (tile-native [ceil32(M), hidden]) and, in dfp (tile-native [ceil32(M), 2 n_film hidden]),
 *        dL/dF_i in columns i hidden.. and dL/dphase_i in columns (n_film + i) hidden..; dfp_rowmax [ceil32(M)] = max |dfp| of each
 *        batch row.  F and phase are re-formed from h_last (the last mapping activation), z_save[i] is read back.
 *   nsky_film_chain_bwd_map (direction 2): dfp, dfp_rowmax, h_save[l] -> dpre_save[l] = dL/d(pre-activation of mapping layer l)
 *        (tile-native) and d_cond [M, ldcond] (row-major, optional): the first pad4(cond_dim) columns of a row are written, the pad
 *        columns among them with zero; columns beyond them (ldcond may be wider) are left as they are.
 * gmax (caller zero-fills): largest magnitude of each gradient matrix, for nsky_gemm_f32's a_scale_max -- bwd_film writes
 *        [i] = max |dz_save[i]| (i < n_film) and [n_film] = max |dfp|; bwd_map writes [l] = max |dpre_save[l]| (l < n_map).
 * Frozen weights (only the weight gradients read dz_save / dpre_save; d_x, dfp, dfp_rowmax, gmax[n_film] and d_cond are the same
 *        bits either way):
 *        bwd_film, hidden 128 or 256: dz_save = NULL or every entry NULL -> no dz is stored and gmax[i], i < n_film, stays as passed.
 *        bwd_map, hidden 128: dpre_save = NULL or every entry NULL -> dpre stays in registers from layer to layer.
 *        bwd_map, hidden 256: every dpre_save[l] the SAME [ceil32(M), hidden] buffer (n_map > 1; scratch: a wave reads only the tiles
 *        it stored, and has layer l in registers before it stores the first tile of layer l - 1).  Also accepted at hidden 128.
 *        In both forms bwd_map leaves gmax[l] as passed.  A mix of NULL and non-NULL entries, or of shared and distinct ones, is
 *        an error, and so is a NULL dpre_save at hidden 256.
 * hidden must be a multiple of 128 for the backward streams.  d_x (optional, [M, ldx], ldx <= 16; the first pad4(x_dim) columns of a row
 * are written, as for d_cond): gradient w.r.t. the FiLM input rows (the DDF's multi-view rays differentiate through their direction
 * rows, neusky/models/ddf_model.py:297-322). */
int nsky_film_chain_bwd_film(const nsky_film_net* net, const void* stream_buf, const float* table, int32_t M, const float* d_res,
                             int32_t ldres, const float* h_last, const float* const* z_save, float* const* dz_save, float* dfp,
                             float* dfp_rowmax, float* gmax, float* d_x, int32_t ldx, nsky_stream_t stream);
int nsky_film_chain_bwd_map(const nsky_film_net* net, const void* stream_buf, const float* table, int32_t M, const float* dfp,
                            const float* dfp_rowmax, const float* const* h_save, float* const* dpre_save, float* d_cond,
                            int32_t ldcond, float* gmax, nsky_stream_t stream);
/* The chain on SAVED FiLM operands: instead of re-forming F and phase from h_last in the backward (two hidden x hidden products per
 * FiLM layer), the forward keeps what its epilogue forms from them and the backward reads it back.
 *   nsky_film_chain_fwd_saved: nsky_film_chain_fwd plus f_save[i] = 15 F_i + 30 and arg_save[i] = f_i z_i + phase_i (the sine's argument),
 *        each a tile-native [ceil32(M), hidden] matrix like z_save[i]; every entry of both lists is required.  res and the other side
 *        outputs are the bits nsky_film_chain_fwd writes.
 *   nsky_film_chain_bwd_film_saved: nsky_film_chain_bwd_film with z_save[i], f_save[i], arg_save[i] in place of h_last; stream / table
 *        packed with direction 3 (direction 1 without the F and phase tiles: the transposed FiLM tiles of layers n_film-1 .. 1, then
 *        the layer-0 input tile).  dz_save, dfp, dfp_rowmax, gmax and d_x as in nsky_film_chain_bwd_film, frozen form included, and
 *        the same bits: g = dY cos(arg), dz = g f, dF = 15 g z, dphase = g on the values the re-form would rebuild. */
int nsky_film_chain_fwd_saved(const nsky_film_net* net, const void* stream_buf, const float* table, const float* cond,
                              int32_t ldcond, const float* x, int32_t ldx, int32_t M, float* const* h_save, float* const* z_save,
                              float* const* y_save, float* const* f_save, float* const* arg_save, float* res, int32_t ldres,
                              nsky_stream_t stream);
int nsky_film_chain_bwd_film_saved(const nsky_film_net* net, const void* stream_buf, const float* table, int32_t M, const float* d_res,
                                   int32_t ldres, const float* const* z_save, const float* const* f_save, const float* const* arg_save,
                                   float* const* dz_save, float* dfp, float* dfp_rowmax, float* gmax, float* d_x, int32_t ldx,
                                   nsky_stream_t stream);
/* SDF value chain: SDFAlbedoField.get_sdf_at_pos (neusky/fields/sdf_albedo_field.py:169-174; nerfstudio SDFField geometry network:
 * Linear + Softplus(beta) twice, then the sdf row of the last Linear) for M encode rows, forward and backward as one kernel each
 * (csrc/sdf_chain.hip; the weight-stream machinery of the FiLM-SIREN chain, csrc/chain.h: nsky_sdf_stream_layout / nsky_sdf_pack once per optimizer step and
 * direction, 0 = forward, 1 = backward).  a0_save / a1_save: the two softplus outputs, tile-native [ceil32(M), hidden] (scratch in
 * inference).  _bwd: g_sdf [M] -> dz1 / dz0 (tile-native pre-activation gradients: the operands of the weight gradients,
 * nsky_wgrad_native), dE [M, ldE] (optional), dw2 [hidden] += sum_rows g a1 and db2 [1] += sum_rows g (optional), gmax [2] = max |dz1|, max |dz0| (caller
 * zero-fills).  hidden = 256, in_dim 4..80 (multiple of 4).
 * What is read and written: _fwd reads columns [0, in_dim) of rows [0, M) of E (ldE >= in_dim, ldE % 4 == 0: the columns behind them and
 * the rows behind M are never read) and writes sdf[0 .. M).  _bwd writes columns [0, in_dim) of rows [0, M) of dE and nothing else:
 * whatever a wider ldE leaves behind them, and every row from M on, is left as it is.  The tile-native matrices are written for the
 * rows < M (the rows of the last wave tile behind M: unspecified).  E, dE and the tile-native matrices are 16-byte aligned.  Anything
 * else (M <= 0 included) is refused with an error return and nothing is launched. */
typedef struct {
  int32_t in_dim, hidden;
  const float* w0; int32_t ld0; const float* b0;   /* [hidden, in_dim] */
  const float* w1; int32_t ld1; const float* b1;   /* [hidden, hidden] */
  const float* w2; const float* b2;                /* the sdf row [hidden] of the last layer and its bias (1 value; may be null) */
  float beta;
} nsky_sdf_net;
int nsky_sdf_stream_layout(const nsky_sdf_net* net, int32_t direction, int64_t* stream_bytes, int32_t* n_tiles);
int nsky_sdf_pack(const nsky_sdf_net* net, int32_t direction, void* stream_buf, float* table, nsky_stream_t stream);
int nsky_sdf_chain_fwd(const nsky_sdf_net* net, const void* stream_buf, const float* table, const float* E, int32_t ldE, int32_t M,
                       float* a0_save, float* a1_save, float* sdf, nsky_stream_t stream);
int nsky_sdf_chain_bwd(const nsky_sdf_net* net, const void* stream_buf, const float* table, int32_t M, const float* g_sdf,
                       const float* a0_save, const float* a1_save, float* dz1, float* dz0, float* dE, int32_t ldE, float* dw2,
                       float* db2, float* gmax, nsky_stream_t stream);

/* Weight and bias gradient of one dense layer of the chain straight over two tile-native matrices (what autograd's
 * AddmmBackward / the MmBackward pair of nn.Linear computes for siren.py:59-66, :167-172 and the mapping network's layers):
 *     dW[n, k] += sum_rows dZ[row, n] X[row, k]   (n < 32 nnt_a, k < 32 nnt_b; dW row-major, leading dimension ldw)
 *     db[n]    += sum_rows dZ[row, n]             (db optional)
 * dW / db are ACCUMULATED into (float atomics over a batch split): the caller zero-fills them or passes a gradient slab.
 * nnt_a and nnt_b must be multiples of 4 (128 features).  a_scale_max: device scalar holding max |dZ| (gmax above), or null;
 * b_scale: power of two applied to X before the fp16 hi + residual split (2^6 suits activations up to ~500).  Products are
 * fp32-grade (three fp16 MFMAs per product, fp32 accumulation). */
int nsky_wgrad_native(const float* dZ, int32_t nnt_a, const float* X, int32_t nnt_b, int32_t rows, float* dW, int32_t ldw,
                      float* db, const float* a_scale_max, float b_scale, nsky_stream_t stream);
/* The same for up to NSKY_WGRAD_MAX_PROBLEMS layers that share the batch (every layer of a chain's backward) in ONE launch:
 * the batch split is shared, so the reduction traffic and the launch cost are paid once instead of per layer. */
#define NSKY_WGRAD_MAX_PROBLEMS 16
typedef struct {
  const float* dZ; int32_t nnt_a;
  const float* X;  int32_t nnt_b;
  float* dW;       int32_t ldw;
  float* db;                 /* may be null */
  const float* a_scale_max;  /* may be null */
  float b_scale;
  /* ROW-MAJOR operands instead of tile-native ones (the SDF / colour field's weight gradients, autograd's MmBackward of
   * sdf_albedo_field.py:147-161,199-207): lda, ldb > 0 = leading dimensions of dZ [rows, width_a] and X [rows, width_b] (widths and
   * leading dimensions multiples of 4; nnt_*, a_scale_max, b_scale unused); the products are then the 2-term bf16 split (2^-16 per
   * product, no pre-scaling).  All problems of one launch are of the same kind.  bias_rows > 0: db sums only the first bias_rows rows
   * (stacked value + tangent rows: only the value rows carry a bias). */
  int32_t lda, ldb, width_a, width_b, bias_rows;
  /* tile-native operands only: width_a / width_b > 0 = features of dZ / X that exist (dW is [width_a, width_b], ldw >= width_b; the
   * tiles beyond are walked but their outputs dropped); bias_row_mod = 4: db sums the rows with row % 4 == 0 only (quad-native
   * matrices of the SDF field, nsky_field_geo_bwd: row 4 n + j is row-set j of point n and only the value rows carry a bias). */
  int32_t bias_row_mod;
  /* tile-native operands only: device scalar holding max |X| (may be null: the constant b_scale applies).  Operands that carry input
   * tangents -- the quad-native encode rows and hidden activations of the SDF field -- have no a-priori bound (a hash level of resolution
   * 2048 with table differences of order one has d feature / d x in the thousands): nsky_field_geo_fwd publishes their maxima. */
  const float* b_scale_max;
} nsky_wgrad_problem;
int nsky_wgrad_native_batch(const nsky_wgrad_problem* problems, int32_t n_problems, int32_t rows, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SDF / albedo field as chain kernels (csrc/field_chain.hip).  Replaces SDFAlbedoField.get_outputs / get_colors,
 * neusky/fields/sdf_albedo_field.py:185-269: the geometry network it inherits from nerfstudio's SDFField ([x | PE6 | hash] -> Linear +
 * Softplus(beta) -> Linear + Softplus(beta) -> Linear -> [sdf | feat]), torch.autograd.grad(sdf, x, create_graph=True) (:231-238; here the
 * encode row's three tangent rows ride through the layers in forward mode) and the colour network (:147-161,199-207), forward and
 * backward (the reference's double backward) as two kernels each on the weight-stream machinery of the FiLM-SIREN chain.
 *
 * Packed weight streams of arbitrary layer lists: a layer is a [rows, K] matrix (transposed = 0: W[r][k] = W[r * ld + k]; transposed = 1:
 * W[r][k] = W[k * ld + r], i.e. the torch [out, in] matrix walked by input feature), cut into ceil(rows / 32) tiles of 32 output rows,
 * K <= 320.  nsky_chain_pack writes the stream and one reciprocal power-of-two scale per tile (scales[n_tiles]).
 */
#define NSKY_CHAIN_MAX_LAYERS 8
typedef struct { const float* W; int32_t ld, rows, K, transposed; } nsky_chain_layer;
int nsky_chain_stream_layout(const nsky_chain_layer* layers, int32_t n_layers, int64_t* stream_bytes, int32_t* n_tiles, int32_t* n_groups);
int nsky_chain_pack(const nsky_chain_layer* layers, int32_t n_layers, void* stream_buf, float* scales, nsky_stream_t stream);
/* The small vectors of the field the kernels keep in LDS (hidden width 256, geometric feature width 256).  The weight matrices come as
 * packed streams (total_groups = their n_groups), in this order:
 *   geo_fwd    : W0 [256, in_dim], W1 [256, 256]
 *   colour_fwd : W2f [256, 256] (feature rows of the last geometry layer), Wc0 [256, 300] (columns [feat 256 | 0 0 0 0 | x PE | 0]), Wc1 [256, 256]
 *   colour_bwd : Wc1^T, Wc0^T (rows = its 300 input columns), W2f^T      (transposed = 1)
 *   geo_bwd    : W1^T, W0^T (rows = in_dim)                              (transposed = 1) */
typedef struct nsky_field_net {
  int32_t in_dim;                         /* width of an encode row (multiple of 4; 68..80): [x | PE | hash] */
  int32_t npe;                            /* its leading x / PE columns that also feed the colour net (<= 39) */
  float beta;                             /* Softplus beta (sdf_albedo_field.py:163) */
  const float* b0; const float* b1;       /* [256] biases of the two hidden geometry layers */
  const float* w_sdf; const float* b_sdf; /* the sdf row [256] of the last geometry layer and its bias [1] (may be null) */
  const float* b2f;                       /* [256] bias of its feature rows */
  const float* bc0; const float* bc1;     /* [256] */
  const float* wc2; int32_t ldc2; const float* bc2;  /* output layer of the colour net [3, 256] (row stride ldc2), [3] */
} nsky_field_net;
/* QUAD-NATIVE matrices: tile-native [ceil32(4 N), width] whose row 4 n + j is row-set j of point n (j = 0: value, j = 1..3: d/dx_k).
 * ET: the stacked encode matrix [4 N, ldE] of nsky_encode_fwd (row j N + n).  Outputs: sdf [N], grad [N, 3] (d sdf / dx), a0q / a1q
 * (the two hidden layers' outputs, quad-native, width 256), Eq (optional; quad-native copy of the encode rows, width 128, for the first
 * layer's weight gradient), a1max [N] (optional: largest |a1| of each value row, the colour path's operand scale), qmax [2] (optional; the
 * caller zero-fills it: max |Eq| and max |a0q| over value and tangent rows, the b_scale_max of the first two layers' weight gradients). */
int nsky_field_geo_fwd(const nsky_field_net* net, const void* stream_buf, const float* scales, int32_t total_groups, const float* ET,
                       int32_t ldE, int32_t N, float* a0q, float* a1q, float* Eq, float* a1max, float* sdf, float* grad, float* qmax,
                       nsky_stream_t stream);
/* feat = W2f a1 + b2f; albedo = sigmoid(Wc2 relu(Wc1 relu(Wc0 [feat | x PE] + bc0) + bc1) + bc2) -> alb [N, 4] (3 used).  Saves (tile-
 * native, rows = points): a1v [ceil32(N), 256] (optional: value rows of a1), feat [ceil32(N), 256] and xpe [ceil32(N), 128] (columns 0..255
 * and 256..303 of the colour net's input; xpe's columns 48.. are not written), c0, c1 [ceil32(N), 256]. */
int nsky_field_colour_fwd(const nsky_field_net* net, const void* stream_buf, const float* scales, int32_t total_groups, const float* ET,
                          int32_t ldE, int32_t N, const float* a1q, const float* a1max, float* a1v, float* feat, float* xpe, float* c0, float* c1,
                          float* alb, nsky_stream_t stream);
/* g_alb [N, 3] -> dpc2 [N, 4] (output layer's pre-activation gradient, row-major), dpc1 / dpc0 / dfeat (tile-native pre-activation
 * gradients: weight-gradient operands), dxpe [N, 40] (optional: gradient of the encode row's x / PE columns), da1v (tile-native: gradient
 * of a1's value rows from the feature rows), gmax [3] = max |dpc1|, |dpc0|, |dfeat| (caller zero-fills). */
int nsky_field_colour_bwd(const nsky_field_net* net, const void* stream_buf, const float* scales, int32_t total_groups, int32_t N,
                          const float* g_alb, const float* alb, const float* c0, const float* c1, float* dpc2, float* dpc1, float* dpc0,
                          float* dfeat, float* dxpe, float* da1v, float* gmax, nsky_stream_t stream);
/* g_sdf [N], g_grad [N, 3], da1v, dxpe (each optional) -> d1q / d0q (quad-native pre-activation gradients of the two hidden layers),
 * dET [4 N, ldE] (stacked, optional), gmax [2] = max |d1q|, |d0q| (caller zero-fills). */
int nsky_field_geo_bwd(const nsky_field_net* net, const void* stream_buf, const float* scales, int32_t total_groups, int32_t N,
                       const float* g_sdf, const float* g_grad, const float* da1v, const float* dxpe, const float* a0q, const float* a1q,
                       float* d1q, float* d0q, float* dET, int32_t ldE, float* gmax, nsky_stream_t stream);
/* out[o][f] += sum_rows w[row][o] X[row][f] (o < n_out <= 4) over a tile-native X [rows, 32 nt]; bias[o] += sum_rows w[row][o] (optional):
 * the weight gradients of the field's narrow output layers.  w4 [rows, 4] row-major, or (w4 null, n_out 1) the quad form over a
 * quad-native X: w(row) = g_sdf[row / 4] on value rows (the only ones that count for the bias), g_grad[row / 4][row % 4 - 1] on tangent rows. */
int nsky_native_weighted_colsum(const float* X, int32_t nt, int32_t rows, const float* w4, int32_t n_out, const float* g_sdf,
                                const float* g_grad, float* out, int32_t ldo, float* bias, nsky_stream_t stream);
/* DIRECTIONAL mode of the geometry kernels: one forward-mode tangent per point, along a direction d (a pass whose only consumer of the
 * sdf's gradient is its derivative along the ray).  A point is TWO row-sets {value, tangent along d}; PAIR-NATIVE matrices are tile-native
 * [ceil32(2 N), width] whose row 2 n + j is row-set j of point n.  ET: the stacked encode matrix [2 N, ldE] = [E; Td] of
 * nsky_encode_fwd_dir.  Outputs: sdf [N], cosv [N] (d sdf / dx . d), a0q / a1q / Eq pair-native; qmax as nsky_field_geo_fwd.  Same
 * packed weight streams as the quad kernels. */
int nsky_field_geo_fwd_dir(const nsky_field_net* net, const void* stream_buf, const float* scales, int32_t total_groups, const float* ET,
                           int32_t ldE, int32_t N, float* a0q, float* a1q, float* Eq, float* sdf, float* cosv, float* qmax,
                           nsky_stream_t stream);
/* g_sdf [N], g_cos [N] (each optional) -> d1q / d0q (pair-native), dET [2 N, ldE] (stacked [dE; dTd], optional), gmax [2]. */
int nsky_field_geo_bwd_dir(const nsky_field_net* net, const void* stream_buf, const float* scales, int32_t total_groups, int32_t N,
                           const float* g_sdf, const float* g_cos, const float* a0q, const float* a1q, float* d1q, float* d0q, float* dET,
                           int32_t ldE, float* gmax, nsky_stream_t stream);
/* the pair form of nsky_native_weighted_colsum's quad weights over a pair-native X (one output): w(row) = g_sdf[row / 2] on even rows
 * (the only ones that count for the bias), g_cos[row / 2] on odd rows. */
int nsky_native_weighted_colsum_pair(const float* X, int32_t nt, int32_t rows, const float* g_sdf, const float* g_cos, float* out,
                                     int32_t ldo, float* bias, nsky_stream_t stream);

/* Per-ray reductions of the renderers, one pass each way: expected depth clipped to the global [min, max] of the sample mid
 * points and, if max_clamp > 0, to max_clamp (nerfstudio DepthRenderer('expected'); neusky_model.py:591, :1342-1353),
 * accumulation (:595), weighted normal (:812, :1357) and albedo on white (:813).  weights / starts / ends [R,S]; normals / albedo
 * [R,S,3] (optional, with their outputs); sums [R,8] and bounds [2] are scratch kept for the backward: the caller sets bounds to
 * (+inf, -inf) before the forward call. */
int nsky_ray_reduce_fwd(const float* weights, const float* starts, const float* ends, const float* normals, const float* albedo,
                        int32_t R, int32_t S, float max_clamp, float* sums, float* bounds, float* p2p, float* accumulation,
                        float* normal, float* albedo_acc, nsky_stream_t stream);
int nsky_ray_reduce_bwd(const float* weights, const float* starts, const float* ends, const float* normals, const float* albedo,
                        const float* sums, const float* bounds, int32_t R, int32_t S, float max_clamp, const float* d_p2p,
                        const float* d_accumulation, const float* d_normal, const float* d_albedo_acc, float* d_weights,
                        float* d_normals, float* d_albedo, nsky_stream_t stream);


/* NeuS alphas of P isolated samples for three interval lengths each (the hash-grid density probe, neusky_model.py:715-732:
 * nerfstudio SDFField.get_alpha with `deltas` = the three axis gaps broadcast against [P,1]): alphas [P,3]; backward to sdf [P],
 * gradients [P,3] and the variance parameter (d_variance += ; may be NULL).  gap3_host: three floats in HOST memory. */
int nsky_point_alphas_fwd(const float* sdf, const float* grad, const float* dirs, const float* gap3_host, const float* variance, float anneal,
                          int32_t P, float* alphas, nsky_stream_t stream);
int nsky_point_alphas_bwd(const float* sdf, const float* grad, const float* dirs, const float* gap3_host, const float* variance, float anneal,
                          int32_t P, const float* d_alphas, float* d_sdf, float* d_grad, float* d_variance, nsky_stream_t stream);

/* The DDF's output activation (neusky/fields/directional_distance_field.py:297-299): t [n] = scale sigmoid(raw[:, 0]) on the padded
 * [n, ld] head output of the chain; backward d_raw [n, ld] = (d_t scale s (1 - s) | 0 ...). */
int nsky_sigmoid_column_fwd(const float* raw, int32_t ld, int64_t n, float scale, float* t, nsky_stream_t stream);
int nsky_sigmoid_column_bwd(const float* raw, int32_t ld, int64_t n, float scale, const float* d_t, float* d_raw, nsky_stream_t stream);

/* The proposal networks' density MLP (nerfstudio HashMLPDensityField, hidden_dim 16: Linear(in_dim, 16) + ReLU -> Linear(16, 1); called
 * through ProposalNetworkSampler at neusky/models/neusky_model.py:561) on P hash-encoded rows feat [P, ldf]: raw [P] = the density
 * head's pre-activation, both layers in registers.  Backward: d_raw [P] -> d_feat [P, ldf] (optional; pad columns zeroed) and the
 * parameter gradients, ADDED into dw0 [16, ldw0] / db0 [16] / dw1 [16] / db1 [1] (caller zero-fills).  w0 [16, ldw0], w1 [16]: torch
 * nn.Linear layout; hidden must be 16, in_dim <= 12. */
int nsky_proposal_mlp_fwd(const float* feat, int32_t ldf, int64_t P, int32_t in_dim, int32_t hidden, const float* w0, int32_t ldw0,
                          const float* b0, const float* w1, const float* b1, float* raw, nsky_stream_t stream);
int nsky_proposal_mlp_bwd(const float* feat, int32_t ldf, int64_t P, int32_t in_dim, int32_t hidden, const float* w0, int32_t ldw0,
                          const float* b0, const float* w1, const float* b1, const float* d_raw, float* d_feat, float* dw0, float* db0,
                          float* dw1, float* db1, nsky_stream_t stream);
/* Points along rays: out[i] = origins[i] + sign t[i] dirs[i % n_dirs] (the DDF's predicted termination points: ddf_model.py:243,
 * neusky_model.py:1716-1724 with the R x Dv visibility rows sharing their Dv directions), and its backward
 * d_t[i] = sign <d_out[i], dirs[i % n_dirs]> (origins and directions carry no gradient on this path). */
int nsky_ray_points_fwd(const float* origins, const float* dirs, int32_t n_dirs, float sign, const float* t, int64_t n, float* out,
                        nsky_stream_t stream);
int nsky_ray_points_bwd(const float* dirs, int32_t n_dirs, float sign, const float* d_out, int64_t n, float* d_t, nsky_stream_t stream);
/* unit rows of g [P,3] (torch.nn.functional.normalize(p=2, eps=1e-12), sdf_albedo_field.py:256) and its backward */
int nsky_normalize3_fwd(const float* g, int64_t P, float* n, nsky_stream_t stream);
int nsky_normalize3_bwd(const float* g, const float* d_n, int64_t P, float* d_g, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sample generators (replace host-side torch RNG + upload in the reference).  Counter-based RNG (Philox4x32-10) keyed by
 * (seed, *counter); every call advances *counter (a device uint64 the caller owns) by one, so a replayed HIP graph draws
 * fresh numbers.  Distributions follow the reference, RNG streams do not.
 *
 * nsky_ddf_vmf_samples: VMFDDFSampler.generate_ddf_samples (neusky/model_components/ddf_sampler.py:249-286 with
 *   random_vmf :205-247): n_positions points on the unit sphere (z >= 0 when upper_hemisphere), each with n_directions
 *   directions from the vMF lobe (concentration kappa) about its inward normal.  origins [n_positions * n_directions, 3] =
 *   point * radius (repeated), directions likewise. */
int nsky_ddf_vmf_samples(int32_t n_positions, int32_t n_directions, float kappa, float radius, int32_t upper_hemisphere,
                         uint64_t seed, uint64_t* counter, float* origins, float* directions, nsky_stream_t stream);

/* nsky_ddf_fit_rows_fwd: the DDF evaluations of DDFModel.get_outputs (neusky/models/ddf_model.py:193-219 the fit rays,
 *   :279-321 one multi-view ray per fit ray, :324-360 the sky rays), as rows for the DDF network: E = N + (want_mv ? N : 0) + Ns
 *   rows of q_pos [E,3] (sphere positions) and xrow [E,ldx] = [d_loc | NeRF2(d_loc) | 0] (get_localised_transforms :158-181 +
 *   directional_distance_field.py:188-191,270-271).  mv_points_in null: the multi-view points are drawn here (seed, *counter,
 *   advanced by one); mv_points_out [N,3] receives the points used (z folded to >= 0).  sky_gt [Ns] = |o - sphere exit| (:343);
 *   distance_weight [N] (optional) = 1 - (|p| / radius)^weight_exp (:224-238).
 * nsky_ddf_fit_rows_bwd: d_term_dist [N] from d_xrow_mv = gradient of the N multi-view rows (the only differentiable input is the
 *   fit rays' termination distance, :287). */
int nsky_ddf_fit_rows_fwd(const float* positions, const float* directions, const float* term_dist, int32_t N,
                          const float* mv_points_in, uint64_t seed, uint64_t* counter, const float* sky_o, const float* sky_d,
                          int32_t Ns, float radius, int32_t want_mv, float weight_exp, int32_t weight_include_z, float* q_pos,
                          float* xrow, int32_t ldx, float* mv_points_out, float* sky_gt, float* distance_weight, nsky_stream_t stream);
int nsky_ddf_fit_rows_bwd(const float* positions, const float* directions, const float* term_dist, const float* mv_points,
                          int32_t N, const float* d_xrow_mv, int32_t ldx, float* d_term_dist, nsky_stream_t stream);


/* Probe points of the hash-grid density loss (neusky_model.py:704-724): positions [P,3] = lattice + (u gap - gap / 2), u ~ U(0,1)^3,
 * directions [P,3] uniform on the sphere; gap3_host: three floats in HOST memory (the cell size per axis); (seed, *counter): Philox,
 * the counter is advanced by one. */
int nsky_grid_probe_points(const float* lattice, const float* gap3_host, int32_t P, uint64_t seed, uint64_t* counter, float* positions,
                           float* directions, nsky_stream_t stream);

/* HDR output of the RENI++ decoder for the direction grid and the batch's own rays (neusky_model.py:488-549: exp output activation,
 * unnormalised by the per-image scale): raw [U D + R, ldr] (the chain's head output, 3 used columns) ->
 * grid [U D, 3] = exp(raw) scale[u], rays [R, 3] = exp(raw) scale[ray_latent[r]].  _bwd: d_raw [U D + R, ldr] (pad columns zeroed;
 * d_grid / d_rays may be NULL = zero), d_scale [U] += (caller zero-fills; NULL = not wanted). */
int nsky_reni_output_fwd(const float* raw, int32_t ldr, const float* scale, const int64_t* ray_latent, int32_t U, int32_t D, int32_t R,
                         float* grid, float* rays, nsky_stream_t stream);
int nsky_reni_output_bwd(const float* raw, int32_t ldr, const float* scale, const int64_t* ray_latent, int32_t U, int32_t D, int32_t R,
                         const float* d_grid, const float* d_rays, float* d_raw, float* d_scale, nsky_stream_t stream);

/* Illumination directions of one step: IcosahedronSampler with a random rotation (neusky/model_components/illumination_samplers.py:75-110,
 * drawn per step at neusky_model.py:456-458) and the upper-hemisphere subset of the rotated set (neusky_model.py:1650-1657).
 * base [D,3]; rotation_in: a 3x3 row-major matrix, or NULL = drawn from (seed, *counter) (Philox; the counter is advanced by one);
 * dirs [D,3] = base R^T; sel [D/2] = indices of the D/2 largest z, ascending (= the z > 0 subset of a centrally symmetric set);
 * rot_out [9] optional.  D even, <= 1024. */
int nsky_illumination_directions(const float* base, int32_t D, const float* rotation_in, uint64_t seed, uint64_t* counter, float* dirs,
                                 int32_t* sel, float* rot_out, nsky_stream_t stream);
/* RENI++ decoder inputs (the rotation-invariant representation of RENIField, as fed at neusky_model.py:1207-1252): for latent
 * codes Z [U,L,3], a direction set [D,3] and R further (direction, latent index) pairs -- the batch's own rays (:535-549) --
 * rows u D + d (every latent set against every direction), then U D + r, of cond [U D + R, ldcond] = [|Z_xy|, Z_z, Z_xy . d_xy] per
 * latent (3 L columns, pad columns zeroed) and of xrow [.., ldx] = [|d_xy|, d_z | NeRF2(2 freqs, 0..2) of those | 0].
 * _bwd: d_latents [U,L,3] (overwritten) from d_cond. */
int nsky_reni_grid_inputs_fwd(const float* latents, const float* directions, int32_t U, int32_t L, int32_t D, const float* ray_dirs,
                              const int64_t* ray_latent, int32_t R, float* cond, int32_t ldcond, float* xrow, int32_t ldx,
                              nsky_stream_t stream);
int nsky_reni_grid_inputs_bwd(const float* latents, const float* directions, int32_t U, int32_t L, int32_t D, const float* ray_dirs,
                              const int64_t* ray_latent, int32_t R, const float* d_cond, int32_t ldcond, float* d_latents,
                              nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multiresolution hash-grid encode (tiny-cuda-nn HashGrid semantics, fp32) fused with the rest of
 * the MLP input row.  Replaces tcnn.Encoding + NeRFEncoding + torch.cat at
 *   neusky/fields/sdf_albedo_field.py:119-130 (+ inherited forward_geonetwork, called :172,180,233)
 *   neusky/fields/directional_distance_field.py:146-156, :267-268
 * and, with `tangents`, the forward-mode input Jacobian that the reference obtains with
 * torch.autograd.grad(sdf, inputs, create_graph=True) (sdf_albedo_field.py:235-238).
 *
 * Row layout written to Y (ldy >= width, pad columns are zeroed):
 *   [ x (3, if include_x) | PE: sin(2 pi x_i 2^e_f) (3*pe_freqs), sin(.. + pi/2) (3*pe_freqs) | hash features (2*L) ]
 *   with e_f = f * pe_max_exp / (pe_freqs - 1)  (nerfstudio NeRFEncoding, min_freq_exp = 0)
 * mode: 0 = feed x raw to the grid (DDF); 1 = (contract_Linf(x)+2)/4; 2 = (contract_L2(x)+2)/4.
 * T (optional): three more row blocks [3][P][ldy], d(row)/d(x_k).
 */
typedef struct nsky_hashgrid_desc {
  const float* table;      /* [offset[L]][2] */
  int32_t n_levels;        /* <= 16, 2 features per level */
  int32_t smoothstep;      /* 1: Smoothstep interpolation, 0: Linear */
  float scale[16];
  int32_t resolution[16];
  uint32_t offset[17];     /* rows; level l owns rows offset[l]..offset[l+1] */
} nsky_hashgrid_desc;

int nsky_encode_fwd(const nsky_hashgrid_desc* g, const float* x, int32_t P, int32_t mode, int32_t include_x,
                    int32_t pe_freqs, float pe_max_exp, float* Y, int32_t ldy, float* T, nsky_stream_t stream);

/* Backward of nsky_encode_fwd.  dY [P,lddy] = gradient w.r.t. the rows; dT (optional) [3][P][lddy] =
 * gradient w.r.t. the tangent rows (second-order path: eikonal / normals).  Accumulates (float adds, order not
 * fixed) into dtable [offset[L]][2] (NULL: a frozen table, only dx is formed); dx (optional, [P,3], overwritten) = dY . d(row)/dx.
 * workspace (optional): nsky_encode_bwd_workspace_bytes(g, P, dT != NULL) bytes of scratch, 256-byte aligned; with it, and at
 * least NSKY_ENCODE_BWD_OWNER_MIN_POINTS points, the table gradient is accumulated by chunk-owning workgroups in LDS
 * instead of by global atomics (same result up to the order of the float adds). */
#define NSKY_ENCODE_BWD_OWNER_MIN_POINTS 32768
int64_t nsky_encode_bwd_workspace_bytes(const nsky_hashgrid_desc* g, int32_t P, int32_t tangents);
int nsky_encode_bwd(const nsky_hashgrid_desc* g, const float* x, int32_t P, int32_t mode, int32_t include_x,
                    int32_t pe_freqs, float pe_max_exp, const float* dY, int32_t lddy, const float* dT, float* dtable,
                    float* dx, void* workspace, nsky_stream_t stream);
/* Directional mode: ONE tangent row-set along a per-ray direction, Td = sum_a d_a T_a [P, ldy] (stacked with Y: [Y; Td]), formed in
 * registers from the three per-axis terms.  dirs [ceil(P / spr), 3]: point p takes direction p / spr (spr samples per ray; 1 = one
 * direction per point).  The backward takes dTd [P, lddy] and adds to dtable what nsky_encode_bwd adds for dT_a = d_a dTd (workspace as
 * for a tangent call of nsky_encode_bwd); positions get no gradient. */
int nsky_encode_fwd_dir(const nsky_hashgrid_desc* g, const float* x, int32_t P, int32_t mode, int32_t include_x, int32_t pe_freqs,
                        float pe_max_exp, const float* dirs, int32_t spr, float* Y, int32_t ldy, float* Td, nsky_stream_t stream);
int nsky_encode_bwd_dir(const nsky_hashgrid_desc* g, const float* x, int32_t P, int32_t mode, int32_t include_x, int32_t pe_freqs,
                        float pe_max_exp, const float* dirs, int32_t spr, const float* dY, int32_t lddy, const float* dTd,
                        float* dtable, void* workspace, nsky_stream_t stream);

/* corner rows (uint32 [P][L][8]) exactly as the encode kernels address the table - the integer
 * part of the hash encode, exposed for BIT-EXACT parity tests. */
int nsky_hash_indices(const nsky_hashgrid_desc* g, const float* x, int32_t P, int32_t mode, uint32_t* idx,
                      nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Hemisphere integral + alpha composite + sRGB on COMPACT inputs.  Replaces
 * RGBLambertianRendererWithVisibility.render_and_combine_rgb, neusky/model_components/renderers.py:60-130
 * (and the [R*S,D,*] broadcasts built at neusky/models/neusky_model.py:512-525, 1755-1759).
 *   albedo, normals [R,S,3]; weights [R,S]; dirs [D,3]; cam_colours [U,D,3]; cam_of_ray [R] (row of cam_colours);
 *   vis [R,D] or NULL; bg [R,3]  ->  rgb [R,3] (sRGB, clamped to [0,1]); lin [R,3] (optional: linear composite,
 *   needed by the backward).  D <= 1024.
 */
int nsky_hemi_composite_fwd(const float* albedo, const float* normals, const float* weights, const float* dirs,
                            const float* cam_colours, const int32_t* cam_of_ray, const float* vis, const float* bg,
                            int32_t R, int32_t S, int32_t D, float* rgb, float* lin, nsky_stream_t stream);
/* d_cam_colours [U,D,3] is ACCUMULATED (atomic adds; zero it first); d_vis / d_cam_colours may be NULL. */
int nsky_hemi_composite_bwd(const float* albedo, const float* normals, const float* weights, const float* dirs,
                            const float* cam_colours, const int32_t* cam_of_ray, const float* vis, const float* bg,
                            const float* lin, const float* d_rgb, int32_t R, int32_t S, int32_t D, float* d_albedo,
                            float* d_normals, float* d_weights, float* d_cam_colours, float* d_vis, float* d_bg,
                            nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * NeuS alpha -> transmittance -> weights (+ accumulation, expected depth).  Replaces nerfstudio
 * SDFField.get_alpha (called neusky/fields/sdf_albedo_field.py:266), RaySamples.get_weights_and_
 * transmittance_from_alphas (neusky/models/neusky_model.py:565-568) and the accumulation / expected-depth
 * renderers (:591-595).  sdf, starts, ends [R,S]; grad [R,S,3]; ray_dirs [R,3]; variance: device scalar
 * (LearnedVariance parameter; inv_s = clip(exp(10 v), 1e-6, 1e6)).  S <= 256.
 * depth is sum(w mid)/(sum(w)+1e-10) WITHOUT the batch-global clip to [min mid, max mid] (host applies it).
 */
int nsky_neus_weights_fwd(const float* sdf, const float* grad, const float* ray_dirs, const float* starts,
                          const float* ends, const float* variance, float cos_anneal, int32_t R, int32_t S,
                          float* alpha, float* weights, float* trans_bg, float* accumulation, float* depth,
                          nsky_stream_t stream);
/* d_variance (device scalar) is ACCUMULATED. */
int nsky_neus_weights_bwd(const float* sdf, const float* grad, const float* ray_dirs, const float* starts,
                          const float* ends, const float* variance, float cos_anneal, int32_t R, int32_t S,
                          const float* d_weights, const float* d_trans_bg, float* d_sdf, float* d_grad,
                          float* d_variance, nsky_stream_t stream);
/* The same with the gradient as ONE precomputed column: cosv [R,S] = ray_dir . grad(sdf) (the directional field pass); the backward
 * writes d_cos [R,S]. */
int nsky_neus_weights_cos_fwd(const float* sdf, const float* cosv, const float* starts, const float* ends, const float* variance,
                              float cos_anneal, int32_t R, int32_t S, float* alpha, float* weights, float* trans_bg,
                              float* accumulation, float* depth, nsky_stream_t stream);
int nsky_neus_weights_cos_bwd(const float* sdf, const float* cosv, const float* starts, const float* ends, const float* variance,
                              float cos_anneal, int32_t R, int32_t S, const float* d_weights, const float* d_trans_bg, float* d_sdf,
                              float* d_cos, float* d_variance, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DDF sky-visibility ray set-up and sigmoid.  Replaces the geometry of NeuSkyFactoModel.compute_visibility,
 * neusky/models/neusky_model.py:1667-1709 (surface point incl. the outside-sphere fix-up :1674-1683,
 * ray_sphere_intersection :1590-1622) + DDFModel.get_localised_transforms / einsum, neusky/models/ddf_model.py:158-200
 * + the NeRF direction encoding, neusky/fields/directional_distance_field.py:188-191,270-271.
 *   origins, ray_dirs [R,3]; depth [R]; sel_dirs [Dv,3] (the upper-hemisphere subset, :1650-1657)
 *   -> sphere_pts [R*Dv,3]; xrow [R*Dv,ldx] = [d_loc | NeRF2(d_loc) | 0]; surf_dist [R*Dv] = min(|x-p|, 2r) (:1724-1727);
 *      term_dist [R*Dv] (optional, :1697).
 */
int nsky_visibility_rays(const float* origins, const float* ray_dirs, const float* depth, const float* sel_dirs,
                         int32_t R, int32_t Dv, float radius, float* sphere_pts, float* xrow, int32_t ldx,
                         float* surf_dist, float* term_dist, nsky_stream_t stream);
/* vis[r, sel_index[j]] = 1 - sigmoid(scale * (surf_dist - t_hat - threshold))  (:1730-1740); the caller pre-fills
 * vis [R,D] with the lower-hemisphere constant (:1745-1748).  threshold: device scalar. */
int nsky_visibility_finish_fwd(const float* t_hat, const float* surf_dist, const float* threshold, float scale,
                               const int32_t* sel_index, int32_t R, int32_t Dv, int32_t D, float* vis,
                               nsky_stream_t stream);
/* d_threshold (device scalar) is ACCUMULATED. */
int nsky_visibility_finish_bwd(const float* t_hat, const float* surf_dist, const float* threshold, float scale,
                               const int32_t* sel_index, int32_t R, int32_t Dv, int32_t D, const float* d_vis,
                               float* d_t_hat, float* d_threshold, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Interlevel (proposal) loss, nerfstudio interlevel_loss as neusky/models/neusky_model.py:987-988 calls it.
 *   c [R,S+1] final spacing bins, w [R,S] final weights (both constants), sb [R,n+1] / wp [R,n] one proposal level.
 *   per_ray[r] = sum_s max(w_s - w_outer_s, 0)^2 / (w_s + 1e-7)   (the loss term is mean over R*S = sum(per_ray)/(R S))
 * Backward: d_per_ray [R] -> d_wp [R,n] (every element written).  n <= 4096.
 */
int nsky_interlevel_fwd(const float* c, const float* w, const float* sb, const float* wp, int32_t R, int32_t S, int32_t n,
                        float* per_ray, nsky_stream_t stream);
int nsky_interlevel_bwd(const float* c, const float* w, const float* sb, const float* wp, const float* d_per_ray, int32_t R,
                        int32_t S, int32_t n, float* d_wp, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Ray set-up of the proposal sampler (nerfstudio SphereCollider + UniformSampler + the spacing->euclidean map and
 * bin mid-points that ProposalNetworkSampler applies between levels; driven from neusky/models/neusky_model.py:213,561).
 * No gradient flows through any of these.
 *   nsky_sphere_collider : origins, directions [R,3] -> nears, fars [R] against the sphere |x| = radius
 *                          (nears >= near_plane, fars >= nears + 1e-6; rays that miss get [near_plane, near_plane + 1e-6])
 *   nsky_uniform_bins    : sbins [R,n+1] = linspace(0,1,n+1) jittered inside its own bin by jitter[R] (NULL: plain
 *                          lattice), ebins = sbins * far + (1 - sbins) * near
 *   nsky_bins_to_samples : sbins [R,n+1] -> ebins [R,n+1] (optional) and positions [R,n,3] = o + d (e_i + e_{i+1}) / 2
 *                          (optional)
 */
int nsky_sphere_collider(const float* origins, const float* directions, int32_t R, float radius, float near_plane, float* nears,
                         float* fars, nsky_stream_t stream);
int nsky_uniform_bins(const float* nears, const float* fars, const float* jitter, int32_t R, int32_t n, float* sbins, float* ebins,
                      nsky_stream_t stream);
int nsky_bins_to_samples(const float* sbins, const float* nears, const float* fars, const float* origins, const float* directions,
                         int32_t R, int32_t n, float* ebins, float* positions, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Proposal-network weights: nerfstudio HashMLPDensityField's trunc_exp density + RaySamples.get_weights, as the proposal
 * sampler drives them (neusky/models/neusky_model.py:561).  raw [R*n] with element stride ld_raw (the padded output of
 * the 1-wide density head), ebins [R,n+1] euclidean bin edges -> weights [R,n] =
 * nan_to_num((1 - exp(-delta sigma)) exp(-cumsum_excl(delta sigma))), sigma = exp(raw).  n <= 256.
 * Backward writes d_raw with the same stride (the ld_raw-1 pad columns are zero-filled).
 */
int nsky_density_weights_fwd(const float* raw, int32_t ld_raw, const float* ebins, int32_t R, int32_t n, float* weights,
                             nsky_stream_t stream);
int nsky_density_weights_bwd(const float* raw, int32_t ld_raw, const float* ebins, const float* d_weights, int32_t R, int32_t n,
                             float* d_raw, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Reverse-over-forward step of one Softplus layer that carries three input tangents.  Together with
 * nsky_gemm_f32 (NSKY_EPI_MUL_AUX) this replaces the double backward that the reference gets from
 * torch.autograd.grad(..., create_graph=True) at neusky/fields/sdf_albedo_field.py:235-238 feeding the eikonal
 * loss (neusky/models/neusky_model.py:958-960) and the shading normals (:251).
 *   s = sigmoid(beta z) [N,ld]; ta = tangent activations [3][N,ld]; da (optional) [N,ld];
 *   dta [3][N,ld]  OR  the outer product ggrad[N,3] x wvec[C];   out: dz [N,ld], du [3][N,ld];
 *   wsum (optional, outer-product form only) [C] += sum_{n,k} ggrad[n,k] ta_k[n,:] = the gradient of wvec, from the same pass.
 */
int nsky_softplus_tangent_bwd(const float* da, const float* s, const float* ta, const float* dta, const float* ggrad,
                              const float* wvec, float beta, int32_t N, int32_t C, int32_t ld, float* dz, float* du,
                              float* wsum, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Proposal PDF re-sampling: nerfstudio PDFSampler.generate_ray_samples as driven by
 * ProposalNetworkSampler (called at neusky/models/neusky_model.py:561).  weights [R,n0] (already annealed),
 * bins [R,n0+1] (spacing domain), u_base [nb] = linspace(0, 1-1/nb, nb) (+ 1/(2nb) when not stratified),
 * jitter [R] in [0,1) or NULL  ->  new_bins [R,nb], inds [R,nb] (optional; searchsorted(cdf,u,right)).
 * The CDF is accumulated sequentially in fp32, so inds are bit-reproducible against the oracle.
 */
int nsky_pdf_sample(const float* weights, const float* bins, const float* u_base, const float* jitter, int32_t R,
                    int32_t n0, int32_t nb, float histogram_padding, float eps, float* new_bins, int32_t* inds,
                    nsky_stream_t stream);

/*
 * Weight-norm parameterisation of the SDF / colour layers (nn.utils.weight_norm as nerfstudio's SDFField applies it;
 * used by neusky/fields/sdf_albedo_field.py:147-161 for the colour net and the inherited geo net), fused with the row /
 * column re-ordering and zero padding the consuming GEMMs want:
 *   out[r][c] = g[sr] * v[sr][sc] / ||v[sr]||_2,  sr = row_map[r], sc = col_map[c]; -1 marks a structural zero.
 * v [out_features, in_features] (ldv), g [out_features], inv_norm [out_features] (written; saved for the backward).
 * Every source row must appear at most once in row_map, every source column at most once in col_map.
 * Backward: d_out [n_rows_out, ldo] -> dv [out_features, ldv-strided rows listed in row_map], dg [out_features];
 * inverse_col[sc] = output column reading source column sc, or -1.  Rows of v absent from row_map are not written.
 */
int nsky_weight_norm_fwd(const float* v, const float* g, int32_t n_rows_out, int32_t n_cols_out, int32_t in_features,
                         int32_t ldv, const int32_t* row_map, const int32_t* col_map, float* out, int32_t ldo,
                         float* inv_norm, nsky_stream_t stream);
int nsky_weight_norm_bwd(const float* d_out, int32_t ldo, const float* v, const float* g, const float* inv_norm,
                         int32_t n_rows_out, int32_t in_features, int32_t ldv, const int32_t* row_map,
                         const int32_t* inverse_col, float* dv, float* dg, nsky_stream_t stream);

/* Copies n_segments float runs (src -> dst, n floats each) in one launch: the parameter gradients autograd keeps in tensors of its
 * own (torch's AccumulateGrad with an undefined .grad) into their places in the optimizer's gradient slab, instead of one add
 * kernel per parameter (nerfstudio Optimizers.zero_grad_all / optimizer_scheduler_step_all around neusky_config.py:216-237). */
typedef struct { const float* src; float* dst; int64_t n; } nsky_segment;
int nsky_gather_segments(const nsky_segment* segments, int32_t n_segments, nsky_stream_t stream);
/* The same for byte runs of any element type (host arrays of device pointers and byte counts): the next step's input tensors into the
 * static buffers a captured graph reads (nerfstudio's datamanager.next_train hand-over), one launch instead of one copy per tensor. */
int nsky_copy_segments(const void* const* src, void* const* dst, const int64_t* nbytes, int32_t n_segments, nsky_stream_t stream);

/* Adam update (torch.optim.Adam semantics, no weight decay / amsgrad) over a flat slab of n floats;
 * the five optimizer groups of neusky/configs/neusky_config.py:216-237.  grad_scale multiplies g first.  The hyper-parameters are
 * DOUBLES (ABI 16): torch forms 1 - beta, lr / (1 - beta1^t) and sqrt(1 - beta2^t) in double from the Python scalars and rounds each to
 * float once; a float beta2 = 0.999 already puts 1 - beta2 off by 1.3e-5 relative. */
int nsky_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                   double eps, int32_t step, float grad_scale, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Closed-form loss terms, one launch each way per model (instead of ~300 small torch launches per step).
 * NeuSky model, train branch of get_loss_dict, neusky/models/neusky_model.py:933-1035 (+ RENISkyPixelLoss,
 * neusky/model_components/losses.py:44-58, linear_to_sRGB neusky/utils/utils.py:25-30, nerfstudio monosdf_normal_loss):
 *   terms[8] = { rgb_l1 (:947-950), eikonal (:958-960), fg_mask BCE (:963-967), hashgrid density L1 (:990-993),
 *                ground-plane normal (:995-1000), sky pixel (:1002-1009), visibility-threshold MSE (:1011-1030),
 *                sdf level set (:1032-1035) }, UNSCALED (the coefficients are applied by the caller); a term whose input
 *   pointer is NULL is left 0.  wsum [R] (side output) = per-ray weight sums, needed by the backward.
 *   Backward: d_terms[8] -> gradients (every element written) for the inputs whose output pointer is non-NULL.
 */
typedef struct nsky_main_losses_desc {
  int32_t R, S, P, M;     /* rays, samples per ray, hash-grid probe points, sdf-at-termination rows */
  const float* rgb;       /* [R,3] rendered radiance */
  const float* image;     /* [R,3] */
  const float* mask;      /* [R,4] float {static, fg, ground, sky} (neusky_dataset.py:290) */
  const float* eik;       /* [R*S,3] sdf gradients */
  const float* weights;   /* [R,S] */
  const float* normal;    /* [R,3] rendered normals */
  const float* hdr_bg;    /* [R,3] linear HDR background */
  const float* grid;      /* [P*3] hash-grid probe alphas */
  const float* sdf_term;  /* [M] */
  const float* vis_thr;   /* [1] learnable visibility threshold */
  float sky_alpha, vis_target;
} nsky_main_losses_desc;
int nsky_main_losses_fwd(const nsky_main_losses_desc* d, float* terms, float* wsum, nsky_stream_t stream);
int nsky_main_losses_bwd(const nsky_main_losses_desc* d, const float* wsum, const float* d_terms, float* d_rgb, float* d_eik,
                         float* d_weights, float* d_normal, float* d_hdr_bg, float* d_grid, float* d_sdf_term, float* d_vis_thr,
                         nsky_stream_t stream);


/* Scalar training metrics of a model in one launch: out[0] = 10 log10(peak_sq / mean(((pred - gt) mask)^2)) over n elements (mask
 * optional: PSNR of neusky_model.py:1066-1068 with peak 1; depth PSNR of ddf_model.py:381-405 with peak = the DDF radius and the batch
 * mask); with variance (the NeuS deviation parameter, 1 float): out[1] = clip(exp(10 v), 1e-6, 1e6), out[2] = 1 / out[1]
 * (neusky_model.py:1071-1072).  None of it is differentiated. */
int nsky_train_metrics(const float* pred, const float* gt, const float* mask, int64_t n, float peak_sq, const float* variance, float* out,
                       nsky_stream_t stream);
/* Attention core of the RENI++ transformer decoder -- the illumination model the reference configures (neusky/configs/neusky_config.py:78-95:
 * conditioning="Attention", VN invariance, SO2 about z, 8 heads x 6 layers, hidden 128) and decodes at neusky/models/neusky_model.py:488-506,
 * 535-549.  The `reni` package holding the decoder is absent from the reference tree: the arithmetic follows the published architecture as
 * restated in oracle/neusky_oracle.py:reni_attention_decode (PARITY UNPINNED).  For every camera u, direction d and head h (head width 16):
 *     q~ = scale * [d_x q | d_y q | q],   s_n = q~ . K~[u,h,n],   p = softmax_n(s),   o = d_x (p V~)[0:16] + d_y (p V~)[16:32] + (p V~)[32:48]
 * with K~, V~ [U, n_heads, L, 48] the per-camera key / value parts (the token is linear in (d_x, d_y): three 16-wide parts per token, L <= 128),
 * Q, O, dO, dQ [U, D, 16 n_heads] row-major, dirs [U, D, 3], row_max / row_sum [U, n_heads, D] (saved by the forward for the backward).
 * Replaces the per-head `softmax(Q K^T) V` of the decoder's cross-attention (two batched matrix products, a softmax and their autograd nodes per
 * layer).  Arithmetic: D >= 32 rows per camera: matrix cores, fp32-grade fp16 hi + residual products (the chain kernels' arithmetic); a camera's
 * short blocks (a ray's own row): exact fp32 on the vector units.  _bwd returns dQ and the per-camera dK~, dV~ (summed over the camera's D rows); directions carry no gradient. */
int nsky_attn_core_fwd(const float* Q, const float* dirs, const float* Kt, const float* Vt, int32_t U, int32_t D, int32_t L, int32_t n_heads,
                       float scale, float* O, float* row_max, float* row_sum, nsky_stream_t stream);
int nsky_attn_core_bwd(const float* Q, const float* dirs, const float* Kt, const float* Vt, const float* O, const float* row_max,
                       const float* row_sum, const float* dO, int32_t U, int32_t D, int32_t L, int32_t n_heads, float scale, float* dQ,
                       float* dKt, float* dVt, float* drow_scratch /* U n_heads (D + 4) floats: D = dO . O per row and head, then the operand maxima of every (camera, head) */,
                       nsky_stream_t stream);
/* The rays' own rows of the same decoder (the background radiance along a ray's own direction, neusky_model.py:535-549): a ray attends to
 * the keys / values of ITS camera.  Q, O, dO, dQ [R, 16 n_heads], dirs [R, 3], row_max / row_sum [R, n_heads]; the rays sorted by camera:
 * perm[i] = the ray at sorted position i, seg[u] .. seg[u + 1] the positions of camera u (seg [U + 1]).  _bwd ADDS the rays' part to
 * dKt / dVt (which hold the grid rows' sums from nsky_attn_core_bwd, launched earlier on the same stream).  Exact fp32 on the vector units.
 * Replaces decoding the rays as R one-direction cameras (which projects R x 3 L token rows per layer). */
int nsky_attn_core_rays_fwd(const float* Q, const float* dirs, const int32_t* perm, const int32_t* seg, const float* Kt, const float* Vt, int32_t U,
                            int32_t R, int32_t L, int32_t n_heads, float scale, float* O, float* row_max, float* row_sum, nsky_stream_t stream);
int nsky_attn_core_rays_bwd(const float* Q, const float* dirs, const int32_t* perm, const int32_t* seg, const float* Kt, const float* Vt, const float* O,
                            const float* row_max, const float* row_sum, const float* dO, int32_t U, int32_t R, int32_t L, int32_t n_heads, float scale,
                            float* dQ, float* dKt, float* dVt, nsky_stream_t stream);
/* Residual add + layer norm of the decoder's row stream ([M, W] row-major, W = 64, 128, 256 or 512): s = x + r (r NULL: s = x, not stored),
 * y = LayerNorm(s) gamma + beta (biased variance, eps inside the root: torch.nn.LayerNorm), stats [M, 2] = (mean, rstd) of every row.
 * _bwd, for frozen gamma / beta (the RENI++ decoder is fixed, neusky_config.py:87): ds = d LayerNorm / d s (dy) + ds_in (ds_in NULL: none) --
 * the gradient of x and of r alike.  Replace torch's add + native_layer_norm (+ their backward nodes) of every decoder block. */
int nsky_add_layer_norm_fwd(const float* x, const float* r, const float* gamma, const float* beta, int64_t M, int32_t W, float eps, float* s, float* y,
                            float* stats, nsky_stream_t stream);
int nsky_add_layer_norm_bwd(const float* s, const float* stats, const float* gamma, const float* dy, const float* ds_in, int64_t M, int32_t W, float* ds,
                            nsky_stream_t stream);
/* The step's objective: total = sum over segments of scale_s * sum_i coef_s[i] x_s[i] (coef NULL: 1).  Replaces the dozen scalar
 * multiplies, sums and adds that scale and merge the loss dictionaries (nerfstudio scale_dict + functools.reduce(torch.add, ...),
 * neusky_pipeline.py:283-289; interlevel_loss' mean, neusky_model.py:987-988) by one launch each way.  One workgroup; bwd writes
 * grad_s[i] = g[0] * scale_s * coef_s[i] for every segment whose grad pointer is set. */
#define NSKY_TOTAL_MAX_SEGMENTS 8
typedef struct nsky_total_segment {
  const float* x;      /* [n] */
  const float* coef;   /* [n] or NULL */
  float* grad;         /* [n] or NULL (bwd) */
  int32_t n;
  float scale;
} nsky_total_segment;
int nsky_weighted_total_fwd(const nsky_total_segment* segments, int32_t n_segments, float* total, nsky_stream_t stream);
int nsky_weighted_total_bwd(const nsky_total_segment* segments, int32_t n_segments, const float* g, nsky_stream_t stream);
/* DDF model, get_loss_dict, neusky/models/ddf_model.py:407-493:
 *   terms[5] = { depth L1 x scene-centre weight (:427-433), sdf L2, sdf L1, multi-view hinge^2 with the reference's
 *                [M] - [M,1] -> [M,M] broadcast (:475-483), sky-ray L1 (:485-490) }, unscaled. */
typedef struct nsky_ddf_losses_desc {
  int32_t Mr, Mm, Ms;          /* fit rays, multi-view rays, sky rays */
  const float* expected;       /* [Mr] expected termination distance */
  const float* term;           /* [Mr] target termination distance */
  const float* mask;           /* [Mr] */
  const float* dist_weight;    /* [Mr] or NULL */
  const float* sdf;            /* [Mr] sdf at termination or NULL */
  const float* mv_expected; const float* mv_term;    /* [Mm] */
  const float* sky_expected; const float* sky_term;  /* [Ms] */
  int32_t want_depth, want_sdf_l2, want_sdf_l1, mask_to_circumference, inverse_depth_weight;
  float radius;
} nsky_ddf_losses_desc;
int nsky_ddf_losses_fwd(const nsky_ddf_losses_desc* d, float* terms, nsky_stream_t stream);
/* d_term / d_mv_term: gradients w.r.t. the target distances (the field's own rendering of the fit rays; NULL when the pipeline
 * detached them, neusky_pipeline.py stop_sdf_gradients) */
int nsky_ddf_losses_bwd(const nsky_ddf_losses_desc* d, const float* d_terms, float* d_expected, float* d_sdf, float* d_mv_expected,
                        float* d_sky_expected, float* d_term, float* d_mv_term, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Marching cubes over a dense fp32 volume [nx, ny, nz] (C-contiguous, z fastest; every dimension >= 2).  No counterpart in the
 * reference (it has no mesh export); the package's exporter (neusky_amd/exporter) drives these three passes.
 *   inside: value < level.  Point (i, j, k) owns its +x, +y, +z edges; one vertex per owned edge whose ends differ, at
 *   t = (level - v_a) / (v_b - v_a).  Vertices ordered by owner flat index, then axis; faces by cell (= its minimum point's) flat
 *   index, then case-table order; faces wind counter-clockwise seen from the outside (increasing value) side.
 *   Points are processed in tiles of NSKY_MC_TILE consecutive flat indices; n_tiles = ceil(nx ny nz / NSKY_MC_TILE).
 * nsky_mc_count:    tile_counts[4][n_tiles] = { vertices, faces, non-finite values, 0 } of each tile (rows: scanned in place by the
 *                   caller, an inner-dimension scan).
 * nsky_mc_vertices: tile_vertex_offsets[n_tiles] = exclusive scan of the tile vertex counts; writes vertices[V][3] (point
 *                   (i, j, k) at box_min + (i, j, k) / (n - 1) * (box_max - box_min)), base[nx ny nz] (first vertex id of each
 *                   point) and edge_mask[nx ny nz] (bit a: the point's +a edge crosses).
 * nsky_mc_faces:    tile_face_offsets[n_tiles] = exclusive scan of the tile face counts; writes faces[F][3] (vertex ids).
 * V and F must fit int32 (the caller checks the totals before the second pass). */
#define NSKY_MC_TILE 256
int nsky_mc_count(const float* volume, int64_t nx, int64_t ny, int64_t nz, float level, int32_t* tile_counts, nsky_stream_t stream);
int nsky_mc_vertices(const float* volume, int64_t nx, int64_t ny, int64_t nz, float level, float min_x, float min_y, float min_z,
                     float max_x, float max_y, float max_z, const int64_t* tile_vertex_offsets, int32_t* base, uint8_t* edge_mask,
                     float* vertices, nsky_stream_t stream);
int nsky_mc_faces(const float* volume, int64_t nx, int64_t ny, int64_t nz, float level, const int64_t* tile_face_offsets,
                  const int32_t* base, const uint8_t* edge_mask, int32_t* faces, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mesh simplification by vertex clustering with quadric-error placement (Lindstrom, "Out-of-core simplification of large polygonal
 * models", SIGGRAPH 2000).  No counterpart in the reference; neusky_amd/exporter/simplify.py drives these kernels (csrc/simplify.hip).
 *   inputs:   vertices [V][3] fp32, faces [F][3] int32 (V, F fit int32), optional normals [V][3] fp32 and colours [V][3] uint8; a grid
 *             origin lo and a cell edge h > 0 (doubles).  All arithmetic is float64 on the fp32 inputs, coordinates relative to lo;
 *             results are rounded to fp32 once, at the end.
 *   1 cell:   i_a = clamp(floor((p_a - lo_a) / h), 0, 2^21 - 1) per axis; key = i_x << 42 | i_y << 21 | i_z (int64).  Output vertex j is
 *             the j-th occupied cell in ascending key order (its rank).
 *   2 face:   corners a, b, c; m = (b - a) x (c - a); |m| = 0 contributes nothing; else n = m / |m|, w = |m| / 2, d = n.a and the face
 *             adds A += w n n^T, b += w d n, c += w d^2 to the cell of each of its three corners (three records per face, also when
 *             corners share a cell).
 *   3 place:  xbar = mean of the cell's vertices; A = sum_i lambda_i e_i e_i^T; x = xbar + sum_{i: lambda_i > tau lambda_max}
 *             e_i e_i^T (b - A xbar) / lambda_i with tau = NSKY_MESH_TAU; x = xbar when lambda_max <= 0 or when x leaves the cell's box
 *             [i h, (i + 1) h] on any axis.
 *   4 faces:  every index becomes its cell's rank; a face with two equal indices is dropped; survivors are rotated (orientation kept)
 *             so that the smallest index leads; of identical triples the first in input order stays; survivors keep the input order.
 *   5 attrib: the cell's normal is the normalised sum of its vertices' normals ((0,0,1) for a zero sum), its colour the mean of its
 *             vertices' colours rounded to nearest (ties to even).
 *   6 repeat: no floating-point atomics.  A cell's sums run over records brought together by stable sorts (its vertices in ascending
 *             vertex index; its face records 3 f + corner in ascending order): lane l of a group of G lanes adds records l, l + G, ...
 *             in that order, then an xor butterfly adds the G partials.  Two runs on one input agree bit for bit.
 * nsky_mesh_cell_keys:       keys[V] of all vertices.
 * nsky_mesh_cluster_count:   *count += the faces whose three corners lie in three different cells of (lo, h); the caller zeroes *count
 *                            (int64, device memory).  No sort, no scratch; an integer atomic per workgroup.
 * nsky_mesh_vertex_cells:    vertex_order[V] = the permutation of a stable ascending sort of the keys, rank_sorted[V] = the rank of
 *                            each sorted entry's cell  ->  vertex_cell[V] (int32), the rank of every vertex's cell.
 * nsky_mesh_remap_faces:     corner_cells[F][3] = the cell ranks of every face's corners (-1 for an index outside [0, V));
 *                            face_keys[F] = smallest << 32 | its successor in the rotated face, -1 for a dropped face.
 * nsky_mesh_cluster_reduce:  cell_start[C + 1] = first sorted vertex of each cell; sorted_corner_cells[3 F] / corner_order[3 F] = the
 *                            stable ascending sort of corner_cells (flat) and its permutation.  cell_sums[C][NSKY_MESH_CELL_SUMS] =
 *                            A00 A01 A02 A11 A12 A22, b0 b1 b2, c, sum (p - lo) [3], sum normals [3], sum colours [3], vertex count.
 *                            normals / colours may be NULL (zero sums).  group: lanes per cell, 8 or 64; 0 picks 64 when a cell holds
 *                            more than NSKY_MESH_WIDE_GROUP_RECORDS records ((3 F + V) / C) on average, else 8.
 * nsky_mesh_cluster_solve:   cell_keys[C] = the occupied cells' keys ascending  ->  vertices_out[C][3] and, unless NULL, normals_out[C][3]
 *                            and colours_out[C][3].  Cyclic Jacobi, a fixed number of sweeps.
 * nsky_mesh_flag_duplicates: sorted_keys[F] / face_order[F] = the stable ascending sort of face_keys and its permutation  ->  keep[F]
 *                            (int32 0 / 1): not dropped and not a repetition of an earlier face.
 * nsky_mesh_compact_faces:   ends[F] = inclusive scan of keep, F_out = ends[F - 1]  ->  faces_out[F_out][3], rotated. */
#define NSKY_MESH_KEY_BITS 21
#define NSKY_MESH_TAU 1e-3
#define NSKY_MESH_CELL_SUMS 20
#define NSKY_MESH_WIDE_GROUP_RECORDS 1024
int nsky_mesh_cell_keys(const float* vertices, int64_t V, double lo_x, double lo_y, double lo_z, double h, int64_t* keys,
                        nsky_stream_t stream);
int nsky_mesh_cluster_count(const float* vertices, int64_t V, const int32_t* faces, int64_t F, double lo_x, double lo_y, double lo_z,
                            double h, int64_t* count, nsky_stream_t stream);
int nsky_mesh_vertex_cells(const int64_t* vertex_order, const int64_t* rank_sorted, int64_t V, int32_t* vertex_cell, nsky_stream_t stream);
int nsky_mesh_remap_faces(const int32_t* faces, int64_t F, const int32_t* vertex_cell, int64_t V, int32_t* corner_cells,
                          int64_t* face_keys, nsky_stream_t stream);
int nsky_mesh_cluster_reduce(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* normals,
                             const uint8_t* colours, double lo_x, double lo_y, double lo_z, double h, const int64_t* vertex_order,
                             const int64_t* cell_start, int64_t C, const int32_t* sorted_corner_cells, const int64_t* corner_order,
                             int32_t group, double* cell_sums, nsky_stream_t stream);
int nsky_mesh_cluster_solve(const double* cell_sums, const int64_t* cell_keys, int64_t C, double lo_x, double lo_y, double lo_z, double h,
                            float* vertices_out, float* normals_out, uint8_t* colours_out, nsky_stream_t stream);
int nsky_mesh_flag_duplicates(const int32_t* corner_cells, int64_t F, const int64_t* sorted_keys, const int64_t* face_order, int32_t* keep,
                              nsky_stream_t stream);
int nsky_mesh_compact_faces(const int32_t* corner_cells, int64_t F, const int32_t* keep, const int64_t* ends, int64_t F_out,
                            int32_t* faces_out, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Connected components of a mesh, and the removal of the small ones ("floaters").  No counterpart in the reference;
 * neusky_amd/exporter/components.py drives these kernels (csrc/components.hip), before simplification.
 *   inputs:   faces [F][3] int32 over V vertices (V, F fit int32); for the compaction also vertices [V][3] fp32 and the optional normals
 *             [V][3] fp32 and colours [V][3] uint8.  Only integers are compared and only bits are copied: no tolerance anywhere.
 *   1 connect: two faces are connected when they share a vertex INDEX (not a position: marching cubes emits one vertex per crossing
 *             grid edge, so its faces share indices).  A component is a class of the transitive closure.  This is vertex
 *             connectivity; libraries that split by edge adjacency differ from it only where two bodies touch in one vertex.
 *   2 root:   the root of a component is its smallest vertex index: a property of the mesh alone, so nothing below depends on the
 *             order of the faces or on scheduling.
 *   3 size:   the size of a component is its face count (on a marching-cubes mesh triangles are near-uniform, so this is area up to a
 *             factor; an area criterion would need ordered fp64 sums to be repeatable and is not offered).
 *   4 rank:   components sorted by size descending, ties by root ascending; rank 0 is the largest.  The sort key is the int64
 *             (F - size) * 2^31 + root.  C = the number of components (<= F).
 *   5 loose:  a vertex that no face references belongs to no component: label -1.  It is dropped by the compaction.
 *   6 filter: a face stays when keep_component[rank of its component] != 0; a vertex stays when a staying face references it.  Both
 *             keep their input order; a staying face keeps its orientation, its corners re-indexed; attributes are copied bit for bit.
 *   7 union-find (link): parent[V] is the identity on entry.  link(x, y): walk x and y to root candidates; while they differ, with hi the
 *             larger and lo the smaller, old = CAS(&parent[hi], hi, lo): old == hi ends it, else the walk goes on from old (the value
 *             the compare-and-swap returned; nothing is re-read) and lo.  Invariant: parent[x] <= x.  Every access to parent in the
 *             link kernel is an agent-scope relaxed atomic (the per-XCD L2s are not coherent for plain accesses).  Finds halve
 *             paths (parent[x] <- parent[parent[x]], a relaxed atomic store): that only moves a non-root's pointer to an ancestor.
 *   8 ends:   termination does not depend on a load being fresh.  A stale parent value is an ancestor in an older forest: same
 *             component, an index no smaller than the current one.  A failed compare-and-swap returns the memory-side value, strictly
 *             smaller than the node it was tried on.  So every step of every loop descends, a find takes fewer than V steps and a hook
 *             fewer than 2 V rounds; no thread waits for another (no lock, no flag, nothing wave64 divergence could deadlock).  Those
 *             bounds are the loops' caps: a thread that reaches one, or meets parent[x] outside [0, x], ORs a bit into *status and
 *             leaves; the caller reads *status with its other counters and treats non-zero as an error.  One launch each: there is no
 *             "repeat until nothing changes" on the host.
 * nsky_cc_link:    faces, parent[V] (the identity on entry)  ->  parent, a forest whose trees are the components, each rooted at its
 *                  smallest index.  *status |= NSKY_CC_STATUS_INDEX for a face index outside [0, V) (the face is skipped),
 *                  NSKY_CC_STATUS_LINK at a cap.  The caller zeroes *status (int32, device memory).
 * nsky_cc_flatten: a launch of its own, so the link pass is complete and visible  ->  vertex_root[V] (a loose vertex is its own root)
 *                  and face_root[F] = the root of each face's first corner.  Read-only finds.  NSKY_CC_STATUS_FLATTEN at a cap.
 * nsky_cc_select:  face_labels[F] = the rank of each face's component, keep_component[C] uint8  ->  keep[F] uint8 (0 / 1) and
 *                  vertex_used[V] uint8, zeroed by the caller, set to 1 for the corners of kept faces (plain stores of one value).
 * nsky_cc_compact: face_ends[F] / vertex_ends[V] = inclusive scans (int64) of keep / vertex_used, F_out / V_out their last entries  ->
 *                  vertices_out[V_out][3], normals_out / colours_out where normals / colours are not NULL, faces_out[F_out][3]. */
#define NSKY_CC_STATUS_INDEX 1
#define NSKY_CC_STATUS_LINK 2
#define NSKY_CC_STATUS_FLATTEN 4
int nsky_cc_link(const int32_t* faces, int64_t F, int64_t V, int32_t* parent, int32_t* status, nsky_stream_t stream);
int nsky_cc_flatten(const int32_t* parent, int64_t V, const int32_t* faces, int64_t F, int32_t* vertex_root, int32_t* face_root,
                    int32_t* status, nsky_stream_t stream);
int nsky_cc_select(const int32_t* faces, int64_t F, int64_t V, const int32_t* face_labels, const uint8_t* keep_component, int64_t C,
                   uint8_t* keep, uint8_t* vertex_used, nsky_stream_t stream);
int nsky_cc_compact(const float* vertices, const float* normals, const uint8_t* colours, int64_t V, const int32_t* faces, int64_t F,
                    const uint8_t* keep, const int64_t* face_ends, const uint8_t* vertex_used, const int64_t* vertex_ends, int64_t V_out,
                    int64_t F_out, float* vertices_out, float* normals_out, uint8_t* colours_out, int32_t* faces_out, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Texture baking on a per-triangle-pair atlas (the layout of nerfstudio's textured-mesh export, with a gutter).  No counterpart in
 * the reference; neusky_amd/exporter/texture.py drives these two kernels (csrc/texture.hip) around the field's fused value chain.
 *   layout:   P = px_per_uv_triangle >= 1; a square has Q = P + 3 texels per side; faces 2 s (lower) and 2 s + 1 (upper) share square s;
 *             S = ceil(sqrt(ceil(F / 2))) squares per row, square s at column s % S, row s / S; the image is W x W, W = S Q <=
 *             NSKY_TEXTURE_MAX_SIZE, row 0 at the top, uint8 [W][W][3].
 *   corners:  texel (i, j) of a square = column i, row j, a texel's centre being its index.  lower: v0 (0, 0), v1 (P, 0), v2 (0, P),
 *             owns i + j <= P + 2; upper: v0 (P+2, P+2), v1 (2, P+2), v2 (P+2, 2), owns i + j >= P + 3.  A bilinear lookup anywhere in
 *             a face's triangle (edges and corners included) reads only texels that face owns.  Squares past ceil(F / 2), and the
 *             upper half of the last square of an odd F, have no owner and are never written.
 *   point:    lower: b1 = i / P, b2 = j / P; upper: b1 = (P + 2 - i) / P, b2 = (P + 2 - j) / P; b0 = 1 - b1 - b2; negative components
 *             become 0 and the rest are divided by their sum (gutter texels sample the nearest edge or corner of their own triangle);
 *             evaluated as integer numerators over their integer sum, one fp32 division each; position =
 *             fma(b2, v2, fma(b1, v1, b0 v0)) per axis.
 *   encoding: colour = clamp(rint(clamp(srgb(x), 0, 1) * 255), 0, 255) with srgb(x) = x <= 0.0031308 ? 12.92 x : 1.055 |x|^(1/2.4) - 0.055,
 *             fp32, every operation rounded on its own (what the exporter's vertex colours go through); normal = the same
 *             quantisation of g / max(|g|, 1e-12) * 0.5 + 0.5, |g| = sqrt((gx gx + gy gy) + gz gz).
 * nsky_texture_texel_points: the texels of squares [s0, s1), s1 <= S^2, in square-major order (row-major inside a square), n =
 *                            (s1 - s0) Q^2 of them  ->  owner[n] (the face, -1 without one or when the face's indices leave [0, V)),
 *                            offset[n] = y W + x (int64) and points[n][3] (zeros without an owner).
 * nsky_texture_texel_store:  albedo[n][3] (linear), gradient[n][3] (read only with a normal image), owner[n], offset[n]  ->  image and,
 *                            unless NULL, normal_image, both uint8 [W][W][3]; texels with owner -1 (or an offset outside the image)
 *                            are skipped. */
#define NSKY_TEXTURE_MAX_SIZE 16384
int nsky_texture_texel_points(const float* vertices, int64_t V, const int32_t* faces, int64_t F, int32_t px_per_uv_triangle,
                              int64_t squares_per_row, int64_t s0, int64_t s1, int32_t* owner, int64_t* offset, float* points,
                              nsky_stream_t stream);
int nsky_texture_texel_store(const float* albedo, const float* gradient, const int32_t* owner, const int64_t* offset, int64_t n, int64_t W,
                             uint8_t* image, uint8_t* normal_image, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Relighting under an equirectangular HDR environment map.  No counterpart in the reference (it lights frames with RENI++ latents
 * only); the package's relight module (neusky_amd/relight) drives these kernels.
 *   map:         fp32 [H, W, 3] linear radiance, C-contiguous, row 0 at the top.
 *   texel (i,j): theta_i = pi (i + 0.5) / H from +z (the scene's up axis); u_j = (j + 0.5) / W; the azimuth phi from +x toward +y is
 *                NSKY_ENVMAP_NEUSKY: phi = 2 pi u,   NSKY_ENVMAP_BLENDER: phi = pi - 2 pi u   (Blender's world-texture mapping);
 *                direction (sin theta cos phi, sin theta sin phi, cos theta).
 *   solid angle: omega_i = (2 pi / W) (cos(pi i / H) - cos(pi (i + 1) / H)) = (2 pi / W) 2 sin(theta_i) sin(pi / (2 H)); sums to 4 pi.
 *   rotation:    R (fp32 [3][3] row-major, device memory; NULL = identity): direction d is lit by the map at R d, as the `rotation=`
 *                of the RENI path.  exposure: fp32 scalar in device memory (NULL = 1), multiplies every output.  Both are read by
 *                the kernels, so a captured graph replays with new values.
 *   label(t):    argmax_k <t, R d_k> over the D directions, ties to the lower k; fp32 with one fixed expression order:
 *                R d = (fma(R02, dz, fma(R01, dy, R00 dx)), ...), <t, e> = fma(tz, ez, fma(ty, ey, tx ex)).
 *   c_k:         exposure * sum_{label(t)=k} omega_t L_t / sum_{label(t)=k} omega_t (fp64 sums); a cell without a texel centre takes
 *                the bilinear lookup at R d_k.  cell_weight_k = sum_{label(t)=k} omega_t (0 for an empty cell).
 *   lookup(v):   v = R ray_dir (any length); x = u(phi(v)) W - 0.5, y = theta(v) / pi H - 0.5 (u inverted per convention);
 *                bilinear, columns wrap modulo W, rows clamp to [0, H-1]; times exposure.  Coordinates in fp64; a non-finite v
 *                gives NaN and reads nothing.
 * Flat texel indices are int64 (maps up to 2^31 texels).  No atomics: every output is bitwise repeatable.
 * nsky_envmap_label:  labels[H W] (int16) of every texel, D <= NSKY_ENVMAP_MAX_DIRECTIONS.
 * nsky_envmap_reduce: sorted_labels[H W] = the labels sorted ascending, order[H W] = the texel index of each sorted entry (a stable
 *                     sort: ascending texel index within a cell); one workgroup per direction finds its segment and writes
 *                     colours[D][3] and cell_weight[D].  The per-cell sum runs in a fixed order: strided per-thread partials, then
 *                     a fixed tree.
 * nsky_envmap_lookup: out[N][3] = lookup(R directions[n]). */
#define NSKY_ENVMAP_NEUSKY 0
#define NSKY_ENVMAP_BLENDER 1
#define NSKY_ENVMAP_MAX_DIRECTIONS 1024
int nsky_envmap_label(const float* directions, int32_t D, const float* rotation, int64_t H, int64_t W, int32_t convention, int16_t* labels,
                      nsky_stream_t stream);
int nsky_envmap_reduce(const float* map, int64_t H, int64_t W, int32_t convention, const float* directions, int32_t D, const float* rotation,
                       const float* exposure, const int16_t* sorted_labels, const int64_t* order, float* colours, float* cell_weight,
                       nsky_stream_t stream);
int nsky_envmap_lookup(const float* map, int64_t H, int64_t W, int32_t convention, const float* directions, int64_t N, const float* rotation,
                       const float* exposure, float* out, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The sun of an environment map, lifted out of it into a SunLight (neusky_amd/relight/envmap_sun.py, csrc/envmap_sun.hip).  The D cell
 * averages above smear a sun over a cell hundreds of times its size, so it casts no shadow edge; these kernels find it, take its
 * excess over the surrounding sky out of the map and return that energy as the colour of a directional sun (the section after the
 * transfer's).  Everything is in the MAP frame: texel directions e_t (per convention), solid angles omega_t, row 0 at the top and z up
 * as above.  All arithmetic is fp64 on the fp32 map values, sums run in a fixed order without atomics (two runs agree bit for bit),
 * flat texel indices are int64.
 *   luminance:  Y_t = 0.2126 R + 0.7152 G + 0.0722 B.
 *   excluded:   a texel with a non-finite channel belongs to no set below and is copied to the residual unchanged.
 *   peak:       p = argmax Y_t over the upper hemisphere (rows with (i + 0.5) / H < 0.5), ties to the lowest flat index; e_p its
 *               direction.  No finite texel there: index -1, Y_p = 0, nothing is found and e_p reads +z.
 *   cap, ring:  cap = {t : <e_t, e_p> >= cos rho};  ring = {t : cos 2 rho <= <e_t, e_p> < cos rho}; over all rows: a dot product, not
 *               an index range, so both wrap across the column seam and close over the pole.
 *   sky level:  tau = sum_ring omega Y / sum_ring omega.
 *   found:      the ring is not empty, Y_p > 0 and Y_p >= min_peak_ratio tau (a black sky, tau = 0, with a bright peak counts).
 *   residual:   t in cap with Y_t > tau: L'_t = fp32(L_t tau / Y_t) (the chromaticity kept, the luminance clamped to the sky level,
 *               rounded once); every other texel, and every texel when nothing is found: L'_t = L_t bit for bit.
 *   excess:     x_t = L_t - L'_t in fp64 from the stored fp32 values.
 *   sun:        colour C = (1 / 2 pi) sum_t omega_t x_t (the sun section's unit, C = L Omega / (2 pi));  direction
 *               m = normalize(sum_t omega_t Y(x_t) e_t);  solid angle Omega_sun = sum of omega_t over the texels with an excess.
 *               Nothing found: C = 0, m = e_p, Omega_sun = 0.
 *   conserved:  sum_t omega_t L_t = sum_t omega_t L'_t + 2 pi C, up to fp64 summation.
 *   scene:      the renderer lights direction d with the map at R d, so the sun's scene direction is R^T m; the map's exposure
 *               multiplies C.
 * scratch: NSKY_ENVMAP_SUN_SCRATCH_BYTES of device memory (8-byte aligned) for the workgroups' partials (at most
 *          NSKY_ENVMAP_SUN_MAX_BLOCKS workgroups of up to 7 fp64 each); the three calls may share one buffer on one stream.
 * nsky_envmap_peak:      map [H,W,3], H >= 2  ->  peak: 16 bytes, the int64 texel index then the fp64 Y_p.
 * nsky_envmap_sun_ring:  map, peak, rho (radians, in (0, pi / 4))  ->  ring [2] = sum_ring omega, sum_ring omega Y.  Visits the rows
 *                        within 2 rho of the peak's polar angle only.
 * nsky_envmap_sun_split: map, peak, ring, rho, min_peak_ratio >= 0  ->  residual [H,W,3] (always written completely: a copy when
 *                        nothing is found; must not be the map) and stats [12] = m (3), C (3), Y_p, tau, Omega_sun, found (0 / 1),
 *                        peak row, peak column (-1, -1 without a peak).  The copy streams 16 bytes per lane when map and residual are
 *                        16-byte aligned; only the rows within rho of the peak's polar angle take the angle test.
 * Each call reads what the previous one wrote to device memory and nothing on the host: the three run on one stream without a
 * synchronisation. */
#define NSKY_ENVMAP_SUN_MAX_BLOCKS 1024
#define NSKY_ENVMAP_SUN_SCRATCH_BYTES (NSKY_ENVMAP_SUN_MAX_BLOCKS * 7 * 8)
int nsky_envmap_peak(const float* map, int64_t H, int64_t W, int32_t convention, void* scratch, void* peak, nsky_stream_t stream);
int nsky_envmap_sun_ring(const float* map, int64_t H, int64_t W, int32_t convention, const void* peak, double rho, void* scratch,
                         double* ring, nsky_stream_t stream);
int nsky_envmap_sun_split(const float* map, int64_t H, int64_t W, int32_t convention, const void* peak, const double* ring, double rho,
                          double min_peak_ratio, void* scratch, float* residual, double* stats, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Precomputed radiance transfer of one frame (neusky_amd/relight/transfer.py, csrc/transfer.hip).  nsky_hemi_composite_fwd is linear in
 * the light colours; with its two sums swapped,
 *   T[r,d,c] = vis[r,d] sum_s weights[r,s] albedo[r,s,c] clamp(<normals[r,s], dirs[d]>, 0, 1) / cnt[r,s]
 *   cnt[r,s] = #{d : clamp(<normals[r,s], dirs[d]>, 0, 1) > 0}, 1 when that is 0;        acc[r] = sum_s weights[r,s]
 *   lin[k,r,c] = sum_d T[r,d,c] lights[k,d,c] + bg[k,r,c] (1 - acc[r]);                   rgb = clamp(linear_to_sRGB(lin), 0, 1)
 * T and acc depend on the camera and the scene only; a new light changes `lights` and `bg` alone.
 *   storage:  NSKY_TRANSFER_FP32: T is fp32 [rows][D][3].  NSKY_TRANSFER_FP16: row r is stored as half(T[r] 2^exponents[r]) (round to
 *             nearest even), exponents[r] chosen so that the row maximum of |T[r]| 2^exponents[r] lies in [0.5, 1); a row of zeros
 *             takes 0.  (Raw values are ~ weights / cnt, 1e-3 .. 1e-9: fp16 subnormals without the scale.)
 * nsky_transfer_bake:    albedo, normals [R,S,3]; weights [R,S]; dirs [D,3]; vis [R,D] or NULL, as nsky_hemi_composite_fwd  ->
 *                        rows [row0, row0 + R) of T; exponents [R] (fp16 storage only, else NULL); acc [R].  1 <= D <= 1024, any S >= 1.
 * nsky_transfer_relight: T [R][D][3] (with exponents [R] for fp16), acc [R], lights [K,D,3], bg [K,R,3]  ->  rgb [K,R,3] and, unless
 *                        NULL, lin [K,R,3].  Any K: up to 8 lights share one pass over T (fewer when K D 12 bytes exceed 64 KiB).
 *                        D a multiple of 4 (fp32) / 8 (fp16) streams 16 bytes per lane; any other D takes a scalar kernel.
 * Flat indices are int64 (R D 3 may exceed 2^31).  No atomics: every output is bitwise repeatable.  Nothing is read on the host. */
#define NSKY_TRANSFER_FP32 0
#define NSKY_TRANSFER_FP16 1
#define NSKY_TRANSFER_MAX_DIRECTIONS 1024
int nsky_transfer_bake(const float* albedo, const float* normals, const float* weights, const float* dirs, const float* vis, int32_t R,
                       int32_t S, int32_t D, int32_t storage, void* T, int64_t row0, int32_t* exponents, float* acc, nsky_stream_t stream);
int nsky_transfer_relight(const void* T, int32_t storage, const int32_t* exponents, const float* acc, const float* lights, const float* bg,
                          int64_t R, int32_t D, int32_t K, float* rgb, float* lin, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A radiance transfer in a basis of the light directions (neusky_amd/relight/transfer_sh.py, csrc/transfer_sh.hip).  The relight above
 * is linear in the light, so with a basis B [D, J] of the directions
 *   C[r,j,c] = sum_d T[r,d,c] B[d,j];      sum_d T[r,d,c] L[d,c] = sum_j C[r,j,c] l[j,c]  with  l = B^T L
 * for every light in the span of an orthonormal B (for any other light: the relight under its projection B B^T L), and a row keeps
 * 3 J numbers in place of 3 D.  Both entries take any B: the real spherical harmonics are one choice, made in Python.
 *   storage:  as above, for T and for C alike; C has row exponents of its own, by the same rule (a power of two, the row maximum of
 *             |C[r]| 2^e in [0.5, 1), a row of zeros takes 0).
 * nsky_transfer_project:       T [R][D][3] (with exponents [R] for fp16: what nsky_transfer_bake wrote), B [D,J] fp32  ->  rows
 *                              [row0, row0 + R) of C [rows][J][3] in out_storage and, for fp16, of out_exponents [rows] (both are
 *                              indexed by the row of C, so a chunk lands in a frame-sized buffer).  1 <= D <= 1024, 1 <= J <= 128.
 *                              fp32 FMAs in the order of d, per row: an entry is within D 2^-24 sum_d |T B| of its definition (plus the
 *                              rounding to fp16, 2^-11 of the row maximum), and a row's bits do not depend on the rows around it.
 * nsky_transfer_relight_short: the contract of nsky_transfer_relight with C, J, lights [K,J,3] in place of T, D, lights [K,D,3], for
 *                              rows of 3 J numbers: any J in 1..128, any K (passes of up to 8 lights, C read once per pass).  The sums
 *                              are taken in fp64 and rounded once with the background.  C starts on a 16-byte boundary.
 * Flat indices are int64.  No atomics and a fixed order: every output is bitwise repeatable.  Nothing is read on the host. */
#define NSKY_TRANSFER_MAX_COEFFICIENTS 128
int nsky_transfer_project(const void* T, int32_t storage, const int32_t* exponents, const float* B, int64_t R, int32_t D, int32_t J,
                          int32_t out_storage, void* C, int64_t row0, int32_t* out_exponents, nsky_stream_t stream);
int nsky_transfer_relight_short(const void* C, int32_t storage, const int32_t* exponents, const float* acc, const float* lights,
                                const float* bg, int64_t R, int32_t J, int32_t K, float* rgb, float* lin, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A directional sun on top of the hemisphere render (neusky_amd/relight/sun.py, csrc/sun.hip).  The frame render sees light as its D
 * directions, one cell of which covers 4 pi / D sr; a sun (6.8e-5 sr) is one direction of its own, with one DDF shadow query per ray.
 *   direction:  the unit vector TOWARDS the sun, z up: s = (cos az cos el, sin az cos el, sin el), azimuth and elevation in degrees.
 *   colour:     C [3] in the renderer's irradiance units.  The hemisphere term of nsky_hemi_composite_fwd is the mean of
 *               clamp(<n,d>, 0, 1) L_d over the directions of the normal's hemisphere, an estimate of (1 / 2 pi) int L cos; a source of
 *               radiance L and solid angle Omega therefore has C = L Omega / (2 pi).
 *   transfer:   t[k,r,c] = sum_s weights[r,s] albedo[r,s,c] clamp(<normals[r,s], s_k>, 0, 1)
 *   shadow:     V[k,r] = vis[k,r] (1 when vis is NULL) if s_k.z > 0 and acc[r] > acc_threshold[0], else 0.  vis is the DDF visibility of
 *               the K sun directions (compute_visibility_compact with sel = 0..K-1).  A sun that has set adds no light and no shadow,
 *               whatever vis holds; the rule is applied on the device.
 *   composite:  lin[k,r,c] = lin_sky[r,c] + C[k,c] V[k,r] t[k,r,c];   rgb = clamp(linear_to_sRGB(lin), 0, 1)
 *               lin_sky is the `lin` output of nsky_hemi_composite_fwd (sky, visibility, background).  The sun's disc is not drawn.
 * nsky_sun_transfer:  albedo, normals [R,S,3]; weights [R,S]; suns [K,3]  ->  out [K,R,3].  One wave per ray, the samples read once
 *                     per pass of up to 8 suns; any S >= 1, any K.  The cosine is taken in fp64 and the sums in fp32: an entry is within
 *                     (3 + S / 64 + 6) 2^-24 sum_s |weights albedo| of its definition.
 * nsky_sun_composite: lin_sky [R,3] with sky_stride 0, one sky under all K suns, or [K,R,3] with sky_stride 3 R, a sky of each sun's
 *                     own (the daylight model below): lin[k,r,c] = lin_sky[k,r,c] + C[k,c] V[k,r] t[k,r,c], and K copies of one sky
 *                     give the one sky's results bit for bit; t [K,R,3]; vis [K,R] or NULL; acc [R]; acc_threshold [1] (device
 *                     memory: a captured graph reads a new threshold on replay); suns, colours [K,3]  ->  rgb [K,R,3] and, unless
 *                     NULL, lin [K,R,3] (the sum in fp64, rounded once) and shadow [K,R] (= V).
 * Flat indices are int64.  No atomics and a fixed reduction order: every output is bitwise repeatable.  Nothing is read on the host. */
int nsky_sun_transfer(const float* albedo, const float* normals, const float* weights, const float* suns, int64_t R, int32_t S, int32_t K,
                      float* out, nsky_stream_t stream);
int nsky_sun_composite(const float* lin_sky, int64_t sky_stride, const float* t, const float* vis, const float* acc,
                       const float* acc_threshold, const float* suns, const float* colours, int64_t R, int32_t K, float* rgb, float* lin,
                       float* shadow, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A clear-sky daylight model whose sky follows the sun (neusky_amd/relight/daylight.py, csrc/daylight.hip): Preetham, Shirley, Smits,
 * "A Practical Analytic Model for Daylight", 1999.  The constants are the paper's tables.
 *   inputs:     turbidity T in [2, 10]; the sun direction s, a unit vector with z up (as above), ts = acos(s.z); a view direction d of any
 *               length, which is normalised; a direction of zero, infinite or NaN length has no sky: its result is 0.
 *   angles:     a direction with d.z < 0 is replaced by its horizon point (z = 0, xy renormalised) and its result multiplied by
 *               ground [3]; a direction straight down takes ground times the zenith value.  ct = d.z after that.
 *               g = atan2(|d x s|, <d, s>)  (not acos of the dot product, which loses half the digits at the sun).
 *   Perez:      F(ct, g) = (1 + A a)(1 + C exp(D g) + E cos^2 g),  a = exp(B / ct) for ct > 0 and 0 for ct = 0;   F0 = F(1, ts)
 *   (A..E) of Y: ( 0.1787 T - 1.4630, -0.3554 T + 0.4275, -0.0227 T + 5.3251,  0.1206 T - 2.5771, -0.0670 T + 0.3703)
 *          of x: (-0.0193 T - 0.2592, -0.0665 T + 0.0008, -0.0004 T + 0.2125, -0.0641 T - 0.8989, -0.0033 T + 0.0452)
 *          of y: (-0.0167 T - 0.2608, -0.0950 T + 0.0092, -0.0079 T + 0.2102, -0.0441 T - 1.6537, -0.0109 T + 0.0529)
 *   zenith:     chi = (4/9 - T/120)(pi - 2 ts);   Yz = (4.0453 T - 4.9710) tan(chi) - 0.2155 T + 2.4192  (kcd / m^2)
 *               xz = [T^2, T, 1] Mx [ts^3, ts^2, ts, 1]^T,  Mx = [[ 0.00166, -0.00375,  0.00209, 0      ],
 *                                                                 [-0.02903,  0.06377, -0.03202, 0.00394],
 *                                                                 [ 0.11693, -0.21196,  0.06052, 0.25886]]
 *               yz likewise,                                My = [[ 0.00275, -0.00610,  0.00317, 0      ],
 *                                                                 [-0.04214,  0.08970, -0.04153, 0.00516],
 *                                                                 [ 0.15346, -0.26756,  0.06670, 0.26688]]
 *   radiance:   Y = Yz F_Y / F0_Y,  x = xz F_x / F0_x,  y = yz F_y / F0_y;   X = x Y / y,  Z = (1 - x - y) Y / y
 *               linear sRGB = M (X, Y, Z),  M = [[ 3.2404542, -1.5371385, -0.4985314],
 *                                                [-0.9692660,  1.8760108,  0.0415560],
 *                                                [ 0.0556434, -0.2040259,  1.0572252]]   (D65)
 *               clamped to >= 0, then multiplied by exposure (and by ground below the horizon).  A sun with s.z <= 0 has set: its
 *               whole sky is 0.
 * nsky_daylight_eval: directions [N,3]; suns [K,3]; turbidity [1], exposure [1], ground [3]  ->  out [K,N,3].  suns and the last three
 *                     are device memory: a captured graph replays with new values.  Any N >= 1, any K >= 1.  The constants of a sun
 *                     (zenith values over F0) are worked out once per sun and workgroup in fp64 and kept in LDS, up to 256 suns per
 *                     launch; a thread owns a direction, reads it once, forms 1 + A a in fp64 and walks the suns in fp32; each
 *                     sun's row is written with coalesced stores.
 *                     Its K skies meet their suns in nsky_sun_composite with sky_stride 3 N.
 * Flat indices are int64.  No atomics: every output is bitwise repeatable.  Nothing is read on the host. */
int nsky_daylight_eval(const float* directions, const float* suns, const float* turbidity, const float* exposure, const float* ground,
                       int64_t N, int32_t K, float* out, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sphere-traced shadow rays through the SDF, with penumbrae (neusky_amd/relight/shadows.py, csrc/sphere_trace.hip): the sun's shadow
 * from the surface the SDF field holds instead of one DDF query.  The march is a loop on the host: the field's sdf at every ray's point
 * (the non-tangent hash encode and nsky_sdf_chain_fwd, or any function of the points), then nsky_sphere_trace_step.
 *
 * The march rule.  A shadow ray has a start point x, a unit direction s and parameters:
 *   N         96     iterations
 *   eps       1e-3   hit threshold
 *   relax     1.0    step scale
 *   min_step  1e-3   smallest step
 *   grace     16     leaving phase, iterations
 *   radius    the model's sphere-collider radius    scene bound
 *   tan_half  tan(angular_diameter / 2); 0 = hard shadow    penumbra width
 * State per ray: t = 0, m = 1, status = ALIVE, outside = false.
 * Iteration i = 0 .. N-1, on ALIVE rays only, in this order:
 *   1. p = x + t s.  If |p| >= radius: status = ESCAPED.
 *   2. f = sdf(p).
 *   3. If f >= eps: outside = true.
 *   4. If f < eps and (outside or i >= grace): status = HIT, m = 0.
 *   5. If still ALIVE, outside, tan_half > 0 and t > 0: m = min(m, clamp(f / (t tan_half), 0, 1)).
 *   6. If still ALIVE: t += max(|f| relax, min_step).
 * Result: visibility = m.  That is 0 for HIT.  For a hard shadow it is 1 otherwise.  A ray still ALIVE after N iterations keeps its m
 * and is reported as EXHAUSTED.  status is int8.  t is the last parameter.
 * The leaving phase (steps 3-4) lets a start point that lies up to a few eps inside the surface climb out instead of shadowing itself.
 * Step 5 is the usual closest-approach penumbra estimate: an approximation of a disc light, not an integral over it.  Every default
 * is a design choice, not a measurement.  A ray that starts outside the radius escapes at once.
 *
 *   rays:    T rays; ray i has direction row i / dir_div (dir_div = R for K suns over R start points: i = k R + r; 1 for a direction
 *            of each ray's own) and start row i % R.
 *   params:  fp32 [6] in device memory = eps, relax, min_step, tan_half, radius, bias: a captured graph replays with new values.
 *            N (`steps`), grace and the iteration index are by value.
 *   state:   fp32 [6][T], one plane each: x (3), t, m, a flag word (int32 bits: status in the low byte, 0x100 = outside).
 * nsky_sphere_trace_begin:        origins, directions [R,3]; depth [R]; normals [R,3] (the rendered normals, any length); suns [K,3]
 *                                 -> state and points [K R,3]:  x = o + depth d + bias n^ (each product and sum one fma); a normal of
 *                                 zero (or non-finite) length is replaced by s_k.  Rule step 1 of iteration 0 is applied here.
 * nsky_sphere_trace_begin_points: starts [M,3]; directions [T / dir_div, 3]  ->  the same from explicit start points (T a multiple of M).
 * nsky_sphere_trace_step:         state, sdf [T] at `points`, directions, params, iteration  ->  state, points [T,3].  Rule steps 3-6 of
 *                                 this iteration, then p = fma(t, s, x) and rule step 1 of the next (none after iteration steps - 1).
 *                                 Dead rays keep their point to the bit (their t no longer moves).  bounds NULL: the rule as above.
 *                                 bounds [2][T] = t_end, tan_half of each ray's own (nsky_light_trace_begin): the march towards a
 *                                 light below; it needs dir_div == 1, directions [T,3].  16-byte accesses when T % 4 == 0 and state,
 *                                 sdf and points (with bounds: directions and bounds too) are 16-byte aligned, else 4-byte ones; the
 *                                 results are the same.
 * nsky_sphere_trace_finish:       state  ->  vis [T] (= m), status [T] (int8, ALIVE reported as EXHAUSTED), t [T].
 * Flat indices are int64.  No atomics: every output is bitwise repeatable.  Nothing is read on the host. */
#define NSKY_TRACE_ALIVE 0
#define NSKY_TRACE_HIT 1
#define NSKY_TRACE_ESCAPED 2
#define NSKY_TRACE_EXHAUSTED 3
#define NSKY_TRACE_PARAMS 6
int nsky_sphere_trace_begin(const float* origins, const float* directions, const float* depth, const float* normals, const float* suns,
                            int64_t R, int32_t K, const float* params, float* state, float* points, nsky_stream_t stream);
int nsky_sphere_trace_begin_points(const float* starts, const float* directions, int64_t M, int64_t T, int64_t dir_div, const float* params,
                                   float* state, float* points, nsky_stream_t stream);
int nsky_sphere_trace_step(float* state, const float* sdf, const float* directions, const float* bounds, int64_t T, int64_t dir_div,
                           const float* params, int32_t iteration, int32_t steps, int32_t grace, float* points, nsky_stream_t stream);
int nsky_sphere_trace_finish(const float* state, int64_t T, float* vis, int8_t* status, float* t, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Point and spot lights inside the scene, with sphere-traced shadows (neusky_amd/relight/lights.py, csrc/lights.hip, and the step of
 * csrc/sphere_trace.hip with bounds).  Every light above is at infinity; a lamp has a direction and a distance of its own at every sample,
 * and its shadow ray ends at the lamp: geometry behind the lamp does not shadow it.
 * A light:
 *   p [3]          position, scene units
 *   I [3]          intensity: the colour C a directional sun would need to light a facing surface as this lamp does from distance 1
 *                  (irradiance units times scene units squared)
 *   rho >= 0       source radius: a spherical source; 0 gives a hard shadow
 *   clearance >= 0 the shadow ray ends this far in front of p, so a lamp placed in or on reconstructed geometry is not shadowed by its
 *                  own post
 *   min_distance > 0   the floor of the inverse-square law
 *   a [3], cos_inner >= cos_outer   a spot cone: the unit axis (the way the lamp points) and the cosines of its two half-angles; an
 *                  omnidirectional light has cos_inner = cos_outer = -1
 * The defaults clearance = max(rho, 0.02), min_distance = max(rho, 0.01) and no cone are design choices, not measurements.
 *   lights:     fp32 [L,16] in device memory; columns p (0..2), a (3..5), cos_inner, cos_outer, rho, clearance, min_distance, pad,
 *               I (12..14), pad.  Only L is by value: a captured graph replays under new positions, colours, cones and radii.
 *   transfer:   x = positions[r,s], the points the field was evaluated at.  v = p - x, q = |v|^2.  If q == 0 the term is 0, otherwise
 *               u = v / sqrt(q);  cosine = clamp(<normals[r,s], u>, 0, 1) (the normals as given, as the sun takes them);  c = -<u, a>;
 *               spot = 1 if c >= cos_inner, else 0 if c <= cos_outer, else h^2 (3 - 2 h) with h = (c - cos_outer) / (cos_inner -
 *               cos_outer) (the tests in this order: the omnidirectional light never divides);  g = spot / max(q, min_distance^2);
 *               t[l,r,c] = sum_s weights[r,s] albedo[r,s,c] cosine g
 *   march:      the march rule above with two changes.  Step 1 becomes: if t >= t_end_i or |p| >= radius: status = ESCAPED (the ray
 *               reached its light, or left the scene towards a light outside the collider).  Step 5 uses a tan_half_i of each ray's
 *               own.  Ray i = l R + r starts at x = o + depth d + bias n^ (the fmas of nsky_sphere_trace_begin; a zero or non-finite
 *               normal is replaced by the unit vector from o + depth d to the light).  v = p_l - x, len = |v|, s_i = v / len,
 *               t_end_i = len - clearance_l, tan_half_i = rho_l / len: the cone from the start point to the source has radius
 *               rho t / len at parameter t, so this is the closest-approach estimate for a sphere of radius rho.  len == 0 gives
 *               s = (0,0,1), t_end = 0, tan_half = 0.  s, t_end and tan_half are formed in fp64 and rounded once.
 *   composite:  V[l,r] = vis[l,r] (1 when vis is NULL) if acc[r] > acc_threshold[0], else 0;  E[r,c] = sum_l I[l,c] V[l,r] t[l,r,c] in
 *               fp64, l ascending;  light_lin = fl32(E);  lin[k,r,c] = fl32(base[k,r,c] + E[r,c]), one rounding, for each of the Kb
 *               base images (a frame under each of K suns; E == 0 leaves the base's bits);  rgb = clamp(linear_to_sRGB(lin), 0, 1).
 *               The L lights add into one frame: they are not alternatives, as K suns are.  A lamp's own disc is not drawn.
 * nsky_light_transfer:  positions, albedo, normals [R,S,3]; weights [R,S]; lights [L,16]  ->  out [L,R,3].  One wave per ray, the
 *                       samples read once per pass of up to 8 lights; any S >= 1, any L >= 1.  The factor cosine g is formed in fp64
 *                       from the fp32 inputs and rounded once, the sums are nsky_sun_transfer's: an entry is within
 *                       (3 + S / 64 + 6) 2^-24 sum_s |weights albedo| cosine g of its definition.
 * nsky_light_trace_begin:  origins, directions [R,3]; depth [R]; normals [R,3]; lights; params [6] (the march's block)  ->  state
 *                       [6][T], points [T,3], ray_dirs [T,3], bounds [2][T] (t_end, tan_half), T = L R.  Rule step 1 of iteration 0
 *                       is applied here.
 * nsky_light_trace_begin_points:  starts [M,3]  ->  the same from explicit start points (T = L M).
 *                       The march is nsky_sphere_trace_step with ray_dirs as its directions, dir_div = 1 and these bounds;
 *                       nsky_sphere_trace_finish ends it.
 * nsky_lights_composite:  base [Kb,R,3] with base_stride = 3 R, or [R,3] with base_stride = 0; t [L,R,3]; vis [L,R] or NULL; acc [R];
 *                       acc_threshold [1] (device memory); lights  ->  rgb, lin [Kb,R,3] (lin may be NULL) and, unless NULL, light_lin
 *                       [R,3] and visibility [L,R] (= V).
 * Flat indices are int64.  No atomics and a fixed reduction order: every output is bitwise repeatable.  Nothing is read on the host. */
#define NSKY_LIGHT_FLOATS 16
int nsky_light_transfer(const float* positions, const float* albedo, const float* normals, const float* weights, const float* lights,
                        int64_t R, int32_t S, int32_t L, float* out, nsky_stream_t stream);
int nsky_light_trace_begin(const float* origins, const float* directions, const float* depth, const float* normals, const float* lights,
                           int64_t R, int32_t L, const float* params, float* state, float* points, float* ray_dirs, float* bounds,
                           nsky_stream_t stream);
int nsky_light_trace_begin_points(const float* starts, const float* lights, int64_t M, int32_t L, const float* params, float* state,
                                  float* points, float* ray_dirs, float* bounds, nsky_stream_t stream);
int nsky_lights_composite(const float* base, int64_t base_stride, const float* t, const float* vis, const float* acc,
                          const float* acc_threshold, const float* lights, int64_t R, int32_t L, int32_t Kb, float* rgb, float* lin,
                          float* light_lin, float* visibility, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Solid props placed in a frame (neusky_amd/relight/props.py, csrc/props.hip): spheres and yawed boxes that the frame's light shades,
 * that the scene shadows and that shadow the scene.  Every shading kernel of a frame is a sum over a ray's samples, and every shadow a
 * factor on a visibility tensor, so a prop changes none of them: its hit becomes one more sample of the ray, and every visibility the
 * frame forms is multiplied by an analytic occlusion test.
 *   props:  fp32 [P,16] in device memory, 1 <= P <= NSKY_MAX_PROPS; columns kind (0 sphere, 1 box), centre c (1..3), half-extents h
 *           (4..6; a sphere: its radius r three times), cos yaw, sin yaw (7, 8), albedo (9..11), visible (12: 0 or 1), casts_shadows
 *           (13: 0 or 1), pad (14, 15).  Only P is by value: a captured graph replays under props that moved, turned, changed size,
 *           colour or flags.
 *   interval:  of a line x(t) = o + t d inside prop p, formed in fp64 from the fp32 inputs, each product, sum and quotient rounded once
 *           (no fused multiply-add).  d need not be unit.
 *           sphere:  oc = o - c, a = <d,d>, b = <oc,d>, q = <oc,oc> - r r, disc = b b - a q (dot products x, y, z ascending).  No
 *                    interval unless disc > 0; then t_in = (-b - sqrt(disc)) / a, t_out = (-b + sqrt(disc)) / a.
 *           box:     o' = (cos oc_x + sin oc_y, cos oc_y - sin oc_x, oc_z) and d' likewise: oc and d turned by -yaw about z.  Axis i with
 *                    d'_i != 0 gives the slab parameters (-h_i - o'_i) / d'_i and (h_i - o'_i) / d'_i; an axis with d'_i == 0 gives no
 *                    interval unless |o'_i| < h_i, and otherwise constrains nothing.  t_in is the largest of the per-axis minima
 *                    (-inf when no axis constrains), t_out the smallest of the per-axis maxima (+inf).  An interval only if
 *                    t_in < t_out.  The entry axis is the one that gave t_in, ties to the lowest axis.
 *   seen:   only props with `visible`.  A ray enters prop p at t_in when it has an interval and t_in > 0: a camera inside a prop does
 *           not see it.  The smallest t_in wins, ties to the lowest index.  The normal is the outward unit normal at the entry point:
 *           a sphere's (oc + t_in d) / r divided by its length; a box's entry axis signed against d' (-1 when d'_axis > 0), turned
 *           back by +yaw: (s cos, s sin, 0), (-s sin, s cos, 0) or (0, 0, s), the block's fp32 cos and sin as they are.  t_hit, the
 *           normal and the albedo are rounded once to fp32.
 *   insert: sample s < S of a ray is in front when fl32(fl32(starts + ends) / 2) < t_hit, the midpoint Frustums.get_positions forms.
 *           Its new weight is its weight if in front, else 0; its starts, ends, albedo and normal are copied bit for bit.  Sample S is the
 *           prop: weight clamp(1 - sum of the weights in front, 0, 1), the sum in fp64 in sample order, rounded once (the transmittance
 *           nsky_hemi_composite_fwd's own background term bg (1 - acc) would use there), 0 when the ray enters no prop; albedo and
 *           normal the prop's, zeros when none; starts = ends = t_hit, or ends[S-1] when none, so that the global depth bounds of
 *           nsky_ray_reduce_fwd see no infinity.  A sample that straddles t_hit is kept or dropped whole: that is the approximation of
 *           this seam, as good as the sampler's spacing at the prop.
 *   shadow: entry (m, n) of a visibility tensor is the light n reaches from point m.  x' = x + bias n^ in fp64, n^ the normal divided
 *           by its length in fp64; a zero or non-finite normal, or none, gives no lift (nsky_sphere_trace_begin's rule, without its
 *           fallback).  Towards a light at infinity the line is x' + t d_n with t_max = +inf.  Towards a lamp at p_n with clearance_n:
 *           v = p_n - x', len = |v|, d = v / len, t_max = len - clearance_n; len == 0 leaves the entry.  The entry is multiplied by 0
 *           when some prop with `casts_shadows` has an interval with t_out > 0 and t_in < t_max, and is otherwise neither read nor
 *           written.  Shadow edges are hard: a penumbra for analytic props is out of scope.
 * nsky_props_intersect:  origins, directions [R,3]; props [P,16]  ->  t_hit [R] (+inf for none), id [R] (int32, -1), normal, albedo [R,3]
 *                        (zeros for none).  One thread per ray, the block staged once per workgroup in LDS.
 * nsky_props_insert:     weights, starts, ends [R,S]; albedo, normals [R,S,3]; t_hit, id, hit_normal, hit_albedo as above  ->  the five
 *                        arrays with S + 1 samples.  One wave per ray; any S >= 1.
 * nsky_props_occlude:    x [M,3]; normals [M,3] or NULL; either directions [N,3], or targets [N,3] with clearance [N]; bias [1] (device
 *                        memory); props  ->  vis, in place, entry (m, n) at vis[m stride_m + n stride_n] (strides in floats, >= 0): the
 *                        sky's [R,D], the suns' [K,R], the lamps' [L,R] and the shafts' rows without a transpose.  One thread per entry,
 *                        consecutive threads along the smaller stride, the block in LDS.
 * prop_bias = 1e-2, the midpoint rule and NSKY_MAX_PROPS = 64 (the block then fills 4 KiB of LDS) are design choices, not measurements.
 * Flat indices are int64.  No atomics, no reduction across threads but the ordered sum: every output is bitwise repeatable.  Nothing is
 * read on the host. */
#define NSKY_PROP_FLOATS 16
#define NSKY_MAX_PROPS 64
int nsky_props_intersect(const float* origins, const float* directions, const float* props, int64_t R, int32_t P, float* t_hit, int32_t* id,
                         float* normal, float* albedo, nsky_stream_t stream);
int nsky_props_insert(const float* weights, const float* starts, const float* ends, const float* albedo, const float* normals,
                      const float* t_hit, const int32_t* id, const float* hit_normal, const float* hit_albedo, int64_t R, int32_t S,
                      float* weights_out, float* starts_out, float* ends_out, float* albedo_out, float* normals_out, nsky_stream_t stream);
int nsky_props_occlude(const float* x, const float* normals, const float* directions, const float* targets, const float* clearance,
                       const float* bias, const float* props, int64_t M, int64_t N, int32_t P, float* vis, int64_t stride_m,
                       int64_t stride_n, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Height fog and haze with shadowed sun shafts (neusky_amd/relight/atmosphere.py, csrc/atmosphere.hip): a participating medium between
 * the camera and what a frame shows, applied to a chunk's linear image after its suns and lamps.
 * The medium:
 *   density [3] >= 0   the extinction coefficient per scene unit at height base_height, per channel
 *   H                  the scale height: sigma_c(z) = density_c exp(-(z - base_height) / H), z up; H = 0 in the block stands for a
 *                      homogeneous medium (sigma_c = density_c everywhere)
 *   albedo [3]         the single-scattering albedo, in [0, 1]
 *   g                  the Henyey-Greenstein parameter, |g| <= 0.99
 *   far > 0            the path length, from the ray origin, given to what lies behind the scene: the background, and the see-through
 *                      share of a ray.  far / H <= 60, so that no exponential overflows
 *   background         whether the sky behind the scene is fogged too
 *   params:  fp32 [12] in device memory = density (0..2), albedo (3..5), H, base_height, g, far, background (1 or 0), pad.  Only M and
 *            Kb are by value: a captured graph replays under a new density, height, albedo, anisotropy, far or background flag.
 * Per ray and per base image b (one per sun of a sun or daylight frame, one for a sky frame), channel c implied:
 *   inputs:  origin o, unit direction d, t_s = clamp(depth, 0, far) (the ray's rendered depth along it), A = clamp(accumulation, 0, 1),
 *            the linear image lin_b after suns and lamps, the background colour B_b behind the ray.
 *   optical depth:  tau(t) = density E t phi(d_z t / H),  E = exp(clamp(-(o_z - base_height) / H, -80, 80)),
 *            phi(u) = (1 - exp(-u)) / u, evaluated as -expm1(-u) / u, and as 1 - u / 2 + u u / 6 for |u| < 1e-4; a homogeneous medium
 *            has E = 1 and phi = 1.  This is the integral of sigma along the ray from 0 to t.  T(t) = exp(-tau(t)).
 *   source:  J_b(m) = albedo (Abar_b + 2 pi p_g(<d, s_k>) C_k V_k(m) up_k)
 *            Abar_b    the mean of the frame's light colours over all D light directions of base b: an equal-area lattice, so this is
 *                      (1 / 4 pi) times the integral of the sky's radiance.  Sky in-scatter is NOT shadowed: an approximation.
 *            s_k, C_k  the sun's direction and colour; C = L Omega / (2 pi), so 2 pi C is the sun's L Omega
 *            p_g(mu) = (1 / 4 pi) (1 - g^2) / (1 + g^2 - 2 g mu)^1.5
 *            up_k = 1 when s_k,z > 0, else 0: a set sun adds nothing.  A sky frame has no sun term.
 *            V_k(m)    the sun's visibility from the midpoint o + (m + 0.5) (far / M) d of segment m; 1 when M = 0 or vis is NULL.
 *   in-scatter to t_e:  with t_m = m far / Mseg for m = 0..Mseg, Mseg = max(M, 1):
 *            S_b(t_e) = sum_m J_b(m) (T(min(t_m, t_e)) - T(min(t_{m+1}, t_e))), m ascending:
 *            exact for a source that is piecewise constant along the ray, for any density profile; with M = 0 it is J (1 - T(t_e)).
 *   pixel:   out_b = T(t_s) (lin_b - (1 - A) B_b) + A S_b(t_s) + (1 - A) X_b,  X_b = T(far) B_b + S_b(far) with `background`, else B_b
 *            rgb = clamp(linear_to_sRGB(out), 0, 1);  transmittance = T(t_s);
 *            inscatter_b = A S_b(t_s) + (1 - A) S_b(far) with `background`, else A S_b(t_s);
 *            light_lin <- light_lin T(t_s), so that it stays the lamps' share of lin.
 * The rule uses the ray's rendered depth, as the suns' and the lamps' shadows do, not a per-sample transmittance inside the alpha
 * composite, and adds no glow around lamps.  Every default of relight.Atmosphere is a design choice, not a measurement.
 * nsky_atmosphere_rows:   origins, directions [R,3]; params; M  ->  row_origins, row_directions [M R,3], row_depth [M R]: row i = m R + r
 *                         holds ray r and the depth (m + 0.5) (far / M), formed in fp64 and rounded once: what nsky_ddf_query_rows and
 *                         nsky_sphere_trace_begin take to put a shadow query at the midpoint of segment m.
 * nsky_atmosphere_apply:  origins, directions [R,3]; depth, accumulation [R]; lin_in [Kb,R,3] through its strides (k, r), in floats, the
 *                         channels contiguous (a frame of K suns is ray-major in memory); background [Kb,R,3] with background_stride =
 *                         3 R, or [R,3] with 0; abar [Kb,3]; sun_dirs, sun_colours [Kb,3] or both NULL; vis [M,Kb,R] through its strides
 *                         (m, k, r) or NULL; params  ->  lin, rgb, inscatter [Kb,R,3] through the strides (k, r) they share;
 *                         transmittance [R,3]; light_lin [R,3] in place, or NULL.  One thread per ray; everything in fp64 from the fp32
 *                         inputs, every output rounded once.
 * Flat indices are int64.  No atomics and a fixed summation order: every output is bitwise repeatable.  Nothing is read on the host. */
#define NSKY_ATMOSPHERE_FLOATS 12
#define NSKY_ATMOSPHERE_MAX_SHAFTS 64
int nsky_atmosphere_rows(const float* origins, const float* directions, const float* params, int64_t R, int32_t M, float* row_origins,
                         float* row_directions, float* row_depth, nsky_stream_t stream);
int nsky_atmosphere_apply(const float* origins, const float* directions, const float* depth, const float* accumulation, const float* lin_in,
                          int64_t lin_stride_k, int64_t lin_stride_r, const float* background, int64_t background_stride, const float* abar,
                          const float* sun_dirs, const float* sun_colours, const float* vis, int64_t vis_stride_m, int64_t vis_stride_k,
                          int64_t vis_stride_r, const float* params, int64_t R, int32_t M, int32_t Kb, float* lin, float* rgb,
                          float* inscatter, int64_t out_stride_k, int64_t out_stride_r, float* transmittance, float* light_lin,
                          nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A display transform: from a linear, high-dynamic-range image to a picture (neusky_amd/relight/display.py, csrc/display.hip):
 * metered exposure, an optional bloom, a tone curve, the sRGB transfer function and the rounding to 8 bits, all on the device.
 * Input: lin [K,H,W,3] fp32 (P = H W pixels per image), and optionally mask [K,H,W] fp32 (a frame's accumulation).
 *
 *   luminance:  Y = (0.2126f r + 0.7152f g) + 0.0722f b in fp32, every product and sum rounded once (no fused multiply-add): a float32
 *               restatement has the same bits.
 *   metered:    a pixel is metered when Y is finite, Y >= 2^-24, and (with a mask) mask > meter_mask_threshold.
 *   bins:       bin = (bits(Y) >> 17) - 6592, clamped above to 3071: 3072 bins, 48 octaves from 2^-24 to 2^24 with 64 bins each (the 6
 *               leading bits of the mantissa), values >= 2^24 in the last.  No logarithm decides a bin: the histogram is an
 *               integer-exact function of the input.  2^-24 -> 0, its predecessor -> none, 1 -> 1536, 1 + 1/64 -> 1537,
 *               nextafter(2, 0) -> 1599, nextafter(2^24, 0) -> 3071, 2^24 -> 3072, clamped to 3071.
 *   histogram:  int64 counts [K][3072], or [1][3072] shared by the K images (a sequence metered as one).  Counts are ADDED to what the
 *               histogram holds: the caller zeroes it, and several calls accumulate.
 *   exposure:   with n metered pixels in a row of the histogram: a = floor(p_lo n), b = n - floor((1 - p_hi) n), in fp64 from the fp32
 *               percentiles.  In sorted order bin j holds the positions [sum_{i<j} c_i, sum_{i<=j} c_i); c'_j is its overlap with [a, b);
 *               m = sum_j c'_j ((j + 0.5) / 64 - 24) / (b - a), the mean over the kept pixels of their bins' centres, a centre being
 *               exponent + mantissa fraction: the piecewise-linear log2, exact at powers of two and at most 0.0861 below log2;
 *               E = key 2^(ev - m) in fp64, stored fp32; E = 1 when b <= a (nothing metered among it).  (j + 0.5) / 64 - 24 is a
 *               multiple of 1 / 128, so the sum is an integer over 128 and exact in any order (the kernel forms it in int64); scaling
 *               the image by 2^k rolls the histogram by 64 k bins and gives E 2^-k.  key = 0.18, percentiles (0.05, 0.95) and ev = 0
 *               are the defaults of relight.DisplayTransform: design choices, not measurements.
 *   bloom:      source s = max(E lin - threshold, 0) per channel (product and difference rounded once each; a NaN gives 0);
 *               B = G_sigma * s, a separable Gaussian of radius r = ceil(3 sigma) <= 96 (0 < sigma <= 32 pixels) whose 2 r + 1 weights
 *               exp(-t^2 / (2 sigma^2)) are normalised in fp64 on the host and rounded to fp32.  Outside the frame the source is zero.
 *               Rows first, then columns, each pass an fp32 fmaf chain in tap order -r..r starting from 0.  Images never mix.
 *   map:        x = min(max(E lin + strength B, 0), 2^60) (without bloom E lin alone, the product rounded once; with it
 *               fma(strength, B, E lin); the max turns a NaN into 0; the min keeps the curves' polynomials finite, where every curve has
 *               long reached its limit);  y = curve(x) per channel;  rgb = clamp(linear_to_sRGB(y), 0, 1), the function every
 *               renderer here ends with;  rgb8 = rint(255 rgb), ties to even, as uint8.
 *   curves:     CLAMP     y = x
 *               REINHARD  y = x (1 + x / w^2) / (1 + x), white point w (default 4)
 *               ACES      Narkowicz's fit: y = x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14)
 *               HABLE     the Uncharted-2 operator h(v) = (v (A v + C B) + D E) / (v (A v + B) + D F) - E / F with
 *                         A, B, C, D, E, F = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30:  y = h(2 x) / h(11.2) (exposure bias 2, white 11.2).
 *                         It is evaluated as h(v) = v (0.042 v + 0.005) / (0.3 (v (0.15 v + 0.5) + 0.06)), the same function with the
 *                         constant terms cancelled on paper, whose value at 0 is exactly 0.
 *               With CLAMP, E = 1 and no bloom, rgb has the bits of the `rgb` the frame's own renderer wrote from the same lin.
 *   params:     fp32 [8] in device memory = key, ev, p_lo, p_hi, white point, bloom threshold, bloom strength, meter_mask_threshold:
 *               with E, what may change between two frames; a captured graph replays with new values.  The curve, the blur's radius
 *               and weights and the shapes are by value or by pointer.
 * nsky_display_histogram: lin [K,P,3]; mask [K,P] or NULL; params  ->  hist (+=) [K][3072], or [1][3072] when `shared` != 0.  A workgroup
 *                         counts in LDS (12 KB) over a grid-stride share of one image and adds its non-zero counts with 64-bit integer
 *                         atomics: exact, and the same bits in every run.  K <= 65535.
 * nsky_display_exposure:  hist [K][3072]; params  ->  E [K].  One workgroup per row.
 * nsky_display_blur:      lin [K,H,W,3]; E [KE], KE = K or 1 (one exposure for all); params; weights [2 radius + 1]; 1 <= radius <= 96
 *                         ->  B [K,H,W,3] through scratch [K,H,W,3].  LDS tiles with a halo of the radius; the radius may exceed the
 *                         tile and the image.
 * nsky_display_map:       lin [K,P,3]; B [K,P,3] or NULL (no bloom); E [KE]; params; curve  ->  rgb8 uint8 [K,P,3] and, unless NULL,
 *                         rgb fp32 [K,P,3].  One pass; 16-byte accesses when P % 4 == 0 and the pointers allow it, the same results
 *                         otherwise.
 * Flat indices are int64.  The only atomics are integer adds: every output is bitwise repeatable.  Nothing is read on the host. */
#define NSKY_DISPLAY_BINS 3072
#define NSKY_DISPLAY_PARAMS 8
#define NSKY_DISPLAY_MAX_RADIUS 96
#define NSKY_DISPLAY_CLAMP 0
#define NSKY_DISPLAY_REINHARD 1
#define NSKY_DISPLAY_ACES 2
#define NSKY_DISPLAY_HABLE 3
int nsky_display_histogram(const float* lin, const float* mask, const float* params, int64_t P, int32_t K, int32_t shared, int64_t* hist,
                           nsky_stream_t stream);
int nsky_display_exposure(const int64_t* hist, const float* params, int32_t K, float* E, nsky_stream_t stream);
int nsky_display_blur(const float* lin, const float* E, int32_t KE, const float* params, const float* weights, int32_t radius, int32_t K,
                      int32_t H, int32_t W, float* scratch, float* B, nsky_stream_t stream);
int nsky_display_map(const float* lin, const float* B, const float* E, int32_t KE, const float* params, int32_t curve, int64_t P, int32_t K,
                     uint8_t* rgb8, float* rgb, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Adaptive antialiasing of a frame (neusky_amd/relight/antialias.py, csrc/antialias.hip): the first pass of a frame takes one ray through
 * every pixel centre; an edge mask marks the pixels whose neighbourhood differs, a second pass traces S - 1 further sub-pixel rays through
 * each marked pixel, and a resolve averages the S samples in linear light.  A frame is H x W pixels, P = H W, pixel p = y W + x.
 *
 *   edge mask:  the neighbours q of pixel p are the up to 4 pixels left, right, above and below it inside the image.  With a the
 *               accumulation, p is marked when for any q one of these holds, every product, sum and difference in fp32 rounded once (no
 *               fused multiply-add), so that a float32 restatement in the same order has the same mask to the bit:
 *                 accumulation  |a_p - a_q| > accumulation
 *                 depth         a_p > covered, a_q > covered and |depth_p - depth_q| > depth * min(depth_p, depth_q)
 *                 normal        a_p > covered, a_q > covered, n_p . n_p >= 1e-12f, n_q . n_q >= 1e-12f and, with d = n_p . n_q,
 *                               d <= 0 or d * d < cos2 * ((n_p . n_p) * (n_q . n_q)): the angle between the rendered normals exceeds
 *                               normal_deg, without a square root.  cos2 = cos^2(normal_deg), formed in fp64 on the host and rounded to
 *                               fp32; a dot product is (x x' + y y') + z z'.  A normal shorter than 1e-6 switches the test off for
 *                               its pairs.
 *                 colour        for any of the K linear images, |Y_p - Y_q| > colour * max(Y_p, Y_q, 1e-4f), Y the display
 *                               transform's luminance (0.2126f r + 0.7152f g) + 0.0722f b: a relative test, the same under any
 *                               exposure.
 *               Every test is symmetric in p and q: both pixels of a differing pair are marked, and no dilation follows.  A comparison
 *               with a NaN is false (min and max return their other operand).  The thresholds are by value: nothing here is captured.
 *               accumulation = 0.1, depth = 0.02, normal_deg = 15, colour = 0.1 and covered = 0.5 are the defaults of
 *               relight.Antialias: design choices, not measurements.
 *   rays:       from the frame's own bundle, no camera: D = directions * directions_norm (norm 1 when NULL), g_x = D(y, x + 1) - D(y, x)
 *               (in the last column D(y, x) - D(y, x - 1); zero when W = 1), g_y the same along rows;
 *               D' = (D + dx g_x) + dy g_y per component, fp32, every operation rounded once; directions_norm' = |D'| =
 *               sqrt((x x + y y) + z z), directions' = D' / |D'|.  Origins, pixel_area and camera_indices are the pixel's.  The
 *               un-normalised pinhole direction is affine in the pixel coordinate, so for a pinhole bundle this is the ray through
 *               (x + 0.5 + dx, y + 0.5 + dy) up to fp32 rounding (3e-7 on a component at 1080p).  Ray (e, s) of the E pixels and S - 1
 *               offsets is row e (S - 1) + s: pixel-major.
 *   resolve:    F[k, pixels[e], c] = (F[k, pixels[e], c] + sum_s X[k, e, s, c]) / S, S = S1 + 1: the sum in fp64 in the order F, s = 0 ..
 *               S1 - 1, the quotient in fp64, rounded to fp32 once.  With rgb, rgb[k, pixels[e], c] = clamp(linear_to_sRGB(.), 0, 1)
 *               of the value written, the function every renderer here ends with.  Pixels not listed are not touched.
 * nsky_aa_edge_mask:      depth [P], normal [P,3], accumulation [P]; lin: channel c of pixel p of image k at lin[k ls_k + p ls_p + c]
 *                         (strides in floats; K >= 0; K = 0: no colour test, lin may be NULL)  ->  mask uint8 [P], 1 marked, 0 not.
 *                         One thread per pixel.
 * nsky_aa_subpixel_rays:  origins, directions [P,3]; norm [P] or NULL; pixel_area [P] or NULL; camera_indices int64 [P] or NULL;
 *                         pixels int64 [E]; offsets [S1,2] = (dx, dy)  ->  out_origins, out_directions [E S1, 3], out_norm [E S1] and,
 *                         where the input is given, out_pixel_area [E S1], out_camera_indices int64 [E S1].  One thread per ray.  A pixel
 *                         index outside [0, P) is clamped into it (no access leaves the frame); the caller checks its own list.
 * nsky_aa_resolve:        F (in place): element (k, p, c) at F[k fs_k + p fs_p + c]; X: element (k, e, s, c) at
 *                         X[k xs_k + e xs_e + s xs_s + c]; rgb, or NULL: element (k, p, c) at rgb[k rs_k + p rs_p + c].  All strides are
 *                         in floats and name the layout as it is: a frame of K suns is assembled from ray-major chunks and K leads only
 *                         in its shape (a frame [P,K,C] seen as [K,P,C] has fs_k = C, fs_p = K C), and the second pass's chunks arrive
 *                         ray-major, [E S1, K, C] (xs_k = C, xs_s = K C, xs_e = S1 K C): nothing is transposed for this kernel.
 *                         pixels int64 [E], pairwise distinct (two entries naming one pixel would race).  One thread per (e, k, c).  An
 *                         index outside [0, P) is skipped.
 * Flat indices are int64.  No atomics: every output is bitwise repeatable.  Nothing is read on the host. */
int nsky_aa_edge_mask(const float* depth, const float* normal, const float* accumulation, const float* lin, int64_t ls_k, int64_t ls_p,
                      int32_t K, int32_t H, int32_t W, float t_accumulation, float t_depth, float cos2, float t_colour, float covered,
                      uint8_t* mask, nsky_stream_t stream);
int nsky_aa_subpixel_rays(const float* origins, const float* directions, const float* norm, const float* pixel_area,
                          const int64_t* camera_indices, const int64_t* pixels, const float* offsets, int32_t H, int32_t W, int64_t E,
                          int32_t S1, float* out_origins, float* out_directions, float* out_norm, float* out_pixel_area,
                          int64_t* out_camera_indices, nsky_stream_t stream);
int nsky_aa_resolve(float* F, int64_t fs_k, int64_t fs_p, const float* X, int64_t xs_k, int64_t xs_e, int64_t xs_s, const int64_t* pixels,
                    int32_t K, int64_t P, int64_t E, int32_t S1, int32_t C, float* rgb, int64_t rs_k, int64_t rs_p, nsky_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Depth of field of a frame (neusky_amd/relight/depth_of_field.py, csrc/dof.hip): the first pass of a frame is a pinhole's, one ray through
 * the lens centre and every pixel centre: sample 0.  A circle of confusion per pixel from that pass's depth and accumulation, a mark on
 * every pixel some blurred pixel's disc reaches, S - 1 thin-lens rays through each marked pixel, and nsky_aa_resolve (above, as it is)
 * averages the S samples in linear light.  A frame is H x W pixels, P = H W, pixel p = y W + x.  All fp32 arithmetic is rounded once per
 * operation, no fused multiply-add, division and square root correctly rounded: a float32 restatement in the same order has the same
 * bits for the circle of confusion and the same mask.
 *
 *   lens:       float [12] on the device = r^ (3), s^ (3), w^ (3), a, 1 / z_f, a f_px.  With D = directions * directions_norm and g_x, g_y
 *               of the rays rule above taken at the centre pixel (W / 2, H / 2) (integer division): r^ = g_x / |g_x|, s^ = g_y / |g_y|,
 *               w^ = +-(r^ x s^) with the sign that makes D . w^ > 0: the image plane's axes and the optical axis, from the bundle alone,
 *               no camera.  f_px = 1 / |g_x|: the focal length in pixels, for D has D . w^ = 1 in a pinhole bundle.  a: the lens radius in
 *               scene units.  z_f: the depth of the plane in focus along w^, in the units of the frame's `depth` = p2p_dist /
 *               directions_norm (a pinhole's z-depth); 1 / z_f = 0 focuses at infinity.  The caller forms the block in fp64 and rounds it.
 *   coc:        iz_p = 1 / depth_p when accumulation_p > covered and not depth_p <= 0, else 0: an uncovered pixel is at infinity (a
 *               comparison with a NaN is false: a covered pixel's NaN depth stays a NaN, an uncovered pixel's does not count).
 *               c_p = (a f_px) * |iz_p - 1 / z_f|: the blur radius, in pixels, of a point at that depth, for a lens point at offset l
 *               shifts the image of a point at depth z by f_px l (1 / z - 1 / z_f).  A NaN c marks nothing.
 *               With focus_pixel >= 0 the plane of focus goes through what the first pass saw at that pixel: 1 / z_f = 1 / depth there
 *               when its accumulation > covered and its depth > 0, else 0; it is read on the device, used in place of lens[10] and
 *               written to lens[10] (by one thread; no thread reads lens[10] in that case).  With focus_pixel < 0, lens[10] is read.
 *   mark:       p is marked when some pixel q of the image has |q_x - p_x| <= reach, |q_y - p_y| <= reach, c_q >= threshold and
 *               c_q + 0.5f >= (float) max(|q_x - p_x|, |q_y - p_y|); q = p counts.  The scatter of every blurred pixel's disc, in its
 *               square (conservative) form, written as a gather: a sharp pixel behind a blurred foreground edge, a sharp pixel in front
 *               of a blurred background and every pixel that is itself out of focus take lens samples.  Two approximations: `reach`
 *               (1..64) caps how far a disc marks (the lens rays themselves are exact at any blur), and a surface the pinhole pass
 *               never saw can appear only inside marked regions.  Evaluated as: r_q = min(reach, floor(c_q + 0.5f)) where c_q >=
 *               threshold, else -1 (the distances are integers, so c_q + 0.5f >= d is d <= r_q); m(x, y') = the largest r_q among the q
 *               of row y' with |q_x - x| <= r_q, else -1; p is marked when |y' - p_y| <= m(p_x, y') for some row y'.  The same set.
 *   table:      [S - 1, 4] rows (dx, dy, u, v), made on the host in fp64 and rounded: row s = 1 .. S - 1 from t = frac(0.5 + s (1 / g,
 *               1 / g^2, 1 / g^3, 1 / g^4)), g the real root of g^5 = g + 1 (the R2 sequence in four dimensions); (dx, dy) = (t_0, t_1) -
 *               0.5; (u, v) the concentric square-to-disc map (Shirley and Chiu) of (a, b) = 2 (t_2, t_3) - 1: (0, 0) at a = b = 0; for
 *               |a| > |b|, a (cos phi, sin phi) with phi = (pi / 4) (b / a); else b (cos phi, sin phi) with phi = pi / 2 - (pi / 4)
 *               (a / b).  |dx|, |dy| <= 0.5, u^2 + v^2 <= 1.  Sample 0 is the first pass: dx = dy = u = v = 0.
 *   lens rays:  D' = (D + dx g_x) + dy g_y with pixel p's own g_x, g_y: the antialiasing rule.  With `rotate`, theta = (float) h * tau,
 *               tau = 2 pi 2^-24 rounded to fp32, h = hash(p) >> 8 (the top 24 bits), and (u, v) <- (u cos theta - v sin theta,
 *               u sin theta + v cos theta), sine and cosine in fp32; hash is on the low 32 bits of p, all in uint32:
 *                 x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *               (without the turn every pixel repeats one lens pattern: S ghost images instead of noise).  l = a * (u r^ + v s^) per
 *               component; k = D' . w^ = (x x' + y y') + z z'; t = k * (1 / z_f); D'' = D' - t * l; origins' = o + l; directions' =
 *               D'' / |D''|; directions_norm' = |D''| / k, so that depth = p2p_dist / directions_norm stays the z-depth and focus at
 *               infinity needs no case of its own.  Every lens ray of a pixel passes through o + D' z_f / k.  pixel_area and
 *               camera_indices are the pixel's.  Ray (e, s) of the E pixels and S - 1 rows is row e (S - 1) + s: pixel-major.
 * nsky_dof_coc:        depth, accumulation [P]; lens [12] (lens[10] written when focus_pixel >= 0); focus_pixel in [-1, P)  ->  coc [P].
 *                      One thread per pixel.
 * nsky_dof_mark:       coc [P]; reach in 1..64  ->  mask uint8 [P], 1 marked, 0 not.  One block of 256 threads per 64 x 64 pixels, the
 *                      radii of the tile and its halo and the row pass's result in LDS ((64 + 2 reach)^2 + (64 + 2 reach) 64 bytes).
 *                      Pixels outside the image have no disc.  H <= 65535 * 64.
 * nsky_dof_lens_rays:  the bundle as for nsky_aa_subpixel_rays; pixels int64 [E]; table [S1, 4]; lens [12]; rotate 0 or 1  ->  the same
 *                      members for the E S1 rays.  One thread per ray.  A pixel index outside [0, P) is clamped into it (no access
 *                      leaves the frame); the caller checks its own list.
 * threshold = 0.5 pixel, reach = 16, covered = 0.5 and S = 16 are the defaults of relight.DepthOfField: design choices, not measurements.
 * Flat indices are int64.  No atomics: every output is bitwise repeatable.  Nothing is read on the host. */
int nsky_dof_coc(const float* depth, const float* accumulation, float* lens, int32_t H, int32_t W, int64_t focus_pixel, float covered,
                 float* coc, nsky_stream_t stream);
int nsky_dof_mark(const float* coc, int32_t H, int32_t W, float threshold, int32_t reach, uint8_t* mask, nsky_stream_t stream);
int nsky_dof_lens_rays(const float* origins, const float* directions, const float* norm, const float* pixel_area,
                       const int64_t* camera_indices, const int64_t* pixels, const float* table, const float* lens, int32_t H, int32_t W,
                       int64_t E, int32_t S1, int32_t rotate, float* out_origins, float* out_directions, float* out_norm,
                       float* out_pixel_area, int64_t* out_camera_indices, nsky_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NEUSKY_HIP_H */
