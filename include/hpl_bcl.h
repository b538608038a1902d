/*
 * hpl_bcl.h -- C ABI of libhplbcl.so: the MI355X (gfx950) implementation of
 * HPLFlowNet's bilateral-convolution hot path.
 *
 * This is the drop-in boundary (SURVEY.md §8 b).  The reference has no native ops
 * for the layer half of the path (it composes ATen calls) and a 4-function khash
 * FFI for the lattice half; each entry point below names the reference lines it
 * replaces (paths relative to the reference repository root).  All pointers are
 * DEVICE pointers unless marked HOST; all kernels are enqueued on `stream`
 * (a hipStream_t passed as void*) and return without synchronising.  No torch
 * types appear here: hplflownet_amd/_lib.py binds this header with ctypes and
 * passes tensor.data_ptr() values.
 *
 * Conventions
 *   - activations are CHANNEL-LAST float32: X[row * ld + channel]; `ld` (row stride
 *     in floats) lets a kernel read or write a column slice of a wider buffer, which
 *     is how the torch.cat calls of models/HPLFlowNet.py:242-423 disappear;
 *   - index tables are int32 (converted once per sample from the reference's int64
 *     wire format); -1 means "no such lattice vertex" and reads as
 *     an all-zero row (the reference's "+1 / zero column" trick,
 *     models/bilateralNN.py:158-162,215-217);
 *   - float4 fast paths need ld % 4 == 0, channel counts % 4 == 0 and 16-byte
 *     aligned bases; other shapes take a scalar path (same results).
 *   - return value: 0 on success, negative HPL_E* on failure; hpl_last_error()
 *     gives the message of the calling thread's last failure.
 */
#ifndef HPL_BCL_H
#define HPL_BCL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPL_OK 0
#define HPL_EINVAL (-1)   /* bad argument (shape, alignment, null pointer) */
#define HPL_EHIP (-2)     /* a HIP runtime call or kernel launch failed */
#define HPL_ENODEV (-3)   /* no gfx950 device visible */

#define HPL_ACT_NONE 0
#define HPL_ACT_LEAKY 1   /* y > 0 ? y : slope * y   (models/module_utils.py:6,14) */

typedef void *hplStream;

int hpl_version(void);
const char *hpl_last_error(void);
/* HOST outputs. arch receives e.g. "gfx950". */
int hpl_device_info(int device, int *cu_count, int *wave_size, char *arch, int arch_len);

/* ------------------------------------------------------------------------ *
 * Index tables
 * ------------------------------------------------------------------------ */
/* int64 -> int32 narrowing of any reference table (lattice_offset, blur_neighbors,
 * pc1_corr_indices; transforms/transforms.py:471-483). */
int hpl_index_narrow(const int64_t *src, int32_t *dst, int64_t n, hplStream stream);

/* pc2_corr_indices [F][K][H] int64 (models/bnn_flow.py:195-197, index order
 * transforms/transforms.py:232-241) -> int32 [K][F*H]: row k of the result is the
 * neighbour table of the F*H "virtual vertices" m = f*H + h used by the
 * patch-correlation gather-GEMM. */
int hpl_corr2_permute(const int64_t *src, int32_t *dst, int F, int K, int64_t H, hplStream stream);
/* same from an int32 [F][K][H] source (device-built lattices) */
int hpl_corr2_permute32(const int32_t *src, int32_t *dst, int F, int K, int64_t H, hplStream stream);

/* CSR of the splat: for `off` (int32, n_entries values in [0,H); for a lattice_offset table
 * entry e = r*N + n and n_entries = 4*N) and per-entry weights `bary` ([n_entries]) produce
 *   csr_ptr [H+1]        segment bounds per vertex,
 *   csr_pt  [n_entries]  source row (e % pt_mod; pt_mod = N gives the point index) of each
 *                        contribution, ascending e within a vertex,
 *   csr_w   [n_entries]  its weight,
 *   norm    [H]          1 / (sum of weights + 1e-5)   (models/bilateralNN.py:168-183).
 * `scratch` needs (H + 1) + n_entries + 1026 int32.  Replaces the COO coalesce inside
 * torch.sparse.FloatTensor(...).to_dense() (models/bilateralNN.py:24-29): the sort is
 * done once per lattice instead of once per layer call, and is deterministic. */
int hpl_csr_build(const int32_t *off, const float *bary, int64_t n_entries, int64_t pt_mod, int64_t H,
                  int32_t *csr_ptr, int32_t *csr_pt, float *csr_w, float *norm,
                  int32_t *scratch, hplStream stream);
/* The same for a pair of clouds treated as one: points [0,N0) + [N0,N0+N1), vertices [0,H0) +
 * [H0,H0+H1) (off1 values are shifted by H0 here).  off0, off1, bary0, bary1 are the per-cloud [4][N] tables.
 * Outputs sized for H = H0+H1 and 4*(N0+N1) entries; scratch (H+1) + 4*(N0+N1) + 1026 int32.
 * A vertex belongs to one cloud, so each segment is identical to the per-cloud CSR. */
int hpl_csr_build_pair(const int32_t *off0, const float *bary0, int64_t N0, int64_t H0,
                       const int32_t *off1, const float *bary1, int64_t N1, int64_t H1,
                       int32_t *csr_ptr, int32_t *csr_pt, float *csr_w, float *norm,
                       int32_t *scratch, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Splat / slice  (HBM-bound gathers)
 * ------------------------------------------------------------------------ */
/* out[v, c] = (norm ? norm[v] : 1) * sum_{j in csr(v)} csr_w[j] * feat[csr_pt[j], c]
 * Forward splat + density normalisation: models/bilateralNN.py:151-186 and
 * models/bnn_flow.py:119-151 (SparseSum.forward, bilateralNN.py:9-30).
 * With norm == NULL it is also the backward of hpl_slice w.r.t. Y. */
int hpl_splat(const float *feat, int64_t ldf, int C, const int32_t *csr_ptr, const int32_t *csr_pt,
              const float *csr_w, const float *norm, int64_t H, float *out, int64_t ldo,
              hplStream stream);

/* out[n, c] = (bias ? bias[c] : 0) + sum_{r<4} bary[r*N+n] * (vscale ? vscale[v] : 1) * Y[v, c],
 * v = off[r*N+n].   Slice + bias: models/bilateralNN.py:223-238.  With vscale = norm it is
 * also the backward of hpl_splat w.r.t. feat (SparseSum.backward, bilateralNN.py:33-40). */
int hpl_slice(const float *Y, int64_t ldy, int C, const float *bary, const int32_t *off, int64_t N,
              const float *vscale, const float *bias, float *out, int64_t ldo, hplStream stream);
/* The same two kernels ADDING to what `out` holds: a feature matrix with several consumers collects their gradients
 * (autograd's accumulation of models/HPLFlowNet.py's torch.cat / reuse of a tensor). */
int hpl_splat_add(const float *feat, int64_t ldf, int C, const int32_t *csr_ptr, const int32_t *csr_pt,
                  const float *csr_w, const float *norm, int64_t H, float *out, int64_t ldo,
                  hplStream stream);
int hpl_slice_add(const float *Y, int64_t ldy, int C, const float *bary, const int32_t *off, int64_t N,
                  const float *vscale, const float *bias, float *out, int64_t ldo, hplStream stream);

/* Patch correlation from per-tap projections.  The pc2 half of the Conv3d((1,15,1)) of models/bnn_flow.py:195-202 gathers the
 * same pc2 vertex row for up to 225 (filter tap, correlation tap) pairs and multiplies each copy by W_k; projecting every pc2
 * vertex ONCE per correlation tap, Z[v, k*N + n] = sum_c f2[v, c] * W[n, c, k] (a small dense GEMM), leaves
 *   Y[m, n] = act(bias[n] + res[(m % res_mod) * ldres + n] + sum_{k<K} Z[nbr[k][m] * ldz + k*col_step + n])    (nbr < 0: nothing)
 * with col_step = N -- a gather of N-float rows instead of C-float rows and no 8.7-GFLOP contraction (N = 32, C = 64,
 * M = 15 * H1).  N % 4 == 0, K <= 15, 16-byte aligned rows; taps are added in ascending k (deterministic).
 * Its gradient w.r.t. Z is the same kernel through the INVERSE table (hpl_table_invert) with col_step = 0:
 * dZ[(v*K + k)*N + n] = sum_f G[inv[f][v*K + k] * ldg + n] -- no atomics. */
int hpl_gather_sum(const float *Z, int64_t ldz, const int32_t *nbr, int64_t nbr_stride, int64_t M, int K, int N, int col_step,
                   const float *bias, const float *res, int64_t ldres, int64_t res_mod, int act, float slope, float *Y,
                   int64_t ldy, hplStream stream);
/* T [K][stride >= F*H0] with values in [0, H1) or -1 whose F blocks of H0 columns are injective (the permuted pc2_corr_indices:
 * for a fixed (filter tap f, correlation tap k) the map h -> T2(key1_h + offset) is one to one -- also under the reference's
 * unchecked key packing, which is linear in the key) -> inv int32 [F][K*H1]: inv[f][v*K + k] = f*H0 + h where
 * T[k][f*H0 + h] = v, else -1. */
int hpl_table_invert(const int32_t *T, int64_t stride, int K, int64_t H0, int F, int64_t H1, int32_t *inv, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Per-vertex dense contraction: gather-GEMM on fp32 MFMA
 * ------------------------------------------------------------------------ */
/* Weight re-layout.  Source element (r, q, f) lives at W[base + r*sr + q*sq + f*sf];
 * destination Wt[(fdst*R + r) * ldw + q] with fdst = fmap ? fmap[f] : f.  Rows beyond
 * F*R (up to k_rows) and columns beyond Q (up to ldw) are zero-filled.
 *   forward  of Conv2d (O,C,F,1) / Conv3d (O,Ctot,1,K,1) / Conv1d (O,C,1):
 *            r = input channel, q = output channel  -> Wt[(f*C + c)][o]
 *   backward-data: r = output channel, q = input channel, fmap[f] = (15-f)%15 style
 *            mirror. */
int hpl_weight_relayout(const float *W, int64_t base, int R, int Q, int F, int64_t sr, int64_t sq,
                        int64_t sf, const int32_t *fmap, float *Wt, int64_t k_rows, int64_t ldw,
                        hplStream stream);
/* Many re-layouts in one launch (training re-lays every conv weight after each optimiser step, in
 * the forward and in the data-gradient direction).  jobs / prefix live in DEVICE memory; job j writes
 * destination elements [prefix[j], prefix[j+1]) of dst as an image [k_rows][ldw] with the meaning of
 * hpl_weight_relayout; mirror != 0 stores tap f at position (F - f) % F.  total = prefix[njobs]. */
typedef struct hpl_relayout_job {
    const float *W;         /* source parameter */
    int64_t base, sr, sq, sf;
    int32_t R, Q, F, mirror;
    int64_t ldw;            /* row length of the destination image (multiple of 4) */
} hpl_relayout_job;
int hpl_weight_relayout_batch(const hpl_relayout_job *jobs /* DEVICE */, int njobs,
                              const int64_t *prefix /* DEVICE, njobs + 1 */, int64_t total, float *dst,
                              hplStream stream);
/* Fold of a bias-only 1x1 conv into the conv that reads its result.  W is the consumer's weight in the
 * parameter's own layout [O][C][F] (Conv2d (O,C,F,1) / Conv1d (O,C,1)); its columns [up0, up0 + up_w) read
 * Wb u + b_tot, Wb [up_w][Cb] the producer's trailing 1x1 and b_tot = bias_a + bias_b (either or both may be NULL; both
 * given: their fp32 sum).  out [O][Cout][F], same layout, reads u instead:
 *   columns of W before the up block: copied;  up block: out[o][up0' + j][f] = sum_k W[o][up0 + k][f] Wb[k][j], j < Cb;
 *   columns behind it: copied;  ones_col >= 0 (<= up0, needs b_tot): four columns are inserted at ones_col, the first
 *   holds sum_k W[o][up0 + k][f] b_tot[k] -- the weight of a constant-1 input column --, the other three are zero.
 * Cout = C - up_w + Cb + (ones_col >= 0 ? 4 : 0); out_elems = O * Cout * F (checked).
 * out_bias (F == 1 only; [O]): own_bias[o] (NULL: 0) + sum_k W[o][up0 + k] b_tot[k] -- the bias of a folded dense layer.
 * A b_tot that neither ones_col nor out_bias takes up is refused.  Every sum runs in double in the order of k and is
 * rounded to fp32 once; no atomics: the same inputs give the same bits. */
int hpl_weight_fold(const float *W, int O, int C, int F, int up0, int up_w, const float *Wb, int Cb,
                    const float *bias_a, const float *bias_b, int ones_col, float *out, int64_t out_elems,
                    const float *own_bias, float *out_bias, hplStream stream);

/* mirror == 2 ("taps as column blocks"): the image is [roundup(R, 32)][ldw >= F*Q] with element (r, f*Q + q) =
 * W[base + r*sr + q*sq + f*sf] -- the operand of the scatter / regular data gradients of the correlation layer
 * (models/bnn_flow.py:202-205 backward: G[m, (f, c)] = g[m] . W[:, c, f]). */
/* The inverse of the batch call, for the weight gradients of a whole training step: job j reads its image
 * [k_rows][ldw] at src + (prefix[j] - prefix[0]) and writes W[base + r*sr + q*sq + f*sf] = src_j[(f*R + r)*ldw + q]
 * (mirror 0 or 2); W is then the job's gradient tensor in the parameter's own layout (main.py:214 loss.backward()).
 * total = elements of all images (sizes the grid). */
int hpl_weight_unlayout_batch(const hpl_relayout_job *jobs /* DEVICE */, int njobs,
                              const int64_t *prefix /* DEVICE, njobs + 1 */, int64_t total, const float *src,
                              hplStream stream);

/* Split weight image for the bf16-MFMA path: Wt [k_rows][ldw] fp32 (k_rows % 8 == 0) -> three planes p = 0 (hi),
 * 1 (mid), 2 (lo) of bf16, each [k_rows/8][ldw][8] (element (k, n) at ((k/8)*ldw + n)*8 + k%8: the 8 consecutive k of
 * one output column are one 16-byte MFMA B fragment), plane p at dst + p*plane_stride bytes; hi = bf16_rne(w),
 * mid = bf16_rne(w - hi), lo = bf16_rne(w - hi - mid): w == hi + mid + lo exactly.  plane_stride >= k_rows*ldw*2. */
int hpl_weight_split3(const float *Wt, int64_t k_rows, int64_t ldw, void *dst, int64_t plane_stride, hplStream stream);
/* The fp16-pair form (hpl_gconv_desc.wt3_planes == 2): *amax (DEVICE) = the image's largest magnitude, s = the power of two
 * that puts it into [2^14, 2^15); two planes of fp16 in the same fragment order, hi = f16_rne(w s), lo = f16_rne(w s - hi). */
int hpl_weight_split2h(const float *Wt, int64_t k_rows, int64_t ldw, void *dst, int64_t plane_stride, float *amax,
                       hplStream stream);
/* The same for many images in one launch (a training step re-splits every wide image after the optimiser step): jobs in DEVICE
 * memory, max_elems = the largest k_rows * ldw among them (sizes the grid). */
typedef struct hpl_split3_job {
    const float *Wt;
    void *dst;
    int64_t k_rows, ldw, plane_stride;
    float *amax;              /* planes == 2: DEVICE scalar the job's largest magnitude is written to */
    int32_t planes;           /* 2: fp16 pairs (hpl_weight_split2h); 0 / 3: bf16 triples */
    int32_t pad_;
} hpl_split3_job;
/* any_pairs: nonzero when any job has planes == 2 (their largest magnitudes are reduced first: two more launches). */
int hpl_weight_split3_batch(const hpl_split3_job *jobs /* DEVICE */, int njobs, int64_t max_elems, int any_pairs,
                            hplStream stream);

/* inverse scatter for weight gradients: W[base + r*sr + q*sq + f*sf] (+)= Wt[(f*R + r)*ldw + q] */
int hpl_weight_unlayout(const float *Wt, int64_t ldw, int R, int Q, int F, float *W, int64_t base,
                        int64_t sr, int64_t sq, int64_t sf, int accumulate, hplStream stream);

typedef struct hpl_gconv_desc {
    /* A operand: rows of a channel-last matrix, gathered through a neighbour table */
    const float *A;         /* [rows_a][lda] */
    int64_t lda;
    int64_t rows_a;         /* rows addressable in A (indices are checked against it in debug) */
    const int32_t *nbr;     /* nbr[f * nbr_stride + m] in [-1, rows_a); NULL: see reg_stride */
    int64_t nbr_stride;
    int64_t reg_stride;     /* used when nbr == NULL: source row = f * reg_stride + m
                               (F == 1, reg_stride == 0 is a plain GEMM) */
    int64_t M;              /* output rows (lattice vertices, or F*H virtual vertices) */
    int32_t C;              /* channels taken from each gathered row */
    int32_t F;              /* filter taps, <= 15 per call (radius 1); contraction length K = F * C <= 32768.
                             * Wider stencils (radius 2: 65 taps) = consecutive calls over tap ranges, each a row
                             * range of nbr and of Wt (w_rows), accumulating through res = Y */
    /* B operand: re-laid-out weights (hpl_weight_relayout) */
    const float *Wt;        /* [>= roundup(F*C, 32)][ldw], zero padded */
    int64_t ldw;            /* multiple of 4, >= N */
    int32_t N;              /* output channels */
    int32_t act;            /* HPL_ACT_* applied after bias and residual */
    float slope;
    const float *bias;      /* [N] or NULL */
    const float *res;       /* optional addend res[(m % res_mod) * ldres + n] (before act) */
    int64_t ldres;
    int64_t res_mod;
    float *Y;               /* [M][ldy] */
    int64_t ldy;
    /* optional scatter epilogue (backward-data through a non-symmetric table): when
     * scat != NULL the result is NOT stored to Y[m]; column n = k*scat_c + c is
     * atomically added to Y[scat[k*scat_stride + m] * ldy + c] (skipped when < 0). */
    const int32_t *scat;
    int64_t scat_stride;
    int32_t scat_c;
    /* rows of Wt that exist (0 = roundup(F*C, 32), i.e. a zero-padded image).  A smaller value
     * (>= F*C) lets Wt be a row range of a bigger image -- one tap group of it: rows past w_rows
     * read as zero. */
    int32_t w_rows;
    /* optional permutation of the M output rows (hpl_tap_order): tile row j computes and writes
     * output row row_perm[j]; the result is unchanged, rows of one tile share absent taps so that
     * whole contraction slices can be skipped.  NULL = identity. */
    const int32_t *row_perm;
    /* optional workspace for split-K (M*N*4 bytes per split, up to 16 splits; small and mid-size launches);
     * NULL = never split.  Partial tiles are summed in split order (cut points are slice indices): results are
     * deterministic and independent of the row order. */
    float *ws;
    int64_t ws_bytes;
    /* optional, with row_perm: per-tile gather indices and tap masks precomputed by hpl_tile_index for tiles of
     * tile_bm rows.  Used when the launch picks that tile height (ignored otherwise): the tile prologue is then
     * one round of coalesced loads instead of the dependent chain row_perm -> nbr -> masks. */
    const int32_t *tile_idx;
    const int32_t *tile_mask;
    int32_t tile_bm;
    /* optional diagnostic (DEVICE, 2 x int64, zeroed by the caller): every 64th workgroup adds its residence time in
     * shader cycles to [0] and in 100 MHz wall ticks to [1] -- [0] / [1] * 100 MHz is the clock the chip sustains
     * under this kernel (it clocks to its power budget). */
    int64_t *clock_probe;
    /* optional second destination (forward only, not with scat): rows m < rows2 of the result are ALSO stored to
     * Y2[m * ldy2 + n] -- a layer's output that feeds two concatenation buffers is written once by its producer
     * instead of copied (the reference builds both with torch.cat, models/HPLFlowNet.py:299-393). */
    float *Y2;
    int64_t ldy2;
    int64_t rows2;
    /* optional: the same weights as three bf16 planes (hpl_weight_split3 of the image Wt points into, at the same
     * first row, which must be a multiple of 8).  Launches that qualify (wide row-ordered stencil passes) then run
     * on the bf16 matrix pipe with every fp32 operand carried EXACTLY as hi + mid + lo bf16 terms and the six
     * leading partial products accumulated in fp32 (csrc/gconv3.hip: per-product error <= 2^-24 relative, the fp32
     * rounding class; 16/6 of the fp32-MFMA rate).  NULL: fp32 MFMA. */
    const void *Wt3;
    int64_t wt3_plane_stride;   /* bytes between the planes */
    /* wt3_planes == 2 (round 5): Wt3 is hpl_weight_split2h of the image -- two fp16 planes hi / lo of w * s_w -- and the
     * launch splits A the same way: a * s_a = hi + lo (one rounding each), the three partial products hi*hi + hi*lo + lo*hi
     * on the fp16 MFMA, fp32 accumulate, the result times 1 / (s_a s_w).  s = the power of two that puts the matrix's
     * largest magnitude into [2^14, 2^15): a_amax / w_amax are DEVICE scalars holding those magnitudes (hpl_amax of the
     * rows and channels of A the launch can read -- or of any superset --; the one hpl_weight_split2h wrote).  Per product
     * the error is <= 2^-21 |a b| for every a within 2^-18 of the largest (smaller ones: 2^-40 of the largest, absolute), per
     * output <= (2^-21 + (3K/16) 2^-24) sum|a||w| -- below the (K - 1) 2^-24 sum|a||w| of an fp32 dot product of length K >= 12
     * in any order; measured against float64 the sums are closer than the fp32 MFMA's and the triples'
     * (tests/test_gpu_split3.py) at half the bf16-triple form's MFMA work.  Both scalars must be given
     * (else the launch runs on the fp32 MFMA).  wt3_planes == 0 / 3: bf16 triples as above. */
    int32_t wt3_planes;
    const float *a_amax;
    const float *w_amax;
    /* optional (DEVICE, cleared by the caller; not with scat): *y_amax = max(*y_amax, largest |Y[m][n]| this call stores) -- the
     * a_amax of a wide launch that reads Y next, from the epilogue's registers where the launch allows, else by one more pass. */
    float *y_amax;
    /* Range guard of the fp16-pair form (round 6; all optional, wt3_planes == 2 only).  ONE scale per matrix leaves a row whose
     * entries are all below 2^-18 of the matrix's largest magnitude with an ABSOLUTE error (2^-40 of that magnitude) -- fine for
     * the sums of loud rows, not for a quiet row's own outputs.  a_guard: DEVICE word written by hpl_amax_rows (or left by a
     * producer through y_guard): the smallest non-zero ROW maximum of A, stored as ~bits (0 = unknown: no guard).  When the
     * largest magnitude exceeds it by 2^18 or more (exponent gap), the launch runs a SECOND pass over its slice list with the
     * residuals of the first split, (a s - hi - lo) 2^24, again as fp16 pairs, into the same accumulators: every element then
     * carries >= 21 significand bits down to 2^-41 of the largest magnitude (2^-63 of it, absolute, below that) -- fp32-class
     * results per OUTPUT ROW over 12 decades of row loudness, at twice the matrix-pipe work of that launch only.  y_guard: the companion of y_amax (cleared by the
     * caller): the guard word of Y from this launch's epilogue (row maxima over the 64 columns a wave holds: never larger
     * than the true row maximum, i.e. conservative), else by hpl_amax_rows.  guard_trips: DEVICE counter, +1 per launch that
     * took the second pass. */
    const uint32_t *a_guard;
    uint32_t *y_guard;
    int32_t *guard_trips;
} hpl_gconv_desc;

/* Largest magnitude of X[0 .. rows)[0 .. cols) (row stride ld) -> *slot (DEVICE; NaN if X holds one). */
int hpl_amax(const float *X, int64_t ld, int64_t rows, int32_t cols, float *slot, hplStream stream);
/* The same, and the range-guard word of X (hpl_gconv_desc.a_guard): *guard = max over the rows with a non-zero entry of
 * ~bits(largest magnitude of the row), 0 if every row is zero.  Both slots are cleared by the call. */
int hpl_amax_rows(const float *X, int64_t ld, int64_t rows, int32_t cols, float *slot, uint32_t *guard, hplStream stream);

/* Row order for tap skipping: perm = the M vertices grouped by their F-bit tap-presence mask (bit f set iff
 * nbr[f*nbr_stride + m] >= 0; F <= 15), the groups in Gray-code order of their masks (neighbouring groups differ in
 * one tap), ties by ascending row id (a stable radix sort: the order is deterministic and does not affect results).  scratch: hpl_tap_order_scratch_ints(M) int32, 8-byte aligned. */
int64_t hpl_tap_order_scratch_ints(int64_t M);
int hpl_tap_order(const int32_t *nbr, int64_t nbr_stride, int F, int64_t M, int32_t *perm,
                  int32_t *scratch, hplStream stream);
/* Per-tile gather indices of a row-ordered launch: tile j covers output rows row_perm[j*BM .. j*BM+BM) (identity
 * when row_perm is NULL); tile_idx[j][f][r] = nbr[f][row_perm[j*BM + r]] (-1 past M), tile_mask[j][0] = taps present
 * in the tile, [2 + b] = taps present in its b-th block of 32 rows, [j][6] = the tile that is scheduled j-th (most taps
 * first: a launch's workgroups then finish within one light tile of each other; equal tap counts in tile order, so
 * that tiles scheduled back to back are neighbours in the row order), the rest 0.  Sizes: ceil(M/BM)*F*BM and
 * ceil(M/BM)*8 int32.  Built once per lattice and row order (models/bilateralNN.py:215-217 gathers through the same
 * table in every layer call). */
int hpl_tile_index(const int32_t *nbr, int64_t nbr_stride, int F, int64_t M, const int32_t *row_perm, int BM,
                   int32_t *tile_idx, int32_t *tile_mask, hplStream stream);

/* Y[m, n] = act(bias[n] + res[...] + sum_{f<F, c<C} A[nbr[f][m], c] * Wt[f*C + c, n]).
 * One call covers: the blur Conv2d((15,1)) over gathered neighbours
 * (models/bilateralNN.py:199-221), every 1x1 Conv2d/Conv3d/Conv1d that follows
 * (bilateralNN.py:219, bnn_flow.py:202-205, HPLFlowNet.py:239-240,426-428), the patch
 * correlation Conv3d((1,15,1)) split into its f-independent pc1 half and its pc2 half
 * (bnn_flow.py:189-202) and the displacement filter Conv2d((15,1))
 * (bnn_flow.py:205).  The gathered tensor is never materialised. */
int hpl_gconv_forward(const hpl_gconv_desc *desc /* HOST */, hplStream stream);
/* same contract, one thread per output element, no MFMA: test/debug reference only */
int hpl_gconv_forward_naive(const hpl_gconv_desc *desc /* HOST */, hplStream stream);

/* dWt[f*C + c, n] (+)= sum_m A[nbr[f][m], c] * dY[m, n]    (weight gradient; split over m
 * with fp32 atomics, so dWt must be zero-initialised by the caller unless accumulating).
 * tap_m / tap_row / tap_ptr (optional, from hpl_tap_lists; tap_max = longest list, M if the
 * centre tap is always present): the sum of tap f then runs over its present vertices only.
 * dbias (optional, [N], zero-initialised by the caller): dbias[n] += sum_m dY[m, n], the bias
 * gradient, from the dY tiles the kernel loads anyway.
 * Wide layers (N >= 256, N % 4 == 0, C >= 128, C % 4 == 0, M >= 8192, 16-byte aligned operands, tap lists given or a dense
 * 1x1 layer without a table, rows_a * lda * 4 and M * lddy * 4 below 2^31) run with both fp32 operands split exactly into
 * three bf16 terms on the bf16 matrix pipe (csrc/wgrad3.hip: fp32-class accuracy, tests/test_gpu_wgrad3.py); HPL_WGRAD3=0 or
 * HPL_MATH=f32 in the environment keep the fp32-MFMA kernel. */
int hpl_gconv_wgrad(const float *A, int64_t lda, int64_t rows_a, const int32_t *nbr,
                    int64_t nbr_stride, int64_t reg_stride, int64_t M, int C, int F,
                    const float *dY, int64_t lddy, int N, float *dWt, int64_t ldw,
                    const int32_t *tap_m, const int32_t *tap_row, const int32_t *tap_ptr,
                    int64_t tap_max, float *dbias, hplStream stream);
/* The same with the largest magnitudes of A (the rows and channels the launch can read) and of dY (hpl_amax; DEVICE scalars):
 * the wide layers then run with both operands as scaled fp16 pairs on the fp16 MFMA (hpl_gconv_desc.wt3_planes == 2: the same
 * arithmetic, half the MFMA work of the bf16 triples).  Either NULL (or HPL_MATH=bf16x3): as hpl_gconv_wgrad. */
int hpl_gconv_wgrad_scaled(const float *A, int64_t lda, int64_t rows_a, const int32_t *nbr,
                           int64_t nbr_stride, int64_t reg_stride, int64_t M, int C, int F,
                           const float *dY, int64_t lddy, int N, float *dWt, int64_t ldw,
                           const int32_t *tap_m, const int32_t *tap_row, const int32_t *tap_ptr,
                           int64_t tap_max, float *dbias, const float *a_amax, const float *dy_amax, hplStream stream);

/* Which kernel instance a launch takes.  hpl_gconv_forward / hpl_gconv_wgrad_scaled pick one of many instances from the
 * shape, the strides and the alignment of the operands; the two queries below run the SAME selection (the launch path launches
 * from the struct they fill) and report it.  They call no HIP function and read no device memory: a pointer counts only as NULL
 * or not and by its 16-byte alignment, so they run on a machine without a GPU.  They return what the launch would return for
 * the same arguments (HPL_EINVAL with hpl_last_error() set for a refused launch); M == 0 leaves the struct zeroed. */
#define HPL_FAMILY_FP32 0      /* fp32 operands on the fp32 MFMA (csrc/gconv.hip) */
#define HPL_FAMILY_PAIRS 2     /* fp16 pairs (csrc/gconv3.hip, csrc/wgrad3.hip) */
#define HPL_FAMILY_TRIPLES 3   /* bf16 triples */
#define HPL_FINISH_NONE 0      /* no split-K: the tiles store the result */
#define HPL_FINISH_SCALAR 1    /* partial tiles summed by the scalar finish kernel */
#define HPL_FINISH_VEC4 2      /* ... by the float4 finish kernel */
typedef struct hpl_gconv_info {
    int32_t family;            /* HPL_FAMILY_* */
    int32_t bm, bn;            /* tile: rows x columns of the output */
    int32_t threads;           /* workgroup size */
    int32_t avec;              /* 16-byte loads of the gathered rows (C % 4 == 0, lda % 4 == 0, A aligned) */
    int32_t f_lds;             /* taps whose indices a tile stages in LDS: 1, 8 or 15 */
    int32_t compact;           /* the three-workgroups-per-CU instance of the 64 x 128 tile (tap groups) */
    int32_t splits;            /* split-K: workgroups per tile (1 = none) */
    int32_t guard_sets;        /* passes over the tiles: 2 = a pair launch with a range guard (split-K: a second set of partial tiles) */
    int32_t col_share;         /* XCD order of a row-permuted launch: XCDs per column tile (0: not column-major, -1: row-major) */
    int32_t col_rows;          /* tile-rows per virtual column in that order */
    int32_t tile_tables;       /* the caller's tile index tables are used (cut for this tile height) */
    int32_t epi_fast;          /* 32-bit buffer addressing in the epilogue */
    int32_t finish;            /* HPL_FINISH_* */
    int32_t tiles_m, tiles_n;
    int64_t grid;              /* workgroups of the (first) tile launch */
} hpl_gconv_info;
int hpl_gconv_launch_info(const hpl_gconv_desc *desc /* HOST */, hpl_gconv_info *info /* HOST */);

#define HPL_WBIAS_NONE 0       /* no bias gradient asked for */
#define HPL_WBIAS_KERNEL 1     /* by the k-tile-0 workgroups of the weight-gradient kernel */
#define HPL_WBIAS_COLSUM 2     /* by a column-sum launch of its own (tap mode, wgrad3) */
typedef struct hpl_wgrad_info {
    int32_t family;            /* HPL_FAMILY_FP32, or the wgrad3 kernel's HPL_FAMILY_PAIRS / HPL_FAMILY_TRIPLES */
    int32_t bn;                /* columns of dWt per tile (rows: 128) */
    int32_t vec;               /* 16-byte loads of A and dY */
    int32_t tap;               /* tap mode: k tiles = (tap, 128-channel block), vertex loops over the tap lists */
    int32_t threads;           /* 256 or 512 */
    int32_t deep;              /* two register sets in flight (the 512-thread form) */
    int32_t tiles_k, tiles_n;
    int32_t bias;              /* HPL_WBIAS_* */
    int32_t pad_;
    int64_t tiles;             /* grid.x = tiles_k * tiles_n */
    int64_t splits;            /* grid.y: slabs of the vertex loop */
    int64_t m_per_split;       /* vertices per slab (tap mode: of the longest list) */
} hpl_wgrad_info;
int hpl_wgrad_launch_info(const float *A, int64_t lda, int64_t rows_a, const int32_t *nbr,
                          int64_t nbr_stride, int64_t reg_stride, int64_t M, int C, int F,
                          const float *dY, int64_t lddy, int N, float *dWt, int64_t ldw,
                          const int32_t *tap_m, const int32_t *tap_row, const int32_t *tap_ptr,
                          int64_t tap_max, float *dbias, const float *a_amax, const float *dy_amax,
                          hpl_wgrad_info *info /* HOST */);

/* out[n] = sum_m X[m*ld + n]   (bias gradients) */
int hpl_colsum(const float *X, int64_t ld, int64_t M, int N, float *out, hplStream stream);
/* dX = dY * (Y > 0 ? 1 : slope)   element-wise on [M][N] views (LeakyReLU backward) */
int hpl_leaky_bwd(const float *dY, int64_t lddy, const float *Y, int64_t ldy, float slope,
                  float *dX, int64_t lddx, int64_t M, int N, hplStream stream);
/* The same; amax (optional, DEVICE): *amax = max(*amax, largest |dX|) -- the operand scale of the wide gradient launches that
 * read dX (hpl_gconv_desc.a_amax), taken while the values are in registers.  The caller clears *amax. */
int hpl_leaky_bwd_amax(const float *dY, int64_t lddy, const float *Y, int64_t ldy, float slope,
                       float *dX, int64_t lddx, int64_t M, int N, float *amax, hplStream stream);
/* out[h, n] (+)= sum_j X[(j*mod + h)*ldx + n], j < rows / mod: the gradient of a residual that was broadcast over the
 * rows / mod blocks of a result (the f-independent pc1 half of the patch correlation, models/bnn_flow.py:192). */
int hpl_psum(const float *X, int64_t ldx, int64_t rows, int64_t mod, int N, float *out, int64_t ldo, int accumulate,
             hplStream stream);
/* out[(f*M + m)*ldo + c] (+)= G[m*ldg + f*C + c]: the data gradient of the displacement filter (whose tap f of vertex m
 * reads row f*M + m, models/bnn_flow.py:205) from the plain GEMM G = g . W. */
int hpl_regroup(const float *G, int64_t ldg, int64_t M, int F, int C, float *out, int64_t ldo, int accumulate,
                hplStream stream);
/* EPE3DLoss (models/epe3d_loss.py:9-10, main.py:213) and its gradient in one launch: pred [N][3] point-major (the
 * flow hpl_plan_run writes), sf (3, N); *loss = mean_n ||pred_n - sf_n||_2 (one workgroup, fixed-order sum:
 * deterministic), grad[n][c] = (pred - sf) / (N * ||.||) (0 where the norm is 0). */
int hpl_epe3d(const float *pred, const float *sf, int64_t N, float *grad, float *loss, hplStream stream);
/* The per-pair losses of a batch (reporting only: the training program's HPL_OP_EPE3D keeps the batch mean and its gradient):
 * pred [batch x n][3] and sf (3, batch x n) pair-major; pair_loss[b] (DEVICE, batch floats) = hpl_epe3d of pair b's rows alone,
 * bit for bit (one workgroup per pair, the same rows per thread, the same tree).  1 <= batch <= 64. */
int hpl_epe3d_pairs(const float *pred, const float *sf, int batch, int64_t n, float *pair_loss, hplStream stream);
/* Pair losses: the loss op of a training batch whose per-pair losses and their gradients somebody else computed
 * (hpl_selfsup_loss).  grad[i][c] = dflow[i][c] * (1 / batch) over rows x 3 contiguous floats: the gradient of the mean over the
 * `batch` (1 .. 64) pairs, what W ranks of one pair each average (16-byte accesses where dflow and grad reach a 16-byte boundary
 * together, scalar before, after and otherwise).  *loss (DEVICE) = the float32 sum of pair_loss[b * loss_stride], b = 0 .. batch - 1
 * in ascending order from 0, divided by (float)batch -- a second launch of one wave; no atomic, no workgroup waits for another
 * (loss_stride = 4 reads column L of hpl_selfsup_loss's [batch][4] output).  grad or loss may be NULL, not both.  Stream-ordered.
 * HPL_EINVAL before any launch (and without a device): batch outside 1 .. 64; a null dflow with grad; neither grad nor loss
 * asked for; loss without pair_loss or with loss_stride < 1; a pointer that is not 4-byte aligned; rows < 0 or >= 2^31 / 3. */
int hpl_pair_grad(const float *dflow, int64_t rows, int batch, const float *pair_loss, int loss_stride, float *grad, float *loss,
                  hplStream stream);
/* One pair of hpl_flow_metrics: n points; component k of point p of pred at pred[k * pred_sc + p * pred_sp] (elements), gt and
 * pc1 likewise -- (3, N) clouds (sc = N, sp = 1), the point-major [N][3] flow the forward writes (sc = 1, sp = 3) and column
 * slices of wider buffers are all read in place.  camera = (f, cx, cy, constx, consty, constz) of utils/geometry.py:42-65,
 * used when has_camera != 0. */
typedef struct hpl_metrics_pair {
    const float *pred;
    const float *gt;
    const float *pc1;
    int64_t n;
    int64_t pred_sc, pred_sp, gt_sc, gt_sp, pc1_sc, pc1_sp;
    float camera[6];
    int32_t has_camera;
    int32_t pad_;
} hpl_metrics_pair;
/* The evaluation metrics of `batch` (1 .. 64) pairs in ONE launch (evaluation_utils.py:4-36, utils/geometry.py:6-65), one
 * workgroup per pair.  out (DEVICE) gets 8 doubles per pair, row b for pairs[b]: [0] n, [1] sum of ||gt - pred||, [2] [3] [4]
 * the counts of the ACC3DS / ACC3DR / Outliers3D predicates, [5] the sum of the 2D end-point error of pc1 + gt against
 * pc1 + pred projected into the pair's camera, [6] the count of the ACC2D predicate, [7] 0.  Slots 5 and 6 are not written
 * for a pair without a camera.  Per point the reference's float32 arithmetic in its order (IEEE division and sqrt); sums
 * in fp64 and counts as integers in a fixed order, so a pair's row is the same bits alone or anywhere in a batch.
 * `pairs` (HOST) is copied into `stage` (DEVICE, batch entries) with hipMemcpyAsync on `stream`: pass pinned memory and
 * keep it unchanged until the copy has run.  HPL_EINVAL before any copy or launch for a batch outside 1 .. 64, a count
 * < 1, a null pointer or a negative stride. */
int hpl_flow_metrics(const hpl_metrics_pair *pairs /* HOST */, int batch, hpl_metrics_pair *stage, double *out,
                     hplStream stream);
/* The scalars of one hpl_transform_pair call, drawn on the host (transforms/transforms.py:565-606).  m: the together matrix
 * scale . rot_y^T, row-major (a = p . m + bias); m2: cloud 2's rotation, row-major (b = b . m2^T + shift2).  Jitter k of
 * component c is clip(jitter_sigmaK * N(0, 1), -jitter_clipK, jitter_clipK) as float32; a clip of 0 gives exactly ±0.  The
 * depth cut keeps a point when a.z < depth_threshold and b.z < depth_threshold, or always when depth_threshold <= 0.  augment
 * = 0: ProcessData (a = p1, b = p2, sf = p2 - p1: m, shift, m2, shift2 and the jitter are unused).  seed is the Philox key,
 * counter the call number (two words of the Philox counter). */
typedef struct hpl_transform_params {
    float m[9];
    float shift[3];
    float m2[9];
    float shift2[3];
    double jitter_sigma1, jitter_clip1, jitter_sigma2, jitter_clip2;
    float depth_threshold;
    int32_t no_corr;
    int32_t num_points;
    int32_t allow_less_points;
    int32_t augment;
    int32_t pad_;
    uint64_t seed;
    uint64_t counter;
} hpl_transform_params;
/* Augmentation.__call__ / ProcessData.__call__ (transforms/transforms.py:494-640) of ONE pair, from the raw clouds to the
 * sampled (pc1, pc2, sf), in one enqueue.  pc1, pc2: the clouds as loaded, (M, 3) float32 row-major, the same M (the
 * reference pairs them point by point).  Per point the reference's operations in its order (bias = shift + jitter1,
 * a = p1 . m + bias, b = p2 . m + bias, b = b . m2^T + shift2, sf = b - a, b += jitter2 unless no_corr), each product
 * column as fmaf(z, m[2][c], fmaf(y, m[1][c], x * m[0][c])) -- numpy's float32 chain; then the depth cut (:509-512) and the
 * sampling (:514-532).  Random draws come from Philox4x32-10 keyed by params->seed, counter (point, counter lo, counter hi,
 * purpose): 0 jitter 1, 1 jitter 2 (Box-Muller in fp64), 2 / 3 the 63-bit selection keys of cloud 1 / cloud 2.  The emitted
 * rows: the num_points valid points of smallest (key, index) in ascending key order when at least num_points are valid; every
 * valid point in index order when num_points <= 0, or when fewer are valid and allow_less_points is set; none (a
 * rejection) when fewer are valid without it, or when none is.  no_corr: cloud 2's rows are drawn independently from the
 * same valid set (purpose 3), else they are cloud 1's; sf rows always follow cloud 1.
 * Outputs: out_pc1 / out_pc2 / out_sf hold `capacity` x 3 floats each; k emitted rows are written as (3, k) row-major at
 * their start.  counts (DEVICE, 2 int32) = (valid points, k), k = 0 for a rejection -- the one word pair the host reads back.
 * Test hook (NULL otherwise): jitter1 / jitter2 (DEVICE, (M, 3) float32) replace the jitter draws; sel1 / sel2 (DEVICE,
 * n_sel indices into the raw clouds, 0 <= index < M; sel2 needed with no_corr) replace the selection when any point is
 * valid (k = n_sel).  `params` (HOST) is copied with hipMemcpyAsync on `stream` into the workspace: pass pinned memory and
 * keep it unchanged until the copy has run.  workspace (DEVICE, 256-byte aligned): hpl_transform_workspace_bytes(M).
 * HPL_EINVAL before any copy or launch for a null or misaligned pointer (arrays 4-byte aligned), M < 1 or M >= 2^31 - 1,
 * a capacity below what num_points can emit (hpl_transform_capacity), a short workspace, a negative clip, or hook
 * indices without their pair or outside 1 .. capacity. */
int hpl_transform_pair(const float *pc1, const float *pc2, int64_t M, const hpl_transform_params *params /* HOST */,
                       const float *jitter1, const float *jitter2, const int32_t *sel1, const int32_t *sel2, int64_t n_sel,
                       float *out_pc1, float *out_pc2, float *out_sf, int64_t capacity, int32_t *counts, void *workspace,
                       int64_t workspace_bytes, hplStream stream);
/* bytes of hpl_transform_pair's workspace for M points (0 for M outside 1 .. 2^31 - 2) */
int64_t hpl_transform_workspace_bytes(int64_t M);
/* *capacity = the most rows hpl_transform_pair can emit for M points: min(num_points, M), or M when num_points <= 0.
 * HPL_EINVAL for M outside 1 .. 2^31 - 2 or a null pointer. */
int hpl_transform_capacity(int64_t M, int num_points, int64_t *capacity /* HOST */);
/* the Philox4x32-10 block hpl_transform_pair draws from, on the host: out = philox(counter[4], key[2]) (HOST arrays) */
int hpl_philox4x32_10(const uint32_t *counter, const uint32_t *key, uint32_t *out);
/* optimizer.step() of main.py:216 for the Adam of main.py:138-140 (lr 1e-4, weight_decay 0, no amsgrad) over FLAT fp32 arrays,
 * step >= 1 counting this one: m = lerp(m, g, 1 - beta1); v = beta2 v + (1 - beta2) g^2;
 * p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps) -- torch's fused Adam operation by operation, the
 * scalars computed in double and rounded once as there.  The training plan keeps parameters, gradients and both moments of a
 * model in four arrays of one layout, so a step is ONE launch over 19.3 M elements instead of four multi-tensor launches.
 * All pointers 16-byte aligned. */
int hpl_adam_flat(float *p, const float *g, float *m, float *v, int64_t n, double lr, double beta1, double beta2, double eps,
                  int64_t step, hplStream stream);

/* Per-tap lists of present vertices: list_m[tap_ptr[f] .. tap_ptr[f+1]) = { m : nbr[f][m] >= 0 }
 * ascending, list_row = their source rows nbr[f][m]; both hold up to F*M entries, tap_ptr F+1
 * (DEVICE).  scratch: 2*F*ceil(M/1024) + 1100 int32.  Consumer: hpl_gconv_wgrad (exact skipping
 * of absent neighbours, indices prefetched as plain streams). */
int hpl_tap_lists(const int32_t *nbr, int64_t nbr_stride, int F, int64_t M, int32_t *list_m,
                  int32_t *list_row, int32_t *tap_ptr, int32_t *scratch, hplStream stream);

/* *flag (int32, DEVICE, set to 1 by the caller) is cleared unless the table is symmetric:
 * nbr[0][m] == m and nbr[f][m] = g >= 0  =>  nbr[F-f][g] == m (f >= 1).  A symmetric blur / corr
 * table lets the backward w.r.t. the features run as a gather with mirrored taps instead of
 * fp32 atomics (true by construction unless the reference's unchecked key
 * packing aliased a neighbour key, A.2).  Several tables can share one stream and be read back once. */
int hpl_table_symmetric(const int32_t *nbr, int64_t nbr_stride, int F, int64_t M, int32_t *flag,
                        hplStream stream);

/* dst[m*ldd + c] = src[c*lds + m]  (channel-first <-> channel-last at the API edge) */
int hpl_transpose(const float *src, int64_t lds, float *dst, int64_t ldd, int64_t rows_src,
                  int64_t cols_src, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Lattice construction on the device (replaces the Numba + CFFI khash path:
 * transforms/transforms.py:133-261,300-353,358-485 and models/khash_int2int.h:8-33)
 * ------------------------------------------------------------------------ */
/* Float part, transforms/transforms.py:300-353.  pc (3, N) float32 (unscaled), the level
 * scale is applied inside (:377-378).  keys: int32 [4 coord][N][4 remainder]; bary (4, N);
 * emg (el_minus_gr): (4, N) like the reference when emg_ld == 0, else point-major
 * emg[n*emg_ld + j] (emg_ld >= 4: the channel-last layout the layers consume, so that both
 * clouds of a pair can be written into one matrix).  Bit-identical to oracle/lattice_oracle.c
 * (explicit fmaf chain, half-even rounding, stable descending rank). */
int hpl_lattice_keys(const float *pc, int64_t N, float scale, int32_t *keys, float *bary,
                     float *emg, int64_t emg_ld, hplStream stream);

/* The same for both clouds of a level in one launch.  Points: (3, n) arrays pc1 / pc2, or -- when
 * pc1 == pc2 == NULL -- the vertices of the previous level given by their integer keys vk1 / vk2
 * ([4][vstride], first n columns) and `divisor`, computed on the fly exactly as
 * hpl_lattice_next_points does (the (3, H) arrays of transforms.py:461-467 are never written). */
int hpl_lattice_keys_pair(const float *pc1, const float *pc2, const int32_t *vk1, const int32_t *vk2,
                          int64_t vstride1, int64_t vstride2, float divisor, int64_t n1, int64_t n2,
                          float scale, int32_t *keys1, int32_t *keys2, float *bary1, float *bary2,
                          float *emg1, float *emg2, int64_t emg_ld, hplStream stream);

/* Integer part, stage 1 (transforms/transforms.py:171-207 and :384-391): per-coordinate
 * key range over both clouds, mixed-radix packing (key2int, :70-86), one open-addressing
 * 64-bit table per cloud -- each workgroup first deduplicates its 1024 keys in an LDS
 * table, then only distinct keys CAS into the global table -- and vertex ids in
 * first-appearance order (points outer, remainder inner).  Outputs:
 *   off1/off2 int32 [4][n]   lattice_offset
 *   vkeys1/2  int32 [4][4n]  key of every vertex (first H columns valid)
 *   counts    int32 [2]      H1, H2  (DEVICE; the host reads them to size stage 2)
 * `workspace` (hpl_lattice_workspace_bytes(n1, n2) bytes) keeps the tables for stage 2. */
int64_t hpl_lattice_workspace_bytes(int64_t n1, int64_t n2);
int hpl_lattice_hash(const int32_t *keys1, int64_t n1, const int32_t *keys2, int64_t n2,
                     int32_t *off1, int32_t *off2, int32_t *vkeys1, int32_t *vkeys2,
                     int32_t *counts, void *workspace, int64_t workspace_bytes, hplStream stream);

/* Integer part, stage 2 (transforms/transforms.py:209-255): neighbour tables by hash lookup.
 * Radius -1 skips a table (pointer may be NULL).  H1, H2 are the counts read back from
 * stage 1.  blur1 [F][H1], blur2 [F][H2], corr1 [K][H1] (may be NULL with corr2 given: the caller
 * reuses blur1 when the radii are equal); corr2 is written directly in the
 * kernel-ready permuted layout [K][F*H1] (see hpl_corr2_permute).  Misses are -1; like the
 * reference, neighbour keys are packed without a range check.
 * blur_stride == 0: both blur tables are dense ([F][H1], [F][H2]).  Otherwise both have row
 * stride blur_stride and the ids in blur2 are shifted by blur2_shift: with blur2 = blur1 + H1,
 * blur_stride = H1 + H2, blur2_shift = H1 the two tables form ONE table [F][H1+H2] of the pair
 * (cloud 2's vertices numbered behind cloud 1's) -- the Down layers then run once per pair. */
int hpl_lattice_neighbors(const void *workspace, int64_t n1, int64_t n2,
                          const int32_t *vkeys1, const int32_t *vkeys2, int64_t H1, int64_t H2,
                          int bcn_radius, int corr_filter_radius, int corr_corr_radius,
                          int32_t *blur1, int32_t *blur2, int64_t blur_stride, int64_t blur2_shift,
                          int32_t *corr1, int32_t *corr2, hplStream stream);

/* Next level's points (transforms.py:461-467): out (3, H) = E^T (vkeys / divisor), divisor =
 * (float)(expected_std * scale) computed by the caller in double like the reference. */
int hpl_lattice_next_points(const int32_t *vkeys, int64_t vstride, int64_t H, float divisor,
                            float *out, hplStream stream);


/* ------------------------------------------------------------------------ *
 * Native forward executor: a whole model forward in ONE call
 *
 * The reference's forward (models/HPLFlowNet.py:238-430, models/HPLFlowNet_shallow.py:171-311) is ~130 kernel
 * launches per pair whose shapes follow the pair's vertex counts.  Issuing them from Python costs more host time
 * than the GPU needs on dense clouds; here the host side prepares a PLAN once per model -- the list of
 * operations with symbolic row counts, weight images and biases already resolved to device pointers -- and every
 * forward is one hpl_plan_run() that walks it with the lattice tables of the pair (hpl_level_tables).
 * The plan knows nothing about HPLFlowNet: hplflownet_amd/plan.py writes the program from the model's wiring.
 * ------------------------------------------------------------------------ */
/* Row-count symbols.  Level L (0-based) owns symbols HPL_SYM_LEVEL0 + 8*L + k. */
#define HPL_SYM_ZERO (-1)
#define HPL_SYM_N0 0          /* points of cloud 1 */
#define HPL_SYM_N1 1          /* points of cloud 2 */
#define HPL_SYM_NP 2          /* N0 + N1 */
#define HPL_SYM_LEVEL0 8
#define HPL_SYM_H0 0          /* vertices of cloud 1 at level L */
#define HPL_SYM_H1 1          /* vertices of cloud 2 */
#define HPL_SYM_HP 2          /* H0 + H1 */
#define HPL_SYM_FH0 3         /* 15 * H0: virtual vertices of the patch correlation */
#define HPL_SYM_IN0 4         /* input points of cloud 1 at level L (N0, or H0 of level L-1) */
#define HPL_SYM_INP 5         /* input points of both clouds */
#define HPL_SYM_FH1 6         /* 15 * H1: rows of the inverse pc2 correlation table per tap */
#define HPL_MAX_LEVELS 8

#define HPL_OP_GCONV 1        /* hpl_gconv_forward (incl. tap-group passes) */
#define HPL_OP_SPLAT 2        /* hpl_splat */
#define HPL_OP_SLICE 3        /* hpl_slice */
#define HPL_OP_COPY 4         /* out[:, cols] = a[:, cols]   (the torch.cat calls of the reference forward) */
                              /* a.buf == -1: el_minus_gr of `level`, C == 4; C == 8: el_minus_gr | 1, 0, 0, 0 (the constant input
                               * column of a folded bias, hpl_weight_fold) */
#define HPL_OP_LOAD 5         /* out rows = transpose of an external (3, N) cloud (ext: 0 = pc1, 1 = pc2) */

/* Training (hpl_plan_run_range): the backward of the same program as more operations of the same plan.  Each is the
 * hand-written gradient of one forward op (what autograd derives for models/bilateralNN.py:151-238 and
 * models/bnn_flow.py:119-208), written by hplflownet_amd/plan.py in reverse order. */
#define HPL_OP_WGRAD 6        /* hpl_gconv_wgrad: a = the forward op's input, b = the gradient of its output; weight = index of
                                 the gradient image, bias = index of the bias-gradient vector or -1 */
#define HPL_OP_LEAKY_BWD 7    /* hpl_leaky_bwd: a = dY, b = Y, out = dX (may be a) */
#define HPL_OP_COLSUM 8       /* hpl_colsum of a [m_sym][C] into bias vector `bias` */
#define HPL_OP_SPLAT_BWD 9    /* gradient of HPL_OP_SPLAT: hpl_slice with the normaliser as vertex scale (pair CSR: one per cloud) */
#define HPL_OP_PSUM 10        /* hpl_psum: a [F*m_sym][N] -> out [m_sym][N] */
#define HPL_OP_REGROUP 11     /* hpl_regroup: a [m_sym][F*C] -> out [F*m_sym][C] */
#define HPL_OP_ZERO 12        /* out = 0 */
#define HPL_OP_EPE3D 13       /* the run's loss (hpl_plan_run_range_loss loss_kind; hpl_epe3d on the run's flow / sf / loss by default); out = gradient [N0][3] */
/* loss_kind of hpl_plan_run_range_loss: what HPL_OP_EPE3D computes (1 is not assigned: it is kept for a per-pair EPE3D and refused) */
#define HPL_LOSS_ROWS 0         /* hpl_epe3d: the mean over all N0 rows (one pair, or pairs of equal counts) */
#define HPL_LOSS_GRAD 2         /* hpl_pair_grad: a per-pair loss and its gradient computed between the ranges (sf may be NULL) */
#define HPL_OP_VCOPY 14       /* bias vector `bias` = bias vector `weight` (N entries): a gradient shared by two parameters */
#define HPL_OP_UNLAYOUT 15    /* hpl_weight_unlayout_batch of bucket `aux` (hpl_plan_set_unlayout) */
#define HPL_OP_GSUM 16        /* hpl_gather_sum: a = Z, out [m_sym][N], F = taps, table HPL_TBL_CORR2 (forward, col_step = N) or, with
                                 HPL_FLAG_INVERSE, through the inverse table held (as int32) by buffer b (col_step = 0, out = dense rows of N) */
#define HPL_OP_INVERT 17      /* hpl_table_invert of the level's corr2 table into buffer `out` (as int32 [15][15*H1]) */

#define HPL_FLAG_ACCUM 1      /* the op adds to what `out` holds (gconv: first pass with res = out) */
#define HPL_FLAG_SCATTER 2    /* gconv: scatter epilogue through the level's corr2 table, aux = channels per tap (scat_c) */
#define HPL_FLAG_TAPS 4       /* wgrad: sum over the per-tap vertex lists of the level's cloud-1 blur table (when the run has them) */
#define HPL_FLAG_INVERSE 16   /* HPL_OP_GSUM: see there */
#define HPL_FLAG_SIDE 8       /* the op is a leaf of the backward graph: it may run on the side stream of hpl_plan_run_range */
#define HPL_FLAG_NOYAMAX 64   /* gconv: no wide launch reads the result (a slice does): its largest magnitude is not reduced */
#define HPL_FLAG_NOGUARD 32   /* gconv: the fp16-pair form of this op runs WITHOUT its range guard (hpl_gconv_desc.a_guard): the data gradients
                                 of the training program -- a quiet row of a gradient matrix is a vertex whose share of every weight gradient
                                 lies below the rounding of the sums; the guard would run their launches twice (round 6: 1.4 ms of a step) */

#define HPL_TBL_NONE 0
#define HPL_TBL_BLUR_PAIR 1   /* blur table of the stacked pair [15][H0+H1]          (Down convs) */
#define HPL_TBL_BLUR0 2       /* its cloud-1 columns                                  (Up convs) */
#define HPL_TBL_CORR1 3       /* pc1_corr_indices [15][H0] */
#define HPL_TBL_CORR2 4       /* pc2_corr_indices, permuted [15][15*H0] */
#define HPL_TBL_REGULAR 5     /* no table: tap f of row m reads row f*sym[reg_stride_sym] + m */
#define HPL_TBL_CSR_PAIR 6    /* splat CSR of the stacked pair */
#define HPL_TBL_CSR_C0 7      /* splat CSR of cloud 1 alone (prefix of the pair CSR) */
#define HPL_TBL_CLOUD0 8      /* barycentric / offsets of cloud 1's input points (slice) */

#define HPL_ORD_NONE 0
#define HPL_ORD_PERM 1        /* rows in the table's single-pass tap order when the lattice has one */
#define HPL_ORD_GROUPS 2      /* tap-group passes when the lattice has group orders, else as HPL_ORD_PERM */

#define HPL_COND_ALWAYS 0
#define HPL_COND_SHRINK 1     /* the level's slice shrinks the row count: input points of cloud 1 < its vertices
                                 (the slice-before-1x1 order of an Up layer pays, bcl.BilateralConvFlex.forward_cl) */
#define HPL_COND_NOT_SHRINK 2

#define HPL_BUF_OUT (-2)      /* hpl_ref.buf: the caller's output matrix [N0][3] */

typedef struct hpl_ref {      /* rows [sym[row_off_sym], + sym[rows_sym]) x columns [col_off, col_off+cols) of buffer `buf` */
    int32_t buf;              /* index into the plan's buffers, HPL_BUF_OUT, or -1 = absent */
    int32_t row_off_sym;      /* HPL_SYM_ZERO: from the first row */
    int32_t rows_sym;         /* HPL_SYM_ZERO: to the last row */
    int32_t col_off;
    int32_t cols;
} hpl_ref;

typedef struct hpl_buf {      /* an activation matrix the executor allocates from the workspace per run */
    int32_t rows_sym;
    int32_t cols;
} hpl_buf;

typedef struct hpl_weight {   /* a re-laid weight image (hpl_weight_relayout) */
    const float *Wt;
    int64_t ldw;
    int64_t rows;
    const void *Wt3;          /* optional: hpl_weight_split3 / hpl_weight_split2h of the whole image (NULL: the layer stays on the fp32 MFMA) */
    int64_t wt3_plane_stride;
    const float *w_amax;      /* wt3_planes == 2: the scalar hpl_weight_split2h wrote */
    int32_t wt3_planes;
    int32_t pad_;
} hpl_weight;

typedef struct hpl_op {
    int32_t kind;             /* HPL_OP_* */
    int32_t tag;              /* profiling class (hpl_plan_profile) */
    hpl_ref a, out, res;
    int32_t m_sym;            /* rows produced: gconv M, splat H, slice N, copy / load rows */
    int32_t res_mod_sym;      /* gconv residual period (HPL_SYM_ZERO: the residual has M rows) */
    int32_t level;            /* lattice level whose tables are used */
    int32_t table;            /* HPL_TBL_* */
    int32_t order;            /* HPL_ORD_* */
    int32_t F, C, N;          /* taps, channels taken from `a`, output channels */
    int32_t weight;           /* index into the plan's weight images, -1 = none */
    int32_t bias;             /* index into the plan's bias pointers, -1 = none */
    int32_t act;              /* HPL_ACT_* */
    float slope;
    int32_t use_norm;         /* splat: density normalisation */
    int32_t reg_stride_sym;   /* HPL_TBL_REGULAR */
    int32_t ext;              /* HPL_OP_LOAD: 0 = pc1, 1 = pc2 */
    int32_t cond;             /* HPL_COND_*: run the op only if the condition holds at level cond_level */
    int32_t cond_level;
    hpl_ref out2;             /* gconv: optional second destination (buf == -1: none), see hpl_gconv_desc.Y2 */
    int32_t rows2_sym;        /* rows of the result that go to out2 as well */
    hpl_ref b;                /* second input of the backward ops (buf == -1: none) */
    int32_t flags;            /* HPL_FLAG_* */
    int32_t aux;
} hpl_op;

/* Kernel-ready tables of one lattice level of a pair (what hplflownet_amd.lattice builds on the device;
 * the schema of `generated_data`, transforms/transforms.py:471-483, in int32 / CSR form). */
typedef struct hpl_level_tables {
    int64_t n0, n1;                   /* input points per cloud */
    int64_t H0, H1;                   /* vertices per cloud */
    const float *emg_pair;            /* el_minus_gr, both clouds, point-major [n0+n1][4] */
    const int32_t *csr_ptr;           /* pair CSR (hpl_csr_build_pair): [H0+H1+1] */
    const int32_t *csr_pt;            /* [4*(n0+n1)] */
    const float *csr_w;
    const float *csr_norm;            /* [H0+H1] */
    const float *bary0;               /* cloud 1: [4][n0] */
    const int32_t *off0;
    const int32_t *blur;              /* pair blur table [15][blur_stride], NULL if the level has none */
    int64_t blur_stride;
    const int32_t *blur_perm;         /* hpl_tap_order of the pair table or NULL */
    const int32_t *up_perm;           /* hpl_tap_order of its cloud-1 columns or NULL */
    int32_t n_up_groups;              /* >= 2: tap groups [cut[i], cut[i+1]) with their own row orders */
    int32_t up_group_cut[5];
    const int32_t *up_group_perm[4];
    const int32_t *corr1;             /* [15][corr1_stride] or NULL */
    int64_t corr1_stride;
    const int32_t *corr1_perm;
    const int32_t *corr2;             /* [15][15*H0] or NULL */
    /* optional per-tile index tables (hpl_tile_index, tiles of tile_bm rows) of the row orders above; NULL = none */
    int32_t tile_bm;
    int32_t group_tile_bm;            /* tile height of the up_group tables (128: the split-operand kernel's tiles) */
    const int32_t *blur_perm_tidx, *blur_perm_tmask;
    const int32_t *up_perm_tidx, *up_perm_tmask;
    const int32_t *up_group_tidx[4], *up_group_tmask[4];
    const int32_t *corr1_perm_tidx, *corr1_perm_tmask;
    /* training only (zero otherwise): cloud 2's barycentric weights / offsets [4][n1] (the splat's gradient), and the per-tap
     * vertex lists of the cloud-1 blur table (hpl_tap_lists; up_tap_max = its longest list or H0) */
    const float *bary1;
    const int32_t *off1;
    const int32_t *up_tap_m, *up_tap_row, *up_tap_ptr;
    int64_t up_tap_max;
} hpl_level_tables;

typedef struct hpl_plan hpl_plan;   /* not thread-safe: one thread runs a given plan at a time (any number of streams) */

/* HOST arrays, copied.  The weight images and biases must stay alive (and may be refreshed in place). */
hpl_plan *hpl_plan_create(const hpl_op *ops, int n_ops, const hpl_buf *bufs, int n_bufs,
                          const hpl_weight *weights, int n_weights, const float *const *biases, int n_biases);
void hpl_plan_destroy(hpl_plan *plan);
/* bytes of workspace a run with these tables needs (activations + 64 MB of split-K partials) */
int64_t hpl_plan_workspace_bytes(const hpl_plan *plan, const hpl_level_tables *levels /* HOST */, int n_levels);
/* One forward: pc1 (3, n0), pc2 (3, n1) float32 -> out [n0][3] (the flow, point-major); everything is enqueued
 * on `stream`; `workspace` must not be reused before the run has finished on the device. */
int hpl_plan_run(hpl_plan *plan, const hpl_level_tables *levels /* HOST */, int n_levels, const float *pc1,
                 const float *pc2, float *out, void *workspace, int64_t workspace_bytes, hplStream stream);
/* Ops [op_begin, op_end) of the plan only (same carving of the workspace in every call: a step may be issued in
 * pieces, e.g. to start a gradient all-reduce between them).  sf (3, n0) and loss (DEVICE, one float) serve HPL_OP_EPE3D
 * (NULL: such an op is an error); side_stream (or NULL): ops flagged HPL_FLAG_SIDE are enqueued there behind an event on
 * `stream` (an un-layout flagged that way follows the weight gradients it reads on that stream); `stream` waits for them before
 * an HPL_OP_UNLAYOUT that runs on it and, with join != 0, at the end of the range (always join in the LAST range of a step). */
int hpl_plan_run_range(hpl_plan *plan, const hpl_level_tables *levels /* HOST */, int n_levels, const float *pc1,
                       const float *pc2, const float *sf, float *out, float *loss, void *workspace,
                       int64_t workspace_bytes, hplStream stream, hplStream side_stream, int op_begin, int op_end, int join);
/* hpl_plan_run_range with the loss of HPL_OP_EPE3D chosen at run time (HPL_LOSS_*).  HPL_LOSS_GRAD: `batch`
 * (1 .. 64) pairs whose first rows are prefix[0 .. batch] (HOST; prefix[batch] must be the run's n0); pair_loss (DEVICE) holds the
 * per-pair losses at pair_loss[b * loss_stride] and dflow [n0][3] their gradients, both written between the forward range and
 * the range with the loss op (they are read where that op runs); *loss becomes the mean over the pairs, the loss gradient dflow
 * / batch; sf may be NULL.  HPL_LOSS_ROWS ignores the six and is hpl_plan_run_range. */
int hpl_plan_run_range_loss(hpl_plan *plan, const hpl_level_tables *levels /* HOST */, int n_levels, const float *pc1,
                            const float *pc2, const float *sf, float *out, float *loss, void *workspace, int64_t workspace_bytes,
                            hplStream stream, hplStream side_stream, int op_begin, int op_end, int join, int loss_kind, int batch,
                            const int64_t *prefix /* HOST */, float *pair_loss, int loss_stride, const float *dflow);
/* The un-layout jobs of HPL_OP_UNLAYOUT: bucket i = jobs [bucket_first[i], bucket_first[i+1]) of the DEVICE tables
 * (hpl_weight_unlayout_batch); src = the gradient images (image of job j at src + prefix[j]). */
int hpl_plan_set_unlayout(hpl_plan *plan, const hpl_relayout_job *jobs /* DEVICE */, const int64_t *prefix /* DEVICE */,
                          const float *src, const int32_t *bucket_first /* HOST, n_buckets + 1 */,
                          const int64_t *bucket_offset /* HOST, n_buckets + 1: prefix[bucket_first[i]] */, int n_buckets);
/* Profiling: with tag >= 0 every following run brackets the ops of that tag with HIP events on the run's stream
 * (tag < 0: off).  hpl_plan_profile_read waits for the recorded events and returns the number of bracketed
 * launches, their total duration in ms, and resets the record. */
int hpl_plan_profile(hpl_plan *plan, int tag);
/* Launches of this plan's runs so far that took the second pass of the fp16-pair form's range guard (hpl_gconv_desc.a_guard):
 * an operand with a row 2^18 or more below the matrix's largest magnitude.  Synchronises with the device. */
int hpl_plan_guard_trips(hpl_plan *plan, int64_t *count);
/* clock_probe (DEVICE, 2 x int64, or NULL) is handed to the gather-GEMM launches of the profiled tag
 * (hpl_gconv_desc.clock_probe): they accumulate their samples there. */
int hpl_plan_clock_probe(hpl_plan *plan, int64_t *clock_probe);
int hpl_plan_profile_read(hpl_plan *plan, int *launches, float *total_ms);
/* Batched inference (the reference's forward takes one pair: README.md:57, models/HPLFlowNet.py:238-430).  `levels` are
 * the tables of a batch of `batch` pairs built by hpl_lattice_begin_batch: one pair of clouds whose rows are pair-major
 * and whose tables link no two pairs, so the program runs unchanged on the summed row counts.  pc1 (batch, 3, n0 / batch),
 * pc2 (batch, 3, n1 / batch) DEVICE float32; out (DEVICE) receives the flow as (batch, n0 / batch, 3) rows.  One launch
 * lays the clouds out pair-major in the workspace's tail: workspace_bytes >= hpl_plan_workspace_bytes +
 * hpl_plan_batch_extra_bytes.  batch = 1 is hpl_plan_run. */
int64_t hpl_plan_batch_extra_bytes(const hpl_level_tables *levels /* HOST */, int n_levels);
int hpl_plan_run_batch(hpl_plan *plan, const hpl_level_tables *levels /* HOST */, int n_levels, int batch, const float *pc1,
                       const float *pc2, float *out, void *workspace, int64_t workspace_bytes, hplStream stream);
/* Batched training: pc1 (batch, 3, n1), pc2 (batch, 3, n2) and, if not NULL, sf (batch, 3, n1), all DEVICE float32, laid out
 * as (3, batch x n) pair-major matrices dst1 / dst2 / dst_sf in one launch (16-byte accesses when n1 and n2 are multiples of 4
 * and every pointer is 16-byte aligned).  The training plan then runs hpl_plan_run_range on them unchanged. */
int hpl_batch_stage(int batch, int64_t n1, int64_t n2, const float *pc1, const float *pc2, const float *sf, float *dst1,
                    float *dst2, float *dst_sf, hplStream stream);
/* Ragged batches (pairs of their own point counts; the reference's KITTI evaluation keeps every point of a short frame,
 * configs/test_ours_KITTI.yaml allow_less_points, transforms/transforms.py:517-532, and evaluates one pair per forward,
 * configs/test_ours_KITTI.yaml:15 batch_size 1): B = `batch` (1 .. 64) per-pair clouds per side -- pc1[b] (3, ld1[b]) with n1[b] points, pc2[b] (3, ld2[b])
 * with n2[b] points and, if sf is not NULL, sf[b] (3, ldsf[b]) with n1[b] points; HOST arrays of DEVICE float32 pointers,
 * row k of pair b at pc1[b] + k * ld1[b], so pc[b, :, :n_b] slices of a padded (B, 3, Nmax) tensor need no copy -- laid out as
 * the (3, sum n1) / (3, sum n2) / (3, sum n1) pair-major matrices dst1 / dst2 / dst_sf in ONE launch (the descriptors travel
 * in its arguments; 16-byte accesses when every count and stride is a multiple of 4 and every pointer 16-byte aligned).
 * hpl_lattice_begin_ragged builds on them and hpl_plan_run runs on them unchanged. */
int hpl_ragged_stage(int batch, const float *const *pc1, const int64_t *n1, const int64_t *ld1, const float *const *pc2,
                     const int64_t *n2, const int64_t *ld2, const float *const *sf, const int64_t *ldsf, float *dst1, float *dst2,
                     float *dst_sf, hplStream stream);


/* ------------------------------------------------------------------------ *
 * Native lattice builder: GenerateDataUnsymmetric.__call__ (transforms/transforms.py:358-485) as a state machine
 * over the stage functions above.  One builder = one pair under construction: hpl_lattice_begin launches level 0
 * up to the read-back of its vertex counts (they size the next arrays); hpl_lattice_advance launches the rest of
 * that level (neighbour tables, splat CSR, row orders, per-tile index tables) and the next level up to ITS
 * read-back, and so on.  Every table is carved out of the caller's `arena` (DEVICE, 256-byte aligned); the
 * finished hpl_level_tables point into it.  The host never blocks unless it calls advance before ready.
 * ------------------------------------------------------------------------ */
#define HPL_ENOMEM (-4)   /* the arena is too small: retry with a bigger one */

typedef struct hpl_lattice_spec {
    int32_t n_levels;
    float scale[HPL_MAX_LEVELS];                 /* scales_filter_map[k][0] */
    int32_t bcn_radius[HPL_MAX_LEVELS];          /* [k][1] */
    int32_t corr_filter_radius[HPL_MAX_LEVELS];  /* [k][2], -1 = no correlation at this level */
    int32_t corr_corr_radius[HPL_MAX_LEVELS];    /* [k][3] */
    float next_divisor[HPL_MAX_LEVELS];          /* (float)(expected_std * scale), transforms.py:462-463 */
    int32_t wide_up[HPL_MAX_LEVELS];             /* 1: the level's Up conv runs as tap-group passes, 0: single pass, -1: both */
    int32_t n_groups;                            /* tap groups (>= 2) and their cuts, e.g. {0, 8, 15} */
    int32_t group_cut[5];
    float groups_min_sparsity;                   /* groups only where H0 / n0 >= this */
    int64_t perm_min_rows;                       /* single-pass row orders only for tables with at least this many rows */
    int64_t groups_min_rows;                     /* tap-group row orders (wide, sparse levels) from this many cloud-1 vertices on (0 = perm_min_rows) */
    int32_t group_tile_bm;                       /* tile height of the tap-group tile tables: 64 or 128 (0 = 64) */
    int32_t fused;                               /* != 0: hpl_lattice_begin enqueues the whole build, the vertex counts stay on the
                                                    device and are read back once (csrc/lattice_fused.hip); radius-1 specs only */
} hpl_lattice_spec;

typedef struct hpl_lattice hpl_lattice;   /* one pair under construction per builder; use several builders to overlap pairs */

hpl_lattice *hpl_lattice_create(const hpl_lattice_spec *spec /* HOST */);
void hpl_lattice_destroy(hpl_lattice *b);
/* Fused builds size every array by a bound: a level's vertices per cloud <= min(4 x its input points, bounds[L]), bounds[L]
 * = 0 meaning 18 x max(n0, n1) + 64.  hpl_lattice_arena_bytes: the arena a build of (n0, n1) points needs under the current bounds
 * (0 for a staged builder: its arena is a guess that HPL_ENOMEM corrects).  A pair that outgrows a bound is rebuilt by the
 * staged driver inside the same hpl_lattice_advance protocol (hpl_lattice_stats counts it), so bounds only cost memory and
 * idle workgroups -- e.g. twice the largest counts seen so far.  hpl_lattice_stats: out[0] = kernel launches of the last
 * fused enqueue, out[1] = 1 if the last finished build came from the fused driver, out[2] = builds of this handle that fell back to the staged one. */
int64_t hpl_lattice_arena_bytes(const hpl_lattice *b, int64_t n0, int64_t n1);
int hpl_lattice_set_bounds(hpl_lattice *b, const int64_t *bounds /* HOST, HPL_MAX_LEVELS entries, or NULL */);
int hpl_lattice_stats(const hpl_lattice *b, int32_t *out /* HOST, 3 */);
/* pc1 (3, n0), pc2 (3, n1) float32 DEVICE, must stay valid until the build is complete */
int hpl_lattice_begin(hpl_lattice *b, const float *pc1, const float *pc2, int64_t n0, int64_t n1, void *arena,
                      int64_t arena_bytes, hplStream stream);
/* A batch of `batch` pairs (1 .. 64) in ONE fused build (transforms/transforms.py:358-485 per pair; the reference builds one
 * pair per call, README.md:57): pc1 (batch, 3, n0), pc2 (batch, 3, n1) float32 DEVICE, contiguous, read in place.  The
 * tables are those of one pair of clouds of batch x n0 / batch x n1 pair-major points: pair b's vertices follow pair
 * b - 1's at every level and no table links two pairs; pair b's slice of every table is its single-pair build's plus the
 * offsets.  Same enqueue (about 33 launches) and ONE read-back whatever `batch` is.  Bounds (hpl_lattice_set_bounds) are per
 * pair; a batch that outgrows them is rebuilt on the fused path under the default bounds (hpl_lattice_stats out[2] counts
 * it; HPL_ENOMEM from hpl_lattice_advance if that needs a bigger arena: set the bounds to 0 and begin again).  A pair whose
 * key range at some level does not fit below the pair digit (63 - ceil(log2 batch) bits) fails the build with HPL_EINVAL.  batch = 1 is hpl_lattice_begin.
 * Fused builders only. */
int hpl_lattice_begin_batch(hpl_lattice *b, const float *pc1, const float *pc2, int64_t batch, int64_t n0, int64_t n1,
                            void *arena, int64_t arena_bytes, hplStream stream);
/* the arena hpl_lattice_begin_batch needs for `batch` pairs of (n0, n1) points under the current bounds (-1: bad arguments) */
int64_t hpl_lattice_arena_bytes_batch(const hpl_lattice *b, int64_t batch, int64_t n0, int64_t n1);
/* A ragged batch of `batch` pairs (1 .. 64) in ONE fused build (transforms/transforms.py:358-485 per pair, the pairs'
 * point counts differing as configs/test_ours_KITTI.yaml allow_less_points makes them): pair b has n0[b] / n1[b] >= 1
 * points (HOST arrays), pc1 (3, sum n0) and pc2 (3, sum n1) float32 DEVICE are the pair-major clouds of hpl_ragged_stage.
 * Everything else is hpl_lattice_begin_batch's: pair b's slice of every table is its single-pair build's plus the vertex /
 * point offsets, no table links two pairs, ~33 launches and one read-back, bounds per pair (set them from the largest),
 * the same overflow rebuild and key-range refusal, hpl_lattice_pair_counts.  HPL_EINVAL before any launch for a batch
 * outside 1 .. 64, a count < 1, or a side of more than 163 840 points (the forward's 32-bit offsets).
 * batch = 1 is hpl_lattice_begin.  Fused builders only. */
int hpl_lattice_begin_ragged(hpl_lattice *b, const float *pc1, const float *pc2, int64_t batch, const int64_t *n0 /* HOST */,
                             const int64_t *n1 /* HOST */, void *arena, int64_t arena_bytes, hplStream stream);
/* the arena hpl_lattice_begin_ragged needs under the current bounds (-1: bad arguments) */
int64_t hpl_lattice_arena_bytes_ragged(const hpl_lattice *b, int64_t batch, const int64_t *n0 /* HOST */,
                                       const int64_t *n1 /* HOST */);
/* vertices of every pair of the finished build: out[(L * 2 + cloud) * batch + pair], n_levels x 2 x batch entries */
int hpl_lattice_pair_counts(const hpl_lattice *b, int64_t *out /* HOST */);
/* 1 if hpl_lattice_advance would not block (the pending read-back has landed, or the build is done), else 0 */
int hpl_lattice_ready(hpl_lattice *b);
/* *done = 1 once every launch of the build has been enqueued (the tables are valid for work ordered behind them
 * on the same stream).  HPL_ENOMEM: the arena overflowed, the build is abandoned. */
int hpl_lattice_advance(hpl_lattice *b, int *done);
/* tables of the finished build (n_levels entries, owned by the builder, valid until its next begin) */
const hpl_level_tables *hpl_lattice_tables(const hpl_lattice *b);
/* extra per-level pointers the forward does not need (cloud 2's barycentric / offsets): out[2*L] = bary1,
 * out[2*L+1] = off1; and the bytes of the arena in use */
int hpl_lattice_extras(const hpl_lattice *b, const void **out /* HOST, 2 * n_levels */, int64_t *arena_used);

/* ------------------------------------------------------------------------ *
 * Lattice queries (csrc/lattice_query.hip): where arbitrary points fall in level 0 of cloud 1 of a finished build, without
 * inserting.  The forward's level-0 slice of cloud 1 (bcn1_, models/HPLFlowNet.py:418-430) at the queries' own simplices.
 * ------------------------------------------------------------------------ */
typedef struct hpl_query_info {
    const void *slots;        /* fused build: cloud 1's level-0 table, 16-byte slots {key lo, key hi, first entry, vertex id} */
    const int64_t *keys;      /* staged build (a single pair that outgrew its bounds, or spec.fused == 0): packed keys ... */
    const int32_t *ids;       /* ... and the vertex id of each slot of the same table */
    uint64_t mask;            /* slots of the table - 1 */
    const int32_t *mm;        /* DEVICE [8]: the level's per-coordinate key minima [4] and maxima [4] (single pair) */
    const int32_t *pmm;       /* DEVICE [batch][8]: every pair's own range (batch > 1), else NULL */
    int32_t batch, pair_shift; /* pairs of the build; a batch's packed key is pair << pair_shift | key within the pair's range */
    float scale;              /* level-0 scale (scales_filter_map[0][0]) */
    int32_t H0;               /* level-0 vertices of cloud 1, all pairs (the ids are global, pair-major) */
} hpl_query_info;

/* Call right after hpl_lattice_advance reported done (the pointers stay valid as long as the arena and until the next begin on
 * `b` rewrites the arena; no launch, no copy).  HPL_EINVAL without a finished build. */
int hpl_lattice_query_info(const hpl_lattice *b, hpl_query_info *out /* HOST */);
/* Per query point q (3, Q) float32: its 4 level-0 simplex vertices and barycentric weights (the float statements of the
 * builders' keys stage), each vertex looked up in cloud 1's table.  A vertex whose key lies outside the level's (a batch: its
 * pair's) per-coordinate key range is missing without a probe (the packing is only injective inside it); so is one the table
 * does not hold.  Outputs: off (4, Q) int32 vertex ids (a missing vertex: 0, weight 0), bary (4, Q) float32, coverage (Q)
 * float32 = 1 when every vertex of nonzero weight was found, else the sum of the found weights.  renormalize != 0: the found
 * weights of a query with 0 < coverage < 1 are divided by its coverage (a fully covered query keeps its weights' bits).
 * pair_prefix (HOST, batch + 1 ints, NULL for batch 1): queries [pair_prefix[b], pair_prefix[b + 1]) belong to pair b.
 * HPL_EINVAL before any launch for bad arguments (Q < 1 or >= 2^31, null or misaligned pointers, a prefix that does not
 * start at 0, decreases or ends short of Q).  Stream-ordered, no host synchronisation. */
int hpl_lattice_query(const hpl_query_info *info /* HOST */, const float *q, int64_t Q, const int64_t *pair_prefix /* HOST */,
                      int renormalize, float *bary, int32_t *off, float *coverage, hplStream stream);

/* ------------------------------------------------------------------------ *
 * k nearest neighbours and inverse-distance interpolation (csrc/knn_interp.hip): the feature propagation of point-based
 * scene-flow networks, exact by brute force.  Fills the dense queries the level-0 lattice does not cover.
 * ------------------------------------------------------------------------ */
/* For every query q (3, Q) float32 SoA (row stride q_ld >= Q): its k (1 .. 8) nearest points of ref (3, N) float32 SoA (row
 * stride ref_ld >= N) and the interpolation of val [N][C] float32 row-major (1 <= C <= 16) from them.  batch (1 .. 64) pairs:
 * ref_prefix / q_prefix (HOST, batch + 1 ints each, from 0 to N / Q, non-decreasing) give every pair's points and queries; a
 * query searches its own pair's points only (a pair with queries has >= 1 point).  The prefixes travel in the kernel arguments:
 * stream-ordered, no copy, no host synchronisation.
 * Arithmetic (float32, no contraction; tests/knn_oracle.py restates it in numpy): d2 = (dx * dx + dy * dy) + dz * dz with
 * dx = q.x - p.x; candidates in index order, an entry replaced only by a strictly smaller d2 (ties: the smaller index; a d2
 * that is not below +inf never enters); w_i = 1 / (d2_i + eps); interp = (sum_i w_i * v_i) / (sum_i w_i), i ascending; a
 * nearest d2 of exactly 0 copies that point's row bit for bit.  A query with no neighbour at all (finite coordinates so far
 * apart that every d2 overflows to +inf) gets idx = -1 throughout and a NaN interpolation (0 / 0), also through the blend.
 * idx (k, Q) int32 / dist2 (k, Q) float32, both optional: the neighbours in ascending d2, indices into the packed ref; a pair
 * of fewer than k points leaves idx = -1, dist2 = +inf, and such entries take no part in the interpolation.
 * out [Q][C] float32.  coverage == NULL: out = interp.  coverage (Q) float32: out holds a base value per query and is updated in
 * place: a query of coverage == 1 is neither searched nor written (out, idx, dist2 keep their bits), any other gets
 * coverage * base + (1 - coverage) * interp.
 * HPL_EINVAL before any launch (and without a device): k, C, batch out of range; eps < 0 or not finite; a prefix that does not
 * start at 0 or decreases; a row stride below its count; null ref / val / q / out / prefixes; misaligned arrays; Q * C,
 * N * C or k * Q >= 2^31.  Q == 0 is a no-op. */
int hpl_knn_interp(const float *ref, int64_t ref_ld, const float *val, int C, const float *q, int64_t q_ld, int k, float eps,
                   int batch, const int64_t *ref_prefix /* HOST */, const int64_t *q_prefix /* HOST */, int32_t *idx,
                   float *dist2, float *out, const float *coverage, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Rigid motion from flow (csrc/rigid_fit.hip): the rotation R and translation t that explain most of a pair's scene flow --
 * ego-motion on a mostly static scene --, fitted robustly on the device, and the flow refined by it.
 * ------------------------------------------------------------------------ */
/* Workspace of hpl_rigid_fit for `batch` pairs of n_total points together, in bytes (monotone in both); -1 for a batch
 * outside 1 .. 64 or n_total outside 0 .. 2^31 / 3 - 1. */
int64_t hpl_rigid_fit_workspace_bytes(int batch, int64_t n_total);
/* pc (3, N) float32 SoA (row stride pc_ld >= N); component k of the flow of point i at flow[k * flow_sc + i * flow_sp]
 * (elements, both >= 1 and not overlapping: (3, N) rows and the forward's point-major [N][3] rows are read in place);
 * weight (N) float32 or NULL (all 1).  batch (1 .. 64) pairs: prefix (HOST, batch + 1 ints from 0 to N, non-decreasing) gives
 * every pair's points; it travels in the kernel arguments: stream-ordered, no copy, no host synchronisation,
 * 2 (iters + 1) + 1 launches.
 * Arithmetic per pair (float64 throughout, from the float32 inputs; tests/rigid_oracle.py restates it in numpy with an SVD
 * in place of the quaternion), q_i = p_i + f_i: the effective base weight w_i is the given weight, 0 when that is not in
 * (0, inf) (NaN included) or when a coordinate or a flow component of the point is not finite.  Round 0 uses u_i = w_i; for
 * round k = 0 .. iters (0 .. 16): SOLVE W = sum u_i, the u-weighted centroids mp, mq, H = sum u_i (p_i - mp)(q_i - mq)^T
 * (accumulated about the pair's first point), R = the proper rotation maximising tr(R H) (Horn's unit quaternion: the dominant
 * eigenvector of the symmetric 4x4 matrix of H, cyclic Jacobi; never a reflection), t = mq - R mp; then, if k < iters, REWEIGHT
 * (Geman-McClure) r_i = |R p_i + t - q_i|, u_i = w_i / (1 + (r_i / tau)^2)^2, tau > 0 finite.
 * Rt [batch][12] float32: R row-major, then t, of the last solve.  residual (N) or NULL: r_i against that solve.  A point is
 * an inlier when r_i <= tau and w_i > 0.  refined [N][3] point-major or NULL: R p_i + t - p_i for an inlier, the input flow
 * bit for bit for any other point.  stats [batch][4] float32: status, the inlier share of the pair's points, the rotation
 * angle in degrees, |t|.  status = 1 for a fit; 0 for a pair of fewer than 3 points or whose W is not > 0 (or not finite) at
 * any round: then R = I, t = 0, share 0, residual = |f_i|, refined = the input flow.  All sums in a fixed order, no
 * floating-point atomic: a pair's outputs are the same bits alone, anywhere in a batch and beside other work.
 * workspace: DEVICE, 8-byte aligned, >= hpl_rigid_fit_workspace_bytes(batch, N); refined must not overlap the inputs.
 * HPL_EINVAL before any launch (and without a device): batch, iters or tau out of range; a prefix that does not start at 0
 * or decreases; pc_ld < N; flow strides < 1 or overlapping; null pc / flow / Rt / stats / prefix / workspace; a workspace that
 * is too small; misaligned arrays; N >= 2^31 / 3.  N == 0 is a no-op. */
int hpl_rigid_fit(const float *pc, int64_t pc_ld, const float *flow, int64_t flow_sc, int64_t flow_sp, const float *weight,
                  int batch, const int64_t *prefix /* HOST */, int iters, float tau, float *Rt, float *stats, float *residual,
                  float *refined, void *workspace, int64_t workspace_bytes, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Moving objects from flow (csrc/motion_segment.hip): the points a rigid fit leaves unexplained, grouped into connected
 * components over position and flow, numbered, with each object's size, centroid and mean flow.
 * ------------------------------------------------------------------------ */
/* Workspace of hpl_motion_segment for `batch` pairs of n_total points together, in bytes (monotone in both); -1 for a batch
 * outside 1 .. 64 or n_total outside 0 .. 2^31 / 3 - 1. */
int64_t hpl_motion_segment_workspace_bytes(int batch, int64_t n_total);
/* pc (3, N) float32 SoA (row stride pc_ld >= N), flow through flow_sc / flow_sp and prefix (HOST, batch + 1 ints, batch
 * 1 .. 64) exactly as hpl_rigid_fit reads them; residual (N) float32 as hpl_rigid_fit writes it.  tau > 0 finite, eps > 0
 * finite, dv > 0 (+inf: no flow criterion), min_points >= 1, 1 <= max_objects <= 4096.
 * MOVER: point i is a mover when residual_i > tau (a NaN residual is not), its three coordinates and three flow components
 * are finite, and its cell is representable: cell_k = floor(x_k * (1 / (1.001 * eps))) in float64 (the product 1.001 * eps,
 * the quotient and the product with x_k each rounded once) with |cell_k| <= 2^18 - 2 for k = x, y, z.
 * EDGE: movers i, j of the same pair are linked when d2 <= eps2 and g2 <= dv2, with d2 = (dx * dx + dy * dy) + dz * dz over
 * the positions and g2 the same over the flows, in float32 with every operation rounded and no contraction (the arithmetic of
 * hpl_knn_interp); eps2 = eps * eps and dv2 = dv * dv rounded once to float32.  Points of different pairs never link.
 * COMPONENT: a connected component of that graph; its root is its smallest point index.  OBJECT: a component of at least
 * min_points movers; a pair's objects are numbered 0, 1, ... in ascending root order.
 * labels (N) int32: the object number of a mover in an object (numbers run past max_objects: nothing is dropped here); -1 no
 * mover; -2 noise (a mover in a smaller component); -3 out of range (a mover but for its cell).
 * obj_info [batch][max_objects][2] int32: root (index within the pair) and point count of the pair's first max_objects
 * objects; unused rows -1, 0.  obj_motion [batch][max_objects][6] float32: centroid and mean flow of each: float64 sums of the
 * float32 inputs in a fixed order (no floating-point atomic), divided by the count, rounded once; unused rows 0.
 * stats [batch][4] int32: movers, objects (the true count, which may exceed max_objects), points in objects, points out of
 * range.  Every output of a pair is the same bits alone, anywhere in a batch and beside other work.
 * The grid is an accelerator only: the result is the all-pairs predicate's (tests/segment_oracle.py restates it in numpy).
 * Stream-ordered, a fixed number of launches whose sizes depend on N, batch and max_objects alone, no copy back, no host
 * synchronisation; no lane or workgroup waits for another.
 * workspace: DEVICE, 256-byte aligned, >= hpl_motion_segment_workspace_bytes(batch, N).
 * HPL_EINVAL before any launch (and without a device): batch, tau, eps, dv, min_points or max_objects out of range or NaN; a
 * prefix that does not start at 0 or decreases; pc_ld < N; flow strides < 1 or overlapping; a null array, prefix or
 * workspace; misaligned arrays; a workspace that is too small; N >= 2^31 / 3.  N == 0 is a no-op. */
int hpl_motion_segment(const float *pc, int64_t pc_ld, const float *flow, int64_t flow_sc, int64_t flow_sp,
                       const float *residual, int batch, const int64_t *prefix /* HOST */, float tau, float eps, float dv,
                       int min_points, int max_objects, int32_t *labels, int32_t *obj_info, float *obj_motion, int32_t *stats,
                       void *workspace, int64_t workspace_bytes, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Object motions from flow (csrc/object_fit.hip): hpl_rigid_fit per labelled object -- the rigid motion of every object that
 * hpl_motion_segment (or any other labelling) lists -- and the piecewise-rigid flow, without a read-back.
 * ------------------------------------------------------------------------ */
/* Workspace of hpl_object_fit for `batch` pairs of n_total points together and max_objects objects a pair, in bytes (monotone
 * in all three); -1 for a batch outside 1 .. 64, n_total outside 0 .. 2^31 / 3 - 1 or max_objects outside 1 .. 4096. */
int64_t hpl_object_fit_workspace_bytes(int batch, int64_t n_total, int max_objects);
/* pc, pc_ld, flow, flow_sc / flow_sp, weight (N) or NULL, prefix (HOST, batch + 1 ints, batch 1 .. 64), iters (0 .. 16) and
 * tau exactly as hpl_rigid_fit takes them; labels (N) int32, 1 <= max_objects <= 4096.
 * MEMBERS: object o (0 <= o < max_objects) of pair b has as members that pair's points i with labels[i] == o, in ascending
 * point index.  The labels alone decide (hpl_motion_segment's obj_info is not read; any labelling will do); a label that is
 * negative or >= max_objects belongs to no object.
 * FIT: an object's outputs are hpl_rigid_fit's on its members, gathered in that order as one pair, bit for bit: the same
 * effective base weight (the gathered weight), rounds, pivot (the object's first member: the root hpl_motion_segment
 * reports), status rule (fewer than 3 members or a W that is not > 0: status 0, R = I, t = 0), quaternion and order of every
 * sum (spans of 1024 consecutive members, lane l of 256 taking members l, l + 256, l + 512, l + 768 of a span, one LDS tree a
 * span, the spans in 16 strided runs, then the runs in order).
 * obj_Rt [batch][max_objects][12] float32: R row-major, then t.  obj_stats [batch][max_objects][4] float32: status, the
 * inlier share of the object's members, the rotation angle in degrees, |t|.  A row without members: R = I, t = 0, stats 0.
 * residual (N) or NULL and refined [N][3] point-major or NULL are UPDATED IN PLACE: residual[i] is written for every member
 * of a listed object (r_i against its own object's last solve), refined[i] only for the inliers of a fitted object
 * (R_o p_i + t_o - p_i, rounded as hpl_rigid_fit rounds it); every other row of both is not touched.  Handed the arrays that
 * hpl_rigid_fit wrote, with hpl_motion_segment's labels of that fit's residuals, the call leaves the piecewise-rigid flow and
 * its residual: the movers have r > tau against the ego-motion, so the two sets of replaced rows are disjoint.
 * No floating-point atomic (no atomic at all): an object's outputs are the same bits alone, anywhere in a batch and beside
 * other work.  Stream-ordered, a fixed number of launches whose sizes depend on N, batch, max_objects and iters alone, no copy
 * back, no host synchronisation; no lane or workgroup waits for another; every loop is bounded by a member count or a search
 * depth.
 * workspace: DEVICE, 256-byte aligned, >= hpl_object_fit_workspace_bytes(batch, N, max_objects); residual and refined must
 * not overlap the inputs.
 * HPL_EINVAL before any launch (and without a device): batch, max_objects, iters or tau out of range; a prefix that does not
 * start at 0 or decreases; pc_ld < N; flow strides < 1 or overlapping; null pc / flow / labels / obj_Rt / obj_stats / prefix /
 * workspace; a workspace that is too small; misaligned arrays; N >= 2^31 / 3.  N == 0 is a no-op. */
int hpl_object_fit(const float *pc, int64_t pc_ld, const float *flow, int64_t flow_sc, int64_t flow_sp,
                   const float *weight /* (N) or NULL */, const int32_t *labels /* (N) */, int batch,
                   const int64_t *prefix /* HOST */, int max_objects, int iters, float tau,
                   float *obj_Rt /* [batch][max_objects][12] */, float *obj_stats /* [batch][max_objects][4] */,
                   float *residual /* (N) or NULL, in/out */, float *refined /* [N][3] or NULL, in/out */,
                   void *workspace, int64_t workspace_bytes, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Self-supervised loss (csrc/selfsup_loss.hip): Chamfer distance between the warped cloud pc1 + flow and pc2, plus the
 * smoothness of the flow over pc1's k-nearest-neighbour graph, with the gradient by the flow.
 * ------------------------------------------------------------------------ */
/* Workspace of hpl_selfsup_loss for `batch` pairs of n1_total / n2_total points together and k neighbours, in bytes (monotone
 * in all four); -1 for a batch outside 1 .. 64, k outside 0 .. 8, a count outside 0 .. 2^31 / 3 - 1 or k n1_total >= 2^31. */
int64_t hpl_selfsup_loss_workspace_bytes(int batch, int64_t n1_total, int64_t n2_total, int k);
/* pc1 (3, N1) and pc2 (3, N2) float32 SoA (row strides pc1_ld >= N1, pc2_ld >= N2); the flow of pc1's points through
 * flow_sc / flow_sp exactly as hpl_rigid_fit reads it.  batch (1 .. 64) pairs: prefix1 / prefix2 (HOST, batch + 1 ints each
 * from 0 to N1 / N2, non-decreasing, empty pairs allowed) travel in the kernel arguments.  k 1 .. 8, or 0 with w_smooth == 0
 * (no graph search); w_chamfer, w_smooth finite and >= 0.
 * Per pair, x_i point i of pc1, f_i its flow, p_i = x_i + f_i (per component, rounded once to float32), q_j point j of pc2.
 * SEARCH: the arithmetic of hpl_knn_interp -- float32 d2 = (dx * dx + dy * dy) + dz * dz, no contraction, candidates in
 * index order, an entry replaced only by a strictly smaller d2 (ties go to the smaller index), a d2 that is not below +inf
 * (NaN included) never enters.  a(i): the nearest q to p_i.  b(j): the nearest p to q_j.  N(i): the k nearest x to x_i among
 * the indices other than i (another index at the same position is a neighbour), nearest first; k_i = |N(i)| < k in a pair of
 * fewer than k + 1 points.
 * LOSS, float64 sums of the float32 inputs in a fixed order: C12 = (1 / N1) sum_i d2(p_i, q_a(i)) and C21 = (1 / N2) sum_j
 * d2(q_j, p_b(j)) over the float32 d2 the search kept (a point without a neighbour adds 0); S = (1 / N1) sum_i (1 / k_i)
 * sum_{n in N(i)} |f_i - f_n|^2, the differences in float64 (k_i = 0 adds 0; k = 0: S = 0).  A pair with N1 = 0 has all
 * components 0, one with N2 = 0 has C12 = C21 = 0.  L = w_chamfer (C12 + C21) + w_smooth S (k = 0: the first product alone).
 * loss [batch][4] float32: L, C12, C21, S, each rounded once.
 * GRADIENT, the assignments a, b, N taken as constants, float64, rounded once: dflow [N1][3] point-major (or NULL: not
 * computed), dL/df_i = w_chamfer [ (2 / N1)(p_i - q_a(i)) + (2 / N2) sum_{j: b(j) = i} (p_i - q_j) ]
 *                   + w_smooth (2 / N1) [ (1 / k_i) sum_{n in N(i)} (f_i - f_n) + sum_{m: i in N(m)} (1 / k_m)(f_i - f_m) ]
 * (k = 0: the first product alone); the sums over j and m run in ascending j / m order, each from 0, and join the point's own
 * terms afterwards.  The graph is over positions alone: a non-finite flow spreads to the S of its pair and to the gradient of
 * the points that list it, while a non-finite p_i or q_j is nobody's nearest point and adds 0 to C12 / C21.
 * nn12 (N1), nn21 (N2), nbr (k, N1) int32 or NULL: a, b, N as indices into the packed arrays, -1 where absent.
 * No floating-point atomic; a pair's outputs are the same bits alone, anywhere in a batch and beside other work.  Stream-
 * ordered, a fixed number of launches whose sizes depend on N1, N2, batch and k alone (and on whether dflow is asked for), no
 * copy back, no host synchronisation; no lane or workgroup waits for another.
 * workspace: DEVICE, 256-byte aligned, >= hpl_selfsup_loss_workspace_bytes(batch, N1, N2, k); dflow must not overlap pc1,
 * flow or pc2.
 * HPL_EINVAL before any launch (and without a device): batch or k out of range, k = 0 with w_smooth != 0; a weight that is
 * negative, infinite or NaN; a prefix that does not start at 0 or decreases; a row stride below its count; flow strides < 1
 * or overlapping; null pc1 / flow / prefixes / loss / workspace, null pc2 with N2 > 0; misaligned arrays; a workspace that is too small; a
 * count >= 2^31 / 3 or k N1 >= 2^31; dflow overlapping an input.  N1 == 0 is a no-op. */
int hpl_selfsup_loss(const float *pc1, int64_t pc1_ld, const float *flow, int64_t flow_sc, int64_t flow_sp, const float *pc2,
                     int64_t pc2_ld, int batch, const int64_t *prefix1 /* HOST */, const int64_t *prefix2 /* HOST */, int k,
                     float w_chamfer, float w_smooth, float *loss, float *dflow, int32_t *nn12, int32_t *nn21, int32_t *nbr,
                     void *workspace, int64_t workspace_bytes, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Ground removal (csrc/ground_fit.hip): per cloud the ground plane by RANSAC with a tilt gate against a given up vector,
 * refined by least squares on its inliers; every point classified by its signed height over the plane, and the indices of
 * the points that are not ground, stably compacted.
 * ------------------------------------------------------------------------ */
/* Workspace of hpl_ground_fit for `batch` clouds of n_total points together and `hyps` hypotheses, in bytes (monotone in all
 * three); -1 for a batch outside 1 .. 64, hyps outside 1 .. 1024 or n_total outside 0 .. 2^31 / 3 - 1. */
int64_t hpl_ground_fit_workspace_bytes(int batch, int64_t n_total, int hyps);
/* pc (3, N) float32 SoA (row stride pc_ld >= N).  batch (1 .. 64) clouds: prefix (HOST, batch + 1 ints from 0 to N,
 * non-decreasing, empty clouds allowed) travels in the kernel arguments.  up (HOST, 3 floats, finite, not zero): the direction
 * the ground's normal points to, of any length.  min_cos in (0, 1]: the cosine of the largest allowed tilt between normal and
 * up.  hyps 1 .. 1024, refine 0 .. 8, tau > 0 finite (inlier distance), cut >= 0 finite.  seed / call: the random stream.
 * Arithmetic per cloud of n points x_0 .. x_{n-1} (indices within the cloud): float64 throughout, computed from the float32
 * inputs (up, min_cos, tau, cut promoted too), every operation rounded once, no contraction; parentheses give the order.
 * VALID: a point whose three coordinates are finite.
 * HYPOTHESIS h (0 .. hyps - 1): r = philox4x32_10(counter = (h, call lo, call hi, 16), key = (seed lo, seed hi));
 * i_k = (uint64(r[k]) * n) >> 32 for k = 0, 1, 2 -- a function of h, n, seed and call alone.  a = x_{i_0}, u = x_{i_1} - a,
 * v = x_{i_2} - a, m = u x v (m_x = u_y v_z - u_z v_y, m_y = u_z v_x - u_x v_z, m_z = u_x v_y - u_y v_x),
 * q = (m_x m_x + m_y m_y) + m_z m_z, c = (m_x up_x + m_y up_y) + m_z up_z, uu the form of q over up; if c < 0, m and c are
 * negated.  The hypothesis is valid when n >= 3, the three points are valid, q > 0 and finite, and
 * c c >= ((min_cos min_cos) uu) q.
 * VOTE: s_i = (m_x (x_i - a_x) + m_y (y_i - a_y)) + m_z (z_i - a_z); point i votes for h when it is valid and
 * s_i s_i <= (tau tau) q.  votes [batch][hyps] int32 or NULL: the count, -1 for an invalid hypothesis.
 * WINNER: the most votes, the smallest h among equals: n = m / sqrt(q) per component, d = -((n_x a_x + n_y a_y) + n_z a_z).
 * A cloud without a valid hypothesis has status 0: plane all 0, nothing ground, height 0 at every point, keep_idx every index,
 * stats (0, -1, 0, n).
 * REFINE, `refine` rounds: the inliers of the current float64 plane are the valid points with |h_i| <= tau,
 * h_i = ((n_x x_i + n_y y_i) + n_z z_i) + d.  With dp = x_i - a (the winner's a), W the inlier count, S1 = sum dp and
 * S2 = sum dp dp^T (float64, a fixed order: per workgroup of 1024 consecutive points a tree, then the workgroups' partials in 16
 * strided runs in index order, then the runs in order): mu = S1 / W, C_ij = S2_ij - (W mu_i) mu_j; the new normal is the unit
 * eigenvector of C's smallest eigenvalue (cyclic Jacobi), negated if its c < 0; d = -((n_x (a_x + mu_x) + n_y (a_y + mu_y))
 * + n_z (a_z + mu_z)).  A round with W < 3, a non-finite sum or result, or a normal with c c < ((min_cos min_cos) uu) (n . n)
 * ends the refinement and keeps the plane it started from.
 * CLASSIFY: plane [batch][4] float32 = (n, d), each rounded once; the classification reads those float32 values back, promoted
 * to float64, so it is reproducible from `plane` alone.  height (N) float32 or NULL: h_i rounded once, NaN for an invalid
 * point.  ground (N) uint8 or NULL: 1 when the point is valid and h_i <= cut (everything at or under the surface plus cut), else
 * 0: invalid points are kept.  keep_idx (N) int32 or NULL: for each cloud from prefix[b] on, the indices into the packed
 * arrays of its points that are not ground, ascending; the rest of the cloud's range -1.  stats [batch][4] int32: status (1 a
 * fit, 0 none), the winning h, its votes, the kept count.
 * Counts are integers (integer atomic adds commute); no floating-point atomic: a cloud's outputs are the same bits alone,
 * anywhere in a batch and beside other work.  Stream-ordered, 6 + 2 refine launches (5 + 2 refine without keep_idx) whose sizes
 * depend on N, batch, hyps and refine alone, no copy back, no host synchronisation; no lane or workgroup waits for another.
 * workspace: DEVICE, 8-byte aligned, >= hpl_ground_fit_workspace_bytes(batch, N, hyps).
 * HPL_EINVAL before any launch (and without a device): batch, hyps, refine, tau, cut or min_cos out of range or NaN; an up
 * that is zero or not finite; a prefix that does not start at 0 or decreases; pc_ld < N; null pc / prefix / up / plane / stats
 * / workspace; misaligned arrays; a workspace that is too small; N >= 2^31 / 3.  N == 0 is a no-op. */
int hpl_ground_fit(const float *pc, int64_t pc_ld, int batch, const int64_t *prefix /* HOST */, const float *up /* HOST, 3 */,
                   float min_cos, int hyps, float tau, int refine, float cut, uint64_t seed, uint64_t call,
                   float *plane /* [batch][4] */, int32_t *stats /* [batch][4] */, int32_t *votes /* [batch][hyps] or NULL */,
                   float *height /* (N) or NULL */, uint8_t *ground /* (N) or NULL */, int32_t *keep_idx /* (N) or NULL */,
                   void *workspace, int64_t workspace_bytes, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Voxel-grid downsampling (csrc/voxel_grid.hip): one point per occupied cell of a grid of edge `voxel` -- the cell's centroid
 * or the member nearest to it --, with attribute channels riding along and every point's voxel.
 * ------------------------------------------------------------------------ */
#define HPL_VOXEL_CENTROID 0
#define HPL_VOXEL_NEAREST 1
/* Workspace of hpl_voxel_downsample for `batch` clouds of n_total points together and `channels` attribute channels, in bytes
 * (monotone in all three); -1 for a batch outside 1 .. 64, channels outside 0 .. 8 or n_total outside 0 .. 2^31 / 3 - 1. */
int64_t hpl_voxel_downsample_workspace_bytes(int batch, int64_t n_total, int channels);
/* pc (3, N) float32 SoA (row stride pc_ld >= N); attr (channels, N) float32 SoA (row stride attr_ld >= N) riding along,
 * channels 0 .. 8 (attr may be NULL with channels == 0).  batch (1 .. 64) clouds: prefix (HOST, batch + 1 ints from 0 to N,
 * non-decreasing, empty clouds allowed) travels in the kernel arguments.  voxel > 0 finite; origin (HOST, 3 floats, finite);
 * mode HPL_VOXEL_CENTROID or HPL_VOXEL_NEAREST.
 * CELL: inv = 1.0 / (double)voxel; cell_k = floor(((double)x_k - (double)origin_k) * inv) for k = x, y, z, every operation in
 * float64, rounded once, no contraction.  A point is VALID when its three coordinates are finite and |cell_k| <= 2^18 - 2 on
 * every axis (the range of hpl_motion_segment).  A non-finite point counts in stats[b][2], a finite one out of range in
 * stats[b][3].  Points of different clouds never share a voxel.
 * VOXELS: a cloud's voxels are the distinct cells of its valid points, numbered 0 .. V_b - 1 in ascending lexicographic order
 * of the signed (cell_x, cell_y, cell_z).  Voxel v of cloud b lives at packed position prefix[b] + v of every per-voxel
 * output; the outputs have the input's capacity N (V_b <= n_b).
 * PER VOXEL: count, the number of members.  The centroid c, per coordinate: the float64 sum of the float32 members in
 * ascending point index, one after the other, from 0, divided by the count (as a float64) and rounded once to float32; every
 * attribute channel is averaged the same way.  rep, the member nearest to that float32 centroid by the arithmetic of
 * hpl_knn_interp: float32 d2 = (dx * dx + dy * dy) + dz * dz, no contraction, members in index order, the first member
 * enters and is replaced only by a strictly smaller d2 (ties go to the smaller index); rep is an index into the packed arrays.
 * OUTPUTS: out_pc (3, N) (row stride out_ld >= N) and out_attr (channels, N) (row stride out_attr_ld >= N): in mode CENTROID
 * the means, in mode NEAREST the representative's coordinates and attributes bit for bit (the output is then a subset of the
 * input).  count (N), rep (N) int32.  voxel_of (N) int32: for every input point the packed position of its voxel, -1 for a
 * point that is not valid: a per-voxel result goes back to the points as values[:, voxel_of].  Behind a cloud's V_b voxels the
 * rest of its range is 0 in out_pc / out_attr / count and -1 in rep.  stats [batch][4] int32: V_b, valid points, non-finite
 * points, points out of range.  out_attr, count, rep and voxel_of may each be NULL.  A non-finite attribute of a valid point
 * reaches its voxel's mean (it is not hidden) and no other voxel.
 * Counts are integers (integer atomic adds commute); no floating-point atomic: a cloud's outputs are the same bits alone,
 * anywhere in a batch and beside other work.  Stream-ordered, a fixed number of launches whose sizes depend on N, batch and
 * channels alone, no copy back, no host synchronisation (V_b is known on the device only); no lane or workgroup waits for
 * another.
 * workspace: DEVICE, 256-byte aligned, >= hpl_voxel_downsample_workspace_bytes(batch, N, channels).
 * HPL_EINVAL before any launch (and without a device): batch, channels, mode, voxel or origin out of range or NaN; a prefix
 * that does not start at 0 or decreases; a row stride below N; null pc / prefix / origin / out_pc / stats / workspace, null
 * attr with channels > 0; misaligned arrays; a workspace that is too small or misaligned; N >= 2^31 / 3; an output overlapping
 * an input.  N == 0 is a no-op. */
int hpl_voxel_downsample(const float *pc, int64_t pc_ld, const float *attr, int64_t attr_ld, int channels, int batch,
                         const int64_t *prefix /* HOST */, float voxel, const float *origin /* HOST, 3 */, int mode,
                         float *out_pc, int64_t out_ld, float *out_attr, int64_t out_attr_ld, int32_t *count, int32_t *rep,
                         int32_t *voxel_of, int32_t *stats /* [batch][4] */, void *workspace, int64_t workspace_bytes,
                         hplStream stream);

/* ------------------------------------------------------------------------ *
 * Farthest point sampling (csrc/fps.hip): exactly m points per cloud -- fewer only when a cloud runs out of distinct
 * positions --, each the point farthest from all chosen before it, with attribute channels riding along.
 * ------------------------------------------------------------------------ */
#define HPL_FPS_AUTO 0
#define HPL_FPS_RESIDENT 1
#define HPL_FPS_ROUNDS 2
/* The most points a cloud may hold on the resident path (one workgroup per cloud, the cloud in registers). */
int hpl_fps_resident_capacity(void);
/* Workspace of hpl_fps for `batch` clouds of n_total points together, m samples each and `channels` attribute channels, in
 * bytes (monotone in batch and n_total); -1 for a batch outside 1 .. 64, channels outside 0 .. 8, n_total outside
 * 0 .. 2^31 / 3 - 1, m < 1 or batch * m >= 2^31 / 3. */
int64_t hpl_fps_workspace_bytes(int batch, int64_t n_total, int64_t m, int channels);
/* pc (3, N) float32 SoA (row stride pc_ld >= N); attr (channels, N) float32 SoA (row stride attr_ld >= N) riding along,
 * channels 0 .. 8 (attr may be NULL with channels == 0).  batch (1 .. 64) clouds: prefix (HOST, batch + 1 ints from 0 to N,
 * non-decreasing, empty clouds allowed) travels in the kernel arguments.  m >= 1 samples are asked of every cloud.  start:
 * HOST, batch cloud-local indices, or NULL.  path: HPL_FPS_AUTO, HPL_FPS_RESIDENT or HPL_FPS_ROUNDS.
 * Per cloud b of n_b points, on its own:
 * VALID: a point is valid when its three coordinates are finite.  A point that is not is never selected and never counted.
 * STATE: D_i = +inf for every valid point i.
 * START: sample 0 is start[b]; with start == NULL, or when the point at start[b] is not finite, the smallest valid index.
 * ROUND j >= 1: with s the previous sample, D_i = min(D_i, d2(i, s)), d2 = (dx * dx + dy * dy) + dz * dz in float32, one
 * rounding per operation, no contraction (the arithmetic of hpl_knn_interp).  Sample j is the valid point of the largest D,
 * ties to the SMALLER index: the largest key (bits(D) << 32) | (0xFFFFFFFF - i) as an unsigned integer, since D >= +0.
 * STOP: the cloud stops when the largest D is exactly 0 -- every remaining point then coincides in float32 d2 with a sample,
 * a true duplicate or a d2 that underflowed -- or when it has no valid point.  So count_b <= min(m, valid_b), and a cloud's
 * samples are pairwise distinct indices.  A d2 that overflows to +inf is an ordinary value (min(inf, inf) = inf); the
 * coordinates of valid points are finite, so no NaN can arise.
 * OUTPUTS: idx [batch][m] int32: cloud-local indices in selection order, -1 past count_b.  dist [batch][m] float32: the D of
 * each sample at the moment it was chosen, +inf for sample 0, 0 past count_b; from column 1 on it does not increase (min is
 * exact).  out_pc (3, batch * m) (row stride out_ld >= batch * m): column b * m + j holds sample j of cloud b, 0 past the
 * count.  out_attr (channels, batch * m) (row stride out_attr_ld): the channels gathered the same way; may be NULL.  cover (N)
 * float32 or NULL: every point's final D, its squared distance to its nearest sample, 0 for a point that is not valid.  stats
 * [batch][4] int32: count_b, valid points, points that are not finite, the path taken (HPL_FPS_RESIDENT or HPL_FPS_ROUNDS,
 * one for the whole call).
 * PATHS, the same bits on both: RESIDENT holds a cloud in the registers of one workgroup and runs all m rounds in one launch;
 * it takes clouds of at most hpl_fps_resident_capacity() points.  ROUNDS keeps D in the workspace and takes one launch per
 * round plus one; it takes any size.  AUTO is RESIDENT when every cloud of the call fits, else ROUNDS for the whole call.
 * The only atomics are integer counts; no floating-point atomic: a cloud's outputs are the same bits alone, anywhere in a
 * batch, on either path and beside other work.  Stream-ordered, launches whose number and sizes depend on the prefix and m
 * alone, no copy back, no host synchronisation (count_b is known on the device only); no workgroup waits for another.
 * workspace: DEVICE, 256-byte aligned, >= hpl_fps_workspace_bytes(batch, N, m, channels).
 * HPL_EINVAL before any launch (and without a device): batch, channels, path or m out of range; a prefix that does not start
 * at 0 or decreases; a start outside its cloud (the start of an empty cloud is ignored); a row stride below N (inputs) or
 * batch * m (outputs); null pc / prefix / idx / dist / out_pc / stats / workspace, null attr with channels > 0; misaligned
 * arrays; a workspace that is too small or misaligned; N >= 2^31 / 3; an output overlapping an input; path RESIDENT with a
 * cloud above the capacity.  N == 0 is a no-op (nothing is written). */
int hpl_fps(const float *pc, int64_t pc_ld, const float *attr, int64_t attr_ld, int channels, int batch,
            const int64_t *prefix /* HOST */, const int32_t *start /* HOST [batch] or NULL */, int64_t m, int path,
            int32_t *idx /* [batch][m] */, float *dist /* [batch][m] */, float *out_pc, int64_t out_ld, float *out_attr,
            int64_t out_attr_ld, float *cover /* (N) or NULL */, int32_t *stats /* [batch][4] */, void *workspace,
            int64_t workspace_bytes, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Frames from raw maps (csrc/frames.hip): corresponding point clouds from disparity and optical-flow maps, the valid
 * correspondences of every frame compacted in pixel order.
 * ------------------------------------------------------------------------ */
/* BOTH ENTRIES take a ragged batch of frames: batch 1 .. 64; height[b], width[b] HOST int32, each >= 0; prefix HOST, batch + 1
 * ints from 0 to N: frame b owns pixels prefix[b] .. prefix[b + 1] of every packed per-pixel array, row-major, with
 * prefix[b + 1] - prefix[b] == height[b] * width[b] (empty frames allowed); N < 2^31 / 3.  Pixel (i, j) of a frame -- row i,
 * column j -- has the index i * width + j.
 * OUTPUTS: out_pc1, out_pc2 (3, N) float32 SoA (row strides out1_ld, out2_ld >= N); pixel (N) int32 or NULL; counts [batch]
 * int32.  Frame b's valid correspondences sit at packed positions prefix[b] .. prefix[b] + counts[b] in ascending pixel index
 * -- the order of numpy's boolean-mask indexing, so a frame's clouds are the arrays the reference's preprocessing scripts save,
 * transposed --, pixel holds their i * width + j; the rest of the frame's range is 0 in the clouds and -1 in pixel.
 * Counts are integers; a frame's outputs are the same bits alone, anywhere in a batch and beside other work.  Stream-ordered,
 * three launches whose sizes depend on batch and the prefix alone (count per workgroup, a scan of the workgroup counts inside
 * each frame, emit), no copy back, no host synchronisation (counts[b] is known on the device only); no lane or workgroup
 * waits for another.
 * workspace: DEVICE, 4-byte aligned, >= hpl_frames_workspace_bytes(batch, N).
 * HPL_EINVAL before any launch (and without a device): batch out of range; a null array (pixel alone may be NULL); a negative
 * height or width; a prefix that does not start at 0, decreases or disagrees with height * width; N >= 2^31 / 3; a row stride
 * below N; misaligned arrays (2 bytes for the uint16 arrays, 4 for the float32 and int32 ones); a workspace that is too small
 * or misaligned; a row stride above 2^40; an output overlapping an input, another output or the workspace (row by row: views
 * that interleave inside one buffer are fine); and what each entry adds below.  N == 0 is a no-op (counts is not written). */
/* Workspace of either entry for `batch` frames of n_total pixels together, in bytes (monotone in both); -1 for a batch outside
 * 1 .. 64 or n_total outside 0 .. 2^31 / 3 - 1. */
int64_t hpl_frames_workspace_bytes(int batch, int64_t n_total);
/* KITTI scene flow (kitti_utils.pixel2xyz / disp_2_depth / load_disp / load_op_flow and process_kitti.py of the reference).
 * disp1, disp2 (N) uint16: the raw values of the disp_occ_0 / disp_occ_1 PNGs; flow [N][3] uint16: the raw values of the
 * flow_occ PNG, interleaved (u, v, mask) as the file has them; P HOST [batch][12] float32: each frame's P_rect_02, row-major
 * 3 x 4; baseline (0.54).  Refused as well: a P with P01, P10, P20 or P21 != 0 or P00 != P11 (the reference asserts these),
 * a P00 that is zero or not finite, a baseline that is not finite.
 * Per pixel (i, j) of frame b with raw values r1, r2, (u, v, m), every operation in float32, rounded once, no contraction:
 *   valid = r1 > 0 && r2 > 0 && m == 1
 *   fb = P00 * (float)baseline;  z_k = fb / ((float)r_k / 256 + 1e-5f)
 *   px1 = (float)j, py1 = (float)i;  px2 = (float)j + ((float)u - 32768) / 64, py2 = (float)i + ((float)v - 32768) / 64
 *   X = -(((px * (z + P23)) - ((P02 * z) + P03)) / P00);  Y = -(((py * (z + P23)) - ((P12 * z) + P13)) / P00);  Z = z
 * with (px1, py1, z_1) for pc1 and (px2, py2, z_2) for pc2. */
int hpl_frames_from_kitti(const uint16_t *disp1, const uint16_t *disp2, const uint16_t *flow /* [N][3] */, int batch,
                          const int32_t *height /* HOST */, const int32_t *width /* HOST */, const int64_t *prefix /* HOST */,
                          const float *P /* HOST [batch][12] */, float baseline, float *out_pc1, int64_t out1_ld, float *out_pc2,
                          int64_t out2_ld, int32_t *pixel /* (N) or NULL */, int32_t *counts /* [batch] */, void *workspace,
                          int64_t workspace_bytes, hplStream stream);
/* FlyingThings3D subset (flyingthings3d_utils.pixel2pc / next_pixel2pc and process_flyingthings3d_subset.py of the reference).
 * disp, dchange (N) float32: disparity and disparity change; flow [N][2] float32 interleaved (x, y); occ1, occ2 (N) uint8: the
 * disparity and flow occlusion masks; f, cx, cy (-1050, 479.5, 269.5); use_near 0 or 1, near_z the near cut (-35).  Refused as
 * well: use_near outside 0 / 1, a NaN near_z with use_near.
 * Per pixel (i, j) with px = (float)j, py = (float)i, flow (fx, fy), every operation in float32, rounded once, no contraction:
 *   nf = (float)(-(double)f);  d1 = disp, d2 = disp + dchange;  z_k = nf / d_k
 *   x1 = (-(px - cx)) / d1, y1 = (py - cy) / d1;  x2 = (-((px - cx) + fx)) / d2, y2 = ((py - cy) + fy) / d2
 *   valid = occ1 == 0 && occ2 == 0, with use_near also z1 > near_z && z2 > near_z (a NaN depth is dropped)
 * A zero disparity gives the IEEE infinity or NaN that numpy gives, and it is kept unless the near cut drops it.  The sign
 * flip of x and z that the dataset reader applies is the reader's (data.FlyingThings3DRaw). */
int hpl_frames_from_ft3d(const float *disp, const float *dchange, const float *flow /* [N][2] */, const uint8_t *occ1,
                         const uint8_t *occ2, int batch, const int32_t *height /* HOST */, const int32_t *width /* HOST */,
                         const int64_t *prefix /* HOST */, float f, float cx, float cy, int use_near, float near_z, float *out_pc1,
                         int64_t out1_ld, float *out_pc2, int64_t out2_ld, int32_t *pixel /* (N) or NULL */,
                         int32_t *counts /* [batch] */, void *workspace, int64_t workspace_bytes, hplStream stream);
/* HOST only: undoes the PNG row filters in place (data.read_png inflates with zlib and calls this).  rows: `height` rows of
 * `stride` bytes, each a filter-type byte (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) followed by stride - 1 data bytes; bpp: the
 * bytes of a whole pixel, 1 .. 8 (the distance to the byte "to the left").  The filter bytes are left as they are.
 * HPL_EINVAL: height < 0, stride < 1, bpp outside 1 .. 8, null rows with height > 0, or a filter byte above 4 (the rows before
 * it are already unfiltered). */
int hpl_png_unfilter(uint8_t *rows, int64_t height, int64_t stride, int bpp);

/* ------------------------------------------------------------------------ *
 * Rigid registration of a cloud pair (csrc/icp.hip): the motion (R, t) that lays src onto dst, from the clouds alone, by
 * robust point-to-point ICP with an exact nearest-neighbour search within a radius on a sorted grid.
 * ------------------------------------------------------------------------ */
/* Workspace of hpl_icp for `batch` pairs of n_src / n_dst points together, in bytes (monotone in all three); -1 for a batch
 * outside 1 .. 64 or a count outside 0 .. 2^31 / 3 - 1. */
int64_t hpl_icp_workspace_bytes(int batch, int64_t n_src, int64_t n_dst);
/* src (3, N) and dst (3, M) float32 SoA (row strides src_ld >= N, dst_ld >= M).  batch (1 .. 64) pairs: src_prefix /
 * dst_prefix (HOST, batch + 1 ints each from 0 to N / M, non-decreasing, empty pairs allowed, N_b != M_b allowed) travel in
 * the kernel arguments.  weight (N) float32 or NULL (all 1): the effective base weight w_i is the given weight, 0 when that is
 * not in (0, inf) (NaN included) or a coordinate of the src point is not finite.  init [batch][12] float32 (DEVICE) or NULL
 * (identity): R row-major, then t.  iters 0 .. 64; max_dist, tau finite and > 0; tol_rot, tol_trans >= 0.
 * GRID (an accelerator only: the match below is defined over all pairs; tests/icp_oracle.py restates it in numpy without a
 * grid): cell_k = floor(x_k * (1 / (1.001 * max_dist))) in float64 (the product 1.001 * max_dist, the quotient and the product
 * with x_k each rounded once).  A dst point takes part when its three coordinates are finite and |cell_k| <= 2^18 - 2 for
 * k = x, y, z; a query whose cell fails the same test has no match.
 * MATCH of src point p under a float32 motion (R, t), every entry widened to float64: y_k = ((R[k][0] px + R[k][1] py) +
 * R[k][2] pz) + t_k in float64, the query yq = float32(y); d2 = (dx * dx + dy * dy) + dz * dz in float32 with dx = yq.x - q.x,
 * every operation rounded, no contraction (the arithmetic of hpl_knn_interp).  The match is the dst point of the same pair
 * that takes part with the smallest d2, ties to the smaller dst index; it is accepted when d2 <= float32(max_dist * max_dist)
 * (the product in float32); otherwise the point has no match (match -1, dist2 +inf).
 * ROUND from the motion (R, t): r2_i = sum_k (y_k - q_k)^2 in float64 (k ascending, from 0) against the matched q;
 * u_i = w_i / (s * s), s = 1 + r2_i * (1 / (tau * tau)) (Geman-McClure; tau widened first); u_i = 0 without a match.  The 16
 * sums W = sum u, sum u dp, sum u dq, sum u dp dq^T about the pair's first src point (0 for a non-finite coordinate of it) are
 * hpl_rigid_fit's, in its order (workgroups of 1024 consecutive points, lane l taking points l, l + 256, l + 512, l + 768, one
 * LDS tree, then the fold of the workgroups' partials), and so is the solve (Horn's quaternion, csrc/rigid_solve.h).  The
 * motion a round hands on is that solve's (R, t) ROUNDED TO FLOAT32 -- exactly what Rt holds: a call with iters = T equals T
 * chained calls with iters = 1, each given the previous Rt as init, bit for bit (but for stats[5]) at tol = 0.
 * STOP: a pair is finished when |new - old| <= tol_rot for every R entry and <= tol_trans for every t entry of the float32
 * motions (the differences in float64); its later rounds are skipped.  At tol = 0 that skips bitwise fixpoints only.
 * FAILURE: a pair with N_b < 3 or M_b = 0 has status 0 and runs no round.  A round fails when W is not > 0 or a sum or the
 * new float32 motion is not finite: the pair ends with status 0 and keeps the motion that round started from (init at the
 * first).  The failed round counts in stats[5].
 * FINISH: one more match under the final motion writes match (N) int32 (the packed dst index, -1 for none), dist2 (N) float32
 * (the match's d2, +inf for none) and flow [N][3] float32 = float32(y_k - p_k), the difference in float64 (each may be NULL).
 * Rt [batch][12] float32: the final motion.  stats [batch][6] float32: status; matched share = accepted matches of points
 * with w_i > 0 / N_b (0 for N_b = 0); RMSE = sqrt(sum r2 / count) over those points, a float64 sum in a fixed order (per
 * workgroup as above, then one fold per pair), rounded once, 0 for none; the angle of the final float32 R in degrees,
 * atan2(|v|, tr R - 1) with v = (R21 - R12, R02 - R20, R10 - R01), in float64; |t| = sqrt((t0^2 + t1^2) + t2^2) in float64;
 * rounds run.  No floating-point atomic; a pair's outputs are the same bits alone, anywhere in a batch and beside other work.
 * Stream-ordered: keys, one stable radix sort of dst, 2 iters launches, finish, fold; no copy back, no host synchronisation;
 * no lane or workgroup waits for another.
 * workspace: DEVICE, 256-byte aligned, >= hpl_icp_workspace_bytes(batch, N, M); the outputs must not overlap the inputs.
 * HPL_EINVAL before any launch (and without a device): batch or iters out of range; max_dist or tau <= 0 or not finite; a
 * negative or NaN tolerance; a prefix that does not start at 0 or decreases; a row stride below its count; null src / Rt /
 * stats / prefixes / workspace, null dst with M > 0; misaligned arrays; a workspace that is too small or misaligned; N or M >= 2^31 / 3.
 * N == 0 is a no-op (the caller pre-fills Rt and stats). */
int hpl_icp(const float *src, int64_t src_ld, const float *dst, int64_t dst_ld, const float *weight, const float *init,
            int batch, const int64_t *src_prefix /* HOST */, const int64_t *dst_prefix /* HOST */, int iters, float max_dist,
            float tau, float tol_rot, float tol_trans, float *Rt, float *stats, int32_t *match, float *dist2, float *flow,
            void *workspace, int64_t workspace_bytes, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Surface normals of packed ragged clouds (csrc/normals.hip): per point its k nearest neighbours within a radius, exact, on
 * a sorted grid over the cloud itself, and the principal-component normal of that neighbourhood.
 * ------------------------------------------------------------------------ */
/* Workspace of hpl_normals for `batch` clouds of n_total points together, in bytes (monotone in n_total); -1 for a batch
 * outside 1 .. 64 or a count outside 0 .. 2^31 / 3 - 1. */
int64_t hpl_normals_workspace_bytes(int batch, int64_t n_total);
/* pc (3, N) float32 SoA (row stride pc_ld >= N).  batch (1 .. 64) clouds: prefix (HOST, batch + 1 ints from 0 to N,
 * non-decreasing, empty clouds allowed) travels in the kernel arguments.  k 3 .. 32; radius finite and > 0; viewpoint (HOST,
 * [batch][3] float32, finite) or NULL (the origin for every cloud).
 * GRID (an accelerator only: the neighbourhood below is defined over all pairs of a cloud; tests/normals_oracle.py restates it
 * in numpy without a grid): cell_k = floor(x_k * (1 / (1.001 * radius))) in float64 (the product 1.001 * radius, the quotient
 * and the product with x_k each rounded once).  A point TAKES PART when its three coordinates are finite and
 * |cell_k| <= 2^18 - 2 for k = x, y, z; a point that does not has count 0, no neighbour and no normal.
 * DISTANCE d2(i, j) = (dx * dx + dy * dy) + dz * dz in float32 with dx = p_i.x - p_j.x, every operation rounded, no
 * contraction (the arithmetic of hpl_knn_interp).
 * NEIGHBOURHOOD N(i) of a point that takes part: the points j of the same cloud that take part with d2(i, j) <=
 * float32(radius * radius) (the product in float32), i itself included (d2 = 0), ordered by (d2, j) ascending -- equal d2:
 * the smaller index first --, the first k of them.  count (N) int32 = |N(i)| <= k.  nbr [N][k] int32: the packed indices in
 * that order, then -1; nbr_d2 [N][k] float32: their d2, then +inf (each of curvature, count, nbr, nbr_d2 may be NULL).
 * COVARIANCE in float64, in neighbourhood order, every sum from 0: m = (sum p_j) / count; the six sums
 * C_ab = sum (p_ja - m_a) (p_jb - m_b), a <= b.
 * EIGENPAIR: cyclic Jacobi (csrc/cloud_common.h, at most 12 sweeps, as hpl_ground_fit) on the symmetric C; lambda_0 ..
 * lambda_2 are the diagonal afterwards.  The normal is the eigenvector column of the smallest lambda (equal lambdas: the
 * smaller column), divided once by its length sqrt((n0 n0 + n1 n1) + n2 n2) in float64.
 * ORIENTATION: s = (n0 (v0 - p0) + n1 (v1 - p1)) + n2 (v2 - p2) in float64, v the cloud's viewpoint and p the point, widened
 * from float32.  The normal is negated when s < 0; when s == 0, when its first non-zero component is negative.
 * VALID when count >= 3, the three lambdas are finite and the largest is > 0: normal (3, N) float32 SoA (row stride
 * normal_ld >= N) = float32(n), a unit vector; curvature (N) float32 = float32(max(lambda_min, 0) / ((lambda_0 + lambda_1) +
 * lambda_2)), the surface variation.  Otherwise the normal is (0, 0, 0) and the curvature 0.
 * No floating-point atomic; a point's outputs are the same bits alone, anywhere in a batch and beside other work.
 * Stream-ordered: keys, one stable radix sort of (key, 16-byte record), one search-and-PCA launch (a lane per sorted record;
 * the list of the best k kept in registers, instances of 8, 16 and 32 entries); no copy back, no host synchronisation; no
 * lane or workgroup waits for another; every loop is bounded by a cell's population or log2 N.  The search costs the
 * population of 27 cells per point: all points in one cell is quadratic.
 * workspace: DEVICE, 256-byte aligned, >= hpl_normals_workspace_bytes(batch, N).
 * HPL_EINVAL before any launch (and without a device): batch or k out of range; radius <= 0 or not finite; a non-finite
 * viewpoint; a prefix that does not start at 0 or decreases; N >= 2^31 / 3; N k >= 2^31 with nbr or nbr_d2 given; a row stride
 * below N; null pc / normal / prefix / workspace; misaligned arrays; a workspace that is too small or misaligned; an output
 * that overlaps pc or the workspace.  N == 0 is a no-op. */
int hpl_normals(const float *pc, int64_t pc_ld, int batch, const int64_t *prefix /* HOST */, int k, float radius,
                const float *viewpoint /* HOST [batch][3] or NULL */, float *normal, int64_t normal_ld, float *curvature,
                int32_t *count, int32_t *nbr, float *nbr_d2, void *workspace, int64_t workspace_bytes, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Point-to-plane ICP (csrc/icp_plane.hip; what it shares with csrc/icp.hip lives in csrc/icp_common.h): hpl_icp with the
 * residual taken along the matched dst point's normal.
 * ------------------------------------------------------------------------ */
/* Workspace of hpl_icp_plane, in bytes (monotone in all three); -1 as hpl_icp_workspace_bytes. */
int64_t hpl_icp_plane_workspace_bytes(int batch, int64_t n_src, int64_t n_dst);
/* hpl_icp's arguments, and dst_normal (3, M) float32 SoA (row stride dnormal_ld >= M), e.g. hpl_normals' output for dst.
 * Everything hpl_icp states holds -- grid, match, weights, stop, failure, finish (which reports EVERY point-to-point match),
 * Rt, stats, chaining, determinism --; the ROUND differs:
 * A matched dst point's normal n (widened to float64) is VALID when its three components are finite and not all zero; a match
 * on an invalid normal has u = 0 in the round.
 * r = sum_k (y_k - q_k) n_k in float64 (k ascending, from 0); u = w / (s * s), s = 1 + (r * r) * (1 / (tau * tau)).
 * a = (y - c) x n with c the pair's pivot (its first src point, 0 for a non-finite coordinate); J = (a0, a1, a2, n0, n1, n2).
 * The 28 sums W = sum u, the 21 upper entries of H = sum (u J_p) J_q (row-major) and g_p = sum (u J_p) r go through
 * hpl_icp's workgroup order (one LDS tree per 1024 src points, then a fold of the workgroups' partials in 8 strided runs).
 * SOLVE (float64): cyclic Jacobi on the 6 x 6 H, at most 16 sweeps; lambda = the diagonal, V = the eigenvector columns;
 * x = - sum over {i: lambda_i > 1e-10 lambda_max} V_i (V_i . g) / lambda_i, the minimum-norm step: a direction the geometry does
 * not observe (sliding along a single plane) gets no update and does not fail the pair.  (omega, delta) = x;
 * E = I + sin(theta) / theta K + (1 - cos(theta)) / theta^2 K^2 with K = [omega]x, theta = |omega| (theta < 1e-12: E = I + K);
 * R' = E R, t' = E (t - c) + c + delta, then ROUNDED TO FLOAT32: iters = T equals T chained calls bit for bit at tol = 0.
 * FAILURE as hpl_icp: W not > 0, lambda_max not > 0, or a sum or the new motion not finite.
 * DRIFT: R is a product of one rotation per round, each product rounded to float32 and never re-projected: after T rounds
 * R^T R differs from I by at most about 6 T 2^-24 per entry.
 * workspace >= hpl_icp_plane_workspace_bytes(batch, N, M).  HPL_EINVAL as hpl_icp, and for a null dst_normal with M > 0, a
 * misaligned dst_normal or dnormal_ld < M. */
int hpl_icp_plane(const float *src, int64_t src_ld, const float *dst, int64_t dst_ld, const float *dst_normal, int64_t dnormal_ld,
                  const float *weight, const float *init, int batch, const int64_t *src_prefix /* HOST */,
                  const int64_t *dst_prefix /* HOST */, int iters, float max_dist, float tau, float tol_rot, float tol_trans,
                  float *Rt, float *stats, int32_t *match, float *dist2, float *flow, void *workspace, int64_t workspace_bytes,
                  hplStream stream);

/* ------------------------------------------------------------------------ *
 * Outlier removal on packed ragged clouds (csrc/outlier_filter.hip): the statistical filter (mean distance to the k nearest
 * neighbours against the cloud's mu + std_ratio sigma) and the radius filter (at least min_neighbors within a radius),
 * exact, on a sorted grid over the cloud itself.
 * ------------------------------------------------------------------------ */
/* Workspace of hpl_outlier_filter for `batch` clouds of n_total points together, in bytes (monotone in n_total); -1 for a
 * batch outside 1 .. 64 or a count outside 0 .. 2^31 / 3 - 1. */
int64_t hpl_outlier_filter_workspace_bytes(int batch, int64_t n_total);
/* pc (3, N) float32 SoA (row stride pc_ld >= N).  batch (1 .. 64) clouds: prefix (HOST, batch + 1 ints from 0 to N,
 * non-decreasing, empty clouds allowed) travels in the kernel arguments.  mode 0 statistical (k 1 .. 32, std_ratio finite and
 * >= 0; min_neighbors is not read), 1 radius (min_neighbors 1 .. 2^31 - 1; k and std_ratio are not read; mean_dist and nbr_d2
 * must be NULL).  radius finite and > 0 in both.
 * The definition is over ALL PAIRS of a cloud; the grid is an accelerator only (tests/outlier_oracle.py restates the
 * definition in numpy without a grid).
 * TAKING PART (hpl_normals' rule): cell_k = floor(x_k * (1 / (1.001 * radius))) in float64 (the product 1.001 * radius, the
 * quotient and the product with x_k each rounded once); a point takes part when its three coordinates are finite and
 * |cell_k| <= 2^18 - 2 for k = x, y, z.  A point that does not is REMOVED: keep 0, count 0, mean_dist +inf (nbr_d2 +inf); it
 * is in nobody's neighbourhood and in no statistic.
 * DISTANCE d2(i, j) = (dx * dx + dy * dy) + dz * dz in float32 with dx = p_i.x - p_j.x, every operation rounded, no
 * contraction (the arithmetic of hpl_knn_interp and hpl_normals).  r2 = float32(radius * radius), the product in float32.
 * NEIGHBOURS of a point i that takes part: the OTHER indices j != i of the same cloud that take part with d2(i, j) <= r2 (and
 * d2 < +inf: a distance that overflows float32 is nobody's).  Another index at the same position is a neighbour with d2 = 0.
 * STATISTICAL: c_i = min(k, neighbours); the c_i smallest d2, ascending (values only: ties need no index rule);
 * S = sum_t sqrt((double)d2_t) in float64 in that order from 0, the root correctly rounded;
 * s = S + (double)(k - c_i) * (double)radius -- a neighbour that was not found counts at the radius: an isolated point gets
 * `radius`, a stray pair does not look dense --; mean_dist[i] = float32(s / (double)k); count[i] = c_i; nbr_d2 [N][k] float32 =
 * the list, then +inf.
 * Per cloud b over its n' participating points and their float32 mean_dist m widened to float64: mu = (sum m) / n';
 * sigma = sqrt(sum (m - mu)^2 / (n' - 1)) (two passes, the sample form; 0 for n' < 2; mu = 0 for n' = 0);
 * T = mu + (double)std_ratio * sigma; thresh[b] = float32(mu, sigma, T, 0).  KEEP iff the point takes part and
 * mean_dist[i] <= thresh[b][2]: the float32 values compared as published, so the classification can be recomputed from the
 * two outputs alone.  Order of the float64 sums: workgroups of 1024 consecutive points that never straddle clouds; lane l of
 * 256 adds its points l, l + 256, l + 512, l + 768 in that order from 0; one LDS tree over the lanes (halving strides); the
 * workgroups' partials folded in 16 strided runs in index order, then the runs in order.  The order depends on the cloud's
 * point count alone.
 * RADIUS: count[i] = the number of neighbours (not capped); KEEP iff the point takes part and count[i] >= min_neighbors;
 * thresh[b] = 0.
 * keep (N) uint8; keep_idx (N) int32: per cloud from prefix[b] on the packed indices of its kept points, ascending, then -1;
 * stats [batch][4] int32 = (points taking part, kept, removed though taking part, not taking part); thresh [batch][4]
 * float32.  An empty cloud of a batch with N > 0 gets zeros in thresh and stats from the call itself.  Each of keep, keep_idx,
 * mean_dist, count, nbr_d2 may be NULL.
 * No floating-point atomic; a cloud's outputs are the same bits alone, anywhere in a batch and beside other work.
 * Stream-ordered, a fixed number of launches: keys, one stable radix sort of (key, 16-byte record), one search launch (a
 * lane per sorted record; the list of the smallest d2 in registers, instances of 8, 16 and 32 entries, and a count-only
 * instance for the radius mode); statistical only: two sum launches; then thresh (a workgroup per cloud), classify, scan (a
 * workgroup per cloud; writes stats) and, with keep_idx, emit.  Beside the sort: 8 launches statistical, 6 radius, one
 * fewer without keep_idx.  No copy back, no host synchronisation; no lane or workgroup waits for another; every loop is
 * bounded by a cell's population, log2 N or a cloud's workgroups.  The search costs the population of 27 cells per point: all
 * points in one cell is quadratic.
 * workspace: DEVICE, 256-byte aligned, >= hpl_outlier_filter_workspace_bytes(batch, N).
 * HPL_EINVAL before any launch (and without a device): null pc / prefix / thresh / stats / workspace; batch or mode out of
 * range; radius <= 0 or not finite; statistical: k outside 1 .. 32, std_ratio < 0 or not finite; radius: min_neighbors < 1,
 * mean_dist or nbr_d2 given; a prefix that does not start at 0 or decreases; N >= 2^31 / 3; N k >= 2^31 with nbr_d2 given; a
 * row stride below N; misaligned arrays; a workspace that is too small or misaligned; an output that overlaps pc, the
 * workspace or another output.  N == 0 is a no-op. */
int hpl_outlier_filter(const float *pc, int64_t pc_ld, int batch, const int64_t *prefix /* HOST */,
                       int mode /* 0 statistical, 1 radius */, int k, float radius, float std_ratio, int min_neighbors,
                       uint8_t *keep /* (N) or NULL */, int32_t *keep_idx /* (N) or NULL */,
                       float *mean_dist /* (N) or NULL */, int32_t *count /* (N) or NULL */,
                       float *nbr_d2 /* [N][k] or NULL, statistical only */,
                       float *thresh /* [batch][4] */, int32_t *stats /* [batch][4] */,
                       void *workspace, int64_t workspace_bytes, hplStream stream);

/* ------------------------------------------------------------------------ *
 * Maps from clouds (csrc/render.hip): every point projected through its frame's pinhole camera, a z-buffer that keeps the
 * nearest point per pixel, which points the camera sees, and the raw values of KITTI's three scene-flow PNGs -- the inverse
 * of the frames entries above.
 * ------------------------------------------------------------------------ */
/* BOTH ENTRIES take a ragged batch of clouds and one frame per cloud: batch 1 .. 64; prefix HOST, batch + 1 ints from 0 to N,
 * non-decreasing (empty clouds allowed): cloud b owns the packed points prefix[b] .. prefix[b + 1], and a point's LOCAL index
 * counts from its cloud's start.  height[b], width[b] HOST int32, each >= 0; pixel_prefix HOST, batch + 1 ints from 0 to M with
 * pixel_prefix[b + 1] - pixel_prefix[b] == height[b] * width[b] (empty frames allowed): frame b owns those pixels of every
 * packed per-pixel array, row-major, pixel (i, j) -- row i, column j -- at i * width + j.  N < 2^31 / 3 and M < 2^31 / 3.
 * PROJECTION of a point (X, Y, Z) by the camera (f, cx, cy, constx, consty, constz) -- the six floats of
 * hpl_metrics_pair.camera, the order of the reference's utils/geometry.py:project_3d_to_2d, which is what hpl_flow_metrics
 * computes --, every operation in float32, rounded once, no contraction:
 *   zc = Z + constz;  u = ((X * f + cx * Z) + constx) / zc;  v = ((Y * f + cy * Z) + consty) / zc
 * The point is PROJECTABLE when X, Y, Z are finite and zc >= near_z (a NaN zc is not).  Its pixel is j = rintf(u),
 * i = rintf(v), ties to even; it is INSIDE when it is projectable, 0 <= rintf(u) <= width - 1 and 0 <= rintf(v) <= height - 1,
 * decided on the floats before any conversion to an integer: a huge, infinite or NaN u is outside and is never cast,
 * rintf(-0.5f) = -0.0f is inside.
 * Z-BUFFER: one 64-bit word per pixel, all ones at first.  Every inside point offers the key (bits(zc) << 32) | local index to
 * every pixel of the (2 footprint + 1)^2 square around (i, j) that lies in the image (a point that is not inside offers
 * nothing); the pixel keeps the smallest key (a 64-bit integer atomic minimum).  zc > 0, so its bits order as its value: the
 * pixel's WINNER is the nearest point, ties going to the smaller index, whatever the order of the atomics.  A point looks at
 * the word first and leaves the atomic out when its key cannot lower it: the word only ever decreases.
 * Stream-ordered, launches whose number and sizes depend on the prefixes alone (clear, splat with a lane per point, then a
 * lane per pixel -- hpl_render_maps: and a lane per point again), no copy back, no host synchronisation, no floating-point
 * atomic (the counts are integers); no lane or workgroup waits for another.  A cloud's outputs are the same bits alone,
 * anywhere in a batch and beside other work.
 * workspace: DEVICE, 256-byte aligned, >= hpl_render_workspace_bytes(batch, M): the z-buffer.
 * HPL_EINVAL before any launch (and without a device): batch out of range; a null array (those marked "or NULL" may be, and
 * so may an array of no elements); a prefix that does not start at 0 or decreases; a negative height or width; a pixel prefix that disagrees with height * width;
 * N or M >= 2^31 / 3; footprint outside 0 .. 4; a row stride below its count or above 2^40; misaligned arrays (4 bytes for
 * float32 and int32, 2 for uint16); a workspace that is too small or misaligned; an output that overlaps an input, another
 * output or the workspace (row by row: views that interleave inside one buffer are fine); and what each entry adds below. */
/* Workspace of either entry for `batch` frames of m_total pixels together, in bytes (monotone in m_total); -1 for a batch
 * outside 1 .. 64 or m_total outside 0 .. 2^31 / 3 - 1. */
int64_t hpl_render_workspace_bytes(int batch, int64_t m_total);
/* pc (3, N) float32 SoA (row stride pc_ld >= N); attr (channels, N) float32 SoA (row stride attr_ld >= N) riding along,
 * channels 0 .. 8 (attr may be NULL with channels == 0); camera HOST [batch][6]; rel_tol, abs_tol finite and >= 0; near_z
 * finite and > 0.  Refused as well: channels out of range, an f that is zero or not finite, a negative or non-finite
 * tolerance, near_z <= 0 or not finite.
 * OUTPUTS: pixel_of (N) int32: i * width + j of the point's own pixel, -1 for a point that is not inside.  winner (M) int32:
 * the local index of the pixel's winner, -1 without one.  depth (M) float32: the winner's zc, 0 without one.  attr_map
 * (channels, M) float32 (row stride attr_map_ld >= M) or NULL: the winner's channels, 0 without one.  visible (N) uint8: 1 when
 * the point is inside and zc <= (zmin * (1 + rel_tol)) + abs_tol in float32, each operation (the sum 1 + rel_tol too) rounded
 * once, zmin the depth at the point's own pixel; else 0.  A pixel's winner is always visible; with a footprint the zmin of a
 * point's pixel may belong to a neighbour.  stats [batch][4] int32 = (points inside, pixels covered, points visible, points
 * not projectable).
 * Four launches: clear, splat (writes pixel_of), resolve (winner, depth, attr_map; the covered count a wave reduction and one
 * integer atomic), visibility.  With N == 0 and M == 0 nothing is launched and nothing is written; with one of them 0 the
 * launches of the other side still run (an empty image sees no point, an empty cloud covers no pixel). */
int hpl_render_maps(const float *pc, int64_t pc_ld, const float *attr, int64_t attr_ld, int channels, int batch,
                    const int64_t *prefix /* HOST */, const float *camera /* HOST [batch][6] */, const int32_t *height /* HOST */,
                    const int32_t *width /* HOST */, const int64_t *pixel_prefix /* HOST */, int footprint, float rel_tol,
                    float abs_tol, float near_z, int32_t *pixel_of /* (N) */, int32_t *winner /* (M) */, float *depth /* (M) */,
                    float *attr_map /* (channels, M) or NULL */, int64_t attr_map_ld, uint8_t *visible /* (N) */,
                    int32_t *stats /* [batch][4] */, void *workspace, int64_t workspace_bytes, hplStream stream);
/* The raw values of KITTI's scene-flow PNGs from a frame's two clouds: pc1 (3, N) the cloud of frame 1, pc2 (3, N) its partner
 * pc1 + flow, point for point; P HOST [batch][12]: each frame's P_rect_02 (the rules of hpl_frames_from_kitti: P01, P10, P20,
 * P21 == 0, P00 == P11 finite and not zero); baseline finite.  The camera of frame b is (-P00, P02, P12, P03, P13, P23), near_z
 * is 1e-3f, and the z-buffer is over pc1: a pixel's winner is the nearest pc1 point whose footprint covers it.
 * Per pixel (i, j) with a winner, whose two points are (X1, Y1, Z1) and (X2, Y2, Z2), in float32, every operation rounded once:
 *   fb = P00 * (float)baseline;  (px2, py2) = the projection of (X2, Y2, Z2)
 *   r_k = rintf((fb / Z_k - 1e-5f) * 256) clamped to 1 .. 65535     (Z is the depth the back-projection calls z)
 *   u = rintf((px2 - (float)j) * 64 + 32768) clamped to 0 .. 65535, v likewise with py2 and i;  m = 1
 * (a NaN clamps to the lower end).  disp1, disp2 (M) uint16 take r_1, r_2 and flow [M][3] uint16 takes (u, v, m), interleaved
 * as the flow_occ file has them.  A pixel without a winner gets 0 in all five planes; one whose winner's pc2 point is not
 * projectable gets r_1 alone and 0 elsewhere.  With footprint 0 a frame back-projected by hpl_frames_from_kitti comes back as
 * its raw maps: every valid pixel exactly, 0 at every other.
 * Three launches: clear, splat, emit.  M == 0 is a no-op. */
int hpl_maps_to_kitti(const float *pc1, int64_t pc1_ld, const float *pc2, int64_t pc2_ld, int batch,
                      const int64_t *prefix /* HOST */, const int32_t *height /* HOST */, const int32_t *width /* HOST */,
                      const int64_t *pixel_prefix /* HOST */, const float *P /* HOST [batch][12] */, float baseline, int footprint,
                      uint16_t *disp1 /* (M) */, uint16_t *disp2 /* (M) */, uint16_t *flow /* [M][3] */, void *workspace,
                      int64_t workspace_bytes, hplStream stream);

#ifdef __cplusplus
}
#endif
#endif /* HPL_BCL_H */
