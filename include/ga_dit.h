/*
 * ga_dit.h -- C-ABI of the MI355X-native DiT/SiT denoiser forward (bf16 MFMA, fp32 residual stream).
 *
 * Drop-in boundary for the denoise half of GaussianAnything's render-and-denoise hot path: one call of
 * ga_dit_forward() computes what the reference computes in
 *     DiT_I23D_PCD_PixelArt_noclip.forward              /root/reference/dit/dit_i23d.py:511-567   (stage 1)
 *     DiT_I23D_PCD_PixelArt_noclip_clay_stage2.forward  /root/reference/dit/dit_i23d.py:707-750   (stage 2)
 * i.e. everything torchdiffeq calls per function evaluation through
 *     transport/integrators.py:104-107 -> Transport.velocity_ode (transport/transport.py:209-218) -> model(x, t, **kw).
 * The block arithmetic replaces the third-party kernels the reference reaches through
 *     xformers.ops.memory_efficient_attention   vit/vision_transformer.py:297, ldm/modules/attention.py:538-548
 *     xformers FusedMLP                         dit/dit_models_xformers.py:281-286
 *     RMSNorm (apex or dit/norm.py:29-43), t2i_modulate (dit_models_xformers.py:53-54)
 * The per-op entry points (ga_gemm_bf16, ga_attention_bf16, ...) are exported as well: the parity tests call them
 * one by one, and a maintainer can bind them individually.
 *
 * Conventions: every pointer is a DEVICE pointer unless it says "host"; bf16 tensors are raw uint16 (upper half of the
 * fp32 bit pattern, round-to-nearest-even); row-major; all work is enqueued on `stream` (hipStream_t as void*), no
 * host sync, no allocation; return 0 or a negative GA_DIT_ERR_* code.
 */
#ifndef GA_DIT_H
#define GA_DIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GA_DIT_OK 0
#define GA_DIT_ERR_NULL_ARG (-1)
#define GA_DIT_ERR_BAD_SHAPE (-2) /* K % 64 != 0, N % 4 != 0, head_dim != 64, ... (see each entry point) */
#define GA_DIT_ERR_LAUNCH (-4)

typedef uint16_t ga_bf16;

/* epilogues of ga_gemm_bf16:  acc[m][n] = sum_k A[m][k] * W[n][k]  (fp32 accumulate) */
#define GA_GEMM_EPI_STORE_BF16 0 /* out_bf16[m][n] = acc + bias[n]                                      */
#define GA_GEMM_EPI_GELU_BF16 1  /* out_bf16[m][n] = gelu_erf(acc + bias[n])            (FusedMLP fc1) */
#define GA_GEMM_EPI_RESIDUAL 2   /* x_f32[m][n]   += gate[m / rows_per_batch][n] * (acc + bias[n])      */
#define GA_GEMM_EPI_STORE_F32 3  /* x_f32[m][n]    = acc + bias[n]                                      */

typedef struct GaGemmArgs {
    int32_t M, N, K;          /* K % 64 == 0, N % 4 == 0                                             */
    int32_t epilogue;         /* GA_GEMM_EPI_*                                                       */
    const ga_bf16 *A;         /* [M, lda] activations                                                */
    int64_t lda;              /* elements; >= K, multiple of 8                                       */
    const ga_bf16 *W;         /* [N, K] weight as torch.nn.Linear stores it (out_features, in_features) */
    const float *bias;        /* [N] or NULL                                                         */
    void *out;                /* ga_bf16[M, ldo] (EPI 0/1) or float[M, ldo] (EPI 2/3)                */
    int64_t ldo;              /* elements, multiple of 4                                             */
    const float *gate;        /* EPI 2: [M / rows_per_batch, gate_stride] or NULL (= 1)              */
    int64_t gate_stride;      /* elements between the gate rows of consecutive batch items           */
    int32_t rows_per_batch;   /* EPI 2 / V^T store: tokens per batch item                            */
    /* EPI 0 only, optional: output columns n >= vt_col0 (the V projection) are NOT written to `out` but TRANSPOSED into
     * vt[(b*heads + h)*64 + d][token], b = m / rows_per_batch, token = m % rows_per_batch, h*64 + d = n - vt_col0, row
     * length vt_ld (>= rows_per_batch, multiple of 64; the pad must stay zero) -- the layout ga_attention_bf16 reads. */
    ga_bf16 *vt;
    int32_t vt_col0;
    int64_t vt_ld;
    /* EPI 0 only, optional: per-head RMSNorm (eps 1e-5, dit/norm.py:29-43) of the 64-wide column groups ("heads") of the
     * result before the bf16 store -- columns [0, qk_cols0) with weight qk_w0[64], [qk_cols0, qk_cols1) with qk_w1[64]
     * (multiples of 64; 0 = none).  This is the q_norm / k_norm of MemEffAttention / MemoryEfficientCrossAttention
     * applied where the projection is produced instead of where it is consumed. */
    const float *qk_w0, *qk_w1;
    int32_t qk_cols0, qk_cols1;
    /* Folding an UN-modulated RMSNorm (y = x * rsqrt(mean(x^2) + eps) * weight, dit/norm.py:29-43) that sits between a
     * residual GEMM and the next projection into the two GEMMs (one launch and one pass over the stream less); the norm
     * weight is folded into the consumer's W offline (W'[n][k] = W[n][k] * weight[k]):
     *   producer, EPI 2 only, optional (N % 64 == 0): besides x += ..., write emit_x[m][n] = bf16(x_new[m][n]) and
     *     emit_ss[m][n / 64] = sum of x_new[m][.]^2 over that 64-column group (fixed order: deterministic);
     *   consumer, EPI 0 only, optional: with A = emit_x and W', every output row is scaled by
     *     rsqrt(sum_t row_ss[m][t] / row_ss_dim + row_ss_eps) (t < row_ss_tiles) before the per-head qk-norm and the store.
     *     Row m of emit_ss / row_ss starts (tiles rounded up to a multiple of 4) floats after row m - 1; the producer writes the pad
     *     entries as zeros (round 6: widths that are no multiple of 256 -- 1152: 18 sums, 20 floats per row).  row_ss_tiles <= 16
     *     when K is a multiple of 256, <= 20 otherwise; 16-byte aligned.
     * The activations are rounded to bf16 before instead of after the row scale and weight: the same relative rounding. */
    ga_bf16 *emit_x;
    float *emit_ss;
    int64_t emit_ld;          /* elements per row of emit_x, multiple of 8                           */
    const float *row_ss;
    int32_t row_ss_tiles, row_ss_dim;
    float row_ss_eps;
    /* Round 3: W may be given TILED -- [N/8][K/64][8][64] bf16, i.e. the 8 x 64 block a single 1 KiB LDS-DMA instruction moves is
     * contiguous in memory (N % 8 == 0).  Weights are packed once at load time; on weights that stream from HBM (a DiT evaluation
     * reads 600 MB of them) whole-KiB requests measured 3-6 % faster than eight 128-byte row pieces (tools/gemm_lab.hip). */
    int32_t w_tiled;
    /* Round 4: folding a MODULATED RMSNorm, y = x * rsqrt(mean(x^2) + eps) * weight * (1 + scale_b) + shift_b (the adaLN pre-norms of
     * the self-attention and the MLP: dit/dit_models_xformers.py:775-785), between a residual GEMM and the next projection:
     *     y W^T = rsqrt(.) * ((x * weight * (1 + scale_b)) W^T) + shift_b W^T
     *   producer (EPI 2 with emit_x / emit_ss), optional: emit_x[m][n] = bf16(x_new[m][n] * emit_w[n] * (1 + emit_scale[b][n])),
     *     b = m / rows_per_batch, emit_scale rows emit_scale_stride elements apart; emit_ss stays the sum of the RAW x_new^2;
     *   consumer (EPI 0 or 1): row_ss as above, applied to the accumulator BEFORE the bias, and the bias may be one row per batch
     *     item -- bias[b * bias_stride + n], bias_stride != 0 -- holding bias[n] + sum_k shift_b[k] W[n][k] (ga_dit_shift_bias).
     * k_rows (EPI 2, 0 = M): only the first k_rows rows of A take part in the product; the rows behind them get the epilogue with
     *   a zero accumulator (x += gate * bias, and the emit) -- the batch items whose cross-attention is skipped (ca_batch) still
     *   receive the output bias and the folded pre-norm of the next projection in the same launch.  A is not read past row k_rows. */
    const float *emit_w, *emit_scale;
    int64_t emit_scale_stride;
    int64_t bias_stride;
    int32_t k_rows;
    /* Round 6: optional scratch for a DETERMINISTIC split-K (EPI 0 / 1 / 2 without k_rows: reductions whose output tiles cannot fill the
     * chip -- FusedMLP's second linear up to 3072 rows, every wide projection at 768).  2 or 4 workgroups share the reduction of one 192 x 128 / 96 x 128 output tile; the partial
     * tiles meet in the scratch and are added in split order by whichever workgroup arrives last -- results do not depend on the
     * arrival order (bit-reproducible), nobody waits for anybody.  Layout: GA_GEMM_SPLITK_COUNTER_BYTES of tile counters, which must
     * be ZERO before the call and are left zero by it, then the partial tiles.  ga_gemm_splitk_workspace_bytes(M, N) bytes always
     * suffice; NULL or a smaller buffer = no split-K (the same kernels as before).  256-byte aligned.  One launch at a time per
     * scratch buffer (launches on one stream are; concurrent streams need a buffer each). */
    void *splitk_ws;
    int64_t splitk_ws_bytes;
} GaGemmArgs;

#define GA_GEMM_SPLITK_COUNTER_BYTES 16384
#define GA_GEMM_SPLITK_MAX_TILES (GA_GEMM_SPLITK_COUNTER_BYTES / 4)
size_t ga_gemm_splitk_workspace_bytes(int32_t M, int32_t N);
/* Which split-K configuration calls with a scratch take.  MEASURED SLOWER than the unsplit kernels on every shape of the denoiser
 * (profiles/r6_splitk.txt), therefore OFF by default: -1 (default; or the value of the environment variable GA_GEMM_SPLITK at first use)
 * and 0: none; 1: 192 x 128 tiles x 4 splits; 2: 96 x 128 x 2; 3: 96 x 128 x 4; 4: 192 x 128 x 2 (the only one the bf16-store epilogues
 * have); 6: chosen by shape (splits x tiles must fill 160 ... 256 workgroups); 5: the same for EPI 2 only.  A configuration still needs
 * K / 64 divisible by 4 x splits and >= 8 x splits.  Returns the previous mode.  Process-wide. */
int ga_gemm_splitk_mode(int mode);

int ga_gemm_bf16(const GaGemmArgs *args, void *stream);

/* What ga_gemm_bf16 launches for `args` in this process (its environment switches and ga_gemm_splitk_mode included): the launch
 * itself is taken from this plan.  No HIP call -- answers on a machine without a GPU; pointers are checked for NULL and alignment
 * only, never dereferenced.  Returns the error code ga_gemm_bf16 would return for these arguments, or 0 and fills *plan. */
#define GA_GEMM_FAMILY_GENERAL 0  /* gemm_bf16_kernel: 128 columns x 32 MT rows, 4 waves                                       */
#define GA_GEMM_FAMILY_RING 1     /* gemm_ring_kernel: 192 x 128 (8 waves), 96 x 128, 96 x 64, 64 x 64 (4 waves)               */
#define GA_GEMM_FAMILY_SPLITK 2   /* gemm_ring_kernel with `splits` workgroups per output tile (GaGemmArgs.splitk_ws)           */
typedef struct GaGemmPlan {
    int32_t family;           /* GA_GEMM_FAMILY_*                                                    */
    int32_t epilogue;         /* GA_GEMM_EPI_* of the instance                                       */
    int32_t tile_m, tile_n;   /* output rows x columns of a workgroup tile                           */
    int32_t waves;            /* waves per workgroup (64 lanes each)                                 */
    int32_t slots;            /* LDS ring slots (K-tiles of 64)                                      */
    int32_t rem;              /* ring: K-tiles past a multiple of `slots` in the peeled tail         */
    int32_t mt;               /* general: 16-row fragments per wave (tile_m = 32 mt); 0 otherwise    */
    int32_t splits;           /* split-K: workgroups per output tile (= grid_z); 1 otherwise         */
    int32_t grid_x, grid_y, grid_z;
    int32_t xmap;             /* tile -> XCD blocking of the ring kernels                            */
    int32_t wt;               /* write-through output stores                                         */
    int32_t lds_bytes;        /* dynamic LDS per workgroup                                           */
} GaGemmPlan;
int ga_gemm_plan(const GaGemmArgs *args, GaGemmPlan *plan);
/* Every (kernel instance, epilogue) ga_gemm_bf16 is built with, from the table its launch is looked up in: fills up to `capacity`
 * entries (grid_* and the per-call fields xmap / wt zero) and returns how many there are. */
int ga_gemm_instances(GaGemmPlan *out, int32_t capacity);

/* out[b][n] = bias[n] + sum_k shift[b * shift_stride + k] * W[n][k]  (fp32; W [N, K] bf16, row-major or the tiled image; N % 8 == 0,
 * K % 64 == 0; bias may be NULL): the per-batch bias row of a consumer GEMM behind a folded modulated RMSNorm (GaGemmArgs.bias_stride).
 * ga_dit_forward computes these rows for every block's qkv and fc1 projection in one launch per evaluation. */
int ga_dit_shift_bias(const ga_bf16 *W, int32_t w_tiled, const float *bias, int32_t N, int32_t K, const float *shift,
                      int64_t shift_stride, int32_t batch, float *out, void *stream);

/* softmax(q k^T / sqrt(64)) v with per-head RMSNorm of q and k fused on load (weights qn/kn, eps 1e-5; NULL = none):
 * what MemEffAttention / MemoryEfficientCrossAttention compute between their projections.  head_dim must be 64.
 * q row of (batch b, token i, head h) starts at q + (b*Lq + i)*q_stride + h*64 (same for k, out).
 * V is read TRANSPOSED: vt[(b*heads + h)*64 + d][key], row length vt_ld >= Lk rounded up to 64, zero beyond Lk
 * (written in that layout by ga_gemm_bf16's V^T store).  q, k, vt 16-byte aligned with strides % 8 == 0 (k and vt are moved
 * by LDS-DMA unless k_norm_weight is given), out 8-byte aligned with out_stride % 4 == 0. */
typedef struct GaAttentionArgs {
    int32_t batch, heads, Lq, Lk;
    const ga_bf16 *q, *k, *vt;
    int64_t q_stride, k_stride, vt_ld;    /* elements                                               */
    const float *q_norm_weight, *k_norm_weight; /* [64] each                                        */
    ga_bf16 *out;
    int64_t out_stride;
    /* Optional (round 5): the q PROJECTION inside the attention workgroup -- q = A W^T per head, instead of a projection launch in
     * front (the denoiser's cross-attention, /root/reference/ldm/modules/attention.py:497-522: to_q has no bias).  qp_a != NULL: `q`
     * is not read; row (b, i) of A starts at qp_a + (b*Lq + i)*qp_lda, qp_k elements (qp_k % 64 == 0); qp_w = the [heads*64, qp_k]
     * weight, row-major or the tiled image of GaGemmArgs.w_tiled; qp_row_ss (optional) = the rows' partial sums of squares of a folded
     * RMSNorm as GaGemmArgs.row_ss reads them (row scale rsqrt(sum / qp_row_ss_dim + qp_row_ss_eps) applied to the product).  The
     * per-head RMSNorm q_norm_weight is applied to the product, which is rounded to bf16 as the projection GEMM would have stored it.
     * k_norm_weight must be NULL (the LDS-DMA path). */
    const ga_bf16 *qp_a, *qp_w;
    int64_t qp_lda;
    int32_t qp_k, qp_w_tiled;
    const float *qp_row_ss;
    int32_t qp_row_ss_tiles, qp_row_ss_dim;
    float qp_row_ss_eps;
} GaAttentionArgs;

int ga_attention_bf16(const GaAttentionArgs *args, void *stream);

/* What ga_attention_bf16 launches for `args`: attention_fwd_kernel<nw, ks, knorm> (dit_attention.hip); the launch itself, the tail
 * sizing of ga_dit_forward and its decision to project q inside the workgroups are taken from this plan.  No HIP call -- answers on a
 * machine without a GPU; pointers are checked for NULL and alignment only, never dereferenced.  Returns the error code
 * ga_attention_bf16 would return for these arguments, or 0 and fills *plan. */
typedef struct GaAttentionPlan {
    int32_t nw;               /* query waves per key group, 16 query rows each                                  */
    int32_t ks;               /* key groups: group g walks the 64-key tiles g, g + ks, ...; merged through LDS  */
    int32_t knorm;            /* 1: K is RMS-normalised while it is staged (through registers, not LDS-DMA)     */
    int32_t tps;              /* 64-key tiles per barrier stage (2 only for ks == 1 without knorm)              */
    int32_t queries_per_wg;   /* 16 nw                                                                          */
    int32_t fuses_q;          /* 1: this launch computes the q projection itself (GaAttentionArgs.qp_a)         */
    int32_t grid_x, grid_y, grid_z;   /* the attention grid (tail workgroups of ga_dit_forward not included)    */
    int32_t lds_bytes;        /* LDS per workgroup: ks rings of 3 slots x tps tiles of K and of V^T             */
} GaAttentionPlan;
int ga_attention_plan(const GaAttentionArgs *args, GaAttentionPlan *plan);
/* Every kernel instance ga_attention_bf16 is built with (tuning builds excluded): fills up to `capacity` entries (grid_* and fuses_q
 * zero) and returns how many there are. */
int ga_attention_instances(GaAttentionPlan *out, int32_t capacity);

/* The same attention for SHORT key lists, Lk <= 128 (the 77 caption tokens of the text denoisers' cross-attention), head dim 64:
 * attention_short_kernel (dit_attention_short.hip) stages K and V^T of a head once, runs one S = Q K^T pass over at most 8 key
 * fragments with the key columns >= Lk masked, a one-pass softmax with the true row maximum (no rescale, no merge), then P V.  Same
 * arguments and layouts as ga_attention_bf16, q given or projected inside the workgroup (qp_*: the semantics of the 64-query
 * configuration's projection, the projected q rounded to bf16); k_norm_weight must be NULL.  It is NOT one of ga_attention_bf16's
 * instances: nothing dispatches to it by shape -- ga_dit_forward calls it for the cross-attention of block order 1 when
 * ctx_tokens <= 128 (environment switch GA_DIT_SHORT_CA). */
typedef struct GaAttentionShortPlan {
    int32_t queries_per_wg;   /* 64: four waves of 16 query rows                                                */
    int32_t key_tiles;        /* 64-key tiles staged per workgroup: 1 or 2                                      */
    int32_t fuses_q;          /* 1: this launch computes the q projection itself (GaAttentionArgs.qp_a)         */
    int32_t grid_x, grid_y, grid_z;   /* heads * batch, query tiles, 1                                          */
    int32_t lds_bytes;        /* 16 KiB per key tile (K + V^T); + 48 KiB with fuses_q: the ring of the projection's W / A slices */
} GaAttentionShortPlan;
int ga_attention_short_bf16(const GaAttentionArgs *args, void *stream);
/* Host-only like ga_attention_plan: the error code ga_attention_short_bf16 would return (Lk > 128, k_norm_weight, and every
 * misalignment ga_attention_plan refuses), or 0 and the launch geometry. */
int ga_attention_short_plan(const GaAttentionArgs *args, GaAttentionShortPlan *plan);

/* The same attention for head dims OTHER than 64 (head_dim % 8 == 0, <= 128): DiT-PixArt-PCD-CLAY-XL of the reference registry has 16
 * heads of 72 (/root/reference/dit/dit_i23d.py:1526-1535, 1677).  q, k, v row-major: row (b, i) of q starts at q + (b*Lq + i)*q_stride +
 * h*head_dim (k, v: b*Lk + j); q and k ALREADY carry their per-head RMSNorm (ga_head_rmsnorm_bf16); softmax scale head_dim^-1/2.
 * 16-byte aligned operands, strides % 8 == 0; out 8-byte aligned, out_stride % 4 == 0.  With v row-major: the correctness-first kernel of
 * round 5; with vt (below): the tuned one ga_dit_forward uses. */
typedef struct GaAttentionHdArgs {
    int32_t batch, heads, Lq, Lk, head_dim;
    const ga_bf16 *q, *k, *v;
    int64_t q_stride, k_stride, v_stride;   /* elements */
    ga_bf16 *out;
    int64_t out_stride;
    /* Round 6, the tuned variant: vt != NULL -> v / v_stride are ignored and V is read TRANSPOSED, row (b*heads + h)*head_dim + d of
     * vt holds V[b][:, h, d] with the keys contiguous (vt_ld elements per row, a multiple of 64 >= Lk rounded up to 64, columns >= Lk
     * finite) -- the image GaGemmArgs.vt stores for any width.  q_norm_weight != NULL (fp32 [head_dim], 16-byte aligned; V^T variant
     * only): q arrives WITHOUT its per-head RMSNorm, which is applied here (eps 1e-5, dit/norm.py:29-43). */
    const ga_bf16 *vt;
    int64_t vt_ld;
    const float *q_norm_weight;
    const float *k_norm_weight;   /* the same for k (every workgroup normalises the key rows it stages) */
} GaAttentionHdArgs;

int ga_attention_hd_bf16(const GaAttentionHdArgs *args, void *stream);

/* What ga_attention_hd_bf16 launches for `args` in this process (GA_ATTN_HD_QF included): the launch and the tail sizing of
 * ga_dit_forward are taken from this plan.  Host-only like ga_attention_plan; returns the launch's error code or 0. */
#define GA_ATTN_HD_FAMILY_HDV 1   /* attention_hdv_kernel<hd16, qf, nw, ks>: the V^T variant (GaAttentionHdArgs.vt)   */
#define GA_ATTN_HD_FAMILY_HD 2    /* attention_hd_kernel<hdp>: v row-major, 4 waves x 16 queries                      */
typedef struct GaAttentionHdPlan {
    int32_t family;           /* GA_ATTN_HD_FAMILY_*                                                              */
    int32_t hd16;             /* hdv: head dim in 16-wide steps (1 .. 8); 0 otherwise                             */
    int32_t hdp;              /* hd: head dim rounded up to 32 (32 .. 128); 0 otherwise                           */
    int32_t config;           /* hdv: 1 = 4 waves x 16 queries, 2 = 4 x 32, 3 = 8 x 16, 4 = two key groups of 4 x 16; 0 otherwise */
    int32_t qf;               /* 16-query fragments per wave                                                      */
    int32_t nw;               /* waves per workgroup (all key groups)                                             */
    int32_t ks;               /* key groups                                                                       */
    int32_t forced;           /* plan: the configuration came from GA_ATTN_HD_QF; instance list: only that switch reaches it */
    int32_t queries_per_wg;
    int32_t grid_x, grid_y, grid_z;   /* the attention grid (tail workgroups not included)                        */
    int32_t lds_bytes;        /* LDS per workgroup (hdv: dynamic)                                                 */
} GaAttentionHdPlan;
int ga_attention_hd_plan(const GaAttentionHdArgs *args, GaAttentionHdPlan *plan);
/* Every kernel instance ga_attention_hd_bf16 is built with (grid_* zero); returns how many there are. */
int ga_attention_hd_instances(GaAttentionHdPlan *out, int32_t capacity);

/* In place: x[r][h][:] *= rsqrt(mean(x[r][h][:]^2) + 1e-5) * weight[:] for r < rows, h < heads (bf16 storage, fp32 arithmetic; row r starts
 * at x + r*row_stride): the per-head q / k RMSNorm of dit/norm.py:29-43 for head dims the projection GEMM's epilogue does not cover. */
int ga_head_rmsnorm_bf16(ga_bf16 *x, int64_t rows, int64_t row_stride, int32_t heads, int32_t head_dim, const float *weight, void *stream);

/* out_bf16[m][:] = rmsnorm(x[m][:]; eps 1e-5) * weight * (1 + scale[b][:]) + shift[b][:],  b = m / rows_per_batch
 * (scale / shift NULL = plain RMSNorm).  dit/norm.py:29-43 + t2i_modulate.  D % 4 == 0, D <= 2048. */
typedef struct GaRmsNormArgs {
    int32_t M, D, rows_per_batch;
    const float *x;
    const float *weight;
    const float *scale, *shift; /* [M / rows_per_batch, mod_stride]                                  */
    int64_t mod_stride;
    ga_bf16 *out;
    /* optional: rows >= row_bias_first first receive x[row] += row_bias (WRITTEN BACK to x, which is then not const) --
     * how the residual stream of batch items whose cross-attention was skipped gets the projection bias (see ca_batch) */
    const float *row_bias;      /* [D] or NULL */
    int32_t row_bias_first;
} GaRmsNormArgs;

int ga_rmsnorm_modulate(const GaRmsNormArgs *args, void *stream);

/* Small dense layer for the conditioning path (a handful of rows):
 *   y[b][n] = act_out( sum_k act_in(x[b][k]) * W[n][k] + bias[n] ) (+ add[b][n]);  act: 0 none, 1 SiLU.  B <= 16, K % 8 == 0. */
typedef struct GaSmallLinearArgs {
    int32_t B, N, K, act_in, act_out;   /* act_*: 0 none, 1 SiLU; act_in 2: x is [B] timesteps, the input row is the reference's
                                           sinusoidal timestep_embedding(t, 256) formed on the fly (K = 256)                      */
    const float *x;      /* [B, K]            */
    const ga_bf16 *W;    /* [N, K]            */
    const float *bias;   /* [N] or NULL       */
    const float *add;    /* [B, N] or NULL    */
    float *y;            /* [B, N]            */
} GaSmallLinearArgs;

int ga_small_linear(const GaSmallLinearArgs *args, void *stream);

/* ---- whole forward --------------------------------------------------------------------------------------------- */

typedef struct GaDitBlockWeights {
    /* cross-attention on the image tokens (cross_attn_dino, prenorm_ca_dino) */
    const float *prenorm_ca_w;           /* [D]                                         */
    const ga_bf16 *ca_q_w;               /* [D, D]      to_q (no bias)                  */
    const ga_bf16 *ca_q_w_prenorm;       /* [D, D] or NULL: to_q with prenorm_ca_w folded into its columns (to_q[n][k] *
                                          * prenorm_ca_w[k]); when given, blocks after the first run the pre-norm folded
                                          * into the previous fc2 and this projection (see GaGemmArgs) */
    const ga_bf16 *ca_kv_w;              /* [2D, ctx]   to_k rows then to_v rows        */
    const float *ca_q_norm_w, *ca_k_norm_w; /* [64]                                     */
    const ga_bf16 *ca_out_w;             /* [D, D]      to_out.0                        */
    const float *ca_out_b;               /* [D]                                         */
    /* self-attention (attn, norm1) */
    const float *norm1_w;                /* [D]                                         */
    const ga_bf16 *qkv_w;                /* [3D, D]                                     */
    const float *qkv_b;                  /* [3D]                                        */
    const float *q_norm_w, *k_norm_w;    /* [64]                                        */
    const ga_bf16 *proj_w;               /* [D, D]                                      */
    const float *proj_b;                 /* [D]                                         */
    /* FusedMLP (mlp, norm2) */
    const float *norm2_w;                /* [D]                                         */
    const ga_bf16 *fc1_w;                /* [4D, D]                                     */
    const float *fc1_b;                  /* [4D]                                        */
    const ga_bf16 *fc2_w;                /* [D, 4D]                                     */
    const float *fc2_b;                  /* [D]                                         */
    const float *scale_shift_table;      /* [6, D]                                      */
    /* Text models (dit/dit_trilatent.py, PixelArtTextCondDiTBlock.attention_y_norm), NULL = none: [context_dim] weight of an RMSNorm
     * (eps 1e-5) every block applies to the context tokens before its to_k / to_v: ga_dit_cache_context_ws projects K | V^T of this
     * block from RMSNorm(ctx) * ctx_norm_w.  prenorm_ca_w / ca_* then carry prenorm_ca_text / cross_attn.*. */
    const float *ctx_norm_w;
} GaDitBlockWeights;

typedef struct GaDitModel {
    int32_t hidden, depth, heads, in_channels, out_channels, context_dim, stage2;
    const ga_bf16 *t_mlp0_w; const float *t_mlp0_b;     /* [D,256], [D]   t_embedder.mlp.0            */
    const ga_bf16 *t_mlp2_w; const float *t_mlp2_b;     /* [D,D], [D]     t_embedder.mlp.2            */
    const float *pool_ln_w, *pool_ln_b;                 /* [ctx]          pooled_vec_embedder.0       */
    const ga_bf16 *pool_w; const float *pool_b;         /* [D,ctx], [D]   pooled_vec_embedder.1       */
    const ga_bf16 *adaln_w; const float *adaln_b;       /* [6D,D], [6D]   adaLN_modulation.1          */
    const float *xe_fc1_w, *xe_fc1_b;                   /* [D,C], [D]     x_embedder.fc1 (fp32, K tiny) */
    const ga_bf16 *xe_fc2_w; const float *xe_fc2_b;     /* [D,D], [D]     x_embedder.fc2              */
    const float *xyz_w, *xyz_b;                         /* [D,63], [D]    xyz_pos_embed.xyz_projection (stage 2) */
    const float *final_table;                           /* [2,D]          final_layer.scale_shift_table */
    const float *final_w, *final_b;                     /* [Cout,D], [Cout] final_layer.linear (fp32) */
    const GaDitBlockWeights *blocks;                    /* host array [depth]                          */
    int32_t gemm_weights_tiled;                         /* 1: every bf16 [N, K] weight that goes through ga_gemm_bf16 (block weights,
                                                           xe_fc2_w) is stored tiled, see GaGemmArgs.w_tiled; the small-linear
                                                           weights (t_mlp*, pool_w, adaln_w) stay row-major */
    /* ---- the caption-conditioned twins (DiT_PCD_PixelArt, DiT_PCD_PixelArt_tofeat: /root/reference/dit/dit_trilatent.py:262-419);
     *      every field 0 / NULL = the image models above, launch for launch ---- */
    int32_t block_order;                                /* 0: cross-attention, self-attention, MLP (ImageCondDiTBlockPixelArtRMSNormClayLRM);
                                                           1: self-attention, cross-attention, MLP (PixelArtTextCondDiTBlock, dit_models_xformers.py:357-376).
                                                           Order 1 is built for heads of 64 only: any other head dim (the registry's unreleased
                                                           DiT-PCD-XL-stage2-xyz2feat, 16 x 72) is REFUSED with GA_DIT_ERR_BAD_SHAPE before anything is enqueued */
    const ga_bf16 *final_adaln_w; const float *final_adaln_b;   /* [2D, D], [2D]  final_layer.adaLN_modulation.1, row-major.  When set the final layer is
                                                           the reference's FinalLayer (dit_models_xformers.py:993-1016): (shift | scale) = Linear(SiLU(t)) per batch item
                                                           -- one small-linear launch -- in place of final_table + t; final_table is not read.  The fused sampler
                                                           step (GaDitSamplerStep) works on it unchanged.  pool_* then carry cap_embedder.{0,1} and img_vector the caption vector */
} GaDitModel;

/* Optional sampler step fused into the final layer (GaDitForwardArgs.step): the Euler update of the reference's fixed-grid
 * sampling loop (/root/reference/transport/integrators.py:100-119 with torchdiffeq's euler: y += dt * f(t, y)) around
 * forward_with_cfg (/root/reference/dit/dit_i23d.py:159-172):
 *     v      = cfg ? u + cfg_scale * (c - u) : model output          (c, u: rows of batch item b < B'/2 and b + B'/2)
 *     state += dt * v                                                 (both CFG halves receive the same v)
 *     traj[(*counter + 1) * traj_stride ...] = state                  (the [num_steps, *x.shape] output of sample_ode)
 * every product and sum rounded once, in this order -- bit-identical to the eager PyTorch loop.  `state` is the x of the
 * evaluation (GaDitForwardArgs.x must point at it); `out` is not written.  ga_dit_sampler_advance moves the step on. */
typedef struct GaDitSamplerStep {
    float cfg_scale;
    int32_t cfg;              /* 1: combine the two CFG halves; 0: v = model output                     */
    const float *dt;          /* device scalar: step size of this step                                  */
    float *state;             /* [B', L, Cout] fp32, updated in place                                    */
    float *traj;              /* trajectory base (slice 0 = initial state, written by the caller) or NULL */
    int64_t traj_stride;      /* floats per slice = B' * L * Cout                                        */
    const int32_t *counter;   /* device: index of the grid interval this step integrates                */
    float *velocity;          /* NULL: the Euler step above.  Otherwise ONLY the velocity of the evaluation -- the model output, or with
                                 cfg the guided combination u + s (c - u) in BOTH halves (forward_with_cfg's return value) -- is written
                                 here, [B', L, Cout]; dt / state / traj / counter are not used (the stages of ga_ode_dopri5_*, the evaluations of ga_sde_step) */
} GaDitSamplerStep;

typedef struct GaDitForwardArgs {
    int32_t batch;            /* B' (CFG batch: 2 x samples), <= 16                                    */
    int32_t tokens;           /* L latent tokens per batch item                                        */
    int32_t ctx_tokens;       /* M image tokens per batch item                                         */
    const float *x;           /* [B', L, C]                                                            */
    const float *timesteps;   /* [B']                                                                  */
    const float *img_vector;  /* [B', ctx]                                                             */
    const float *fps_xyz;     /* [B', L, 3] (stage 2) or NULL                                          */
    const ga_bf16 *ca_k;      /* [depth][B'*M, D]        cached K projections of the image tokens (ga_dit_cache_context) */
    const ga_bf16 *ca_vt;     /* [depth][B'*D, Mp] cached V projections, transposed (row b*D + h*head_dim + d), Mp = M rounded up to 64,
                                 zero pad -- the same two images for every head dim since round 6                                     */
    float *out;               /* [B', L, Cout] fp32 (the reference returns x.float())                  */
    void *workspace;          /* ga_dit_workspace_bytes()                                              */
    size_t workspace_bytes;
    /* Number of LEADING batch items whose image tokens are not all zero (<= 0 or > batch: all).  For an all-zero context
     * (the unconditional half of a CFG batch: sgm's force_uc_zero_embeddings) K = V = 0 exactly (to_k / to_v have no bias,
     * RMSNorm(0) = 0), the softmax is uniform over zeros and the block's cross-attention reduces to `x += to_out.bias`:
     * those items skip the q projection, the 1369-key attention and the output projection -- bit-identical result. */
    int32_t ca_batch;
    const GaDitSamplerStep *step;   /* host pointer, NULL = plain function evaluation into `out`                */
    /* [B', D] fp32 or NULL: pooled_vec_embedder(img_vector) = Linear(LayerNorm(img_vector)) (dit_i23d.py:540-545) as ga_dit_pooled_vector
     * computed it for THIS img_vector.  It does not depend on the time: a sampling loop computes it once per conditioning instead of
     * in each of its ~250 evaluations (two launches of the evaluation's serial head).  NULL: computed inside, into the workspace. */
    const float *pooled_vec;
} GaDitForwardArgs;

size_t ga_dit_workspace_bytes(const GaDitModel *model, int32_t batch, int32_t tokens, int32_t ctx_tokens);

/* K/V of every block's cross-attention depend only on the (step-invariant) image tokens: project them once per
 * sample.  img_crossattn: bf16 [B'*M, ctx]; outputs as described in GaDitForwardArgs (ca_vt must be zero-filled by the
 * caller beforehand: only the first M keys of every row are written). */
int ga_dit_cache_context(const GaDitModel *model, int32_t batch, int32_t ctx_tokens, const ga_bf16 *img_crossattn,
                         ga_bf16 *ca_k, ga_bf16 *ca_vt, void *stream);

/* The same with a scratch for the normalised context of models whose blocks carry ctx_norm_w: ga_dit_context_scratch_bytes() bytes
 * (0 for a model without ctx_norm_w), 256-byte aligned.  ga_dit_cache_context is this call without a scratch: it returns
 * GA_DIT_ERR_NULL_ARG for a model that needs one.  Once per conditioning, not hot: a norm pass per block, then the same GEMM. */
size_t ga_dit_context_scratch_bytes(const GaDitModel *model, int32_t batch, int32_t ctx_tokens);
int ga_dit_cache_context_ws(const GaDitModel *model, int32_t batch, int32_t ctx_tokens, const ga_bf16 *ctx, ga_bf16 *ca_k, ga_bf16 *ca_vt,
                            void *scratch, size_t scratch_bytes, void *stream);

int ga_dit_forward(const GaDitModel *model, const GaDitForwardArgs *args, void *stream);

/* pooled_vec_embedder of the reference model (LayerNorm with affine over context_dim, then Linear context_dim -> D, bf16-rounded
 * inputs as under autocast): img_vector [B', ctx] fp32 -> out [B', D] fp32; scratch [B', ctx] fp32.  See GaDitForwardArgs.pooled_vec. */
int ga_dit_pooled_vector(const GaDitModel *model, int32_t batch, const float *img_vector, float *scratch, float *out, void *stream);

/* host: one tiny kernel closing a fused sampler step: ++*counter; timesteps[0..batch) = t_grid[*counter];
 * *dt = dt_grid[*counter] (both grids fp32 device arrays of num_steps - 1 entries; reads past the end are clamped). */
int ga_dit_sampler_advance(int32_t *counter, const float *t_grid, const float *dt_grid, int32_t grid_len, float *timesteps,
                           int32_t batch, float *dt, void *stream);

/* ---- device-resident Dormand-Prince 5(4): the reference's default sampler (Sampler.sample_ode(sampling_method="dopri5"),
 * /root/reference/transport/transport.py:384-431 -> torchdiffeq.odeint, transport/integrators.py:111-118).  One attempted step is
 *     for i in 0..5:  ga_ode_dopri5_stage(o, i);  ga_dit_forward(x = o->ystage, timesteps = o->timesteps, step.velocity = o->k[i + 1])
 *     ga_ode_dopri5_finish(o)
 * -- a fixed launch sequence (capture it into a hipGraph and replay it) that keeps time, step size, the accept / reject decision and
 * the counters in `ctl`; the host only reads ctl[GA_ODE_DONE] after a replay.  Before the first step the caller puts the initial
 * state into y, f(t0, y0) into k[0], and t0 / the first step size / atol / rtol / JNEXT = 1 (out[0] = y0 is the caller's) into ctl. */
#define GA_ODE_T 0          /* time of the state y (fp64)                                  */
#define GA_ODE_DT 1         /* size of the NEXT attempted step                             */
#define GA_ODE_SUMSQ 2      /* sum of squares the last decision was taken on (diagnostic)  */
#define GA_ODE_ATOL 3
#define GA_ODE_RTOL 4
#define GA_ODE_DONE 5       /* 1: the last requested time has been produced (or ERROR set) */
#define GA_ODE_STEPS 6      /* attempted steps                                             */
#define GA_ODE_REJECTED 7
#define GA_ODE_ACCEPT 8     /* the step just attempted was accepted                        */
#define GA_ODE_TA 9         /* its interval                                                */
#define GA_ODE_TB 10
#define GA_ODE_DT_USED 11
#define GA_ODE_JNEXT 12     /* next requested time not produced yet                        */
#define GA_ODE_JBEG 13      /* requested times inside the accepted step: first, count      */
#define GA_ODE_JCOUNT 14
#define GA_ODE_ERROR 15     /* 1: non-finite error ratio (NaN / inf model output), 2: step size underflow */
#define GA_ODE_RATIO 16     /* error ratio of the step just attempted (diagnostic)         */
#define GA_ODE_CTL_WORDS 24          /* the scalar head: what the host reads back after a replay                                      */
#define GA_ODE_MAX_PARTIALS 2048     /* behind the head: one partial sum of the error norm per workgroup of the error launch, added  */
#define GA_ODE_CTL_ALLOC (GA_ODE_CTL_WORDS + GA_ODE_MAX_PARTIALS)   /* by the controller in a fixed order (bit-reproducible steps)      */

typedef struct GaOdeDopri5 {
    int64_t n;              /* floats of the state: B' * L * C                             */
    int32_t batch;          /* B': entries of `timesteps`                                  */
    int32_t grid_len;       /* requested times                                             */
    float *y;               /* [n] state at ctl[T]                                         */
    float *k[7];            /* [n] each: k[0] = f(t, y) (FSAL), k[1..6] the stage derivatives */
    float *ystage;          /* [n] input of the next function evaluation; after stage 5: the 5th-order solution */
    float *timesteps;       /* [B'] time of the next function evaluation (fp32, as the reference passes it)     */
    double *ctl;            /* [GA_ODE_CTL_ALLOC] device scalars (head of GA_ODE_CTL_WORDS) + the error-norm partials */
    const double *t_grid;   /* [grid_len] requested times, increasing                     */
    float *out;             /* [grid_len, n] dense output (slice 0 is the caller's)        */
    int64_t ctl_words;      /* doubles allocated behind `ctl`: at least GA_ODE_CTL_WORDS + min(ceil(n / 256), GA_ODE_MAX_PARTIALS);
                             * GA_ODE_CTL_ALLOC always suffices.  ga_ode_dopri5_finish returns GA_DIT_ERR_BAD_SHAPE below that
                             * (the error launch writes one partial per workgroup behind the head).                          */
} GaOdeDopri5;

int ga_ode_dopri5_stage(const GaOdeDopri5 *ode, int32_t stage, void *stream);
int ga_ode_dopri5_finish(const GaOdeDopri5 *ode, void *stream);

/* ---- device-resident SDE sampling: the reference's Sampler.sample_sde (/root/reference/transport/transport.py:322-382) with its stepper
 * class `sde` (transport/integrators.py:8-75) for a VELOCITY model on the GVP / Linear path.  With v = the model output at (x, t),
 *     score = (r v - x) / var,  drift = v + w score                                              (path.py:70-84, transport.py:282-284)
 * where w(t) is the diffusion coefficient, r = alpha / alpha', var = sigma^2 - r sigma' sigma: one evaluation per point (the reference
 * calls the model once for the drift and once more for the score).  One step is a fixed chain of launches,
 *     Euler-Maruyama:  ga_dit_forward(x = state, step.velocity = velocity);  ga_sde_step(EM);  ga_sde_step(ADVANCE)
 *     Heun:            ga_sde_step(HEUN_PERTURB);  ga_dit_forward(x = xhat, ...);  ga_sde_step(HEUN_PREDICT);
 *                      ga_dit_forward(x = state, ...);  ga_sde_step(HEUN_CORRECT);  ga_sde_step(ADVANCE)
 * that reads the step index, the coefficients and the seed from device memory: capture it into a hipGraph once and replay it
 * num_intervals times -- every replay integrates the next interval with fresh noise.  Then one last step (LAST_*) behind an evaluation
 * at (state, t1).  Phases, each one launch over the n floats, every product / quotient / sum rounded on its own in the order written
 * (xi: the step's normals, see below; c = *counter clamped to [0, num_intervals); row = coef row c):
 *     EM            score = (r v - x) / var; drift = v + w score; mean = x + drift dt; x = mean + g (xi sqrt_dt); traj[c] = x
 *     HEUN_PERTURB  xhat = x + g (xi sqrt_dt)
 *     HEUN_PREDICT  k1 = v + w ((r v - xhat) / var); x = xhat + dt k1; timesteps[0..batch) = t2            (v evaluated at (xhat, t))
 *     HEUN_CORRECT  k2 = v + w2 ((r2 v - x) / var2); x = xhat + half_dt (k1 + k2); traj[c] = x             (v evaluated at (x, t2))
 *     LAST_MEAN     traj[num_intervals] = x + (v + w ((r v - x) / var)) dt          (last row: dt = last_step_size, coefficients at t1)
 *     LAST_TWEEDIE  traj[num_intervals] = x / alpha + sig2a ((r v - x) / var)
 *     LAST_EULER    traj[num_intervals] = x + v dt
 *     LAST_NONE     traj[num_intervals] = x                                        (the reference appends the same tensor twice)
 *     ADVANCE       one thread: c' = min(*counter + 1, num_intervals); timesteps[0..batch) = coef[c'].t; *counter = c'
 * Noise of ga_sde_step (EM and HEUN_PERTURB): Philox4x32-10, key = (seed low word, seed high word), counter =
 * (j / 4, c, phase, 0) for draw index j; with the four output words o0..o3, lane = j % 4, p = lane / 2:
 *     u1 = ((o[2p] >> 8) + 1) * 2^-24  in (0, 1],   u2 = (o[2p + 1] >> 8) * 2^-24  in [0, 1),   radius = sqrt(-2 ln u1),
 *     theta = fp32(2 pi) u2,   xi = radius * (lane odd ? sin theta : cos theta)                 (fp32; |xi| <= sqrt(48 ln 2) = 5.77)
 * n_draw = cfg_pairs ? n / 2 : n; with cfg_pairs elements i and i + n / 2 (the two halves of a doubled CFG state) take the SAME normal
 * j = i mod n / 2, so the halves stay equal -- a deliberate departure from the reference, which draws them independently although
 * forward_with_cfg then evaluates the two halves at different x.  The step index comes from *counter, never from a launch
 * argument: a value baked into a captured graph would repeat the same noise on every replay. */
#define GA_SDE_EM 0
#define GA_SDE_HEUN_PERTURB 1
#define GA_SDE_HEUN_PREDICT 2
#define GA_SDE_HEUN_CORRECT 3
#define GA_SDE_LAST_MEAN 4
#define GA_SDE_LAST_TWEEDIE 5
#define GA_SDE_LAST_EULER 6
#define GA_SDE_LAST_NONE 7
#define GA_SDE_ADVANCE 8
/* columns of a coefficient row (GA_SDE_COEF_STRIDE floats): rows 0 .. num_intervals - 1 one per interval, row num_intervals the last step */
#define GA_SDE_C_T 0         /* time of the interval's left end (last row: t1)                */
#define GA_SDE_C_DT 1        /* step size (last row: last_step_size)                          */
#define GA_SDE_C_SQRT_DT 2
#define GA_SDE_C_W 3         /* diffusion coefficient w(t)                                    */
#define GA_SDE_C_G 4         /* sqrt(2 w)                                                     */
#define GA_SDE_C_R 5         /* alpha / alpha'                                                */
#define GA_SDE_C_VAR 6       /* sigma^2 - r sigma' sigma                                      */
#define GA_SDE_C_T2 7        /* Heun: t + dt (fp32 sum) and w, r, var there                   */
#define GA_SDE_C_W2 8
#define GA_SDE_C_R2 9
#define GA_SDE_C_VAR2 10
#define GA_SDE_C_HALF_DT 11  /* 0.5 dt                                                        */
#define GA_SDE_C_ALPHA 12    /* last row, Tweedie: alpha(t1) and sigma(t1)^2 / alpha(t1)      */
#define GA_SDE_C_SIG2A 13
#define GA_SDE_COEF_STRIDE 16

typedef struct GaSdeStep {
    int64_t n;               /* floats of the state: B' * L * C (<= 2^31 - 1; even with cfg_pairs)   */
    int32_t batch;           /* B': entries of `timesteps` (<= 64)                                   */
    int32_t num_intervals;   /* grid intervals = num_steps - 1                                       */
    int32_t cfg_pairs;       /* 1: the state is a doubled CFG batch, both halves take the same noise */
    float *state;            /* [n] updated in place                                                 */
    const float *velocity;   /* [n] output of the evaluation in front (GaDitSamplerStep.velocity)    */
    float *k1;               /* [n] Heun: first drift                                                */
    float *xhat;             /* [n] Heun: perturbed state, input of the first evaluation             */
    float *traj;             /* [num_intervals + 1, n]: slot k = state after step k, last slot = last step */
    int32_t *counter;        /* device: index of the interval this step integrates                   */
    float *timesteps;        /* [B'] time of the next evaluation                                     */
    const float *coef;       /* [num_intervals + 1, GA_SDE_COEF_STRIDE] device                       */
    const uint64_t *seed;    /* device uint64[1] (not read when `noise` is given)                    */
    const float *noise;      /* optional [num_intervals, n_draw]: read instead of drawing            */
    float *noise_out;        /* optional [n_draw]: the normals this launch used                      */
} GaSdeStep;

/* host only, no HIP call: the error code ga_sde_step returns for (step, phase) before it launches anything, or 0 */
int ga_sde_step_check(const GaSdeStep *step, int32_t phase);
int ga_sde_step(const GaSdeStep *step, int32_t phase, void *stream);

const char *ga_dit_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GA_DIT_H */
