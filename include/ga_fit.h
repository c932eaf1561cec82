/*
 * ga_fit.h -- C-ABI of the glue that turns the surfel rasterizer, its backward and the two device losses into one fitting iteration
 * without a host round trip (csrc/surfel_fit.hip): activation of the raw parameters, the adjoint of the renderer's post-processing,
 * a fused chain-rule + Adam step and the advance of the device-side step counter; and, for fitting against more views than one iteration
 * renders, the selection of this iteration's views from a pool on the device (ga_fit_select_views).
 *
 * Conventions as in ga_loss.h: device pointers unless marked host, caller owns every buffer, work is enqueued on `stream`, 0 or a
 * negative GA_ERR_* code is returned, nothing synchronises, allocates or reads back.
 *
 * PARAMETRISATION (the project's own definition, after 2DGS).  raw [N,13] fp32 in the column order of the renderer's Gaussian tensor:
 *   xyz       0..2    identity
 *   opacity   3       1 / (1 + exp(-r))
 *   scale     4..5    exp(r)
 *   rotation  6..9    r / sqrt(w*w + x*x + y*y + z*z), the sum taken in that order
 *   rgb       10..12  1 / (1 + exp(-r))
 *
 * ARITHMETIC CONTRACT.  fp32, every product, quotient, sum and square root rounded on its own (the translation unit is built without
 * FMA contraction; division and square root are the correctly rounded ones).  exp is the device library's.
 *   chain rule   g_raw = g_o (o (1 - o));  g_s s;  (g_q - qhat <qhat, g_q>) inv_norm, the dot product summed w, x, y, z;
 *                g_c (c (1 - c));  xyz unchanged
 *   Adam         m' = b1 m + (1 - b1) g;  v' = b2 v + ((1 - b2) g) g;  denom = sqrt(v') / sbc2 + eps;  raw' = raw - step_g (m' / denom)
 *   table        row t of `table` [max_steps, GA_FIT_TABLE_COLS]: step_g = lr_g(t) / (1 - b1^(t+1)) for the five groups (xyz, opacity,
 *                scale, rotation, rgb), then sbc2 = sqrt(1 - b2^(t+1)), then two unused words; computed in double by the caller,
 *                stored fp32.  The row is selected by *counter, a DEVICE word: a launch argument would be frozen into a captured graph.
 */
#ifndef GA_FIT_H
#define GA_FIT_H

#include <stddef.h>
#include <stdint.h>

#include "ga_surfel.h" /* GA_OK, GA_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define GA_FIT_PARAMS 13
#define GA_FIT_GROUPS 5        /* xyz, opacity, scale, rotation, rgb */
#define GA_FIT_TABLE_COLS 8    /* five step sizes, sbc2, two unused words */
#define GA_FIT_HISTORY_COLS 8  /* total, ssim, l1, l2, normal, dist, alpha, unused */
#define GA_FIT_VISIBLE_ONLY 1  /* ga_fit_adam: a surfel whose radius is 0 in every view keeps raw, m and v untouched */

/* what the three kernels launch, and the layout of the buffer ga_fit_activate writes (offsets in bytes, each 256-byte aligned) */
typedef struct GaFitPlan {
    int32_t threads;        /* lanes per workgroup of all three kernels                                   */
    int32_t pack_vec;       /* pixels per lane of the pack kernel: 4 when H*W % 4 == 0, else 1            */
    int32_t grid_activate;  /* ceil(N / threads)                                                          */
    int32_t grid_adam;      /* ceil(N / threads)                                                          */
    int32_t grid_pack_x;    /* ceil(H*W / pack_vec / threads)                                             */
    int32_t grid_pack_y;    /* V                                                                          */
    size_t means, opacities, colors, scales, rotations, inv_norm;   /* [N,3] [N] [N,3] [N,2] [N,4] [N]    */
    size_t workspace_bytes; /* the whole of it                                                            */
} GaFitPlan;

/* host only, no HIP call: GA_OK, GA_ERR_NULL_ARG or GA_ERR_BAD_SHAPE (N, V, H, W >= 1, V <= 65535, H*W < 2^31) */
int ga_fit_plan(int32_t num_points, int32_t num_views, int32_t height, int32_t width, GaFitPlan *plan);

typedef struct GaFitActivateArgs {
    int32_t num_points;
    int32_t reserved;
    const float *raw;   /* [N,13] */
    float *means;       /* [N,3]  */
    float *opacities;   /* [N]    */
    float *colors;      /* [N,3]  */
    float *scales;      /* [N,2]  */
    float *rotations;   /* [N,4] normalised */
    float *inv_norm;    /* [N] 1 / sqrt(w*w + x*x + y*y + z*z) */
} GaFitActivateArgs;
int ga_fit_activate(const GaFitActivateArgs *args, void *stream);

/* The exact adjoint of the differentiable branch of GaussianRenderer2DGS.render:
 *   image = clamp(color, 0, 1);  alpha = allmap[1];  rend_normal_d = sum_c allmap[2+c] view[d,c];  depth = nan_to_num(allmap[5], 0, 0);
 *   dist = allmap[6]
 * g_color = g_image where 0 <= color <= 1, else 0;  g_allmap[0] = 0;  [1] = g_alpha;  [2+c] = sum_d g_rend_normal_d view[d,c] (d = 0, 1,
 * 2 in that order, each term after the first a fused multiply-add: the bits of the batched GEMM autograd's einsum runs);  [5] = g_depth where allmap[5] is finite, else g_depth * 0;  [6] = g_dist.  A NULL gradient contributes zero. */
typedef struct GaFitPackArgs {
    int32_t num_views, height, width, reserved;
    const float *color;          /* [V,3,H,W] out_color of ga_surfel_forward  */
    const float *allmap;         /* [V,7,H,W] out_others of ga_surfel_forward */
    const float *view;           /* [V,16] cam_view                           */
    const float *g_image;        /* [V,3,H,W] or NULL */
    const float *g_rend_normal;  /* [V,3,H,W] or NULL */
    const float *g_depth;        /* [V,1,H,W] or NULL */
    const float *g_dist;         /* [V,1,H,W] or NULL */
    const float *g_alpha;        /* [V,1,H,W] or NULL */
    float *g_color;              /* [V,3,H,W] */
    float *g_allmap;             /* [V,7,H,W] */
} GaFitPackArgs;
int ga_fit_pack_grads(const GaFitPackArgs *args, void *stream);

typedef struct GaFitAdamArgs {
    int32_t num_points, num_views, flags, max_steps;
    const float *g_means, *g_opacities, *g_colors, *g_scales, *g_rotations;   /* what ga_surfel_backward wrote             */
    const float *opacities, *colors, *scales, *rotations, *inv_norm;          /* what ga_fit_activate wrote                */
    float *raw, *m, *v;                                                       /* [N,13] each, updated in place            */
    const int32_t *radii;      /* [V,N]; required with GA_FIT_VISIBLE_ONLY, else ignored                                  */
    const float *table;        /* [max_steps, GA_FIT_TABLE_COLS]                                                          */
    const int32_t *counter;    /* device word: the row of `table` (clamped to [0, max_steps - 1]); read, never written    */
    float beta1, one_minus_beta1, beta2, one_minus_beta2, eps;                /* each rounded from double by the caller   */
    int32_t reserved;
    float *raw_grad;           /* [N,13] or NULL: the gradient in raw space                                               */
} GaFitAdamArgs;
int ga_fit_adam(const GaFitAdamArgs *args, void *stream);

/* One thread: history[*counter] = { total, bias + sum_v w_photo[v,0] photo[v,0], sum_v w_photo[v,1] photo[v,1], ... [v,2],
 * sum_v w_geo[v,0] geo[v,0], ... [v,1], ... [v,2], 0 } (sums in double, rounded once; total is the sum of the six terms), then
 * *counter = min(*counter + 1, max_steps - 1); with `status`, the overflow report of this iteration's forward is folded into `seen`.  A launch of its own: no lane that reads the counter may see the increment. */
typedef struct GaFitAdvanceArgs {
    int32_t num_views, max_steps;
    int32_t *counter;
    const float *photo_out;  /* [V,3] of ga_photo_loss_forward, or NULL            */
    const float *geo_out;    /* [V,3] of ga_geo_loss_forward, or NULL              */
    const float *w_photo;    /* [V,3] the grad_out of ga_photo_loss_backward       */
    const float *w_geo;      /* [V,3] the grad_out of ga_geo_loss_backward         */
    float *history;          /* [max_steps, GA_FIT_HISTORY_COLS]                   */
    float ssim_bias;         /* the ssim weight: the term is weight * (1 - SSIM)   */
    int32_t reserved;
    const int64_t *status;   /* the status words of the forward's workspace, or NULL                                              */
    int64_t *seen;           /* [4] or NULL (required with status): seen[0] |= status[GA_STATUS_OVERFLOW], seen[1] and seen[2] the
                                largest GA_STATUS_NUM_RENDERED and GA_STATUS_SEG_WORK so far.  The status words are those of the LAST
                                forward; these outlive it, so a host that looks every k iterations misses no overflow              */
} GaFitAdvanceArgs;
int ga_fit_advance(const GaFitAdvanceArgs *args, void *stream);

/* View mini-batches.  One launch, the first of the iteration's chain: the B-view buffers the rest of the chain reads are filled from a
 * pool of P views that stays on the device.  The row of `schedule` is t = clamp(*counter, 0, max_steps - 1) -- the same device word that
 * selects the Adam table row, so a captured graph draws another row at every replay; ga_fit_advance, the last launch of the chain, is
 * the only writer, so every reader of the counter in iteration t sees t.  Slot b takes pool view clamp(schedule[t*B + b], 0, P - 1): the
 * caller validates the table, the clamp only guarantees that no lane reads outside the pool.  A row may name a view twice.
 * fp32 data are copied bit for bit (NaN payloads, -0, denormals).  With GA_FIT_SELECT_U8_TARGETS pool_targets is uint8 and the batch
 * receives (float)u / 255.0f, the correctly rounded quotient.  Each lane moves 16 bytes where H*W % 4 == 0 and every pointer below but
 * schedule, counter and selected is 16-byte aligned, else one element; the grid is capped and strided.
 * GA_ERR_NULL_ARG: a required pointer is NULL, or mask / normal is given on one side (pool, batch) only.  GA_ERR_BAD_SHAPE: P, B, H, W or
 * max_steps < 1, B > P, H*W >= 2^31.  GA_ERR_BAD_FLAGS: an unknown flag. */
#define GA_FIT_SELECT_U8_TARGETS 1
typedef struct GaFitSelectArgs {
    int32_t pool_views, batch_views, height, width, max_steps, flags;   /* P, B, H, W                                      */
    const int32_t *schedule;     /* [max_steps, B]                                                                           */
    const int32_t *counter;      /* the fitter's device word; read, never written                                            */
    const float *pool_view;      /* [P,16]                                                                                   */
    const float *pool_proj;      /* [P,16]                                                                                   */
    const void *pool_targets;    /* [P,3,H,W] fp32, or uint8 with GA_FIT_SELECT_U8_TARGETS                                   */
    const float *pool_mask;      /* [P,1,H,W] or NULL                                                                        */
    const float *pool_normal;    /* [P,3,H,W] or NULL                                                                        */
    float *view, *proj;          /* [B,16] each                                                                              */
    float *targets;              /* [B,3,H,W]                                                                                */
    float *mask;                 /* [B,1,H,W]; NULL exactly where pool_mask is                                               */
    float *normal;               /* [B,3,H,W]; NULL exactly where pool_normal is                                             */
    int32_t *selected;           /* [B] or NULL: the pool indices used by this iteration                                     */
} GaFitSelectArgs;
int ga_fit_select_views(const GaFitSelectArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GA_FIT_H */
