/*
 * ga_densify.h -- C-ABI of the adaptive density control of the surfel fitter (csrc/surfel_densify.hip): the per-iteration
 * densification statistic, the clone / split / prune round (a stream compaction whose output size is decided on the device) and the
 * opacity reset.
 *
 * Conventions as in ga_fit.h: device pointers unless marked host, caller owns every buffer, work is enqueued on `stream`, 0 or a
 * negative GA_ERR_* code is returned, nothing synchronises, allocates or reads back.  No workgroup of any kernel here waits for
 * another one: the scan behind ga_densify is three launches (per-block sums, one workgroup scanning the sums, per-block rescan and
 * scatter), ordered by the stream alone; their shared pieces are csrc/compact.h.
 *
 * ARITHMETIC CONTRACT.  fp32, every product, quotient, sum and square root rounded on its own, in the order written (the translation
 * unit is built without FMA contraction; division and square root are the correctly rounded ones).  (float) of an int32 is the
 * round-to-nearest conversion.  Comparisons with a NaN are false.
 *
 * THE STATISTIC (ga_fit_accumulate; the project's own definition -- ga_surfel_backward returns no screen-space gradient).  Per surfel
 * n, with (px, py, pz) = means[n], (gx, gy, gz) = g_means[n] and vm = view[v] (16 floats, the layout ga_surfel_forward reads):
 *   visible views   those with radii[v,n] > 0, c their number; c == 0: nothing is written for n
 *   vz_v            ((vm[2] * px + vm[6] * py) + vm[10] * pz) + vm[14]                       (the depth of the rasterizer's preprocess)
 *   zbar            (0 + the vz_v of the visible views, one by one, v ascending) / (float)c
 *   g               sqrt((gx * gx + gy * gy) + gz * gz)
 *   grad_accum[n]   += (g * zbar) * tanfov
 *   denom[n]        += 1
 *   max_radius[n]   = max(max_radius[n], max over v of radii[v,n])
 *
 * CLASSIFICATION (ga_densify), from the ACTIVATED opacities and scales ga_fit_activate wrote and the three statistics:
 *   avg      denom > 0 ? grad_accum / (float)denom : 0;  a NaN avg counts as 0
 *   smax     s0 >= s1 ? s0 : s1
 *   prune    opacity < min_opacity,  or  max_screen_size > 0 and ((float)max_radius > max_screen_size  or  smax > 0.1f * extent)
 *   else     avg >= grad_threshold:  clone when smax <= percent_dense * extent, otherwise split
 *   else     kept
 * (0.1f * extent and percent_dense * extent are fp32 products.)  With GA_DENSIFY_PRUNE_ONLY clone and split count as kept.  A pruned
 * surfel emits no row (it is not split first), kept emits 1, clone and split emit 2.
 *
 * OUTPUT.  Rows in ascending parent order, a parent's two rows adjacent; out_raw / out_m / out_v [N',13], parent [N'] the source row.
 *   kept     raw, m, v copied
 *   clone    row 0: raw, m, v copied;  row 1: raw copied, m = v = 0
 *   split    two children, m = v = 0, raw the parent's except
 *              scale columns 4, 5   raw_s - GA_DENSIFY_LOG_1P6      (log(1.6) rounded once from double: the scale divided by 0.8 * 2)
 *              xyz column k         (p_k + tu_k * (s0 * xa)) + tv_k * (s1 * xb)
 *            with p = raw[0..2], (s0, s1) the activated scales, (xa, xb) = noise (0, 1) for child 0 and (2, 3) for child 1, and tu, tv
 *            the tangent columns of the rasterizer's preprocess from the activated quaternion q = (q0, q1, q2, q3) = (w, x, y, z):
 *              qs = 1 / sqrt(((q3 * q3 + q0 * q0) + q1 * q1) + q2 * q2);   r = q0 * qs, x = q1 * qs, y = q2 * qs, z = q3 * qs
 *              tu = (1 - 2 * (y * y + z * z),  2 * (x * y + r * z),  2 * (x * z - r * y))
 *              tv = (2 * (x * y - r * z),  1 - 2 * (x * x + z * z),  2 * (y * z + r * x))
 * Rows at and past N' are not written.  N' is not clamped: the output buffers hold 2 N rows.
 *
 * NOISE.  One Philox4x32-10 block per split parent: key = the 64-bit seed, counter = (parent index, round, GA_DENSIFY_STREAM, 0); the
 * four words give four normals by the two Box-Muller pairs of ga_dit.h ("noise of ga_sde_step"): (cos, sin) of words (0, 1), then of
 * words (2, 3).  log, sin and cos are the device library's: the normals are not part of the bit-exact contract, noise_out hands them
 * to whoever wants to check the rest.
 */
#ifndef GA_DENSIFY_H
#define GA_DENSIFY_H

#include <stddef.h>
#include <stdint.h>

#include "ga_fit.h" /* GA_FIT_PARAMS; GA_OK, GA_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define GA_DENSIFY_PRUNE_ONLY 1              /* flags: clone and split are treated as kept                              */
#define GA_DENSIFY_THREADS 256               /* lanes per workgroup of every kernel here                                 */
#define GA_DENSIFY_ROWS_PER_LANE 4           /* consecutive surfels per lane of the classify and scatter kernels         */
#define GA_DENSIFY_BLOCK_ROWS (GA_DENSIFY_THREADS * GA_DENSIFY_ROWS_PER_LANE)
#define GA_DENSIFY_STREAM 0x44454E53u        /* the third counter word of this kernel's Philox blocks                    */
#define GA_DENSIFY_LOG_1P6 0x1.e148a2p-2f    /* (float)log(1.6) = 0.4700036346912384                                     */
#define GA_DENSIFY_COUNTS 8                  /* out_counts: N', kept, cloned, split, pruned, N, round, flags            */

typedef struct GaFitAccumulateArgs {
    int32_t num_points, num_views;
    float tanfov;
    int32_t reserved;
    const float *g_means;    /* [N,3] what ga_surfel_backward wrote */
    const float *means;      /* [N,3] what ga_fit_activate wrote    */
    const int32_t *radii;    /* [V,N] of ga_surfel_forward          */
    const float *view;       /* [V,16] cam_view                     */
    float *grad_accum;       /* [N] */
    int32_t *denom;          /* [N] */
    int32_t *max_radius;     /* [N] */
} GaFitAccumulateArgs;
int ga_fit_accumulate(const GaFitAccumulateArgs *args, void *stream);

/* bytes of GaDensifyArgs.workspace for N surfels (four int32 per block of GA_DENSIFY_BLOCK_ROWS surfels); 0 when N < 1 */
size_t ga_densify_workspace_bytes(int32_t num_points);

typedef struct GaDensifyArgs {
    int32_t num_points, flags;
    uint32_t round;            /* the second counter word of the Philox blocks: a launch argument, this call is never captured */
    int32_t reserved;
    float grad_threshold, min_opacity, percent_dense, extent, max_screen_size;   /* max_screen_size <= 0: no size pruning */
    int32_t reserved2;
    uint64_t seed;
    const float *raw, *m, *v;                           /* [N,13] each                                                    */
    const float *opacities, *scales, *rotations;        /* [N] [N,2] [N,4] what ga_fit_activate wrote for `raw`           */
    const float *grad_accum;                            /* [N] */
    const int32_t *denom, *max_radius;                  /* [N] [N] */
    float *out_raw, *out_m, *out_v;                     /* [2N,13] each; rows [0, N') are written                         */
    int32_t *parent;                                    /* [2N]                                                           */
    float *noise_out;                                   /* [N,4] or NULL: the four normals of a split parent, zeros elsewhere */
    int64_t *out_counts;                                /* [GA_DENSIFY_COUNTS]                                            */
    void *workspace;                                    /* ga_densify_workspace_bytes(N), 16-byte aligned                 */
    size_t workspace_bytes;
} GaDensifyArgs;
int ga_densify(const GaDensifyArgs *args, void *stream);

/* raw[:,3] = raw[:,3] > logit_cap ? logit_cap : raw[:,3] (a NaN stays);  m[:,3] = v[:,3] = 0.  logit_cap is the caller's, computed in
 * double and rounded once (2DGS resets to 0.01: logit(0.01)). */
typedef struct GaFitResetOpacityArgs {
    int32_t num_points;
    float logit_cap;
    float *raw, *m, *v;      /* [N,13] each */
} GaFitResetOpacityArgs;
int ga_fit_reset_opacity(const GaFitResetOpacityArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GA_DENSIFY_H */
