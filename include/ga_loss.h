/*
 * ga_loss.h -- C-ABI of the MI355X-native photometric loss: SSIM, L1 and L2 of a predicted image batch against a target batch in
 * one pass, forward and backward (csrc/photo_loss.hip); further down, the geometry losses of a surfel render (csrc/geo_loss.hip).
 *
 * Replaces, for fitting or refining surfels against views and for the reconstruction metrics the reference logs, the torch
 * composition of the reference's `calc_2d_rec_loss` (nsr/losses/builder.py: `gaussian`, `create_window`, `_ssim`, `ssim_loss`, MSE and
 * L1): five grouped 11x11 convolutions plus the element-wise passes, and autograd's mirror of them.
 *
 * Conventions as in ga_pointcloud.h: device pointers unless marked host, caller owns every buffer, work is enqueued on `stream`, 0 or
 * a negative GA_ERR_* code is returned, no exceptions, no host synchronisation.  Every argument the host can see is validated before
 * anything touches the device.
 *
 * ARITHMETIC CONTRACT.  Everything is fp32 (the reductions of the per-pixel values run in fp64 and are rounded once).
 *   window   11 taps, g[k] = (float) exp(-(k - 5)^2 / (2 * 1.5^2)) evaluated in double, w[k] = g[k] / (float)(g[0] + ... + g[10]), the sum
 *            correctly rounded (what torch's fp32 sum of these values gives, so the weights carry the reference's bits);
 *            applied separably (rows, then columns) with ZERO padding: taps outside the image contribute 0 and are not renormalised
 *   moments  mu1 = conv(x), mu2 = conv(y), E11 = conv(x*x), E22 = conv(y*y), E12 = conv(x*y)          x = img1, y = img2
 *            s11 = E11 - mu1^2, s22 = E22 - mu2^2, s12 = E12 - mu1*mu2     (no pivot is subtracted: the cancellation of a flat image
 *            is the reference's own)
 *   SSIM     S = A1*A2 / (B1*B2),  A1 = 2 mu1 mu2 + C1,  A2 = 2 s12 + C2,  B1 = mu1^2 + mu2^2 + C1,  B2 = s11 + s22 + C2
 *            C1 = 0.01^2, C2 = 0.03^2: the reference keeps these range-1 constants for images in [-1, 1] too, and so does this
 *   out      out[n] = { mean S, mean |x - y|, mean (x - y)^2 } over the C*H*W values of image n
 * No floating-point atomics: every sum has a fixed order, two calls on the same input give the same bits.
 */
#ifndef GA_LOSS_H
#define GA_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "ga_surfel.h" /* GA_OK, GA_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define GA_PHOTO_LOSS_SAVE 1 /* forward: also store the three derivative maps ga_photo_loss_backward reads from the workspace */

#define GA_PHOTO_LOSS_WINDOW 11
#define GA_PHOTO_LOSS_OUTPUTS 3 /* per image: SSIM, L1, L2 */
#define GA_PHOTO_LOSS_MAX_SIDE 65536

typedef struct GaPhotoLossArgs {
    int32_t num_images;     /* N >= 1                                                                                   */
    int32_t channels;       /* C >= 1                                                                                   */
    int32_t height;         /* 1 <= H <= GA_PHOTO_LOSS_MAX_SIDE                                                         */
    int32_t width;          /* 1 <= W <= GA_PHOTO_LOSS_MAX_SIDE; the workgroup count of the plan (grid_x) < 2^31        */
    int32_t flags;          /* 0 or GA_PHOTO_LOSS_SAVE; any other bit: GA_ERR_BAD_FLAGS                                 */
    int32_t reserved;       /* 0                                                                                        */
    const float *img1;      /* [N,C,H,W] prediction                                                                     */
    const float *img2;      /* [N,C,H,W] target                                                                         */
    float *out;             /* forward: [N,3] per-image means (SSIM, L1, L2)                                            */
    float *ssim_map;        /* forward: [N,C,H,W] per-pixel S, or NULL                                                  */
    const float *grad_out;  /* backward: [N,3] on the DEVICE, the gradient of the caller's scalar with respect to `out` */
    float *grad_img1;       /* backward: [N,C,H,W]                                                                      */
    void *workspace;        /* ga_photo_loss_workspace_bytes(N, C, H, W, flags) bytes, 16-byte aligned                  */
    size_t workspace_bytes;
} GaPhotoLossArgs;

/* what both launches do: grid_x workgroups of `threads` lanes, each owning one tile_w x tile_h tile of one (n, c) plane (tiles of a
 * plane row by row, planes in memory order) and staging its (tile + 10)^2 halo in `lds_bytes` (forward; the backward needs less) */
typedef struct GaPhotoLossPlan {
    int32_t tile_w;
    int32_t tile_h;
    int32_t threads;
    int32_t tiles_x;        /* ceil(W / tile_w)                                  */
    int32_t tiles_y;        /* ceil(H / tile_h)                                  */
    int32_t lds_bytes;      /* static LDS of the forward kernel                  */
    int64_t grid_x;         /* N * C * tiles_y * tiles_x                         */
    int64_t num_partials;   /* floats in the partials buffer: 3 per workgroup    */
} GaPhotoLossPlan;

/* host only, no HIP call: GA_OK, GA_ERR_NULL_ARG or GA_ERR_BAD_SHAPE */
int ga_photo_loss_plan(int32_t num_images, int32_t channels, int32_t height, int32_t width, GaPhotoLossPlan *plan);
/* host: the partials buffer (rounded up to 256 bytes) plus, with GA_PHOTO_LOSS_SAVE, three fp32 maps of N*C*H*W; 0 for a shape the
 * plan rejects */
size_t ga_photo_loss_workspace_bytes(int32_t num_images, int32_t channels, int32_t height, int32_t width, int32_t flags);

/* Two launches: the tile kernel (per-pixel S, |x-y|, (x-y)^2, three partial sums per workgroup in a fixed order) and one workgroup
 * per image that adds that image's partials in a fixed order and divides by C*H*W.  With GA_PHOTO_LOSS_SAVE the workspace also
 * receives, per pixel p,
 *     dS/dE11 = -A1*A2 / (B1*B2^2)       dS/dE12 = 2*A1 / (B1*B2)
 *     dS/dmu1 = 2 mu2 A2/(B1 B2) - 2 mu1 A1 A2/(B1^2 B2) + 2 mu1 A1 A2/(B1 B2^2) - 2 mu2 A1/(B1 B2)
 * (the last is the total derivative with E11 and E12 held fixed: s11 and s12 depend on mu1). */
int ga_photo_loss_forward(const GaPhotoLossArgs *args, void *stream);

/* One launch, gradient with respect to img1 only.  With s = grad_out[n,0] / (C*H*W), g_l1 = grad_out[n,1] / (C*H*W),
 * g_l2 = grad_out[n,2] / (C*H*W):
 *     grad_img1 = s * (conv(dS/dmu1) + 2 x conv(dS/dE11) + y conv(dS/dE12)) + g_l1 * sign(x - y) + g_l2 * 2 (x - y)
 * with the same zero-padded window (symmetric, so it is its own adjoint) and sign(0) = 0.  `workspace` is the one a forward with
 * GA_PHOTO_LOSS_SAVE on the same images filled; `flags` must carry GA_PHOTO_LOSS_SAVE (else GA_ERR_BAD_FLAGS). */
int ga_photo_loss_backward(const GaPhotoLossArgs *args, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Geometry losses of a 2D-surfel render (csrc/geo_loss.hip): the pseudo surface normal of a depth map, the normal-consistency term,
 * the mean of the distortion map and the L1 of alpha against a mask, in one forward and one backward launch.
 *
 * Restates the reference's `depths_to_points_2` / `depth_to_normal_2` (utils/point_utils.py), the regulariser its renderer comments
 * out (nsr/gs_surfel.py: `surf_normal = depth_to_normal_2(...) * render_alpha.detach()`), the trainer's
 * `normal_error = 1 - (rend_normal * surf_normal).sum(dim=1)`, `rend_dist.mean()` (nsr/train_nv_util.py) and `calc_alpha_loss`
 * (nsr/losses/builder.py: L1 of alpha against the mask).
 *
 * ARITHMETIC CONTRACT, one view, depth d[H,W], ifx = 2 tanfov / W, ify = 2 tanfov / H, u_j = (j - W/2) ifx, v_i = (i - H/2) ify:
 *   point    P(i,j) = d(i,j) (u_j, v_i, 1): pixel centres at integer coordinates, as the reference has them
 *   cross    c = (P(i+1,j) - P(i-1,j)) x (P(i,j+1) - P(i,j-1)): the FIRST factor runs along the rows (the reference calls it dx).  With
 *            dv = d(i+1,j) - d(i-1,j), dh = d(i,j+1) - d(i,j-1), p = (d(i+1,j) + d(i-1,j)) ify, q = (d(i,j+1) + d(i,j-1)) ifx this is
 *                c = ( p dh,  q dv,  -(v_i dv q + u_j dh p + p q) )
 *            which is what the kernel evaluates (fp32): the same value, without the cancellation of the point differences
 *   normal   n_cam = c / max(|c|, 1e-12) (torch's F.normalize), n = R n_cam with R[i][j] = view[4 i + j], i, j < 3; 0 on the one-pixel
 *            border of the map.  The centre depth d(i,j) does not enter.
 *   view     `view` is the renderer's `cam_view`: the TRANSPOSE of the column-vector world-to-camera matrix `depth_to_normal_2` takes,
 *            so its upper-left 3x3 block is the camera-to-world rotation.  THE MATRIX MUST BE RIGID: the reference calls a general
 *            inverse(), this takes the transpose of the rotation block and never looks at the translation (it cancels in both
 *            differences).
 *   terms    out[v] = { mean (1 - sum_c rend_normal_c s_c), mean dist, mean |alpha - mask| (0 without a mask) } over the H*W pixels,
 *            s = n alpha (alpha is a constant of this term: no gradient reaches it), or with GA_GEO_LOSS_TARGET
 *            s = target_normal mask (mask optional; no gradient reaches depth)
 *   |c| < 1e-12 (in practice c == 0: both row neighbours or both column neighbours are holes): the forward value is the reference's
 *            (c / 1e-12); the GRADIENT through that pixel's normal is ZERO, where torch's autograd returns G / 1e-12.
 * No floating-point atomics: every sum has a fixed order (fp64 across lanes, waves and workgroups), the depth gradient is a gather.
 */
#define GA_GEO_LOSS_TARGET 1   /* the normal term is taken against target_normal (* mask) instead of the normals of the depth map */
#define GA_GEO_LOSS_NORMALS 2  /* only the map: forward writes surf_normal_out = n (* alpha when alpha is given), backward turns the
                                  gradient of that map (grad_out is then [V,3,H,W]) into grad_depth; nothing else is read or written */
#define GA_GEO_LOSS_OUTPUTS 3  /* per view: normal, dist, alpha */
#define GA_GEO_LOSS_MAX_SIDE 65536

typedef struct GaGeoLossArgs {
    int32_t num_views;          /* V >= 1                                                                                     */
    int32_t height;             /* 1 <= H <= GA_GEO_LOSS_MAX_SIDE                                                             */
    int32_t width;              /* 1 <= W <= GA_GEO_LOSS_MAX_SIDE; the workgroup count of the plan (grid_x) < 2^31            */
    int32_t flags;              /* 0, GA_GEO_LOSS_TARGET or GA_GEO_LOSS_NORMALS; anything else: GA_ERR_BAD_FLAGS              */
    double tanfov;              /* > 0, finite (host value)                                                                   */
    const float *view;          /* [V,16] row-major 4x4 in cam_view's convention; not needed with GA_GEO_LOSS_TARGET          */
    const float *rend_normal;   /* [V,3,H,W]                                                                                  */
    const float *depth;         /* [V,1,H,W]                                                                                  */
    const float *alpha;         /* [V,1,H,W]; with GA_GEO_LOSS_NORMALS it may be NULL (taken as 1)                            */
    const float *dist;          /* [V,1,H,W]                                                                                  */
    const float *target_normal; /* [V,3,H,W] with GA_GEO_LOSS_TARGET, else ignored                                            */
    const float *mask;          /* [V,1,H,W] or NULL: switches the alpha term on; multiplies target_normal                    */
    float *out;                 /* forward: [V,3] per-view means (normal, dist, alpha)                                        */
    float *surf_normal_out;     /* forward: [V,3,H,W] the s of the normal term, or NULL (required with GA_GEO_LOSS_NORMALS)   */
    const float *grad_out;      /* backward: [V,3] on the DEVICE, the gradient of the caller's scalar with respect to `out`
                                   (with GA_GEO_LOSS_NORMALS: [V,3,H,W], with respect to surf_normal_out)                     */
    float *grad_rend_normal;    /* backward: [V,3,H,W] or NULL                                                                */
    float *grad_depth;          /* backward: [V,1,H,W] or NULL (all zero with GA_GEO_LOSS_TARGET)                             */
    float *grad_dist;           /* backward: [V,1,H,W] or NULL                                                                */
    float *grad_alpha;          /* backward: [V,1,H,W] or NULL (the alpha term only; all zero without a mask)                 */
    void *workspace;            /* forward without GA_GEO_LOSS_NORMALS: ga_geo_loss_workspace_bytes(V, H, W) bytes, 16-byte aligned;
                                   not used by the backward                                                                   */
    size_t workspace_bytes;
} GaGeoLossArgs;

/* what both launches do: grid_x workgroups of `threads` lanes, each owning one tile_w x tile_h tile of one view (tiles row by row,
 * views in memory order) and staging its depth with a halo of 1 (forward) or 2 (backward) in LDS */
typedef struct GaGeoLossPlan {
    int32_t tile_w;
    int32_t tile_h;
    int32_t threads;
    int32_t tiles_x;             /* ceil(W / tile_w)                               */
    int32_t tiles_y;             /* ceil(H / tile_h)                               */
    int32_t lds_bytes;           /* static LDS of the forward kernel               */
    int32_t lds_bytes_backward;  /* static LDS of the backward kernel              */
    int32_t reserved;
    int64_t grid_x;              /* V * tiles_y * tiles_x                          */
    int64_t num_partials;        /* floats in the partials buffer: 3 per workgroup */
} GaGeoLossPlan;

/* host only, no HIP call: GA_OK, GA_ERR_NULL_ARG or GA_ERR_BAD_SHAPE */
int ga_geo_loss_plan(int32_t num_views, int32_t height, int32_t width, GaGeoLossPlan *plan);
/* host: the partials buffer rounded up to 256 bytes; 0 for a shape the plan rejects */
size_t ga_geo_loss_workspace_bytes(int32_t num_views, int32_t height, int32_t width);

/* Two launches (one with GA_GEO_LOSS_NORMALS): the tile kernel (normals from the staged depth, the three per-pixel terms, three
 * partial sums per workgroup in a fixed order, optionally the s map) and one workgroup per view that adds that view's partials in a
 * fixed order and divides by H*W. */
int ga_geo_loss_forward(const GaGeoLossArgs *args, void *stream);

/* One launch; the normals are recomputed from depth.  With g = grad_out[v, 0..2] / (H*W):
 *     grad_rend_normal = -g0 s        grad_dist = g1        grad_alpha = g2 sign(alpha - mask)   (sign(0) = 0; 0 without a mask)
 *     grad_depth(p)    = the sum over the four neighbours q of p of d(-g0 rend_normal(q) . s(q)) / d depth(p): a gather over the halo
 * Every non-NULL gradient output is written at every pixel. */
int ga_geo_loss_backward(const GaGeoLossArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
