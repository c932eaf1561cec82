/*
 * ga_loss.h -- C-ABI of the MI355X-native photometric loss: SSIM, L1 and L2 of a predicted image batch against a target batch in
 * one pass, forward and backward (csrc/photo_loss.hip).
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

#ifdef __cplusplus
}
#endif
#endif
