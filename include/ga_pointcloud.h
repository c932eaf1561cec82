/*
 * ga_pointcloud.h -- C-ABI of the MI355X-native point-cloud operations on the generation side: farthest point sampling,
 * nearest point (the building block of the Chamfer distance), the k nearest neighbours and the gradient of their squared distances;
 * and, on the neighbour lists, PCA normals and the initial 2D surfels of a fit (ga_pc_normals, ga_pc_surfel_init: the project's own
 * definitions), point clouds from posed depth views (ga_pc_unproject) and their cross-view consistency filter and voxel thinning
 * (ga_pc_filter_views, ga_pc_voxel_thin), all at the end of this file.
 *
 * Replaces, for a cloud the USER hands to stage 2 and for the evaluation hand-off of generated surfels,
 *     pytorch3d.ops.sample_farthest_points      (fps-xyz of the stage-2 entry, /root/reference/nsr/lsgm/flow_matching_trainer.py:1079, :1110-1134;
 *                                                fps-4096.ply of /root/reference/scripts/save_pcd_from_gs.py:148-185)
 *     pytorch3d.loss.chamfer_distance           (/root/reference/nsr/train_nv_util.py:2244; squared L2, no normals: two nearest-point passes;
 *                                                as a loss with gradients at :2244-2267: ga_pc_knn_backward with k = 1)
 *     pytorch3d.ops.knn_points / knn_gather     (nsr/srt/encoder.py:884-923 of the reference; ga_pc_knn, k <= GA_PC_KNN_MAX_K)
 * pytorch3d is a third-party dependency that is absent from this image and does not build for ROCm; its published behaviour is
 * restated in tests/_pointcloud_ref.py, parity UNPINNED ('Point clouds').
 *
 * Conventions as in ga_tsdf.h: device pointers unless marked host, caller owns every buffer, work is enqueued on `stream`, 0 or a
 * negative GA_ERR_* code is returned, no exceptions, no host synchronisation.  Every argument the host can see is validated before
 * anything touches the device.
 *
 * ARITHMETIC CONTRACT (every kernel).  Everything is fp32.  The squared distance of two points is
 *     dx = ax - bx; dy = ay - by; dz = az - bz;   d = dx*dx;  d = d + dy*dy;  d = d + dz*dz;
 * with every operation rounded on its own (the translation unit is built with -ffp-contract=off): the results are a function of the
 * inputs alone, and a numpy float32 restatement reproduces them bit for bit.  Non-finite coordinates are the caller's error and are
 * not checked.  Lengths and start indices live on the device and cannot be validated by the host: the caller keeps
 * 1 <= lengths[b] <= N and 0 <= start_idx[b] < lengths[b]; the kernels clamp them into range so that no access leaves the buffers.
 *
 * PADDING.  ga_pc_fps and ga_pc_nearest mark an unused slot with index -1.  ga_pc_knn marks it with index 0 and distance 0, because
 * pytorch3d.ops.knn_points allocates its outputs as zeros and writes valid slots only (restated from its published behaviour, not
 * pinned).  Neither value can be told from the index alone in the second case: validity always comes from the lengths, and
 * ga_pc_knn_backward never dereferences a padding index of either kind.
 */
#ifndef GA_POINTCLOUD_H
#define GA_POINTCLOUD_H

#include <stddef.h>
#include <stdint.h>

#include "ga_surfel.h" /* GA_OK, GA_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define GA_FPS_VARIANT_REGISTER 0  /* (a) every lane keeps its slice of the cloud (x, y, z, closest) in VGPRs for all K iterations */
#define GA_FPS_VARIANT_STREAMING 1 /* (b) coordinates re-read from memory each iteration, `closest` in the workspace                */

#define GA_PC_MAX_BATCH 65535

/* Farthest point sampling of a padded batch (pytorch3d.ops.sample_farthest_points).  For one cloud of length n:
 *     closest[i] = +inf;  sel = start;
 *     repeat min(K, n) times:  emit sel;  closest[i] = min(closest[i], dist2(p[i], p[sel])) for all i < n;
 *                              sel = the LOWEST index attaining max closest
 * Slots past min(K, n) get index -1 and zero points.  Duplicate points are legal. */
typedef struct GaFpsArgs {
    int32_t batch;            /* B, 1 .. GA_PC_MAX_BATCH                                                        */
    int32_t num_points;       /* N, points per (padded) cloud, N * 3 < 2^31                                     */
    int32_t num_samples;      /* K                                                                              */
    const float *points;      /* [B,N,3]                                                                        */
    const int32_t *lengths;   /* [B] or NULL (= all N)                                                          */
    const int32_t *start_idx; /* [B] or NULL (= 0)                                                              */
    int32_t *out_idx;         /* [B,K]                                                                          */
    float *out_points;        /* [B,K,3] or NULL: the selected points, copied bit for bit                       */
    void *workspace;          /* ga_pc_fps_workspace_bytes(B, N, K) bytes, 16-byte aligned; may be NULL when that is 0 */
    size_t workspace_bytes;
} GaFpsArgs;

/* what ga_pc_fps does for clouds of N points: one workgroup of `threads` lanes per cloud */
typedef struct GaFpsPlan {
    int32_t variant;         /* GA_FPS_VARIANT_*                                                                */
    int32_t threads;         /* workgroup size                                                                  */
    int32_t points_per_lane; /* (a): register slots per lane, threads * points_per_lane >= N; (b): ceil(N / threads) trips */
} GaFpsPlan;

/* host: GA_OK, GA_ERR_NULL_ARG or GA_ERR_BAD_SHAPE (N or K <= 0, N * 3 >= 2^31) */
int ga_pc_fps_plan(int32_t num_points, int32_t num_samples, GaFpsPlan *plan);
/* host: bytes of workspace ga_pc_fps needs (0 for the register-resident variant and for shapes ga_pc_fps rejects) */
size_t ga_pc_fps_workspace_bytes(int32_t batch, int32_t num_points, int32_t num_samples);
int ga_pc_fps(const GaFpsArgs *args, void *stream);

/* Nearest target of every query, brute force: out_dist2[b,q] = min_t dist2(query[b,q], target[b,t]) over t < target_lengths[b],
 * out_idx[b,q] = the LOWEST t attaining it.  Query slots past query_lengths[b] get index -1 and distance 0. */
typedef struct GaNearestArgs {
    int32_t batch;                 /* B, 1 .. GA_PC_MAX_BATCH                  */
    int32_t num_query;             /* Nq, Nq * 3 < 2^31                        */
    int32_t num_target;            /* Nt, Nt * 3 < 2^31                        */
    const float *query;            /* [B,Nq,3]                                 */
    const float *target;           /* [B,Nt,3]                                 */
    const int32_t *query_lengths;  /* [B] or NULL (= all Nq)                   */
    const int32_t *target_lengths; /* [B] or NULL (= all Nt)                   */
    float *out_dist2;              /* [B,Nq]                                   */
    int32_t *out_idx;              /* [B,Nq]                                   */
} GaNearestArgs;

int ga_pc_nearest(const GaNearestArgs *args, void *stream);

#define GA_PC_KNN_MAX_K 32

/* The k nearest targets of every query, brute force (pytorch3d.ops.knn_points, squared L2, sorted).  For query q of cloud b, with
 * m = min(k, target_lengths[b]): slots 0 .. m-1 hold the m smallest pairs (dist2, target index) in ascending lexicographic order --
 * among equal distances the lower index comes first, and at the k-th place the lower index is the one that stays.  Slots k' >= m, and
 * every slot of a query past query_lengths[b], hold distance 0 and index 0 (NOT the -1 of ga_pc_nearest: see PADDING above).  A NaN
 * coordinate is the caller's error. */
typedef struct GaKnnArgs {
    int32_t batch;                 /* B, 1 .. GA_PC_MAX_BATCH                                   */
    int32_t num_query;             /* Nq, Nq * 3 < 2^31 and (int64) Nq * k < 2^31               */
    int32_t num_target;            /* Nt, Nt * 3 < 2^31                                         */
    int32_t k;                     /* 1 .. GA_PC_KNN_MAX_K                                      */
    const float *query;            /* [B,Nq,3]                                                  */
    const float *target;           /* [B,Nt,3]                                                  */
    const int32_t *query_lengths;  /* [B] or NULL (= all Nq), clamped by the kernel             */
    const int32_t *target_lengths; /* [B] or NULL (= all Nt), clamped by the kernel             */
    float *out_dist2;              /* [B,Nq,k]                                                  */
    int32_t *out_idx;              /* [B,Nq,k]                                                  */
} GaKnnArgs;

/* what ga_pc_knn launches for one cloud pair: grid (grid_x, grid_y * B) workgroups of `threads` lanes, one lane per query, the sorted
 * list in `k_slots` register pairs, the targets staged in LDS tiles of `tile` points */
typedef struct GaKnnPlan {
    int32_t k_slots; /* register list length of the kernel instance that serves k: the smallest of 1, 2, 4, 8, 16, 32 that is >= k */
    int32_t threads; /* queries per workgroup                                                                                    */
    int32_t tile;    /* targets staged per LDS tile                                                                              */
    int32_t grid_x;  /* ceil(Nq / threads)                                                                                       */
    int32_t grid_y;  /* workgroups per cloud along y (1): targets are not split over workgroups                                  */
} GaKnnPlan;

/* host only, no HIP call: GA_OK, GA_ERR_NULL_ARG or GA_ERR_BAD_SHAPE (the limits of GaKnnArgs) */
int ga_pc_knn_plan(int32_t num_query, int32_t num_target, int32_t k, GaKnnPlan *plan);
int ga_pc_knn(const GaKnnArgs *args, void *stream);

/* Gradient of the squared distances of ga_pc_knn (any k >= 1) or ga_pc_nearest (k = 1) with respect to both clouds.  A pair (i, k') is
 * VALID when i < query_lengths[b] and k' < min(k, target_lengths[b]); validity never comes from the index value, and the index of an
 * invalid pair (0 or -1) is never dereferenced.  For a valid pair with j = idx[b,i,k']:
 *     c = 2 * grad_dist2[b,i,k'];   u_a = c * (query[b,i,a] - target[b,j,a])          a = x, y, z, every operation rounded on its own
 *     grad_query[b,i,a]  = +0, then + u_a   over k' ascending
 *     grad_target[b,j,a] = +0, then + (-u_a) over all valid pairs with idx == j, in ascending (i, k') order
 * Rows past the lengths, and targets nobody selected, get exactly 0.  The order is part of the contract: no floating-point atomics,
 * the result is a function of the inputs alone.  A valid pair's index must lie in [0, target_lengths[b]). */
typedef struct GaKnnBackwardArgs {
    int32_t batch;                 /* B, 1 .. GA_PC_MAX_BATCH                                   */
    int32_t num_query;             /* Nq, Nq * 3 < 2^31 and (int64) Nq * k < 2^31               */
    int32_t num_target;            /* Nt, Nt * 3 < 2^31                                         */
    int32_t k;                     /* >= 1                                                      */
    const float *query;            /* [B,Nq,3]                                                  */
    const float *target;           /* [B,Nt,3]                                                  */
    const int32_t *query_lengths;  /* [B] or NULL                                               */
    const int32_t *target_lengths; /* [B] or NULL                                               */
    const int32_t *idx;            /* [B,Nq,k] as ga_pc_knn / ga_pc_nearest wrote it            */
    const float *grad_dist2;       /* [B,Nq,k]                                                  */
    float *grad_query;             /* [B,Nq,3] or NULL                                          */
    float *grad_target;            /* [B,Nt,3] or NULL                                          */
} GaKnnBackwardArgs;

int ga_pc_knn_backward(const GaKnnBackwardArgs *args, void *stream);

/* ---- normals and the surfel initialiser (csrc/pc_normals.hip) ------------------------------------------------------------------------
 * The definitions below are the project's own: neither Open3D nor pytorch3d runs here, and the sign rule, the invalid-row rule and
 * the frame are pinned to no other library.  The arithmetic contract above holds: fp32, every operation rounded
 * on its own, only + - * / sqrt and comparisons, so tests/_normals_ref.py reproduces every output bit for bit. */

/* Jacobi sweeps of ga_pc_normals.  A numpy restatement of the scheme on a Fibonacci sphere, a noisy plane and the faces of a cube
 * (2048 points each, K = 8 and 16) converged after 4: off-diagonal over diagonal <= 1e-25 and the normals stopped changing; one more. */
#define GA_PC_NORMALS_SWEEPS 5
#define GA_PC_NORMALS_MIN_K 3
#define GA_PC_SURFEL_MIN_K 4
#define GA_PC_SURFEL_FLOATS 13

/* PCA normals from the neighbour lists ga_pc_knn wrote for the cloud against ITSELF (query = target = points, both lengths = lengths).
 * The point's own entry is part of the list and is used like any other neighbour.  For point i of cloud b, with n = lengths[b] (clamped
 * to 0 .. N), m = min(k, n) and j_k' = idx[b,i,k'] clamped to 0 .. n-1:
 *     centroid     c_a  = (+0 + p[j_0,a] + p[j_1,a] + ...) / m                                  k' ascending, a = x, y, z
 *     covariance   A_ab = (+0 + d_0a * d_0b + d_1a * d_1b + ...) / m,  d_k'a = p[j_k',a] - c_a    k' ascending, the six terms a <= b
 *     trace        (A_xx + A_yy) + A_zz
 *     eigen-decomposition of A by cyclic Jacobi: V = I, then GA_PC_NORMALS_SWEEPS sweeps of the rotations (p,q) = (0,1), (0,2), (1,2),
 *     no data-dependent exit; a rotation is skipped only when A_pq is exactly 0; otherwise, r the third index,
 *         theta = (A_qq - A_pp) / (2 * A_pq);   t = 1 / (|theta| + sqrt(theta * theta + 1));   t = theta >= 0 ? t : -t
 *         c = 1 / sqrt(t * t + 1);   s = t * c;   h = t * A_pq
 *         A_pp = A_pp - h;  A_qq = A_qq + h;  A_pq = 0;   (A_rp, A_rq) = (c * A_rp - s * A_rq,  s * A_rp + c * A_rq)
 *         (V_kp, V_kq) = (c * V_kp - s * V_kq,  s * V_kp + c * V_kq)   for k = 0, 1, 2
 *     the eigenvalues (the diagonal) and their columns of V are sorted ascending by compare-and-swap (0,1), (1,2), (0,1), swapping only
 *     on a strict 'greater': the lower index stays first among equals
 *     normal  = column 0, tangent = column 2, each v / sqrt((vx * vx + vy * vy) + vz * vz), then negated when its component of largest
 *               magnitude (the first among equal magnitudes) is negative
 *     with viewpoint: d = viewpoint[b] - p[i]; the normal is negated when ((dx * nx + dy * ny) + dz * nz) < 0 (a dot product of exactly
 *               0 keeps the default sign)
 * INVALID rows -- i >= n, m < 3, or a trace of exactly 0 (all neighbours coincide) -- get normal (0,0,1), tangent (1,0,0) and
 * eigenvalues 0.  Validity never comes from an index value.  One lane per point, no LDS, no atomics, no workspace. */
typedef struct GaNormalsArgs {
    int32_t batch;            /* B, 1 .. GA_PC_MAX_BATCH                                                   */
    int32_t num_points;       /* N, N * 3 < 2^31 and (int64) N * k < 2^31 (the limits of GaKnnArgs)        */
    int32_t k;                /* GA_PC_NORMALS_MIN_K .. GA_PC_KNN_MAX_K: the row length of idx             */
    int32_t reserved;         /* 0                                                                         */
    const float *points;      /* [B,N,3]                                                                   */
    const int32_t *lengths;   /* [B] or NULL (= all N), clamped by the kernel                              */
    const int32_t *idx;       /* [B,N,k] as ga_pc_knn wrote it                                             */
    const float *viewpoint;   /* [B,3] or NULL                                                             */
    float *normal;            /* [B,N,3]                                                                   */
    float *tangent;           /* [B,N,3] or NULL: the unit eigenvector of the largest eigenvalue           */
    float *eigenvalues;       /* [B,N,3] or NULL: ascending                                                */
} GaNormalsArgs;

/* what ga_pc_normals and ga_pc_surfel_init launch: grid (grid_x, grid_y * B) workgroups of `threads` lanes, one lane per point */
typedef struct GaNormalsPlan {
    int32_t threads; /* points per workgroup   */
    int32_t grid_x;  /* ceil(N / threads)      */
    int32_t grid_y;  /* 1                      */
    int32_t sweeps;  /* GA_PC_NORMALS_SWEEPS   */
} GaNormalsPlan;

/* host only, no HIP call: GA_OK, GA_ERR_NULL_ARG or GA_ERR_BAD_SHAPE (k < 3, k > GA_PC_KNN_MAX_K, the limits of GaKnnArgs) */
int ga_pc_normals_plan(int32_t num_points, int32_t k, GaNormalsPlan *plan);
int ga_pc_normals(const GaNormalsArgs *args, void *stream);

/* Activated surfels [B,N,13] -- xyz, opacity, scale(2), rotation wxyz, rgb, the layout fitting.to_raw takes -- from a cloud, a normal
 * and a tangent per point and the squared distances of the same self-kNN call (k >= 4).  For a valid point:
 *     scale     s = scale_factor * sqrt(max(((d2[1] + d2[2]) + d2[3]) / 3, 1e-7)) in both columns: 2DGS's distCUDA2 rule over the three
 *               nearest OTHER points (slot 0 is the point itself)
 *     frame     n = n / sqrt((nx * nx + ny * ny) + nz * nz);   d = (tx * nx + ty * ny) + tz * nz;   u = t - d * n;
 *               t' = u / sqrt((ux * ux + uy * uy) + uz * uz);   b = n x t' = (ny * t'z - nz * t'y, nz * t'x - nx * t'z, nx * t'y - ny * t'x)
 *               R = the matrix with the columns (t', b, n)
 *     rotation  Shepperd's branches in this order, tr = (R00 + R11) + R22:
 *                 tr > 0:                 S = sqrt(tr + 1) * 2;                  q = (S / 4, (R21 - R12) / S, (R02 - R20) / S, (R10 - R01) / S)
 *                 R00 > R11 && R00 > R22: S = sqrt(((1 + R00) - R11) - R22) * 2; q = ((R21 - R12) / S, S / 4, (R01 + R10) / S, (R02 + R20) / S)
 *                 R11 > R22:              S = sqrt(((1 + R11) - R00) - R22) * 2; q = ((R02 - R20) / S, (R01 + R10) / S, S / 4, (R12 + R21) / S)
 *                 otherwise:              S = sqrt(((1 + R22) - R00) - R11) * 2; q = ((R10 - R01) / S, (R02 + R20) / S, (R12 + R21) / S, S / 4)
 *               (S / 4 is 0.25 * S), then q / sqrt(((w * w + x * x) + y * y) + z * z), then negated when w < 0
 *     opacity, and rgb = colors[b,i] or 0.5
 * INVALID rows -- i >= lengths[b], min(k, lengths[b]) < 4, eigenvalues given and not eigenvalues[b,i,2] > 0 (ga_pc_normals writes exactly
 * 0 on its invalid rows), or a normal or projected tangent of length exactly 0 (or NaN) -- get xyz as given, opacity 0, scale 1e-4, the identity
 * quaternion and rgb 0.5: such a row renders nothing and densification can prune it. */
typedef struct GaSurfelInitArgs {
    int32_t batch;            /* B, 1 .. GA_PC_MAX_BATCH                                                   */
    int32_t num_points;       /* N, the limits of GaNormalsArgs                                            */
    int32_t k;                /* GA_PC_SURFEL_MIN_K .. GA_PC_KNN_MAX_K: the row length of dist2            */
    float opacity;
    float scale_factor;
    int32_t reserved;         /* 0                                                                         */
    const float *points;      /* [B,N,3]                                                                   */
    const float *normal;      /* [B,N,3]: ga_pc_normals's, or the caller's (any positive length)           */
    const float *tangent;     /* [B,N,3]                                                                   */
    const float *dist2;       /* [B,N,k] as ga_pc_knn wrote it for the cloud against itself                */
    const int32_t *lengths;   /* [B] or NULL (= all N), clamped by the kernel                              */
    const float *eigenvalues; /* [B,N,3] or NULL                                                           */
    const float *colors;      /* [B,N,3] or NULL (= 0.5)                                                   */
    float *gaussians;         /* [B,N,13]                                                                  */
} GaSurfelInitArgs;

int ga_pc_surfel_init(const GaSurfelInitArgs *args, void *stream);

/* ---- point clouds from posed depth views (csrc/pc_unproject.hip) -------------------------------------------------------------------------
 * V views of H x W: every valid pixel becomes one world-space point, the points compacted in ascending order of their source pixel
 * (v * H + y) * W + x -- the order of the reference's gt_pos[nonzero_mask] (/root/reference/scripts/save_pcd.py:323-403,
 * save_pcd_from_depth; the rays of nsr/volumetric_rendering/ray_sampler.py:211-271).  The arithmetic contract above holds: fp32, every
 * operation rounded on its own, only + - * / sqrt and comparisons, so tests/_unproject_ref.py reproduces every output bit for bit.
 *
 * CAMERA, 21 floats per view: [0..8] the camera-to-world rotation R, row-major; [9..11] the camera position t; [12..16] fx, fy, cx, cy,
 * sk in the reference's normalised-intrinsics units (of a pose25 `c`: c[16], c[20], c[18], c[21], c[17]); [17..20] reserved, 0.
 *
 * POINT of pixel (x, y) of view v with depth z, F(.) the conversion of an integer to fp32:
 *     u  = F(x) * (1 / F(W)) + 0.5 / F(W);   v' = F(y) * (1 / F(H)) + 0.5 / F(H)                   (the reference's create_uv)
 *     xl = (((u - cx) + (cy * sk) / fy) - (sk * v') / fy) / fx;   yl = (v' - cy) / fy
 *     d_a = (R_a0 * xl + R_a1 * yl) + R_a2                                               a = x, y, z
 *     depth_kind GA_PC_DEPTH_RAY only:  l = max(sqrt((dx * dx + dy * dy) + dz * dz), 1e-12);  d_a = d_a / l
 *     p_a = t_a + z * d_a
 *     clip > 0:  p_a = min(max(p_a, -clip), clip)
 * The reference forms d as (R [xl, yl, 1] + t) - t with a matrix product; the order above is ours and is the specification.
 *
 * VALID is a pixel for which all of these hold (a NaN fails every comparison it meets):
 *     y % pixel_stride == 0 and x % pixel_stride == 0
 *     depth_min < z and z < depth_max
 *     mask given: the pixel is foreground, mask >= mask_threshold, and with erode = e > 0 so is every pixel of the image within
 *         |dx| + |dy| <= e of it: e iterations of the 3 x 3 cross erosion (the reference's kornia call, commented out at
 *         save_pcd.py:346-356), pixels outside the image never eroding anything (kornia's geodesic border).  The erosion runs on the full
 *         image, whatever pixel_stride is.
 *     clip > 0: no |p_a| == clip after the clamp (save_pcd.py:389-390: the boundary is dropped, and with it everything beyond it)
 *     drop_zero: no p_a == 0 (:394)
 *
 * OUTPUTS.  Row r < min(count, capacity) holds the r-th valid pixel in ascending source order: points[r] = p; colors[r] = the three
 * planes of color at the pixel, a uint8 colour converted as F(c) / 255; normals[r] = n / l with l = sqrt((nx * nx + ny * ny) + nz * nz),
 * (0, 0, 1) unless l > 0; source[r] = (v * H + y) * W + x.  Rows min(count, capacity) .. capacity - 1 hold zeros and source -1.
 * count[0] is the number of valid pixels even when it exceeds capacity (the only report of overflow), view_counts[v] that of view v.
 *
 * LAUNCHES: three, ordered by the stream, no workgroup waits for another, no atomics (scans and ranks: csrc/compact.h).  A workgroup owns a band of
 * rows_per_block = clamp(GA_PC_UNPROJECT_TILE_PIXELS / W, 1, H) full rows of one view, so workgroup order is source order.
 *     1 flag     validity of every pixel of the band (the thresholded mask staged in LDS with an erode-wide halo when erode > 0), one
 *                byte per pixel and the band's count to the workspace
 *     2 scan     ONE workgroup walks the band counts GA_PC_UNPROJECT_THREADS at a time, leaves exclusive offsets, count and view_counts
 *     3 scatter  ranks the band's flags, computes the point of a valid pixel AGAIN and writes its row; further workgroups write the padding
 * The point is recomputed in the scatter pass, not stored by the flag pass: on gfx950 the lift to the point is about 150 VALU
 * instructions per 64 valid pixels' wave (four divisions, and with ray depth three more and a square root, are most of them) against 24 bytes of extra
 * memory traffic per pixel for a stored point, in a scatter launch that is bound by memory traffic. */
#define GA_PC_DEPTH_Z 0    /* depth is the camera-space z: what the rasterizer's `depth` map holds          */
#define GA_PC_DEPTH_RAY 1  /* depth is the distance along the normalised ray: what the reference's g-buffers hold */
#define GA_PC_COLOR_F32 0
#define GA_PC_COLOR_U8 1
#define GA_PC_UNPROJECT_THREADS 256
#define GA_PC_UNPROJECT_TILE_PIXELS 1024
#define GA_PC_UNPROJECT_MAX_WIDTH 4096
#define GA_PC_UNPROJECT_MAX_ERODE 4
#define GA_PC_CAMERA_FLOATS 21

typedef struct GaUnprojectArgs {
    int32_t num_views;        /* V >= 1, V * H * W < 2^31                                                  */
    int32_t height;           /* H >= 1                                                                    */
    int32_t width;            /* W, 1 .. GA_PC_UNPROJECT_MAX_WIDTH                                         */
    int32_t depth_kind;       /* GA_PC_DEPTH_*                                                             */
    int32_t color_kind;       /* GA_PC_COLOR_*: the element type of `color`                                */
    int32_t erode;            /* 0 .. GA_PC_UNPROJECT_MAX_ERODE; ignored without a mask                    */
    int32_t drop_zero;        /* 0 or 1                                                                    */
    int32_t pixel_stride;     /* >= 1                                                                      */
    int32_t capacity;         /* rows of the outputs, >= 1                                                 */
    float depth_min;          /* not NaN                                                                   */
    float depth_max;          /* not NaN; +inf = no upper bound (an infinite depth is still invalid)       */
    float mask_threshold;     /* not NaN                                                                   */
    float clip;               /* 0 = off, else positive and finite                                         */
    int32_t reserved;         /* 0                                                                         */
    const float *depth;       /* [V,H,W]                                                                   */
    const float *mask;        /* [V,H,W] or NULL                                                           */
    const void *color;        /* [V,3,H,W] fp32 or uint8, or NULL                                          */
    const float *normal;      /* [V,3,H,W] world space, or NULL                                            */
    const float *cameras;     /* [V,GA_PC_CAMERA_FLOATS]                                                   */
    float *points;            /* [capacity,3]                                                              */
    float *colors;            /* [capacity,3]: given exactly when `color` is                               */
    float *normals;           /* [capacity,3]: given exactly when `normal` is                              */
    int32_t *source;          /* [capacity]                                                                */
    int32_t *count;           /* [1]                                                                       */
    int32_t *view_counts;     /* [V]                                                                       */
    void *workspace;          /* ga_pc_unproject_workspace_bytes(V, H, W) bytes, 16-byte aligned           */
    size_t workspace_bytes;
} GaUnprojectArgs;

/* host: bytes of workspace ga_pc_unproject needs, 0 for a shape it rejects */
size_t ga_pc_unproject_workspace_bytes(int32_t num_views, int32_t height, int32_t width);
/* GA_OK, GA_ERR_NULL_ARG, GA_ERR_BAD_SHAPE (the limits above), GA_ERR_BAD_FLAGS (a kind, erode, drop_zero, pixel_stride, reserved or a
 * scalar out of its range), GA_ERR_WORKSPACE or GA_ERR_LAUNCH */
int ga_pc_unproject(const GaUnprojectArgs *args, void *stream);

/* ---- cross-view consistency filter and voxel thinning of a cloud (csrc/pc_filter.hip) ----------------------------------------------------
 * Two ordered compactions of a cloud of `rows` rows, with the arithmetic contract above (fp32, every operation rounded on its own, only
 * + - * / sqrt floor and comparisons), so tests/_pc_filter_ref.py reproduces every output bit for bit.
 *
 * COMMON.  in_count is a device int32 or NULL (= every row is live): only rows r < min(max(in_count[0], 0), rows) are live, read on the
 * device, so an untrimmed ga_pc_unproject result goes straight in.  points [rows,3] is required; colors, normals [rows,3] and source
 * [rows] are optional, each given exactly when its output is.  Every output has `capacity` rows; the kept rows come in ascending input
 * order, row j < min(count, capacity) a copy of input row kept_rows[j]; rows min(count, capacity) .. capacity - 1 hold zeros, source -1
 * and kept_rows -1.  count[0] is the number of kept rows even beyond capacity (the only report of overflow).  view_counts [num_views]
 * (optional, needs source) counts the kept rows, those beyond capacity included, by source / (H * W); a kept row whose source is
 * negative or names no view is counted nowhere.
 *
 * COMPACTION (both calls; scans and ranks: csrc/compact.h): a workgroup of GA_PC_FILTER_THREADS lanes owns a band of GA_PC_FILTER_BAND_ROWS consecutive rows.
 *     flag     one flag byte per row and the band's count to the workspace (the filter's flag pass is its voting kernel)
 *     scan     ONE workgroup walks the band counts GA_PC_FILTER_THREADS at a time with a register carry, leaves exclusive offsets and
 *              count, and zeroes view_counts
 *     scatter  ranks the flags by ballot and popcount, copies the rows and adds them to view_counts (counted in registers, one integer
 *              atomic per view and workgroup for an ordered cloud); further workgroups write the padding
 * No workgroup waits for another, nothing spins, phases are separate launches ordered by the stream; no host read, so both calls can be
 * captured into a graph.
 *
 * ga_pc_filter_views: every live point p votes in every view u except its own, source[r] / (H * W), when source is given and
 * source[r] >= 0.  Cameras are the 21 floats of ga_pc_unproject; a map pixel is SURFACE when depth_min < z < depth_max and, with a mask,
 * mask >= mask_threshold, otherwise EMPTY (a NaN fails every comparison it meets).
 *     1  e = p - t;  q_x = (R_00 * e_x + R_10 * e_y) + R_20 * e_z, q_y with column 1 of R, q_z with column 2; skipped unless q_z > 0
 *     2  xl = q_x / q_z;  yl = q_y / q_z;  v' = yl * fy + cy;  u' = ((xl * fx + cx) - (cy * sk) / fy) + (sk * v') / fy
 *     3  a = u' * F(W);  b = v' * F(H);  skipped unless 0 <= a < F(W) and 0 <= b < F(H);  x = (int)a, y = (int)b (nearest pixel)
 *     4  d = q_z (GA_PC_DEPTH_Z) or sqrt((q_x * q_x + q_y * q_y) + q_z * q_z) (GA_PC_DEPTH_RAY)
 *     5  the window: pixels (x + dx, y + dy), |dx|, |dy| <= window, inside the image; zmin, zmax over its surface pixels;
 *        lo = zmin - (tol_abs + tol_rel * zmin);  hi = zmax + (tol_abs + tol_rel * zmax)
 *     6  support  += 1 when the centre pixel is surface and lo <= d <= hi
 *        conflict += 1 when every window pixel is surface and d < lo (the point floats in front of what u sees), or when carve is set
 *                      and no window pixel is surface (u sees empty space there)
 *        anything else -- behind the seen surface (occluded), a window that straddles a silhouette (undecided) -- is neither
 * A row is kept when support >= min_support and conflicts <= max_conflicts.  support, conflicts [rows] uint8 (optional, each on its
 * own) hold the votes saturated at 255, 0 on rows that are not live.
 *
 * ga_pc_voxel_thin: one kept row per occupied cell of a grid.
 *     g_a = (p_a - origin_a) / voxel_size;  i_a = floor(g_a);  the row is DROPPED unless every g_a is finite and |i_a| <= 2^20 - 1
 *     key = the three indices biased by 2^20, 21 bits each, x highest
 *     GA_PC_VOXEL_CENTER: c_a = (F(i_a) + 0.5) * voxel_size + origin_a;  dl = p - c;  dist2 = (dl_x * dl_x + dl_y * dl_y) + dl_z * dl_z;
 *                         rank = (bits(dist2) << 32) | r      (the bits of a non-negative float order as the float does)
 *     GA_PC_VOXEL_FIRST:  rank = r
 * The kept row of a cell is the one of smallest rank -- nearest the cell centre or first, ties to the lowest row: a measured point with
 * its own colour and normal, never an average.  multiplicity [capacity] (optional) is the number of live rows in the kept row's cell, 0
 * on padding; dropped [1] (optional) the number of dropped rows.
 * MECHANISM: an open-addressing table in the workspace, table_slots slots (a power of two > rows; 0 = the smallest power of two >=
 * 2 * rows) of a 64-bit key, a 64-bit rank and a 32-bit count.  Launches: clear (keys and ranks to all ones, counts and `dropped` to 0),
 * insert (compare-and-swap on the key with linear probing, then min on the rank and add on the count; the slot of every row is kept in
 * the workspace; with GA_PC_VOXEL_WAVE_MERGE a run of neighbouring lanes of a wave with one key is inserted once, with the run's
 * smallest rank and its length: the same table, fewer atomics), then the compaction whose flag pass keeps row r when its slot's rank
 * names r.  Every probe loop is bounded by
 * table_slots iterations (never reached: table_slots > rows leaves an empty slot; a row that did reach it would be dropped and
 * counted); inside the insert launch the table is touched through agent-scope integer atomics alone.  The hash is the implementation's
 * own: no output depends on it or on the table's layout. */
#define GA_PC_FILTER_THREADS 256
#define GA_PC_FILTER_BAND_ROWS 1024
#define GA_PC_FILTER_MAX_ROWS (1 << 30)
#define GA_PC_VOXEL_FIRST 0
#define GA_PC_VOXEL_CENTER 1
#define GA_PC_VOXEL_MAX_INDEX 1048575  /* 2^20 - 1 */
#define GA_PC_VOXEL_WAVE_MERGE 1       /* insert a run of neighbouring lanes with one key once (same outputs, other speed) */

typedef struct GaFilterViewsArgs {
    int32_t rows;             /* 1 .. GA_PC_FILTER_MAX_ROWS                                                */
    int32_t capacity;         /* rows of the outputs, >= 1                                                 */
    int32_t num_views;        /* V >= 1, V * H * W < 2^31                                                  */
    int32_t height;           /* H >= 1                                                                    */
    int32_t width;            /* W >= 1                                                                    */
    int32_t depth_kind;       /* GA_PC_DEPTH_*                                                             */
    int32_t window;           /* 0 or 1                                                                    */
    int32_t min_support;      /* >= 0                                                                      */
    int32_t max_conflicts;    /* >= 0                                                                      */
    int32_t carve;            /* 0 or 1                                                                    */
    float depth_min;          /* not NaN                                                                   */
    float depth_max;          /* not NaN                                                                   */
    float mask_threshold;     /* not NaN                                                                   */
    float tol_abs;            /* >= 0, finite                                                              */
    float tol_rel;            /* >= 0, finite                                                              */
    int32_t reserved;         /* 0                                                                         */
    const int32_t *in_count;  /* [1] or NULL                                                               */
    const float *points;      /* [rows,3]                                                                  */
    const float *colors;      /* [rows,3] or NULL                                                          */
    const float *normals;     /* [rows,3] or NULL                                                          */
    const int32_t *source;    /* [rows] or NULL                                                            */
    const float *depth;       /* [V,H,W]                                                                   */
    const float *mask;        /* [V,H,W] or NULL                                                           */
    const float *cameras;     /* [V,GA_PC_CAMERA_FLOATS]                                                   */
    float *out_points;        /* [capacity,3]                                                              */
    float *out_colors;        /* [capacity,3]: given exactly when `colors` is                              */
    float *out_normals;       /* [capacity,3]: given exactly when `normals` is                             */
    int32_t *out_source;      /* [capacity]: given exactly when `source` is                                */
    int32_t *kept_rows;       /* [capacity]                                                                */
    int32_t *count;           /* [1]                                                                       */
    int32_t *view_counts;     /* [V] or NULL; needs `source`                                               */
    uint8_t *support;         /* [rows] or NULL                                                            */
    uint8_t *conflicts;       /* [rows] or NULL                                                            */
    void *workspace;          /* ga_pc_filter_views_workspace_bytes(rows) bytes, 16-byte aligned           */
    size_t workspace_bytes;
} GaFilterViewsArgs;

typedef struct GaVoxelThinArgs {
    int32_t rows;             /* 1 .. GA_PC_FILTER_MAX_ROWS                                                */
    int32_t capacity;         /* rows of the outputs, >= 1                                                 */
    int32_t keep;             /* GA_PC_VOXEL_*                                                             */
    int32_t num_views;        /* entries of view_counts; >= 1 when it is given, else ignored               */
    int32_t view_pixels;      /* H * W of the views `source` names; >= 1 when view_counts is given         */
    int32_t flags;            /* 0 or GA_PC_VOXEL_WAVE_MERGE                                               */
    float origin[3];          /* finite                                                                    */
    float voxel_size;         /* positive, finite                                                          */
    int64_t table_slots;      /* 0, or a power of two > rows and <= 2^31                                   */
    const int32_t *in_count;  /* [1] or NULL                                                               */
    const float *points;      /* [rows,3]                                                                  */
    const float *colors;      /* [rows,3] or NULL                                                          */
    const float *normals;     /* [rows,3] or NULL                                                          */
    const int32_t *source;    /* [rows] or NULL                                                            */
    float *out_points;        /* [capacity,3]                                                              */
    float *out_colors;        /* [capacity,3]: given exactly when `colors` is                              */
    float *out_normals;       /* [capacity,3]: given exactly when `normals` is                             */
    int32_t *out_source;      /* [capacity]: given exactly when `source` is                                */
    int32_t *kept_rows;       /* [capacity]                                                                */
    int32_t *count;           /* [1]                                                                       */
    int32_t *view_counts;     /* [num_views] or NULL; needs `source`                                       */
    int32_t *multiplicity;    /* [capacity] or NULL                                                        */
    int32_t *dropped;         /* [1] or NULL                                                               */
    void *workspace;          /* ga_pc_voxel_thin_workspace_bytes(rows, table_slots) bytes, 16-byte aligned */
    size_t workspace_bytes;
} GaVoxelThinArgs;

/* host: bytes of workspace each call needs, 0 for a shape it rejects */
size_t ga_pc_filter_views_workspace_bytes(int32_t rows);
size_t ga_pc_voxel_thin_workspace_bytes(int32_t rows, int64_t table_slots);
/* GA_OK, GA_ERR_NULL_ARG (a required pointer, or an optional input without its output or the reverse, or view_counts without source),
 * GA_ERR_BAD_SHAPE (rows, capacity, the views, table_slots), GA_ERR_BAD_FLAGS (a kind, window, carve, keep, reserved, a vote bound or a
 * scalar out of its range), GA_ERR_WORKSPACE or GA_ERR_LAUNCH -- everything but the last before anything touches the device */
int ga_pc_filter_views(const GaFilterViewsArgs *args, void *stream);
int ga_pc_voxel_thin(const GaVoxelThinArgs *args, void *stream);

/* ---- registration: Horn alignment of corresponding points and ICP (csrc/pc_align.hip) ----------------------------------------------------
 * pytorch3d.ops.corresponding_points_alignment (Kabsch / Umeyama) and pytorch3d.ops.iterative_closest_point, restated from their
 * published behaviour, parity UNPINNED.  tests/_align_ref.py reproduces every output bit for bit.
 *
 * TRANSFORM, pytorch3d's convention: Xt = s * X @ R + T, GA_PC_TRANSFORM_FLOATS = 13 fp32 per cloud: [0] s, [1..9] R row-major,
 * [10..12] T.  The transformed point is fp32 with every operation rounded on its own:
 *     xt_b = ((x_0 * R_0b + x_1 * R_1b) + x_2 * R_2b) * s + T_b                                            b = 0, 1, 2
 *
 * PAIRS.  Row i of X (i < its length) has one partner y: row i of Y (ga_pc_align_points), or the nearest row of Y to xt_i exactly as
 * ga_pc_nearest finds it (ga_pc_icp: the dist2 contract above, the lowest index among equals).  d2 is dist2(x_i, y) of the contract for
 * given pairs and dist2(xt_i, y) for matched ones.  The pair's weight is w = weights[b,i] (1 without weights; weights are >= 0, the
 * caller's duty), 0 when a gate is given and d2 > gate2 (fp32 comparison, gate2 = max_distance * max_distance rounded to fp32), and a
 * row past the length, or one with no target to match, contributes exact zeros.
 *
 * SUMS.  GA_PC_ALIGN_TERMS = 19 terms per pair, formed in fp64 from the fp32 values (the ORIGINAL x, never xt):
 *     [0] w   [1..3] w * x_a   [4..6] w * y_a   [7 + 3a + b] (w * x_a) * y_b   [16] w * ((x_0 * x_0 + x_1 * x_1) + x_2 * x_2)
 *     [17] w * ((y_0 * y_0 + y_1 * y_1) + y_2 * y_2)   [18] w * d2
 * A workgroup of 256 consecutive rows sums each term as the balanced tree over the lane index, v[i] += v[i xor 2^l] for l = 0 .. 7, and
 * the workgroups' sums are added in ascending order starting from the first.  No atomics: the sums are a function of the inputs alone.
 *
 * SOLVE, fp64 with only + - * / sqrt, |.| and comparisons.  W = S[0]; x_a = S[1 + a] / W; y_b = S[4 + b] / W;
 *     M_ab = S[7 + 3a + b] / W - x_a * y_b;   vx = S[16] / W - ((x_0 * x_0 + x_1 * x_1) + x_2 * x_2);   rmse = sqrt(S[18] / W)
 * Rotation by Horn's quaternion method (B. K. P. Horn, JOSA A 4(4), 1987).  The symmetric matrix
 *     A_00 = (M_00 + M_11) + M_22   A_11 = (M_00 - M_11) - M_22   A_22 = (M_11 - M_00) - M_22   A_33 = (M_22 - M_00) - M_11
 *     A_01 = M_12 - M_21   A_02 = M_20 - M_02   A_03 = M_01 - M_10   A_12 = M_01 + M_10   A_13 = M_20 + M_02   A_23 = M_12 + M_21
 * is diagonalised by cyclic Jacobi: V = I, then GA_PC_ALIGN_SWEEPS sweeps of the rotations (p,q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
 * with the formulas of ga_pc_normals above (theta, t, c, s, h; both other rows r ascending; V_kp, V_kq for k = 0 .. 3), a rotation
 * skipped only when A_pq is exactly 0, no data-dependent exit.  The quaternion is the column of V under the largest diagonal entry (the
 * lowest column among equals), q / sqrt(((q_0 * q_0 + q_1 * q_1) + q_2 * q_2) + q_3 * q_3) = (w, x, y, z), and
 *     R_00 = 1 - 2 * (yy + zz)   R_01 = 2 * (xy + wz)       R_02 = 2 * (xz - wy)
 *     R_10 = 2 * (xy - wz)       R_11 = 1 - 2 * (xx + zz)   R_12 = 2 * (yz + wx)
 *     R_20 = 2 * (xz + wy)       R_21 = 2 * (yz - wx)       R_22 = 1 - 2 * (xx + yy)          xx = x * x, xy = x * y, wz = w * z, ...
 * always a proper rotation: pytorch3d's allow_reflection=False.  With estimate_scale s = (+0 + R_00 * M_00 + R_01 * M_01 + ... + R_22 *
 * M_22) / vx (row-major order), otherwise s = 1;  T_b = y_b - s * ((x_0 * R_0b + x_1 * R_1b) + x_2 * R_2b).  s, R, T are rounded to fp32.
 * When !(W > 0) the rmse is 0, and then or when the scale is wanted and !(vx > (S[16] / W) * 2^-40) -- no extent: the rounding of the
 * sums leaves a coincident cloud a vx of about 1e-16 of its mean |x|^2, of either sign, so the test is not against 0 -- the
 * transform stays as it was (the identity for ga_pc_align_points) and the cloud's status becomes GA_PC_ALIGN_DEGENERATE.
 *
 * Jacobi sweeps of the solve.  The restatement (tests/_align_ref.py) on the 152 weighted problems of tests/test_align_cpu.py (3 .. 200
 * points, noise 0 .. 0.3, the planar and collinear ones included): the float64 transform still moves by 4e-3 from 3 sweeps to 4 and by
 * 2.7e-10 from 4 to 5, and not in a single bit from 5 to 6 or beyond (the fp32 outputs already agree from 4 on).  5 is the smallest
 * count whose result no longer changes; one more. */
#define GA_PC_ALIGN_SWEEPS 6
#define GA_PC_ALIGN_TERMS 19
#define GA_PC_TRANSFORM_FLOATS 13
#define GA_PC_ALIGN_HISTORY_FLOATS 14 /* a transform and the rmse of the pass that ran under it */
#define GA_PC_ALIGN_RUNNING 0         /* ga_pc_align_points: solved; ga_pc_icp: max_iterations reached without convergence */
#define GA_PC_ALIGN_CONVERGED 1
#define GA_PC_ALIGN_DEGENERATE 2
#define GA_PC_ICP_MAX_ITERATIONS 10000

typedef struct GaAlignArgs {
    int32_t batch;            /* B, 1 .. GA_PC_MAX_BATCH                                                   */
    int32_t num_points;       /* N, N * 3 < 2^31                                                           */
    int32_t estimate_scale;   /* 0 or 1                                                                    */
    int32_t reserved;         /* 0                                                                         */
    const float *x;           /* [B,N,3]                                                                   */
    const float *y;           /* [B,N,3]: row i is the partner of row i of x                               */
    const float *weights;     /* [B,N] or NULL (= 1)                                                       */
    const int32_t *lengths;   /* [B] or NULL (= all N), clamped by the kernel                              */
    float *transform;         /* [B,GA_PC_TRANSFORM_FLOATS]                                                */
    float *rmse;              /* [B]: of the pairs as given, BEFORE the alignment                          */
    int32_t *status;          /* [B]: GA_PC_ALIGN_RUNNING (solved) or GA_PC_ALIGN_DEGENERATE               */
    void *workspace;          /* ga_pc_align_workspace_bytes(B, N) bytes, 16-byte aligned                  */
    size_t workspace_bytes;
} GaAlignArgs;

/* ICP in one enqueue: pass k = 0 .. max_iterations matches under transform k and sums (one launch), then a solve launch of one small
 * workgroup per cloud.  rmse_k is measured BY match pass k under transform k.  Solve k of a running cloud, in this order: writes rmse and
 * history row k (transform k, rmse_k);  !(W > 0) -> DEGENERATE;  k >= 1 and |rmse_(k-1) - rmse_k| <= thr * rmse_(k-1) (fp64, thr the
 * fp32 value widened) -> CONVERGED, decided BEFORE the update, so the transform stays the one whose matches gave rmse_k;  the final pass
 * k = max_iterations stops here;  scale wanted and no extent (above) -> DEGENERATE;  otherwise transform k+1 is solved from the ORIGINAL x and
 * the matches, and iterations[b] += 1.  A CONVERGED or DEGENERATE cloud is frozen: its match workgroups leave after one read of its
 * status, its solves return, iterations[b] stops.  The final pass matches EVERY cloud once more and writes xt, idx and dist2 (padding as
 * ga_pc_nearest: index -1, distance 0, point 0); for a frozen cloud it repeats history row iterations[b] in the rows behind it, so
 * rmse[b] == history[b, iterations[b], 13] always.  Nothing is read back: the call can be captured into a graph.
 *
 * Two deliberate differences from pytorch3d.ops.iterative_closest_point:
 *   rmse         pytorch3d measures it after the update, on the old matches.  Ours is the match pass's own sum of w * d2 -- no second
 *                pass over the points, no cancellation: Open3D's definition.
 *   convergence  the transform is always estimated from the original X, so stable matches give a bit-identical transform, the next
 *                rmse is bit-identical, and convergence follows for any thr >= 0 (thr = 0 included). */
typedef struct GaIcpArgs {
    int32_t batch;               /* B, 1 .. GA_PC_MAX_BATCH                                                */
    int32_t num_points;          /* N, rows of x, N * 3 < 2^31                                             */
    int32_t num_target;          /* Nt, rows of y, Nt * 3 < 2^31                                           */
    int32_t max_iterations;      /* 0 .. GA_PC_ICP_MAX_ITERATIONS                                          */
    int32_t estimate_scale;      /* 0 or 1                                                                 */
    int32_t reserved;            /* 0                                                                      */
    float relative_rmse_thr;     /* >= 0, finite                                                           */
    float max_distance;          /* the gate: 0 = none, else positive and finite                           */
    const float *x;              /* [B,N,3]                                                                */
    const float *y;              /* [B,Nt,3]                                                               */
    const float *weights;        /* [B,N] or NULL (= 1)                                                    */
    const int32_t *x_lengths;    /* [B] or NULL (= all N), clamped by the kernel                           */
    const int32_t *y_lengths;    /* [B] or NULL (= all Nt), clamped by the kernel                          */
    const float *init_transform; /* [B,GA_PC_TRANSFORM_FLOATS] or NULL (= identity); not `transform`       */
    float *transform;            /* [B,GA_PC_TRANSFORM_FLOATS]                                             */
    float *rmse;                 /* [B]                                                                    */
    int32_t *status;             /* [B]: GA_PC_ALIGN_*                                                     */
    int32_t *iterations;         /* [B]: the number of transform updates                                   */
    float *history;              /* [B, max_iterations + 1, GA_PC_ALIGN_HISTORY_FLOATS] or NULL            */
    float *xt;                   /* [B,N,3]: x under the returned transform                                */
    int32_t *idx;                /* [B,N]: ga_pc_nearest of xt against y                                   */
    float *dist2;                /* [B,N]                                                                  */
    void *workspace;             /* ga_pc_align_workspace_bytes(B, N) bytes, 16-byte aligned               */
    size_t workspace_bytes;
} GaIcpArgs;

/* what both calls launch: the accumulate grid (grid_x, B) of `threads` lanes, one lane per row of x, the targets staged in LDS tiles of
 * `tile` points; the solve grid B workgroups of `solve_threads` lanes */
typedef struct GaAlignPlan {
    int32_t threads;
    int32_t tile;
    int32_t grid_x;        /* ceil(N / threads): the partial rows per cloud   */
    int32_t solve_threads;
    int32_t sweeps;        /* GA_PC_ALIGN_SWEEPS                              */
    int32_t terms;         /* GA_PC_ALIGN_TERMS                               */
} GaAlignPlan;

/* host only, no HIP call: GA_OK, GA_ERR_NULL_ARG or GA_ERR_BAD_SHAPE */
int ga_pc_align_plan(int32_t num_points, int32_t num_target, GaAlignPlan *plan);
/* host: bytes of workspace both calls need (the fp64 partial rows and the previous rmse), 0 for a shape they reject */
size_t ga_pc_align_workspace_bytes(int32_t batch, int32_t num_points);
/* GA_OK, GA_ERR_NULL_ARG, GA_ERR_BAD_SHAPE (batch, N, Nt, max_iterations), GA_ERR_BAD_FLAGS (estimate_scale, reserved, the threshold or
 * the gate out of range), GA_ERR_WORKSPACE or GA_ERR_LAUNCH -- everything but the last before anything touches the device */
int ga_pc_align_points(const GaAlignArgs *args, void *stream);
int ga_pc_icp(const GaIcpArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
