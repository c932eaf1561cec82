/*
 * ga_pointcloud.h -- C-ABI of the MI355X-native point-cloud operations on the generation side: farthest point sampling,
 * nearest point (the building block of the Chamfer distance), the k nearest neighbours and the gradient of their squared distances.
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

#ifdef __cplusplus
}
#endif
#endif
