/*
 * ga_mesh.h -- C-ABI of the MI355X-native operations that take a triangle MESH in: area-weighted surface sampling
 * (ga_mesh_sample: what pytorch3d.ops.sample_points_from_meshes does for one mesh) and the distance of points to the surface
 * (ga_mesh_point_distance: closest point over all triangles, brute force).  csrc/mesh_ops.hip; the host side is mesh.py.
 *
 * pytorch3d is absent from this image and does not build for ROCm; what is taken from it is the published barycentric formula of its
 * sampler (w0 = 1 - sqrt(u1), w1 = sqrt(u1) (1 - u2), w2 = sqrt(u1) u2).  The random stream, the face search and the distance are the
 * project's own definitions, restated in numpy in tests/_mesh_ops_ref.py; parity with pytorch3d is UNPINNED ('Meshes in').
 *
 * Conventions as in ga_pointcloud.h: device pointers unless marked host, the caller owns every buffer, work is enqueued on `stream`,
 * 0 or a negative GA_ERR_* code is returned, no exceptions, no host synchronisation, no host read.  Every argument the host can see
 * is validated before anything touches the device.  ONE MESH PER CALL: batches of meshes are not built (a caller loops).
 *
 * ARITHMETIC CONTRACT.  The translation unit is built with -ffp-contract=off: every operation below is rounded on its own, in the
 * order written, division and square root are the correctly rounded ones, so the results are a function of the inputs alone.  No
 * kernel uses an atomic of any kind and no workgroup waits for another one.
 *
 * THE WEIGHT OF A FACE (a, b, c) = vertices[faces[f]] (fp32; twice its area), shared by both operations:
 *     e1 = b - a;  e2 = c - a;                                       (per component)
 *     nx = e1y*e2z - e1z*e2y;  ny = e1z*e2x - e1x*e2z;  nz = e1x*e2y - e1y*e2x;
 *     w  = sqrtf((nx*nx + ny*ny) + nz*nz)
 * A face with an index outside [0, V), or whose w is NaN or +inf, has weight 0: it is never sampled and never the nearest face.
 */
#ifndef GA_MESH_H
#define GA_MESH_H

#include <stddef.h>
#include <stdint.h>

#include "ga_surfel.h" /* GA_OK, GA_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define GA_MESH_THREADS 256          /* workgroup size of every kernel here                                                  */
#define GA_MESH_AREA_FACES 256       /* faces per workgroup of the area pass: one per lane                                   */
#define GA_MESH_SCAN_SUMS 256        /* block sums per trip of the scan                                                      */
#define GA_MESH_PHILOX_STREAM 0x4853454du /* counter word 3 of the sampler's Philox blocks ("MESH")                          */
#define GA_MESH_MAX_FACES (1 << 27)  /* F and V limit: 16 F floats of records and 3 V floats stay below 2^31                 */
#define GA_MESH_MAX_ROWS (1 << 29)   /* S and N limit: 3 rows floats stay below 2^31                                          */
#define GA_MESH_DIST_TILE 256        /* triangle records staged in LDS per trip of the distance kernel (16 KB)               */
#define GA_MESH_DIST_TARGET_GROUPS 1024 /* workgroups the distance grid aims at: 4 per CU                                    */
#define GA_MESH_RECORD_FLOATS 16

/* ---- surface sampling ------------------------------------------------------------------------------------------------------------
 * Three launches ordered by the stream, the form of csrc/compact.h (whose integer scans are not used: these sums are float64):
 *   1 area    workgroup g owns faces 256 g .. 256 g + 255, one per lane: w as above, widened to float64.  ONE lane then adds them in
 *             face order,  acc = 0.0;  acc = acc + w[j];  prefix[256 g + j] = acc   (float64, sequential), and the last acc is the
 *             block sum.  Sequential on purpose: a sum of non-negative terms taken in this order never decreases and stays EQUAL
 *             across a face of weight 0, which is what lets the search below promise that such a face is never drawn; a tree-shaped
 *             scan gives neither.
 *   2 scan    one workgroup stages GA_MESH_SCAN_SUMS block sums per trip in LDS and ONE lane carries on in block order:
 *             off[g] = carry;  carry = carry + sum[g]   (float64, sequential);  total = off[G] = the last carry.
 *   3 sample  one lane per sample s:
 *             (x0, x1, x2, x3) = Philox4x32-10(counter = (s, 0, 0, GA_MESH_PHILOX_STREAM), key = (seed low word, seed high word))
 *             u  = (double)(((uint64)(x0 >> 5) << 26) | (x1 >> 6)) * 2^-53           in [0, 1), exact
 *             t  = u * total                                                          (float64)
 *             g  = the first block with off[g + 1] > t;   if there is none: the first block with off[g + 1] >= total
 *             tl = t - off[g]                                                         (float64)
 *             j  = the first face of block g with prefix[j] > tl;  if there is none: the first with prefix[j] >= the block's last prefix
 *             u1 = (float)((x2 >> 8) + 1) * 2^-24  in (0, 1];   u2 = (float)(x3 >> 8) * 2^-24  in [0, 1)     (csrc/philox.h's uniforms)
 *             r  = sqrtf(u1);  w0 = 1 - r;  w1 = r * (1 - u2);  w2 = r * u2
 *             point  = (w0*a + w1*b) + w2*c                                           (per component)
 *             normal = (nx / w, ny / w, nz / w)  with nx, ny, nz, w of the face as above
 *             color  = (w0*ca + w1*cb) + w2*cc                                        (per component, vertex_colors rows of the face)
 *             Both searches are binary searches over non-decreasing arrays, so "the first" is well defined.
 * If total is 0, NaN or +inf every sample gets face -1 and zeros in bary, point, normal and colour.  */
typedef struct GaMeshSampleArgs {
    int32_t num_vertices;        /* V, 1 .. GA_MESH_MAX_FACES                                                           */
    int32_t num_faces;           /* F, 1 .. GA_MESH_MAX_FACES                                                           */
    int32_t num_samples;         /* S, 1 .. GA_MESH_MAX_ROWS                                                            */
    int32_t reserved;            /* 0                                                                                   */
    uint64_t seed;               /* host value; ignored when seed_words is given                                        */
    const uint32_t *seed_words;  /* NULL, or two DEVICE words (low, high) read by the sample pass: a replayed graph draws fresh
                                    samples after the words are overwritten, as ga_sde_step's seed                      */
    const float *vertices;       /* [V,3]                                                                               */
    const int32_t *faces;        /* [F,3]                                                                               */
    const float *vertex_colors;  /* [V,3] or NULL; given exactly when `colors` is                                       */
    float *points;               /* [S,3]                                                                               */
    int32_t *face;               /* [S]                                                                                 */
    float *bary;                 /* [S,3]  (w0, w1, w2)                                                                 */
    float *normals;              /* [S,3] or NULL: the unit flat normal of the face                                     */
    float *colors;               /* [S,3] or NULL                                                                       */
    void *workspace;             /* GaMeshSamplePlan.workspace_bytes bytes, 16-byte aligned                             */
    size_t workspace_bytes;
} GaMeshSampleArgs;

typedef struct GaMeshSamplePlan {
    int32_t threads;             /* workgroup size of the three launches                                                */
    int32_t faces_per_group;     /* faces per workgroup of the area pass                                                */
    int32_t sums_per_trip;       /* block sums per trip of the scan                                                     */
    int32_t num_groups;          /* G = ceil(F / faces_per_group)                                                       */
    size_t workspace_bytes;      /* G + 1 float64 (off, padded to 16 bytes), then F float64 (prefix)                    */
} GaMeshSamplePlan;

/* host only, no HIP call: GA_OK, GA_ERR_NULL_ARG or GA_ERR_BAD_SHAPE (the limits of GaMeshSampleArgs) */
int ga_mesh_sample_plan(int32_t num_faces, int32_t num_samples, GaMeshSamplePlan *plan);
/* GA_OK, GA_ERR_NULL_ARG (a required pointer; vertex_colors without colors or the reverse), GA_ERR_BAD_SHAPE, GA_ERR_BAD_FLAGS
 * (reserved), GA_ERR_WORKSPACE or GA_ERR_LAUNCH */
int ga_mesh_sample(const GaMeshSampleArgs *args, void *stream);

/* ---- point-to-triangle distance --------------------------------------------------------------------------------------------------
 * For every query p the closest point of the surface, brute force over all F triangles; three launches:
 *   1 prep    one lane per triangle writes its 16-float record into the workspace:
 *             a (3), ab = b - a (3), ac = c - a (3), abab = ab.ab, abac = ab.ac, acac = ac.ac, valid (1.0 or 0.0), 0, 0, 0
 *             with  x.y = (x0*y0 + x1*y1) + x2*y2.  valid = 0 for a face of weight 0 (above): out of range, degenerate or not finite.
 *   2 main    grid (ceil(N / 256), chunks): lane = query, the chunk's triangles go through LDS GA_MESH_DIST_TILE records at a time
 *             (as ga_pc_nearest stages points); every lane of a wave reads the same record (a broadcast).  For a valid triangle, the
 *             region test of Ericson, Real-Time Collision Detection, 5.1.5, with the dot products at b and c derived from those at a:
 *                 ap = p - a;  d1 = ab.ap;  d2 = ac.ap;  d3 = d1 - abab;  d4 = d2 - abac;  d5 = d1 - abac;  d6 = d2 - acac;
 *                 vc = d1*d4 - d3*d2;  vb = d5*d2 - d1*d6;  va = d3*d6 - d5*d4;  e = d4 - d3;  g = d5 - d6;
 *                 first of:  A   d1 <= 0 and d2 <= 0                    v = 0,          w = 0
 *                            B   d3 >= 0 and d4 <= d3                   v = 1,          w = 0
 *                            AB  vc <= 0 and d1 >= 0 and d3 <= 0        v = d1/(d1-d3), w = 0
 *                            C   d6 >= 0 and d5 <= d6                   v = 0,          w = 1
 *                            AC  vb <= 0 and d2 >= 0 and d6 <= 0        v = 0,          w = d2/(d2-d6)
 *                            BC  va <= 0 and e >= 0 and g >= 0          w = e/(e+g),    v = 1 - w
 *                            IN  otherwise                              r = 1/((va+vb)+vc);  v = vb*r;  w = vc*r
 *                 closest = (a + ab*v) + ac*w;   d = p - closest;   dist2 = (dx*dx + dy*dy) + dz*dz
 *             (one division per pair: the numerator and the denominator are selected by region first).  The lane keeps the smallest
 *             dist2 with the LOWEST face index among equals (strict <, faces in ascending order; a NaN never wins) and writes the
 *             pair as one 64-bit word (float bits of dist2) << 32 | face to partial[chunk][q]; dist2 >= 0, so the words order as the
 *             pairs do.
 *   3 merge   one lane per row: the smallest word over the chunks -- the result does not depend on the chunking, ties go to the
 *             lowest face -- then closest and bary = ((1 - v) - w, v, w) of the winning face are computed again by the same code
 *             (the same operations on the same inputs give the same bits).
 * Rows past `count` get dist2 0, face -1 and zeros (the padding of ga_pc_nearest).  A live row with no valid triangle, or a query with
 * a NaN coordinate, gets dist2 +inf, face -1 and zeros.  Cost: N * F pair evaluations of about 90 fp32 operations; there is no
 * acceleration structure. */
typedef struct GaMeshPointDistanceArgs {
    int32_t num_points;          /* N rows, 1 .. GA_MESH_MAX_ROWS                                                       */
    int32_t num_vertices;        /* V, 1 .. GA_MESH_MAX_FACES                                                           */
    int32_t num_faces;           /* F, 1 .. GA_MESH_MAX_FACES                                                           */
    int32_t reserved;            /* 0                                                                                   */
    const float *points;         /* [N,3]                                                                               */
    const int32_t *count;        /* NULL (= N) or one DEVICE word: the live rows, clamped to [0, N] by the kernels      */
    const float *vertices;       /* [V,3]                                                                               */
    const int32_t *faces;        /* [F,3]                                                                               */
    float *dist2;                /* [N]                                                                                 */
    int32_t *face;               /* [N]                                                                                 */
    float *closest;              /* [N,3]                                                                               */
    float *bary;                 /* [N,3]                                                                               */
    void *workspace;             /* GaMeshPointDistancePlan.workspace_bytes bytes, 16-byte aligned                      */
    size_t workspace_bytes;
} GaMeshPointDistanceArgs;

typedef struct GaMeshPointDistancePlan {
    int32_t threads;             /* workgroup size; queries per workgroup of the main launch                            */
    int32_t tile;                /* triangles staged per trip                                                           */
    int32_t tiles_per_chunk;     /* a chunk is tiles_per_chunk * tile consecutive triangles                             */
    int32_t num_chunks;          /* grid.y of the main launch, <= 65535                                                 */
    size_t workspace_bytes;      /* F records of 64 bytes, then num_chunks * N 64-bit partial words                     */
} GaMeshPointDistancePlan;

/* host only, no HIP call: GA_OK, GA_ERR_NULL_ARG or GA_ERR_BAD_SHAPE */
int ga_mesh_point_distance_plan(int32_t num_points, int32_t num_faces, GaMeshPointDistancePlan *plan);
/* GA_OK, GA_ERR_NULL_ARG, GA_ERR_BAD_SHAPE, GA_ERR_BAD_FLAGS (reserved), GA_ERR_WORKSPACE or GA_ERR_LAUNCH */
int ga_mesh_point_distance(const GaMeshPointDistanceArgs *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GA_MESH_H */
