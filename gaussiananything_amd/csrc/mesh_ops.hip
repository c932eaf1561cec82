// mesh_ops.hip -- meshes in, for gfx950 (include/ga_mesh.h): area-weighted surface sampling and the point-to-triangle distance.
//
// Built with -ffp-contract=off: every operation is rounded on its own, division and square root are hipcc's correctly rounded defaults,
// so the kernels are a function of their inputs alone and tests/_mesh_ops_ref.py restates them in numpy bit for bit.  No atomics, no
// workgroup waits for another one, nothing is read back by the host: every launch is capturable.
//
//   sampling   area (weight per face, sequential float64 prefix inside the workgroup) -> scan (one workgroup, sequential float64 carry
//              over the block sums) -> sample (one lane per sample: one Philox block, a two-level binary search, the barycentric point).
//              The two sums are taken by ONE lane each, in index order, on purpose -- see the header: only a sequential sum of
//              non-negative terms is monotone and flat across a zero, which the search relies on.  The price is 256 dependent float64
//              adds out of LDS per workgroup and one per block sum in the scan; the whole call is timed in profiles/mesh_ops_bench.txt.
//   distance   prep (a 16-float record per triangle) -> main (lane = query, triangles through LDS in tiles, grid.y over triangle
//              chunks) -> merge (the smallest 64-bit (dist2 bits, face) word over the chunks, then closest and bary of the winner).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ga_mesh.h"
#include "philox.h"

namespace {

constexpr int kThreads = GA_MESH_THREADS;
constexpr int kAreaFaces = GA_MESH_AREA_FACES;
constexpr int kScanSums = GA_MESH_SCAN_SUMS;
constexpr int kTile = GA_MESH_DIST_TILE;
constexpr int kRec = GA_MESH_RECORD_FLOATS;
static_assert(kAreaFaces == kThreads && kScanSums == kThreads && kTile == kThreads, "one face, block sum or record per lane");

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

struct Tri {
    float ax, ay, az, abx, aby, abz, acx, acy, acz;   // a, b - a, c - a
    float nx, ny, nz, w;                              // (b - a) x (c - a) and its length; w = 0: the face does not count
};

// the face's corners, cross product and weight (the header's "weight of a face"); an out-of-range face reads vertex 0 and gets weight 0
__device__ __forceinline__ void load_tri(const float *__restrict__ vertices, const int32_t *__restrict__ faces, int V, int64_t f, Tri &t,
                                         int &ia, int &ib, int &ic) {
    ia = faces[3 * f]; ib = faces[3 * f + 1]; ic = faces[3 * f + 2];
    const bool in = ia >= 0 && ia < V && ib >= 0 && ib < V && ic >= 0 && ic < V;
    if (!in) { ia = 0; ib = 0; ic = 0; }
    const float *a = vertices + 3 * (int64_t)ia, *b = vertices + 3 * (int64_t)ib, *c = vertices + 3 * (int64_t)ic;
    t.ax = a[0]; t.ay = a[1]; t.az = a[2];
    t.abx = b[0] - t.ax; t.aby = b[1] - t.ay; t.abz = b[2] - t.az;
    t.acx = c[0] - t.ax; t.acy = c[1] - t.ay; t.acz = c[2] - t.az;
    t.nx = t.aby * t.acz - t.abz * t.acy;
    t.ny = t.abz * t.acx - t.abx * t.acz;
    t.nz = t.abx * t.acy - t.aby * t.acx;
    const float w = sqrtf((t.nx * t.nx + t.ny * t.ny) + t.nz * t.nz);
    t.w = (in && w < __builtin_inff()) ? w : 0.f;   // NaN and +inf fail the compare
}

// ---- sampling ---------------------------------------------------------------------------------------------------------------------

__host__ __device__ inline int groups_of(int F) { return (F + kAreaFaces - 1) / kAreaFaces; }
// the workspace: G + 1 float64 (block sums, then offsets and the total), padded to 16 bytes, then F float64 prefixes
__host__ __device__ inline size_t prefix_offset(int G) { return (((size_t)G + 1 + 1) / 2) * 16; }

__global__ __launch_bounds__(kThreads) void mesh_area_kernel(GaMeshSampleArgs a) {
    __shared__ double w[kAreaFaces];
    const int64_t f = (int64_t)blockIdx.x * kAreaFaces + threadIdx.x;
    float mine = 0.f;
    if (f < a.num_faces) {
        Tri t;
        int ia, ib, ic;
        load_tri(a.vertices, a.faces, a.num_vertices, f, t, ia, ib, ic);
        mine = t.w;
    }
    w[threadIdx.x] = (double)mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int j = 0; j < kAreaFaces; ++j) {   // in face order, by one lane: see the header
            acc = acc + w[j];
            w[j] = acc;
        }
        reinterpret_cast<double *>(a.workspace)[blockIdx.x] = acc;   // faces past F added 0.0: the last real prefix
    }
    __syncthreads();
    if (f < a.num_faces)
        reinterpret_cast<double *>(reinterpret_cast<char *>(a.workspace) + prefix_offset(groups_of(a.num_faces)))[f] = w[threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void mesh_scan_kernel(GaMeshSampleArgs a) {
    __shared__ double lds[kScanSums];
    __shared__ double carry_s;
    double *sums = reinterpret_cast<double *>(a.workspace);
    const int G = groups_of(a.num_faces);
    if (threadIdx.x == 0) carry_s = 0.0;
    for (int start = 0; start < G; start += kScanSums) {   // (every lane takes every trip: the barriers are uniform)
        const int g = start + (int)threadIdx.x;
        lds[threadIdx.x] = g < G ? sums[g] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            double carry = carry_s;
            for (int j = 0; j < kScanSums; ++j) {   // in block order, by one lane
                const double s = lds[j];
                lds[j] = carry;
                carry = carry + s;
            }
            carry_s = carry;
        }
        __syncthreads();
        if (g < G) sums[g] = lds[threadIdx.x];   // the block's exclusive offset, in place of its sum
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[G] = carry_s;
}

// first index in [0, n) with arr[i] > x (strict) or arr[i] >= x; n when there is none.  arr is non-decreasing.
template <bool kStrict>
__device__ __forceinline__ int first_above(const double *__restrict__ arr, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double v = arr[mid];
        if (kStrict ? v > x : v >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void mesh_sample_kernel(GaMeshSampleArgs a) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= a.num_samples) return;
    const int F = a.num_faces, G = groups_of(F);
    const double *off = reinterpret_cast<const double *>(a.workspace);
    const double *prefix = reinterpret_cast<const double *>(reinterpret_cast<const char *>(a.workspace) + prefix_offset(G));
    const double total = off[G];
    float w0 = 0.f, w1 = 0.f, w2 = 0.f, px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, cr = 0.f, cg = 0.f, cb = 0.f;
    int face = -1;
    if (total > 0.0 && total < (double)__builtin_inff()) {
        const uint32_t k0 = a.seed_words ? a.seed_words[0] : (uint32_t)a.seed;
        const uint32_t k1 = a.seed_words ? a.seed_words[1] : (uint32_t)(a.seed >> 32);
        uint32_t x[4];
        gaphilox::philox4x32_10((uint32_t)s, 0u, 0u, GA_MESH_PHILOX_STREAM, k0, k1, x);
        const double u = (double)(((uint64_t)(x[0] >> 5) << 26) | (uint64_t)(x[1] >> 6)) * 1.1102230246251565e-16;   // 2^-53
        const double t = u * total;
        int g = first_above<true>(off + 1, G, t);
        if (g == G) g = first_above<false>(off + 1, G, total);
        const double tl = t - off[g];
        const int cnt = F - g * kAreaFaces < kAreaFaces ? F - g * kAreaFaces : kAreaFaces;
        const double *pg = prefix + (int64_t)g * kAreaFaces;
        int j = first_above<true>(pg, cnt, tl);
        if (j == cnt) j = first_above<false>(pg, cnt, pg[cnt - 1]);
        face = g * kAreaFaces + j;
        const float u1 = (float)((x[2] >> 8) + 1u) * 5.9604644775390625e-08f;   // (0, 1]
        const float u2 = (float)(x[3] >> 8) * 5.9604644775390625e-08f;          // [0, 1)
        const float r = sqrtf(u1);
        w0 = 1.f - r;
        w1 = r * (1.f - u2);
        w2 = r * u2;
        Tri t3;
        int ia, ib, ic;
        load_tri(a.vertices, a.faces, a.num_vertices, face, t3, ia, ib, ic);   // a drawn face has weight > 0: its indices are in range
        const float *va = a.vertices + 3 * (int64_t)ia, *vb = a.vertices + 3 * (int64_t)ib, *vc = a.vertices + 3 * (int64_t)ic;
        px = (w0 * va[0] + w1 * vb[0]) + w2 * vc[0];
        py = (w0 * va[1] + w1 * vb[1]) + w2 * vc[1];
        pz = (w0 * va[2] + w1 * vb[2]) + w2 * vc[2];
        nx = t3.nx / t3.w; ny = t3.ny / t3.w; nz = t3.nz / t3.w;
        if (a.colors) {
            const float *ca = a.vertex_colors + 3 * (int64_t)ia, *cbp = a.vertex_colors + 3 * (int64_t)ib, *cc = a.vertex_colors + 3 * (int64_t)ic;
            cr = (w0 * ca[0] + w1 * cbp[0]) + w2 * cc[0];
            cg = (w0 * ca[1] + w1 * cbp[1]) + w2 * cc[1];
            cb = (w0 * ca[2] + w1 * cbp[2]) + w2 * cc[2];
        }
    }
    a.face[s] = face;
    a.bary[3 * s] = w0; a.bary[3 * s + 1] = w1; a.bary[3 * s + 2] = w2;
    a.points[3 * s] = px; a.points[3 * s + 1] = py; a.points[3 * s + 2] = pz;
    if (a.normals) { a.normals[3 * s] = nx; a.normals[3 * s + 1] = ny; a.normals[3 * s + 2] = nz; }
    if (a.colors) { a.colors[3 * s] = cr; a.colors[3 * s + 1] = cg; a.colors[3 * s + 2] = cb; }
}

bool sample_shape_ok(int64_t F, int64_t S) { return F >= 1 && F <= GA_MESH_MAX_FACES && S >= 1 && S <= GA_MESH_MAX_ROWS; }

// ---- distance ---------------------------------------------------------------------------------------------------------------------

struct DistShape {
    int tiles, tiles_per_chunk, chunks;
};

__host__ __device__ inline DistShape dist_shape(int N, int F) {
    DistShape s;
    s.tiles = (F + kTile - 1) / kTile;
    const int qblocks = (N + kThreads - 1) / kThreads;
    int want = (GA_MESH_DIST_TARGET_GROUPS + qblocks - 1) / qblocks;   // chunks that bring the grid to the target, 1 .. 1024
    want = want < s.tiles ? want : s.tiles;
    s.tiles_per_chunk = (s.tiles + want - 1) / want;
    s.chunks = (s.tiles + s.tiles_per_chunk - 1) / s.tiles_per_chunk;
    return s;
}

__host__ __device__ inline size_t partial_offset(int F) { return (size_t)F * kRec * sizeof(float); }

__global__ __launch_bounds__(kThreads) void mesh_prep_kernel(GaMeshPointDistanceArgs a) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= a.num_faces) return;
    Tri t;
    int ia, ib, ic;
    load_tri(a.vertices, a.faces, a.num_vertices, f, t, ia, ib, ic);
    float4 *rec = reinterpret_cast<float4 *>(a.workspace) + 4 * f;
    rec[0] = make_float4(t.ax, t.ay, t.az, t.abx);
    rec[1] = make_float4(t.aby, t.abz, t.acx, t.acy);
    rec[2] = make_float4(t.acz, dot3(t.abx, t.aby, t.abz, t.abx, t.aby, t.abz), dot3(t.abx, t.aby, t.abz, t.acx, t.acy, t.acz),
                         dot3(t.acx, t.acy, t.acz, t.acx, t.acy, t.acz));
    rec[3] = make_float4(t.w > 0.f ? 1.f : 0.f, 0.f, 0.f, 0.f);
}

// closest point of the triangle of record (r0, r1, r2) to p: the header's region test.  Returns dist2; the main loop uses nothing else
// (the rest is dead code there), the merge takes v, w and the point of the winner.
__device__ __forceinline__ float closest_on(const float4 r0, const float4 r1, const float4 r2, float px, float py, float pz, float &v,
                                            float &w, float &cx, float &cy, float &cz) {
    const float ax = r0.x, ay = r0.y, az = r0.z, abx = r0.w, aby = r1.x, abz = r1.y, acx = r1.z, acy = r1.w, acz = r2.x;
    const float abab = r2.y, abac = r2.z, acac = r2.w;
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    const float d3 = d1 - abab, d4 = d2 - abac, d5 = d1 - abac, d6 = d2 - acac;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e = d4 - d3, g = d5 - d6;
    const bool rA = d1 <= 0.f && d2 <= 0.f;
    const bool rB = !rA && d3 >= 0.f && d4 <= d3;
    const bool rAB = !rA && !rB && vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
    const bool pre_c = rA || rB || rAB;
    const bool rC = !pre_c && d6 >= 0.f && d5 <= d6;
    const bool rAC = !pre_c && !rC && vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
    const bool pre_bc = pre_c || rC || rAC;
    const bool rBC = !pre_bc && va <= 0.f && e >= 0.f && g >= 0.f;
    const bool rIN = !pre_bc && !rBC;
    // one division: numerator and denominator by region (a vertex region divides 0 by 1)
    const float num = rAB ? d1 : rAC ? d2 : rBC ? e : rIN ? 1.f : 0.f;
    const float den = rAB ? d1 - d3 : rAC ? d2 - d6 : rBC ? e + g : rIN ? (va + vb) + vc : 1.f;
    const float q = num / den;
    v = rB ? 1.f : rAB ? q : rBC ? 1.f - q : rIN ? vb * q : 0.f;
    w = rC ? 1.f : (rAC || rBC) ? q : rIN ? vc * q : 0.f;
    cx = (ax + abx * v) + acx * w;
    cy = (ay + aby * v) + acy * w;
    cz = (az + abz * v) + acz * w;
    const float dx = px - cx, dy = py - cy, dz = pz - cz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ int live_rows(const GaMeshPointDistanceArgs &a) {
    int n = a.count ? a.count[0] : a.num_points;
    n = n < 0 ? 0 : n;
    return n > a.num_points ? a.num_points : n;
}

__global__ __launch_bounds__(kThreads) void mesh_distance_kernel(GaMeshPointDistanceArgs a, DistShape s) {
    __shared__ float4 rec[kTile * 4];   // 16 KB
    const int tid = threadIdx.x, N = a.num_points, F = a.num_faces;
    const int n = live_rows(a);
    if ((int64_t)blockIdx.x * kThreads >= n) return;   // the whole block is padding (block-uniform); the merge never reads its words
    const int64_t q = (int64_t)blockIdx.x * kThreads + tid;
    const bool live = q < n;
    const float px = live ? a.points[3 * q] : 0.f, py = live ? a.points[3 * q + 1] : 0.f, pz = live ? a.points[3 * q + 2] : 0.f;
    const float4 *records = reinterpret_cast<const float4 *>(a.workspace);
    const int tile0 = blockIdx.y * s.tiles_per_chunk;
    const int tile1 = tile0 + s.tiles_per_chunk < s.tiles ? tile0 + s.tiles_per_chunk : s.tiles;
    float best = __builtin_inff();
    int besti = -1;
    for (int tile = tile0; tile < tile1; ++tile) {
        const int f0 = tile * kTile;
        const int cnt = F - f0 < kTile ? F - f0 : kTile;
        __syncthreads();   // the previous tile has been read by every wave
        if (tid < cnt) {
            const float4 *src = records + 4 * (int64_t)(f0 + tid);
            rec[4 * tid] = src[0]; rec[4 * tid + 1] = src[1]; rec[4 * tid + 2] = src[2]; rec[4 * tid + 3] = src[3];
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) {
            if (rec[4 * j + 3].x == 0.f) continue;   // wave-uniform: every lane reads the same record
            float v, w, cx, cy, cz;
            const float d = closest_on(rec[4 * j], rec[4 * j + 1], rec[4 * j + 2], px, py, pz, v, w, cx, cy, cz);
            if (d < best) { best = d; besti = f0 + j; }
        }
    }
    if (q < N) {
        unsigned long long *partial = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(a.workspace) + partial_offset(F));
        partial[(size_t)blockIdx.y * N + q] = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned int)besti;
    }
}

__global__ __launch_bounds__(kThreads) void mesh_merge_kernel(GaMeshPointDistanceArgs a, DistShape s) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int N = a.num_points;
    if (q >= N) return;
    const bool live = q < live_rows(a);
    float d = 0.f, v = 0.f, w = 0.f, cx = 0.f, cy = 0.f, cz = 0.f, b0 = 0.f;
    int face = -1;
    if (live) {
        const unsigned long long *partial =
            reinterpret_cast<const unsigned long long *>(reinterpret_cast<const char *>(a.workspace) + partial_offset(a.num_faces));
        unsigned long long m = partial[q];
        for (int c = 1; c < s.chunks; ++c) {
            const unsigned long long x = partial[(size_t)c * N + q];
            m = x < m ? x : m;
        }
        d = __uint_as_float((unsigned int)(m >> 32));
        face = (int)(unsigned int)m;   // 0xffffffff -> -1: no valid triangle, or a NaN query
        if (face >= 0) {
            const float4 *r = reinterpret_cast<const float4 *>(a.workspace) + 4 * (int64_t)face;
            closest_on(r[0], r[1], r[2], a.points[3 * q], a.points[3 * q + 1], a.points[3 * q + 2], v, w, cx, cy, cz);
            b0 = (1.f - v) - w;
        }
    }
    a.dist2[q] = d;
    a.face[q] = face;
    a.closest[3 * q] = cx; a.closest[3 * q + 1] = cy; a.closest[3 * q + 2] = cz;
    a.bary[3 * q] = b0; a.bary[3 * q + 1] = v; a.bary[3 * q + 2] = w;
}

bool dist_shape_ok(int64_t N, int64_t F) { return N >= 1 && N <= GA_MESH_MAX_ROWS && F >= 1 && F <= GA_MESH_MAX_FACES; }

}  // namespace

extern "C" int ga_mesh_sample_plan(int32_t num_faces, int32_t num_samples, GaMeshSamplePlan *plan) {
    if (!plan) return GA_ERR_NULL_ARG;
    if (!sample_shape_ok(num_faces, num_samples)) return GA_ERR_BAD_SHAPE;
    const int G = groups_of(num_faces);
    plan->threads = kThreads;
    plan->faces_per_group = kAreaFaces;
    plan->sums_per_trip = kScanSums;
    plan->num_groups = G;
    plan->workspace_bytes = prefix_offset(G) + (((size_t)num_faces + 1) / 2) * 16;
    return GA_OK;
}

extern "C" int ga_mesh_sample(const GaMeshSampleArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaMeshSampleArgs &a = *args;
    if (!sample_shape_ok(a.num_faces, a.num_samples) || a.num_vertices < 1 || a.num_vertices > GA_MESH_MAX_FACES) return GA_ERR_BAD_SHAPE;
    if (a.reserved != 0) return GA_ERR_BAD_FLAGS;
    if (!a.vertices || !a.faces || !a.points || !a.face || !a.bary || !a.workspace) return GA_ERR_NULL_ARG;
    if ((a.vertex_colors != nullptr) != (a.colors != nullptr)) return GA_ERR_NULL_ARG;
    GaMeshSamplePlan plan;
    ga_mesh_sample_plan(a.num_faces, a.num_samples, &plan);
    if (a.workspace_bytes < plan.workspace_bytes || (reinterpret_cast<uintptr_t>(a.workspace) & 15)) return GA_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    hipLaunchKernelGGL(mesh_area_kernel, dim3(plan.num_groups), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)(((int64_t)a.num_samples + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_mesh_point_distance_plan(int32_t num_points, int32_t num_faces, GaMeshPointDistancePlan *plan) {
    if (!plan) return GA_ERR_NULL_ARG;
    if (!dist_shape_ok(num_points, num_faces)) return GA_ERR_BAD_SHAPE;
    const DistShape s = dist_shape(num_points, num_faces);
    plan->threads = kThreads;
    plan->tile = kTile;
    plan->tiles_per_chunk = s.tiles_per_chunk;
    plan->num_chunks = s.chunks;
    plan->workspace_bytes = partial_offset(num_faces) + (size_t)s.chunks * (size_t)num_points * 8;
    return GA_OK;
}

extern "C" int ga_mesh_point_distance(const GaMeshPointDistanceArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaMeshPointDistanceArgs &a = *args;
    if (!dist_shape_ok(a.num_points, a.num_faces) || a.num_vertices < 1 || a.num_vertices > GA_MESH_MAX_FACES) return GA_ERR_BAD_SHAPE;
    if (a.reserved != 0) return GA_ERR_BAD_FLAGS;
    if (!a.points || !a.vertices || !a.faces || !a.dist2 || !a.face || !a.closest || !a.bary || !a.workspace) return GA_ERR_NULL_ARG;
    GaMeshPointDistancePlan plan;
    ga_mesh_point_distance_plan(a.num_points, a.num_faces, &plan);
    if (a.workspace_bytes < plan.workspace_bytes || (reinterpret_cast<uintptr_t>(a.workspace) & 15)) return GA_ERR_WORKSPACE;
    const DistShape s = dist_shape(a.num_points, a.num_faces);
    const unsigned qblocks = (unsigned)(((int64_t)a.num_points + kThreads - 1) / kThreads);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    hipLaunchKernelGGL(mesh_prep_kernel, dim3((unsigned)((a.num_faces + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(mesh_distance_kernel, dim3(qblocks, (unsigned)s.chunks), dim3(kThreads), 0, st, a, s);
    hipLaunchKernelGGL(mesh_merge_kernel, dim3(qblocks), dim3(kThreads), 0, st, a, s);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}
