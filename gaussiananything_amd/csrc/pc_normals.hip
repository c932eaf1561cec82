// pc_normals.hip -- PCA normals of a point cloud and the surfel initialiser built on them, for gfx950 (include/ga_pointcloud.h).
//
// Built with -ffp-contract=off: every operation is rounded on its own, division and square root are hipcc's correctly rounded defaults,
// so both kernels are a function of their inputs alone and tests/_normals_ref.py restates them in numpy float32 bit for bit.
//
// normals: one lane per point.  The neighbour list of ga_pc_knn (cloud against itself, the point's own entry included) is walked twice,
//   once for the centroid and once for the six centred products; the coordinates are gathered straight from the cloud (1.2 MB at 100 000
//   points: L2-resident), nothing is staged.  The symmetric 3x3 is diagonalised by kSweeps cyclic Jacobi sweeps in registers: rotations
//   (0,1), (0,2), (1,2), no data-dependent exit, a rotation skipped only where its off-diagonal entry is exactly 0 (the rotation would be
//   the identity there, and its angle 0 / 0).  Only + - * / sqrt and comparisons.  No LDS, no atomics, no workspace.
// surfel_init: one lane per point, 13 floats out: the 2DGS distance rule for the scale, the frame (t', n x t', n) as a quaternion by
//   Shepperd's branches.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/ga_pointcloud.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSweeps = GA_PC_NORMALS_SWEEPS;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// One Jacobi rotation in the (p, q) plane of the symmetric matrix (app, aqq, apq; arp, arq are the entries of the third row) and of
// the eigenvector matrix, whose columns p and q are (v0p, v1p, v2p) and (v0q, v1q, v2q).
__device__ __forceinline__ void jacobi_rotate(float &app, float &aqq, float &apq, float &arp, float &arq, float &v0p, float &v0q,
                                              float &v1p, float &v1q, float &v2p, float &v2q) {
    if (apq != 0.f) {
        const float theta = (aqq - app) / (2.f * apq);
        float t = 1.f / (fabsf(theta) + sqrtf(theta * theta + 1.f));   // theta * theta may overflow: t = 0 then, the right limit
        t = theta >= 0.f ? t : -t;
        const float c = 1.f / sqrtf(t * t + 1.f);
        const float s = t * c;
        const float h = t * apq;
        app = app - h;
        aqq = aqq + h;
        apq = 0.f;
        const float rp = arp, rq = arq;
        arp = c * rp - s * rq;
        arq = s * rp + c * rq;
        const float a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
        v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
        v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
        v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
    }
}

// (la, column a) and (lb, column b) into ascending order; equal eigenvalues keep their places
__device__ __forceinline__ void order2(float &la, float &lb, float &a0, float &a1, float &a2, float &b0, float &b1, float &b2) {
    if (la > lb) {
        float t;
        t = la; la = lb; lb = t;
        t = a0; a0 = b0; b0 = t;
        t = a1; a1 = b1; b1 = t;
        t = a2; a2 = b2; b2 = t;
    }
}

// re-normalised, the component of largest magnitude (the first among equals) made positive
__device__ __forceinline__ void unit_default_sign(float &x, float &y, float &z) {
    const float l = norm3(x, y, z);
    x = x / l; y = y / l; z = z / l;
    float big = x, ab = fabsf(x);
    if (fabsf(y) > ab) { big = y; ab = fabsf(y); }
    if (fabsf(z) > ab) big = z;
    if (big < 0.f) { x = -x; y = -y; z = -z; }
}

__global__ __launch_bounds__(kThreads) void pc_normals_kernel(const float *__restrict__ points, const int32_t *__restrict__ lengths,
                                                              const int32_t *__restrict__ idx, const float *__restrict__ viewpoint,
                                                              int N, int K, float *__restrict__ normal, float *__restrict__ tangent,
                                                              float *__restrict__ eigenvalues) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const int n = clampi(lengths ? lengths[b] : N, 0, N);
    const int m = K < n ? K : n;
    const float *p = points + (size_t)b * N * 3;
    const size_t row = (size_t)b * N + (size_t)i;
    float nx = 0.f, ny = 0.f, nz = 1.f, tx = 1.f, ty = 0.f, tz = 0.f, l0 = 0.f, l1 = 0.f, l2 = 0.f;
    if (i < n && m >= 3) {
        const int32_t *list = idx + row * (size_t)K;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int k = 0; k < m; ++k) {
            const int j = clampi(list[k], 0, n - 1);   // a list entry is in range by contract; the clamp keeps a broken one in the cloud
            sx = sx + p[3 * (size_t)j];
            sy = sy + p[3 * (size_t)j + 1];
            sz = sz + p[3 * (size_t)j + 2];
        }
        const float fm = (float)m;
        const float cx = sx / fm, cy = sy / fm, cz = sz / fm;
        float a00 = 0.f, a01 = 0.f, a02 = 0.f, a11 = 0.f, a12 = 0.f, a22 = 0.f;
        for (int k = 0; k < m; ++k) {
            const int j = clampi(list[k], 0, n - 1);
            const float dx = p[3 * (size_t)j] - cx, dy = p[3 * (size_t)j + 1] - cy, dz = p[3 * (size_t)j + 2] - cz;
            a00 = a00 + dx * dx; a01 = a01 + dx * dy; a02 = a02 + dx * dz;
            a11 = a11 + dy * dy; a12 = a12 + dy * dz; a22 = a22 + dz * dz;
        }
        a00 = a00 / fm; a01 = a01 / fm; a02 = a02 / fm; a11 = a11 / fm; a12 = a12 / fm; a22 = a22 / fm;
        const float trace = (a00 + a11) + a22;
        if (trace != 0.f) {
            float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;   // v[k][c]
#pragma unroll
            for (int s = 0; s < kSweeps; ++s) {
                jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0,1), third index 2
                jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0,2), third index 1
                jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1,2), third index 0
            }
            order2(a00, a11, v00, v10, v20, v01, v11, v21);
            order2(a11, a22, v01, v11, v21, v02, v12, v22);
            order2(a00, a11, v00, v10, v20, v01, v11, v21);
            nx = v00; ny = v10; nz = v20;
            tx = v02; ty = v12; tz = v22;
            unit_default_sign(nx, ny, nz);
            unit_default_sign(tx, ty, tz);
            if (viewpoint) {
                const float dx = viewpoint[3 * b] - p[3 * (size_t)i], dy = viewpoint[3 * b + 1] - p[3 * (size_t)i + 1],
                            dz = viewpoint[3 * b + 2] - p[3 * (size_t)i + 2];
                if (((dx * nx + dy * ny) + dz * nz) < 0.f) { nx = -nx; ny = -ny; nz = -nz; }
            }
            l0 = a00; l1 = a11; l2 = a22;
        }
    }
    normal[3 * row] = nx; normal[3 * row + 1] = ny; normal[3 * row + 2] = nz;
    if (tangent) { tangent[3 * row] = tx; tangent[3 * row + 1] = ty; tangent[3 * row + 2] = tz; }
    if (eigenvalues) { eigenvalues[3 * row] = l0; eigenvalues[3 * row + 1] = l1; eigenvalues[3 * row + 2] = l2; }
}

__global__ __launch_bounds__(kThreads) void pc_surfel_init_kernel(const float *__restrict__ points, const float *__restrict__ normal,
                                                                  const float *__restrict__ tangent, const float *__restrict__ dist2,
                                                                  const int32_t *__restrict__ lengths,
                                                                  const float *__restrict__ eigenvalues, const float *__restrict__ colors,
                                                                  int N, int K, float opacity, float scale_factor,
                                                                  float *__restrict__ gaussians) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const int n = clampi(lengths ? lengths[b] : N, 0, N);
    const int m = K < n ? K : n;
    const size_t row = (size_t)b * N + (size_t)i;
    float o = 0.f, s = 1e-4f, qw = 1.f, qx = 0.f, qy = 0.f, qz = 0.f, cr = 0.5f, cg = 0.5f, cb = 0.5f;
    if (i < n && m >= 4) {
        float nx = normal[3 * row], ny = normal[3 * row + 1], nz = normal[3 * row + 2];
        const float tx = tangent[3 * row], ty = tangent[3 * row + 1], tz = tangent[3 * row + 2];
        const float nl = norm3(nx, ny, nz);
        nx = nx / nl; ny = ny / nl; nz = nz / nl;
        const float d = (tx * nx + ty * ny) + tz * nz;
        float ux = tx - d * nx, uy = ty - d * ny, uz = tz - d * nz;
        const float ul = norm3(ux, uy, uz);
        const bool spread = eigenvalues ? eigenvalues[3 * row + 2] > 0.f : true;
        if (nl > 0.f && ul > 0.f && spread) {   // (a NaN fails every comparison: the row is invalid)
            const float *d2 = dist2 + row * (size_t)K;
            s = scale_factor * sqrtf(fmaxf(((d2[1] + d2[2]) + d2[3]) / 3.f, 1e-7f));
            ux = ux / ul; uy = uy / ul; uz = uz / ul;
            const float bx = ny * uz - nz * uy, by = nz * ux - nx * uz, bz = nx * uy - ny * ux;
            // R[row][col] with the columns (t', b, n)
            const float R00 = ux, R10 = uy, R20 = uz, R01 = bx, R11 = by, R21 = bz, R02 = nx, R12 = ny, R22 = nz;
            const float tr = (R00 + R11) + R22;
            if (tr > 0.f) {
                const float S = sqrtf(tr + 1.f) * 2.f;
                qw = 0.25f * S; qx = (R21 - R12) / S; qy = (R02 - R20) / S; qz = (R10 - R01) / S;
            } else if (R00 > R11 && R00 > R22) {
                const float S = sqrtf(((1.f + R00) - R11) - R22) * 2.f;
                qw = (R21 - R12) / S; qx = 0.25f * S; qy = (R01 + R10) / S; qz = (R02 + R20) / S;
            } else if (R11 > R22) {
                const float S = sqrtf(((1.f + R11) - R00) - R22) * 2.f;
                qw = (R02 - R20) / S; qx = (R01 + R10) / S; qy = 0.25f * S; qz = (R12 + R21) / S;
            } else {
                const float S = sqrtf(((1.f + R22) - R00) - R11) * 2.f;
                qw = (R10 - R01) / S; qx = (R02 + R20) / S; qy = (R12 + R21) / S; qz = 0.25f * S;
            }
            const float ql = sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
            qw = qw / ql; qx = qx / ql; qy = qy / ql; qz = qz / ql;
            if (qw < 0.f) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
            o = opacity;
            if (colors) { cr = colors[3 * row]; cg = colors[3 * row + 1]; cb = colors[3 * row + 2]; }
        }
    }
    float *g = gaussians + row * GA_PC_SURFEL_FLOATS;
    g[0] = points[3 * row]; g[1] = points[3 * row + 1]; g[2] = points[3 * row + 2];
    g[3] = o; g[4] = s; g[5] = s;
    g[6] = qw; g[7] = qx; g[8] = qy; g[9] = qz;
    g[10] = cr; g[11] = cg; g[12] = cb;
}

bool normals_shape_ok(int64_t B, int64_t N, int64_t K, int64_t kmin) {
    const int64_t lim = int64_t(1) << 31;   // the limits of GaKnnArgs for a cloud against itself
    return B > 0 && B <= GA_PC_MAX_BATCH && N > 0 && K >= kmin && K <= GA_PC_KNN_MAX_K && N * 3 < lim && N * K < lim;
}

void normals_plan(int N, GaNormalsPlan &pl) {
    pl.threads = kThreads;
    pl.grid_x = (N + kThreads - 1) / kThreads;
    pl.grid_y = 1;
    pl.sweeps = kSweeps;
}

}  // namespace

extern "C" int ga_pc_normals_plan(int32_t num_points, int32_t k, GaNormalsPlan *plan) {
    if (!plan) return GA_ERR_NULL_ARG;
    if (!normals_shape_ok(1, num_points, k, 3)) return GA_ERR_BAD_SHAPE;
    normals_plan(num_points, *plan);
    return GA_OK;
}

extern "C" int ga_pc_normals(const GaNormalsArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaNormalsArgs &a = *args;
    if (!normals_shape_ok(a.batch, a.num_points, a.k, 3)) return GA_ERR_BAD_SHAPE;
    if (!a.points || !a.idx || !a.normal) return GA_ERR_NULL_ARG;
    GaNormalsPlan pl;
    normals_plan(a.num_points, pl);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    hipLaunchKernelGGL(pc_normals_kernel, dim3(pl.grid_x, pl.grid_y * a.batch), dim3(pl.threads), 0, s, a.points, a.lengths, a.idx,
                       a.viewpoint, a.num_points, a.k, a.normal, a.tangent, a.eigenvalues);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_pc_surfel_init(const GaSurfelInitArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaSurfelInitArgs &a = *args;
    if (!normals_shape_ok(a.batch, a.num_points, a.k, 4)) return GA_ERR_BAD_SHAPE;
    if (!a.points || !a.normal || !a.tangent || !a.dist2 || !a.gaussians) return GA_ERR_NULL_ARG;
    GaNormalsPlan pl;
    normals_plan(a.num_points, pl);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    hipLaunchKernelGGL(pc_surfel_init_kernel, dim3(pl.grid_x, pl.grid_y * a.batch), dim3(pl.threads), 0, s, a.points, a.normal, a.tangent,
                       a.dist2, a.lengths, a.eigenvalues, a.colors, a.num_points, a.k, a.opacity, a.scale_factor, a.gaussians);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}
