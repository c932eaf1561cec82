// pc_align.hip -- registration of point clouds for gfx950: Horn alignment of corresponding points and ICP (include/ga_pointcloud.h).
//
// Built with -ffp-contract=off: the transformed point and its squared distance are fp32 with every operation rounded on its own, the
// sums and the solve are fp64 with only + - * / sqrt, so tests/_align_ref.py reproduces every output bit for bit.
//
// accumulate: one lane per row of X, kAlignThreads lanes per workgroup, grid (ceil(N / kAlignThreads), B).  With MATCH the lane transforms
//   its point and walks the targets exactly as nearest_kernel of pointcloud.hip does (LDS tiles of kAlignTile points read by broadcast,
//   strict `<` upwards: the lowest index among equals), then forms its 19 fp64 terms from the ORIGINAL x and its partner.  The workgroup
//   sums them as the balanced tree over the lane index -- a butterfly of ds_bpermute pairs inside the wave (19 doubles x 6 levels once
//   per workgroup: nothing beside the target walk), the four waves through 608 bytes of LDS -- and writes one partial row.  No
//   atomics; no workgroup waits for another.
// solve: one workgroup of kSolveThreads lanes per cloud; lanes 0..18 add the partial rows in ascending workgroup order, lane 0 does the
//   4 x 4 Jacobi of Horn's matrix with compile-time indices only (the matrices stay in registers).
// ICP is max_iterations x (accumulate, solve) and one final pass enqueued on the stream; the per-cloud state (transform, status,
//   iterations, previous rmse) lives in device memory and a frozen cloud's workgroups leave after one block-uniform read of its status.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/ga_pointcloud.h"

namespace {

constexpr int kAlignThreads = 256;
constexpr int kAlignTile = 1024;
constexpr int kSolveThreads = 64;
constexpr int kTerms = GA_PC_ALIGN_TERMS;
constexpr int kSweeps = GA_PC_ALIGN_SWEEPS;
constexpr int kXf = GA_PC_TRANSFORM_FLOATS;
constexpr int kHf = GA_PC_ALIGN_HISTORY_FLOATS;

constexpr int kFlagScale = 1, kFlagIcp = 2, kFlagFinal = 4;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    float d = dx * dx;
    d = d + dy * dy;
    d = d + dz * dz;
    return d;
}

__global__ __launch_bounds__(kSolveThreads) void align_init_kernel(const float *__restrict__ init, int B, float *__restrict__ transform,
                                                                   int32_t *__restrict__ status, int32_t *__restrict__ iterations,
                                                                   double *__restrict__ prev) {
    const int b = blockIdx.x * kSolveThreads + threadIdx.x;
    if (b >= B) return;
    for (int j = 0; j < kXf; ++j)
        transform[(size_t)b * kXf + j] = init ? init[(size_t)b * kXf + j] : ((j == 0 || j == 1 || j == 5 || j == 9) ? 1.f : 0.f);
    status[b] = GA_PC_ALIGN_RUNNING;
    if (iterations) iterations[b] = 0;
    prev[b] = 0.0;
}

template <bool MATCH>
__global__ __launch_bounds__(kAlignThreads) void align_accumulate_kernel(
    const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ weights, const int32_t *__restrict__ xlen,
    const int32_t *__restrict__ ylen, const float *__restrict__ transform, const int32_t *__restrict__ status, int Nx, int Ny, float gate2,
    int final_pass, double *__restrict__ partial, float *__restrict__ out_xt, int32_t *__restrict__ out_idx, float *__restrict__ out_d2) {
    __shared__ __attribute__((aligned(16))) float tx[MATCH ? kAlignTile : 4], ty[MATCH ? kAlignTile : 4], tz[MATCH ? kAlignTile : 4];
    __shared__ double wsum[kAlignThreads / 64][kTerms];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (MATCH && !final_pass && status[b] != GA_PC_ALIGN_RUNNING) return;   // a frozen cloud: block-uniform, ahead of every barrier
    const int i = blockIdx.x * kAlignThreads + tid;
    const int nx = clampi(xlen ? xlen[b] : Nx, 0, Nx);
    const int ny = MATCH ? clampi(ylen ? ylen[b] : Ny, 0, Ny) : nx;
    double *prow = partial + ((size_t)b * gridDim.x + blockIdx.x) * kTerms;
    const bool pad_out = MATCH && final_pass && i < Nx;
    if (blockIdx.x * kAlignThreads >= nx) {   // the whole block is padding (block-uniform: no barrier is skipped by a part of it)
        if (tid < kTerms) prow[tid] = 0.0;
        if (pad_out) {
            const size_t o = (size_t)b * Nx + i;
            out_xt[3 * o] = 0.f; out_xt[3 * o + 1] = 0.f; out_xt[3 * o + 2] = 0.f;
            out_idx[o] = -1;
            out_d2[o] = 0.f;
        }
        return;
    }
    const float *xp = x + (size_t)b * Nx * 3, *yp = y + (size_t)b * Ny * 3;
    const bool live = i < nx;
    const float x0 = live ? xp[3 * (size_t)i] : 0.f, x1 = live ? xp[3 * (size_t)i + 1] : 0.f, x2 = live ? xp[3 * (size_t)i + 2] : 0.f;
    float y0 = 0.f, y1 = 0.f, y2 = 0.f, d2 = 0.f;
    bool paired = live;
    if (MATCH) {
        const float *tf = transform + (size_t)b * kXf;
        const float s = tf[0];
        float q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float a = x0 * tf[1 + c];
            a = a + x1 * tf[4 + c];
            a = a + x2 * tf[7 + c];
            a = a * s;
            q[c] = a + tf[10 + c];
        }
        float best = __builtin_inff();
        int besti = -1;
        for (int t0 = 0; t0 < ny; t0 += kAlignTile) {
            const int cnt = ny - t0 < kAlignTile ? ny - t0 : kAlignTile;
            __syncthreads();   // the previous tile has been read by every wave
            for (int j = tid; j < cnt; j += kAlignThreads) {
                const size_t g = 3 * (size_t)(t0 + j);
                tx[j] = yp[g]; ty[j] = yp[g + 1]; tz[j] = yp[g + 2];
            }
            __syncthreads();
            int j = 0;
            for (; j + 4 <= cnt; j += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float d = dist2(q[0], q[1], q[2], tx[j + u], ty[j + u], tz[j + u]);
                    if (d < best) { best = d; besti = t0 + j + u; }
                }
            }
            for (; j < cnt; ++j) {
                const float d = dist2(q[0], q[1], q[2], tx[j], ty[j], tz[j]);
                if (d < best) { best = d; besti = t0 + j; }
            }
        }
        paired = live && besti >= 0;   // besti < 0: an empty target cloud (or NaN coordinates), the pair counts for nothing
        if (paired) {
            y0 = yp[3 * (size_t)besti]; y1 = yp[3 * (size_t)besti + 1]; y2 = yp[3 * (size_t)besti + 2];
            d2 = best;
        }
        if (pad_out) {
            const size_t o = (size_t)b * Nx + i;
            out_xt[3 * o] = live ? q[0] : 0.f; out_xt[3 * o + 1] = live ? q[1] : 0.f; out_xt[3 * o + 2] = live ? q[2] : 0.f;
            out_idx[o] = live ? besti : -1;
            out_d2[o] = live ? best : 0.f;
        }
    } else if (live) {
        y0 = yp[3 * (size_t)i]; y1 = yp[3 * (size_t)i + 1]; y2 = yp[3 * (size_t)i + 2];
        d2 = dist2(x0, x1, x2, y0, y1, y2);
    }
    double v[kTerms];
#pragma unroll
    for (int t = 0; t < kTerms; ++t) v[t] = 0.0;
    if (paired) {
        float wf = weights ? weights[(size_t)b * Nx + i] : 1.f;
        if (gate2 >= 0.f && d2 > gate2) wf = 0.f;
        const double w = wf;
        const double xd[3] = {x0, x1, x2}, yd[3] = {y0, y1, y2};
        v[0] = w;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double wx = w * xd[a];
            v[1 + a] = wx;
            v[4 + a] = w * yd[a];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[7 + 3 * a + c] = wx * yd[c];
        }
        v[16] = w * ((xd[0] * xd[0] + xd[1] * xd[1]) + xd[2] * xd[2]);
        v[17] = w * ((yd[0] * yd[0] + yd[1] * yd[1]) + yd[2] * yd[2]);
        v[18] = w * (double)d2;
    }
    // v[i] += v[i xor 2^l], l = 0 .. 5: both partners form the same sum (addition commutes), every lane ends with the wave's
    const int wave = tid >> 6;
#pragma unroll
    for (int t = 0; t < kTerms; ++t) {
        double a = v[t];
#pragma unroll
        for (int l = 0; l < 6; ++l) a = a + __shfl_xor(a, 1 << l, 64);
        if ((tid & 63) == 0) wsum[wave][t] = a;
    }
    __syncthreads();
    if (tid < kTerms) prow[tid] = (wsum[0][tid] + wsum[1][tid]) + (wsum[2][tid] + wsum[3][tid]);   // l = 6, then l = 7
}

// One Jacobi rotation in the (P, Q) plane of the symmetric 4 x 4 matrix a and of the eigenvector matrix v: the formulas of
// jacobi_rotate in pc_normals.hip, in fp64.  Indices are compile-time constants: a and v live in registers.
template <int P, int Q>
__device__ __forceinline__ void jacobi4(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq != 0.0) {
        const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));   // theta * theta may overflow: t = 0 then, the right limit
        t = theta >= 0.0 ? t : -t;
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        const double h = t * apq;
        a[P][P] = a[P][P] - h;
        a[Q][Q] = a[Q][Q] + h;
        a[P][Q] = 0.0;
        a[Q][P] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r != P && r != Q) {
                const double rp = a[r][P], rq = a[r][Q];
                const double np_ = c * rp - s * rq, nq_ = s * rp + c * rq;
                a[r][P] = np_; a[P][r] = np_;
                a[r][Q] = nq_; a[Q][r] = nq_;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double vp = v[k][P], vq = v[k][Q];
            v[k][P] = c * vp - s * vq;
            v[k][Q] = s * vp + c * vq;
        }
    }
}

__global__ __launch_bounds__(kSolveThreads) void align_solve_kernel(const double *__restrict__ partial, int G, float *__restrict__ transform,
                                                                    float *__restrict__ rmse_out, int32_t *__restrict__ status,
                                                                    int32_t *__restrict__ iterations, float *__restrict__ history,
                                                                    double *__restrict__ prev, int k, int max_iterations, int flags,
                                                                    float thr) {
    __shared__ double S[kTerms];
    const int b = blockIdx.x, tid = threadIdx.x;
    float *tf = transform + (size_t)b * kXf;
    float *hist = history ? history + (size_t)b * (max_iterations + 1) * kHf : nullptr;
    if (status[b] != GA_PC_ALIGN_RUNNING) {   // frozen (block-uniform); the final pass repeats its last history row
        if ((flags & kFlagFinal) && hist && tid < kHf) {
            const int last = iterations[b];
            for (int r = last + 1; r <= max_iterations; ++r) hist[(size_t)r * kHf + tid] = hist[(size_t)last * kHf + tid];
        }
        return;
    }
    if (tid < kTerms) {
        const double *p = partial + (size_t)b * G * kTerms + tid;
        double a = p[0];
        for (int g = 1; g < G; ++g) a = a + p[(size_t)g * kTerms];
        S[tid] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    const double W = S[0];
    const bool has_weight = W > 0.0;
    const double rmse = has_weight ? sqrt(S[18] / W) : 0.0;
    rmse_out[b] = (float)rmse;
    if (hist) {
        for (int j = 0; j < kXf; ++j) hist[(size_t)k * kHf + j] = tf[j];
        hist[(size_t)k * kHf + kXf] = (float)rmse;
    }
    if (!has_weight) { status[b] = GA_PC_ALIGN_DEGENERATE; return; }
    if ((flags & kFlagIcp) && k >= 1) {
        const double p = prev[b];
        if (fabs(p - rmse) <= (double)thr * p) { status[b] = GA_PC_ALIGN_CONVERGED; return; }   // before the update: the transform stays
    }
    if (flags & kFlagFinal) return;
    double xm[3], ym[3], M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { xm[a] = S[1 + a] / W; ym[a] = S[4 + a] / W; }
#pragma unroll
    for (int e = 0; e < 9; ++e) M[e / 3][e % 3] = S[7 + e] / W - xm[e / 3] * ym[e % 3];
    const double vx = S[16] / W - ((xm[0] * xm[0] + xm[1] * xm[1]) + xm[2] * xm[2]);
    // sums of a coincident cloud leave a vx of rounding size, either sign: no extent unless vx exceeds 2^-40 of the mean |x|^2
    if ((flags & kFlagScale) && !(vx > (S[16] / W) * 0x1p-40)) { status[b] = GA_PC_ALIGN_DEGENERATE; return; }
    // Horn's matrix: its eigenvector of the largest eigenvalue is the quaternion (w, x, y, z) of the rotation Q with y ~ Q x
    double A[4][4], V[4][4];
    A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    A[2][2] = (M[1][1] - M[0][0]) - M[2][2];
    A[3][3] = (M[2][2] - M[0][0]) - M[1][1];
    A[0][1] = A[1][0] = M[1][2] - M[2][1];
    A[0][2] = A[2][0] = M[2][0] - M[0][2];
    A[0][3] = A[3][0] = M[0][1] - M[1][0];
    A[1][2] = A[2][1] = M[0][1] + M[1][0];
    A[1][3] = A[3][1] = M[2][0] + M[0][2];
    A[2][3] = A[3][2] = M[1][2] + M[2][1];
#pragma unroll
    for (int e = 0; e < 16; ++e) V[e / 4][e % 4] = e / 4 == e % 4 ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        jacobi4<0, 1>(A, V); jacobi4<0, 2>(A, V); jacobi4<0, 3>(A, V);
        jacobi4<1, 2>(A, V); jacobi4<1, 3>(A, V); jacobi4<2, 3>(A, V);
    }
    // the column under the largest diagonal entry, the lowest among equals: selects of values, no indexed read of V
    double lam = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const double d = A[c][c], c0 = V[0][c], c1 = V[1][c], c2 = V[2][c], c3 = V[3][c];
        const bool up = d > lam;
        lam = up ? d : lam;
        q0 = up ? c0 : q0; q1 = up ? c1 : q1; q2 = up ? c2 : q2; q3 = up ? c3 : q3;
    }
    const double n = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const double qw = q0 / n, qx = q1 / n, qy = q2 / n, qz = q3 / n;
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
    double R[3][3];   // R = Q^T: the row-vector convention Xt = s * X @ R + T
    R[0][0] = 1.0 - 2.0 * (yy + zz); R[1][0] = 2.0 * (xy - wz);       R[2][0] = 2.0 * (xz + wy);
    R[0][1] = 2.0 * (xy + wz);       R[1][1] = 1.0 - 2.0 * (xx + zz); R[2][1] = 2.0 * (yz - wx);
    R[0][2] = 2.0 * (xz - wy);       R[1][2] = 2.0 * (yz + wx);       R[2][2] = 1.0 - 2.0 * (xx + yy);
    double s = 1.0;
    if (flags & kFlagScale) {
        double tr = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) tr = tr + R[e / 3][e % 3] * M[e / 3][e % 3];
        s = tr / vx;
    }
    tf[0] = (float)s;
#pragma unroll
    for (int e = 0; e < 9; ++e) tf[1 + e] = (float)R[e / 3][e % 3];
#pragma unroll
    for (int c = 0; c < 3; ++c) tf[10 + c] = (float)(ym[c] - s * ((xm[0] * R[0][c] + xm[1] * R[1][c]) + xm[2] * R[2][c]));
    prev[b] = rmse;
    if (iterations) iterations[b] = iterations[b] + 1;
}

bool align_shape_ok(int64_t B, int64_t N) { return B > 0 && B <= GA_PC_MAX_BATCH && N > 0 && N * 3 < (int64_t(1) << 31); }

int64_t align_groups(int64_t N) { return (N + kAlignThreads - 1) / kAlignThreads; }

}  // namespace

extern "C" int ga_pc_align_plan(int32_t num_points, int32_t num_target, GaAlignPlan *plan) {
    if (!plan) return GA_ERR_NULL_ARG;
    if (!align_shape_ok(1, num_points) || !align_shape_ok(1, num_target)) return GA_ERR_BAD_SHAPE;
    plan->threads = kAlignThreads;
    plan->tile = kAlignTile;
    plan->grid_x = (int32_t)align_groups(num_points);
    plan->solve_threads = kSolveThreads;
    plan->sweeps = kSweeps;
    plan->terms = kTerms;
    return GA_OK;
}

extern "C" size_t ga_pc_align_workspace_bytes(int32_t batch, int32_t num_points) {
    if (!align_shape_ok(batch, num_points)) return 0;
    // the partial rows [B, ceil(N / threads), 19] and the previous rmse [B], fp64
    const size_t doubles = (size_t)batch * (size_t)align_groups(num_points) * kTerms + (size_t)batch;
    return (doubles * sizeof(double) + 15) / 16 * 16;
}

extern "C" int ga_pc_align_points(const GaAlignArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaAlignArgs &a = *args;
    if (!align_shape_ok(a.batch, a.num_points)) return GA_ERR_BAD_SHAPE;
    if ((a.estimate_scale != 0 && a.estimate_scale != 1) || a.reserved != 0) return GA_ERR_BAD_FLAGS;
    if (!a.x || !a.y || !a.transform || !a.rmse || !a.status || !a.workspace) return GA_ERR_NULL_ARG;
    if (a.workspace_bytes < ga_pc_align_workspace_bytes(a.batch, a.num_points)) return GA_ERR_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    const int G = (int)align_groups(a.num_points);
    double *partial = static_cast<double *>(a.workspace);
    double *prev = partial + (size_t)a.batch * G * kTerms;
    hipLaunchKernelGGL(align_init_kernel, dim3((a.batch + kSolveThreads - 1) / kSolveThreads), dim3(kSolveThreads), 0, s,
                       (const float *)nullptr, a.batch, a.transform, a.status, (int32_t *)nullptr, prev);
    hipLaunchKernelGGL((align_accumulate_kernel<false>), dim3(G, a.batch), dim3(kAlignThreads), 0, s, a.x, a.y, a.weights, a.lengths,
                       a.lengths, (const float *)nullptr, (const int32_t *)nullptr, a.num_points, a.num_points, -1.f, 0, partial,
                       (float *)nullptr, (int32_t *)nullptr, (float *)nullptr);
    hipLaunchKernelGGL(align_solve_kernel, dim3(a.batch), dim3(kSolveThreads), 0, s, partial, G, a.transform, a.rmse, a.status,
                       (int32_t *)nullptr, (float *)nullptr, prev, 0, 0, a.estimate_scale ? kFlagScale : 0, 0.f);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_pc_icp(const GaIcpArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaIcpArgs &a = *args;
    if (!align_shape_ok(a.batch, a.num_points) || !align_shape_ok(a.batch, a.num_target)) return GA_ERR_BAD_SHAPE;
    if (a.max_iterations < 0 || a.max_iterations > GA_PC_ICP_MAX_ITERATIONS) return GA_ERR_BAD_SHAPE;
    if ((a.estimate_scale != 0 && a.estimate_scale != 1) || a.reserved != 0) return GA_ERR_BAD_FLAGS;
    if (!(a.relative_rmse_thr >= 0.f) || !(a.relative_rmse_thr < __builtin_inff())) return GA_ERR_BAD_FLAGS;
    if (!(a.max_distance >= 0.f) || !(a.max_distance < __builtin_inff())) return GA_ERR_BAD_FLAGS;
    if (!a.x || !a.y || !a.transform || !a.rmse || !a.status || !a.iterations || !a.xt || !a.idx || !a.dist2 || !a.workspace)
        return GA_ERR_NULL_ARG;
    if (a.workspace_bytes < ga_pc_align_workspace_bytes(a.batch, a.num_points)) return GA_ERR_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    const int G = (int)align_groups(a.num_points);
    double *partial = static_cast<double *>(a.workspace);
    double *prev = partial + (size_t)a.batch * G * kTerms;
    const float gate2 = a.max_distance > 0.f ? a.max_distance * a.max_distance : -1.f;
    const int flags = kFlagIcp | (a.estimate_scale ? kFlagScale : 0);
    hipLaunchKernelGGL(align_init_kernel, dim3((a.batch + kSolveThreads - 1) / kSolveThreads), dim3(kSolveThreads), 0, s, a.init_transform,
                       a.batch, a.transform, a.status, a.iterations, prev);
    for (int k = 0; k <= a.max_iterations; ++k) {
        const int fin = k == a.max_iterations;
        hipLaunchKernelGGL((align_accumulate_kernel<true>), dim3(G, a.batch), dim3(kAlignThreads), 0, s, a.x, a.y, a.weights, a.x_lengths,
                           a.y_lengths, (const float *)a.transform, (const int32_t *)a.status, a.num_points, a.num_target, gate2, fin,
                           partial, a.xt, a.idx, a.dist2);
        hipLaunchKernelGGL(align_solve_kernel, dim3(a.batch), dim3(kSolveThreads), 0, s, partial, G, a.transform, a.rmse, a.status,
                           a.iterations, a.history, prev, k, a.max_iterations, flags | (fin ? kFlagFinal : 0), a.relative_rmse_thr);
    }
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}
