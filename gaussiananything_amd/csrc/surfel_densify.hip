// surfel_densify.hip -- adaptive density control of the surfel fitter (include/ga_densify.h): the densification statistic of one
// iteration, the clone / split / prune round and the opacity reset.
//
// Built with -ffp-contract=off: the statistic, the classification and the split children are bit-identical to the operation-by-operation
// restatement the tests hold them to (tests/_densify_ref.py); the normals of a split come from the device library's log / sin / cos and
// are handed out (noise_out) instead of being pinned.
//   accumulate   one lane per surfel: V radii and V view rows read, three words updated; part of the captured iteration
//   densify      a stream compaction whose output size is data dependent, as three launches ordered by the stream, built from
//                csrc/compact.h -- no workgroup waits for another one, there is no look-back, no spinning, no device-wide barrier:
//                  1 count     one lane per kRows consecutive surfels: classify, reduce the block's emitted rows and tallies
//                  2 scan      ONE workgroup walks the block sums kThreads at a time (carry in a register), writes each block's
//                              exclusive offset in place and the totals to out_counts
//                  3 scatter   classifies again (the same inputs give the same answer), scans the block's own counts, lists the source
//                              of every output row of the block in LDS and copies raw / m / v with the whole block, consecutive lanes
//                              on consecutive floats of the block's contiguous output range
//   reset        one lane per surfel
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ga_densify.h"
#include "compact.h"
#include "philox.h"

namespace ga {

using namespace gacompact;

constexpr int kThreads = GA_DENSIFY_THREADS;
constexpr int kRows = GA_DENSIFY_ROWS_PER_LANE;
constexpr int kBlockRows = GA_DENSIFY_BLOCK_ROWS;
constexpr int kWaves = kThreads / 64;
enum { kKept = 0, kClone = 1, kSplit = 2, kPruned = 3 };

__global__ __launch_bounds__(kThreads) void fit_accumulate_kernel(GaFitAccumulateArgs a)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.num_points) return;
    const float px = a.means[(int64_t)i * 3], py = a.means[(int64_t)i * 3 + 1], pz = a.means[(int64_t)i * 3 + 2];
    int c = 0, rmax = 0;
    float zsum = 0.f;
    for (int v = 0; v < a.num_views; ++v) {
        const int r = a.radii[(int64_t)v * a.num_points + i];
        rmax = r > rmax ? r : rmax;
        if (r > 0) {
            const float *vm = a.view + 16 * v;
            const float vz = ((vm[2] * px + vm[6] * py) + vm[10] * pz) + vm[14];
            zsum = zsum + vz;
            ++c;
        }
    }
    if (c == 0) return;
    const float gx = a.g_means[(int64_t)i * 3], gy = a.g_means[(int64_t)i * 3 + 1], gz = a.g_means[(int64_t)i * 3 + 2];
    const float zbar = zsum / (float)c;
    const float g = sqrtf((gx * gx + gy * gy) + gz * gz);
    a.grad_accum[i] = a.grad_accum[i] + (g * zbar) * a.tanfov;
    a.denom[i] = a.denom[i] + 1;
    const int before = a.max_radius[i];
    a.max_radius[i] = before > rmax ? before : rmax;
}

__device__ __forceinline__ int densify_classify(const GaDensifyArgs &a, int i)
{
    const float opa = a.opacities[i];
    const float s0 = a.scales[(int64_t)i * 2], s1 = a.scales[(int64_t)i * 2 + 1];
    const float smax = s0 >= s1 ? s0 : s1;
    bool prune = opa < a.min_opacity;
    if (a.max_screen_size > 0.f)
        prune = prune || (float)a.max_radius[i] > a.max_screen_size || smax > 0.1f * a.extent;
    if (prune) return kPruned;
    if (a.flags & GA_DENSIFY_PRUNE_ONLY) return kKept;
    const int d = a.denom[i];
    float avg = d > 0 ? a.grad_accum[i] / (float)d : 0.f;
    avg = avg == avg ? avg : 0.f;
    if (avg >= a.grad_threshold) return smax <= a.percent_dense * a.extent ? kClone : kSplit;
    return kKept;
}

__device__ __forceinline__ int emitted(int code) { return code == kPruned ? 0 : (code == kKept ? 1 : 2); }

__global__ __launch_bounds__(kThreads) void densify_count_kernel(GaDensifyArgs a)
{
    __shared__ int lds[4][kWaves];
    const int first = blockIdx.x * kBlockRows + threadIdx.x * kRows;
    int n[4] = {0, 0, 0, 0};   // rows, cloned, split, pruned
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int i = first + j;
        if (i < a.num_points) {
            const int code = densify_classify(a, i);
            n[0] += emitted(code);
            n[1] += code == kClone;
            n[2] += code == kSplit;
            n[3] += code == kPruned;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n[k] += __shfl_down(n[k], d, 64);
        if (lane == 0) lds[k][wave] = n[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int4 s = make_int4(0, 0, 0, 0);
#pragma unroll
        for (int w = 0; w < kWaves; ++w) { s.x += lds[0][w]; s.y += lds[1][w]; s.z += lds[2][w]; s.w += lds[3][w]; }
        reinterpret_cast<int4 *>(a.workspace)[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kThreads) void densify_scan_kernel(GaDensifyArgs a, int num_blocks)
{
    __shared__ int lds[kWaves];
    __shared__ long long tally[3][kWaves];
    int4 *sums = reinterpret_cast<int4 *>(a.workspace);
    long long carry = 0, t[3] = {0, 0, 0};
    for (int start = 0; start < num_blocks; start += kThreads) {      // (every lane takes every trip: the barriers are uniform)
        const int b = start + (int)threadIdx.x;
        int4 s = make_int4(0, 0, 0, 0);
        if (b < num_blocks) s = sums[b];
        t[0] += s.y; t[1] += s.z; t[2] += s.w;
        int total;
        const int incl = block_inclusive_scan<kWaves>(s.x, lds, total);
        if (b < num_blocks) {
            s.x = (int)(carry + (incl - s.x));                         // the block's exclusive offset, in place of its sum
            sums[b] = s;
        }
        carry += total;
    }
    long long s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = block_sum<kWaves>(t[k], tally[k]);
    if (threadIdx.x == 0) {
        const long long n = a.num_points;
        a.out_counts[0] = carry;
        a.out_counts[1] = n - s[0] - s[1] - s[2];
        a.out_counts[2] = s[0];
        a.out_counts[3] = s[1];
        a.out_counts[4] = s[2];
        a.out_counts[5] = n;
        a.out_counts[6] = (long long)a.round;
        a.out_counts[7] = (long long)a.flags;
    }
}

// the two children of split parent i: their xyz go to rows `row` and `row + 1` of out_raw, the four normals to xi
__device__ __forceinline__ void split_children(const GaDensifyArgs &a, int i, int64_t row, float xi[4])
{
    uint32_t w[4];
    gaphilox::philox4x32_10((uint32_t)i, a.round, GA_DENSIFY_STREAM, 0u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
    xi[0] = gaphilox::box_muller(w[0], w[1], 0);
    xi[1] = gaphilox::box_muller(w[0], w[1], 1);
    xi[2] = gaphilox::box_muller(w[2], w[3], 0);
    xi[3] = gaphilox::box_muller(w[2], w[3], 1);
    const float *q = a.rotations + (int64_t)i * 4;
    const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    // the tangent columns as the rasterizer's preprocess builds them (surfel_preprocess.hip: splat_constants)
    const float qs = 1.0f / sqrtf(((q3 * q3 + q0 * q0) + q1 * q1) + q2 * q2);
    const float r = q0 * qs, x = q1 * qs, y = q2 * qs, z = q3 * qs;
    const float tu[3] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y + r * z), 2.f * (x * z - r * y)};
    const float tv[3] = {2.f * (x * y - r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z + r * x)};
    const float s0 = a.scales[(int64_t)i * 2], s1 = a.scales[(int64_t)i * 2 + 1];
    const float *p = a.raw + (int64_t)i * GA_FIT_PARAMS;
#pragma unroll
    for (int child = 0; child < 2; ++child) {
        const float du = s0 * xi[2 * child], dv = s1 * xi[2 * child + 1];
        float *o = a.out_raw + (row + child) * GA_FIT_PARAMS;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = (p[k] + tu[k] * du) + tv[k] * dv;
    }
}

__global__ __launch_bounds__(kThreads) void densify_scatter_kernel(GaDensifyArgs a)
{
    // the source of every output row of this block: local parent index (bits 0..15) and what the row is (bits 16..17):
    // 0 the parent itself, 1 the copy a clone adds, 2 / 3 the children of a split
    __shared__ uint32_t src[2 * kBlockRows];
    __shared__ int lds[kWaves];
    const int base = blockIdx.x * kBlockRows, local = threadIdx.x * kRows;
    int code[kRows], mine = 0;
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int i = base + local + j;
        code[j] = i < a.num_points ? densify_classify(a, i) : kPruned;
        mine += emitted(code[j]);
    }
    int total;
    int o = block_inclusive_scan<kWaves>(mine, lds, total) - mine;
    const int64_t block_off = reinterpret_cast<const int4 *>(a.workspace)[blockIdx.x].x;
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int i = base + local + j;
        if (i >= a.num_points) break;
        const uint32_t l = (uint32_t)(local + j);
        float xi[4] = {0.f, 0.f, 0.f, 0.f};
        if (code[j] == kKept) {
            src[o] = l;
            o += 1;
        } else if (code[j] == kClone) {
            src[o] = l;
            src[o + 1] = l | (1u << 16);
            o += 2;
        } else if (code[j] == kSplit) {
            split_children(a, i, block_off + o, xi);
            src[o] = l | (2u << 16);
            src[o + 1] = l | (3u << 16);
            o += 2;
        }
        if (a.noise_out) reinterpret_cast<float4 *>(a.noise_out)[i] = make_float4(xi[0], xi[1], xi[2], xi[3]);
    }
    __syncthreads();
    for (int r = threadIdx.x; r < total; r += kThreads) a.parent[block_off + r] = base + (int)(src[r] & 0xFFFFu);
    const int64_t out0 = block_off * GA_FIT_PARAMS;
    for (int e = threadIdx.x; e < total * GA_FIT_PARAMS; e += kThreads) {
        const int r = e / GA_FIT_PARAMS, k = e - r * GA_FIT_PARAMS;
        const uint32_t s = src[r], kind = s >> 16;
        const int64_t gi = (int64_t)(base + (int)(s & 0xFFFFu)) * GA_FIT_PARAMS + k;
        float x = a.raw[gi];
        if (kind >= 2u && (k == 4 || k == 5)) x = x - GA_DENSIFY_LOG_1P6;
        if (!(kind >= 2u && k < 3)) a.out_raw[out0 + e] = x;            // a child's xyz is written by the lane that owns its parent
        a.out_m[out0 + e] = kind == 0u ? a.m[gi] : 0.f;
        a.out_v[out0 + e] = kind == 0u ? a.v[gi] : 0.f;
    }
}

__global__ __launch_bounds__(kThreads) void fit_reset_opacity_kernel(GaFitResetOpacityArgs a)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.num_points) return;
    const int64_t at = (int64_t)i * GA_FIT_PARAMS + 3;
    const float r = a.raw[at];
    a.raw[at] = r > a.logit_cap ? a.logit_cap : r;
    a.m[at] = 0.f;
    a.v[at] = 0.f;
}

static bool densify_n_ok(int32_t n) { return n >= 1 && n <= (1 << 30); }
static unsigned blocks_of(int32_t n, int per_block) { return (unsigned)(((int64_t)n + per_block - 1) / per_block); }

}  // namespace ga

extern "C" int ga_fit_accumulate(const GaFitAccumulateArgs *a, void *stream)
{
    if (!a || !a->g_means || !a->means || !a->radii || !a->view || !a->grad_accum || !a->denom || !a->max_radius) return GA_ERR_NULL_ARG;
    if (!ga::densify_n_ok(a->num_points) || a->num_views < 1 || a->num_views > 65535) return GA_ERR_BAD_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ga::fit_accumulate_kernel, dim3(ga::blocks_of(a->num_points, ga::kThreads)), dim3(ga::kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" size_t ga_densify_workspace_bytes(int32_t num_points)
{
    if (!ga::densify_n_ok(num_points)) return 0;
    return (size_t)ga::blocks_of(num_points, ga::kBlockRows) * 4 * sizeof(int32_t);
}

extern "C" int ga_densify(const GaDensifyArgs *a, void *stream)
{
    if (!a || !a->raw || !a->m || !a->v || !a->opacities || !a->scales || !a->rotations || !a->grad_accum || !a->denom ||
        !a->max_radius || !a->out_raw || !a->out_m || !a->out_v || !a->parent || !a->out_counts || !a->workspace)
        return GA_ERR_NULL_ARG;
    if (a->flags & ~GA_DENSIFY_PRUNE_ONLY) return GA_ERR_BAD_FLAGS;
    if (!ga::densify_n_ok(a->num_points)) return GA_ERR_BAD_SHAPE;
    if (a->workspace_bytes < ga_densify_workspace_bytes(a->num_points) || (reinterpret_cast<uintptr_t>(a->workspace) & 15) ||
        (a->noise_out && (reinterpret_cast<uintptr_t>(a->noise_out) & 15)))
        return GA_ERR_WORKSPACE;
    const unsigned blocks = ga::blocks_of(a->num_points, ga::kBlockRows);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipLaunchKernelGGL(ga::densify_count_kernel, dim3(blocks), dim3(ga::kThreads), 0, s, *a);
    hipLaunchKernelGGL(ga::densify_scan_kernel, dim3(1), dim3(ga::kThreads), 0, s, *a, (int)blocks);
    hipLaunchKernelGGL(ga::densify_scatter_kernel, dim3(blocks), dim3(ga::kThreads), 0, s, *a);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_fit_reset_opacity(const GaFitResetOpacityArgs *a, void *stream)
{
    if (!a || !a->raw || !a->m || !a->v) return GA_ERR_NULL_ARG;
    if (!ga::densify_n_ok(a->num_points)) return GA_ERR_BAD_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ga::fit_reset_opacity_kernel, dim3(ga::blocks_of(a->num_points, ga::kThreads)), dim3(ga::kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}
