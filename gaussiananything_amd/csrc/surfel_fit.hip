// surfel_fit.hip -- the glue of one surfel-fitting iteration (include/ga_fit.h): activation of the raw parameters into the five arrays
// ga_surfel_forward reads, the adjoint of the renderer's post-processing (the gradients of the two loss backwards packed into the
// grad_color / grad_others ga_surfel_backward reads), the chain rule to raw space fused with the Adam step, the advance of the
// device-side step counter, and the selection of the iteration's views from a pool on the device.  Five streaming kernels; with the
// existing forward, loss and backward launches they form one chain on one stream that a HIP graph replays once per iteration: nothing
// here takes a host value that changes between iterations.
//
// Built with -ffp-contract=off: the Adam step and the chain rule are bit-identical to the operation-by-operation restatement the tests
// hold them to (tests/_fit_ref.py); division and square root are hipcc's correctly rounded defaults.
//   activate  one lane per surfel: 13 floats in, 14 out
//   pack      one lane per 4 consecutive pixels of a view (1 when H*W % 4 != 0), as surfel_post.hip: up to 19 planes read, 10 written
//   adam      one lane per surfel: the row of the step table is table[*counter], read from the device
//   advance   one thread, a launch of its own behind adam: the history row, then ++*counter (clamped)
//   select    mini-batches only, the first launch: row *counter of the view schedule names the pool views copied into the batch buffers
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ga_fit.h"

namespace ga {

constexpr int kFitThreads = 256;

__device__ __forceinline__ float fit_sigmoid(float r) { return 1.f / (1.f + expf(-r)); }

__global__ __launch_bounds__(kFitThreads) void fit_activate_kernel(GaFitActivateArgs a)
{
    const int i = blockIdx.x * kFitThreads + threadIdx.x;
    if (i >= a.num_points) return;
    const float *r = a.raw + (int64_t)i * GA_FIT_PARAMS;
    float x[GA_FIT_PARAMS];
#pragma unroll
    for (int k = 0; k < GA_FIT_PARAMS; ++k) x[k] = r[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) a.means[(int64_t)i * 3 + k] = x[k];
    a.opacities[i] = fit_sigmoid(x[3]);
#pragma unroll
    for (int k = 0; k < 2; ++k) a.scales[(int64_t)i * 2 + k] = expf(x[4 + k]);
    const float norm = sqrtf(((x[6] * x[6] + x[7] * x[7]) + x[8] * x[8]) + x[9] * x[9]);
#pragma unroll
    for (int k = 0; k < 4; ++k) a.rotations[(int64_t)i * 4 + k] = x[6 + k] / norm;
    a.inv_norm[i] = 1.f / norm;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.colors[(int64_t)i * 3 + k] = fit_sigmoid(x[10 + k]);
}

template <int VEC>
__global__ __launch_bounds__(kFitThreads) void fit_pack_kernel(GaFitPackArgs a, int64_t P)
{
    const int v = blockIdx.y;
    const int64_t p = ((int64_t)blockIdx.x * kFitThreads + threadIdx.x) * VEC;
    if (p >= P) return;
    const float *vm = a.view + 16 * v;
    float R[3][3];   // R[d][c] = view[d,c]
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[d][c] = vm[4 * d + c];
    auto load = [&](const float *src, float (&dst)[VEC]) {
        if (src == nullptr) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) dst[e] = 0.f;
        } else if (VEC == 4) {
            const float4 t = *reinterpret_cast<const float4 *>(src);
            dst[0] = t.x; dst[1] = t.y; dst[2] = t.z; dst[VEC - 1] = t.w;
        } else {
            dst[0] = src[0];
        }
    };
    auto store = [&](float *dst, const float (&src)[VEC]) {
        if (VEC == 4) *reinterpret_cast<float4 *>(dst) = make_float4(src[0], src[1], src[2], src[VEC - 1]);
        else dst[0] = src[0];
    };
    auto at = [&](const float *base, int planes, int k) -> const float * {
        return base ? base + ((int64_t)v * planes + k) * P + p : nullptr;
    };
    float *gc = a.g_color + (int64_t)v * 3 * P + p, *ga_ = a.g_allmap + (int64_t)v * 7 * P + p;
    float o[VEC], t[VEC];
    // image = clamp(color, 0, 1): the gradient passes where 0 <= color <= 1 (torch's clamp backward; a NaN colour passes nothing)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        load(at(a.color, 3, k), t);
        load(at(a.g_image, 3, k), o);
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = (t[e] >= 0.f && t[e] <= 1.f) ? o[e] : 0.f;
        store(gc + k * P, o);
    }
    // channel 0 (mean depth) feeds nothing; channel 1 = alpha; channel 6 = dist.  (+ 0.f: the sum autograd forms with the zero
    // contributions of the other branches -- it turns a -0 into +0)
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = 0.f;
    store(ga_, o);
    load(at(a.g_alpha, 1, 0), o);
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = o[e] + 0.f;
    store(ga_ + P, o);
    load(at(a.g_dist, 1, 0), o);
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = o[e] + 0.f;
    store(ga_ + 6 * P, o);
    // rend_normal_d = sum_c allmap[2+c] view[d,c]  =>  g_allmap[2+c] = sum_d g_rend_normal_d view[d,c]
    float gn[3][VEC];
#pragma unroll
    for (int d = 0; d < 3; ++d) load(at(a.g_rend_normal, 3, d), gn[d]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int e = 0; e < VEC; ++e)   // accumulated as the batched GEMM behind autograd's einsum does: fused, d ascending
            o[e] = fmaf(gn[2][e], R[2][c], fmaf(gn[1][e], R[1][c], gn[0][e] * R[0][c])) + 0.f;
        store(ga_ + (2 + c) * P, o);
    }
    // depth = nan_to_num(allmap[5], 0, 0): grad * isfinite(allmap[5])
    load(at(a.allmap, 7, 5), t);
    load(at(a.g_depth, 1, 0), o);
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = o[e] * (isfinite(t[e]) ? 1.f : 0.f) + 0.f;
    store(ga_ + 5 * P, o);
}

__device__ __forceinline__ void fit_adam_one(const GaFitAdamArgs &a, float g, float step, float sbc2, float &raw, float &m, float &v)
{
    m = a.beta1 * m + a.one_minus_beta1 * g;
    v = a.beta2 * v + (a.one_minus_beta2 * g) * g;
    const float denom = sqrtf(v) / sbc2 + a.eps;
    raw = raw - step * (m / denom);
}

__global__ __launch_bounds__(kFitThreads) void fit_adam_kernel(GaFitAdamArgs a)
{
    const int i = blockIdx.x * kFitThreads + threadIdx.x;
    if (i >= a.num_points) return;
    int row = *a.counter;                       // the device-side step: the same word for every lane of the launch
    row = row < 0 ? 0 : (row >= a.max_steps ? a.max_steps - 1 : row);
    const float *tab = a.table + (int64_t)row * GA_FIT_TABLE_COLS;
    float g[GA_FIT_PARAMS];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = a.g_means[(int64_t)i * 3 + k];
    const float o = a.opacities[i];
    g[3] = a.g_opacities[i] * (o * (1.f - o));
#pragma unroll
    for (int k = 0; k < 2; ++k) g[4 + k] = a.g_scales[(int64_t)i * 2 + k] * a.scales[(int64_t)i * 2 + k];
    float q[4], gq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        q[k] = a.rotations[(int64_t)i * 4 + k];
        gq[k] = a.g_rotations[(int64_t)i * 4 + k];
    }
    const float dot = ((q[0] * gq[0] + q[1] * gq[1]) + q[2] * gq[2]) + q[3] * gq[3];
    const float inv = a.inv_norm[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) g[6 + k] = (gq[k] - q[k] * dot) * inv;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float c = a.colors[(int64_t)i * 3 + k];
        g[10 + k] = a.g_colors[(int64_t)i * 3 + k] * (c * (1.f - c));
    }
    if (a.raw_grad) {
#pragma unroll
        for (int k = 0; k < GA_FIT_PARAMS; ++k) a.raw_grad[(int64_t)i * GA_FIT_PARAMS + k] = g[k];
    }
    if (a.flags & GA_FIT_VISIBLE_ONLY) {
        bool seen = false;
        for (int vw = 0; vw < a.num_views; ++vw) seen = seen || a.radii[(int64_t)vw * a.num_points + i] != 0;
        if (!seen) return;
    }
    const float sbc2 = tab[GA_FIT_GROUPS];
    float *raw = a.raw + (int64_t)i * GA_FIT_PARAMS, *m = a.m + (int64_t)i * GA_FIT_PARAMS, *v = a.v + (int64_t)i * GA_FIT_PARAMS;
#pragma unroll
    for (int k = 0; k < GA_FIT_PARAMS; ++k) {
        const int group = k < 3 ? 0 : (k < 4 ? 1 : (k < 6 ? 2 : (k < 10 ? 3 : 4)));
        float r = raw[k], mm = m[k], vv = v[k];
        fit_adam_one(a, g[k], tab[group], sbc2, r, mm, vv);
        raw[k] = r;
        m[k] = mm;
        v[k] = vv;
    }
}

__global__ __launch_bounds__(64) void fit_advance_kernel(GaFitAdvanceArgs a)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int c = *a.counter;
    c = c < 0 ? 0 : (c >= a.max_steps ? a.max_steps - 1 : c);
    double term[6] = {(double)a.ssim_bias, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int v = 0; v < a.num_views; ++v)
        for (int k = 0; k < 3; ++k) {
            if (a.photo_out) term[k] += (double)a.w_photo[v * 3 + k] * (double)a.photo_out[v * 3 + k];
            if (a.geo_out) term[3 + k] += (double)a.w_geo[v * 3 + k] * (double)a.geo_out[v * 3 + k];
        }
    float *h = a.history + (int64_t)c * GA_FIT_HISTORY_COLS;
    double total = 0.0;
    for (int k = 0; k < 6; ++k) {
        total += term[k];
        h[1 + k] = (float)term[k];
    }
    h[0] = (float)total;
    h[7] = 0.f;
    *a.counter = c + 1 < a.max_steps ? c + 1 : a.max_steps - 1;
    if (a.status) {   // the status words belong to the last forward only: keep what a later, clean forward would wipe
        a.seen[0] |= a.status[GA_STATUS_OVERFLOW] != 0 ? 1 : 0;
        a.seen[1] = a.status[GA_STATUS_NUM_RENDERED] > a.seen[1] ? a.status[GA_STATUS_NUM_RENDERED] : a.seen[1];
        a.seen[2] = a.status[GA_STATUS_SEG_WORK] > a.seen[2] ? a.status[GA_STATUS_SEG_WORK] : a.seen[2];
    }
}

constexpr int kSelectMaxBlocks = 2048;   // a streaming copy: enough workgroups to fill the device, the rest of the work grid-strided

template <int VEC> struct SelectUnit { typedef uint32_t type; };
template <> struct SelectUnit<4> { typedef uint4 type; };

// The views of iteration *counter, from the pool into the buffers the rest of the chain reads.  blockIdx.y strides over the slots of the
// batch, blockIdx.x over the units (VEC elements) of a slot: its three target planes, then its mask, then its three normal planes.  The
// first workgroup of a slot also moves the two camera matrices and the index.  Integer moves: no float operation touches an fp32 value.
template <int VEC, bool U8>
__global__ __launch_bounds__(kFitThreads) void fit_select_kernel(GaFitSelectArgs a, int64_t hw)
{
    typedef typename SelectUnit<VEC>::type unit_t;
    int t = *a.counter;                         // the device-side step: the same word for every lane of the launch
    t = t < 0 ? 0 : (t >= a.max_steps ? a.max_steps - 1 : t);
    const int32_t *row = a.schedule + (int64_t)t * a.batch_views;
    const int64_t q = hw / VEC;                 // units per plane
    const int64_t n_targets = 3 * q, n_mask = a.pool_mask ? q : 0, n_normal = a.pool_normal ? 3 * q : 0;
    const int64_t units = n_targets + n_mask + n_normal;
    const int64_t stride = (int64_t)gridDim.x * kFitThreads;
    for (int b = blockIdx.y; b < a.batch_views; b += gridDim.y) {
        int p = row[b];
        p = p < 0 ? 0 : (p >= a.pool_views ? a.pool_views - 1 : p);   // the host validates the table; this only keeps the reads inside the pool
        if (blockIdx.x == 0) {
            const int k = threadIdx.x & 15;
            if (threadIdx.x < 16)
                reinterpret_cast<uint32_t *>(a.view)[(int64_t)b * 16 + k] = reinterpret_cast<const uint32_t *>(a.pool_view)[(int64_t)p * 16 + k];
            else if (threadIdx.x < 32)
                reinterpret_cast<uint32_t *>(a.proj)[(int64_t)b * 16 + k] = reinterpret_cast<const uint32_t *>(a.pool_proj)[(int64_t)p * 16 + k];
            else if (threadIdx.x == 32 && a.selected)
                a.selected[b] = p;
        }
        for (int64_t u = (int64_t)blockIdx.x * kFitThreads + threadIdx.x; u < units; u += stride) {
            if (u < n_targets) {
                unit_t *dst = reinterpret_cast<unit_t *>(a.targets) + (int64_t)b * n_targets + u;
                if (U8) {
                    const uint8_t *src = static_cast<const uint8_t *>(a.pool_targets) + ((int64_t)p * n_targets + u) * VEC;
                    float f[VEC];
                    if (VEC == 4) {
                        const uint32_t w = *reinterpret_cast<const uint32_t *>(src);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) f[e] = (float)((w >> (8 * e)) & 255u) / 255.0f;
                    } else {
                        f[0] = (float)src[0] / 255.0f;
                    }
                    float *d = reinterpret_cast<float *>(dst);
                    if (VEC == 4) *reinterpret_cast<float4 *>(d) = make_float4(f[0], f[1], f[2], f[VEC - 1]);
                    else d[0] = f[0];
                } else {
                    *dst = (static_cast<const unit_t *>(a.pool_targets) + (int64_t)p * n_targets)[u];
                }
            } else if (u < n_targets + n_mask) {
                const int64_t r = u - n_targets;
                (reinterpret_cast<unit_t *>(a.mask) + (int64_t)b * n_mask)[r] = (reinterpret_cast<const unit_t *>(a.pool_mask) + (int64_t)p * n_mask)[r];
            } else {
                const int64_t r = u - n_targets - n_mask;
                (reinterpret_cast<unit_t *>(a.normal) + (int64_t)b * n_normal)[r] =
                    (reinterpret_cast<const unit_t *>(a.pool_normal) + (int64_t)p * n_normal)[r];
            }
        }
    }
}

static bool fit_shape_ok(int32_t n, int32_t v, int32_t h, int32_t w)
{
    return n >= 1 && v >= 1 && v <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31) &&
           (int64_t)n * GA_FIT_PARAMS < ((int64_t)1 << 40);
}

}  // namespace ga

extern "C" int ga_fit_plan(int32_t n, int32_t v, int32_t h, int32_t w, GaFitPlan *pl)
{
    if (!pl) return GA_ERR_NULL_ARG;
    if (!ga::fit_shape_ok(n, v, h, w)) return GA_ERR_BAD_SHAPE;
    const int64_t P = (int64_t)h * w;
    pl->threads = ga::kFitThreads;
    pl->pack_vec = P % 4 == 0 ? 4 : 1;
    pl->grid_activate = pl->grid_adam = (int32_t)(((int64_t)n + ga::kFitThreads - 1) / ga::kFitThreads);
    pl->grid_pack_x = (int32_t)((P / pl->pack_vec + ga::kFitThreads - 1) / ga::kFitThreads);
    pl->grid_pack_y = v;
    size_t at = 0;
    auto section = [&](size_t floats) {
        const size_t here = at;
        at += (floats * sizeof(float) + 255) / 256 * 256;
        return here;
    };
    pl->means = section((size_t)n * 3);
    pl->opacities = section((size_t)n);
    pl->colors = section((size_t)n * 3);
    pl->scales = section((size_t)n * 2);
    pl->rotations = section((size_t)n * 4);
    pl->inv_norm = section((size_t)n);
    pl->workspace_bytes = at;
    return GA_OK;
}

extern "C" int ga_fit_activate(const GaFitActivateArgs *a, void *stream)
{
    if (!a || !a->raw || !a->means || !a->opacities || !a->colors || !a->scales || !a->rotations || !a->inv_norm) return GA_ERR_NULL_ARG;
    GaFitPlan pl;
    if (ga_fit_plan(a->num_points, 1, 1, 1, &pl) != GA_OK) return GA_ERR_BAD_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ga::fit_activate_kernel, dim3((unsigned)pl.grid_activate), dim3((unsigned)pl.threads), 0,
                       reinterpret_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_fit_pack_grads(const GaFitPackArgs *a, void *stream)
{
    if (!a || !a->color || !a->allmap || !a->view || !a->g_color || !a->g_allmap) return GA_ERR_NULL_ARG;
    GaFitPlan pl;
    if (ga_fit_plan(1, a->num_views, a->height, a->width, &pl) != GA_OK) return GA_ERR_BAD_SHAPE;
    const int64_t P = (int64_t)a->height * a->width;
    // the 16-byte accesses of the plan need 16-byte aligned planes: a buffer that is not (a view into a larger tensor) takes the
    // one-pixel kernel
    uintptr_t bits = 0;
    for (const void *p : {(const void *)a->color, (const void *)a->allmap, (const void *)a->g_image, (const void *)a->g_rend_normal,
                          (const void *)a->g_depth, (const void *)a->g_dist, (const void *)a->g_alpha, (const void *)a->g_color,
                          (const void *)a->g_allmap})
        bits |= reinterpret_cast<uintptr_t>(p);
    const bool vec4 = pl.pack_vec == 4 && (bits & 15) == 0;
    const dim3 grid(vec4 ? (unsigned)pl.grid_pack_x : (unsigned)((P + pl.threads - 1) / pl.threads), (unsigned)pl.grid_pack_y);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (vec4) hipLaunchKernelGGL((ga::fit_pack_kernel<4>), grid, dim3((unsigned)pl.threads), 0, s, *a, P);
    else hipLaunchKernelGGL((ga::fit_pack_kernel<1>), grid, dim3((unsigned)pl.threads), 0, s, *a, P);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_fit_adam(const GaFitAdamArgs *a, void *stream)
{
    if (!a || !a->g_means || !a->g_opacities || !a->g_colors || !a->g_scales || !a->g_rotations || !a->opacities || !a->colors ||
        !a->scales || !a->rotations || !a->inv_norm || !a->raw || !a->m || !a->v || !a->table || !a->counter)
        return GA_ERR_NULL_ARG;
    if (a->flags & ~GA_FIT_VISIBLE_ONLY) return GA_ERR_BAD_FLAGS;
    if ((a->flags & GA_FIT_VISIBLE_ONLY) && !a->radii) return GA_ERR_NULL_ARG;
    GaFitPlan pl;
    if (a->max_steps < 1 || ga_fit_plan(a->num_points, a->num_views, 1, 1, &pl) != GA_OK) return GA_ERR_BAD_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ga::fit_adam_kernel, dim3((unsigned)pl.grid_adam), dim3((unsigned)pl.threads), 0,
                       reinterpret_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_fit_select_views(const GaFitSelectArgs *a, void *stream)
{
    if (!a || !a->schedule || !a->counter || !a->pool_view || !a->pool_proj || !a->pool_targets || !a->view || !a->proj || !a->targets)
        return GA_ERR_NULL_ARG;
    if ((a->pool_mask == nullptr) != (a->mask == nullptr) || (a->pool_normal == nullptr) != (a->normal == nullptr)) return GA_ERR_NULL_ARG;
    if (a->flags & ~GA_FIT_SELECT_U8_TARGETS) return GA_ERR_BAD_FLAGS;
    if (a->pool_views < 1 || a->batch_views < 1 || a->batch_views > a->pool_views || a->height < 1 || a->width < 1 || a->max_steps < 1 ||
        (int64_t)a->height * a->width >= ((int64_t)1 << 31))
        return GA_ERR_BAD_SHAPE;
    const int64_t hw = (int64_t)a->height * a->width;
    // as ga_fit_pack_grads: 16 bytes per lane need whole planes of 4 elements and 16-byte aligned buffers (a view into a larger tensor
    // may not be); otherwise one element per lane
    uintptr_t bits = 0;
    for (const void *p : {(const void *)a->pool_view, (const void *)a->pool_proj, a->pool_targets, (const void *)a->pool_mask,
                          (const void *)a->pool_normal, (const void *)a->view, (const void *)a->proj, (const void *)a->targets,
                          (const void *)a->mask, (const void *)a->normal})
        bits |= reinterpret_cast<uintptr_t>(p);
    const bool vec4 = hw % 4 == 0 && (bits & 15) == 0;
    const bool u8 = (a->flags & GA_FIT_SELECT_U8_TARGETS) != 0;
    const int64_t units = (hw / (vec4 ? 4 : 1)) * (3 + (a->pool_mask ? 1 : 0) + (a->pool_normal ? 3 : 0));
    const int64_t gy = a->batch_views < ga::kSelectMaxBlocks ? a->batch_views : ga::kSelectMaxBlocks;
    const int64_t want = (units + ga::kFitThreads - 1) / ga::kFitThreads, cap = ga::kSelectMaxBlocks / gy;
    const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)gy), block((unsigned)ga::kFitThreads);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (vec4 && u8) hipLaunchKernelGGL((ga::fit_select_kernel<4, true>), grid, block, 0, s, *a, hw);
    else if (vec4) hipLaunchKernelGGL((ga::fit_select_kernel<4, false>), grid, block, 0, s, *a, hw);
    else if (u8) hipLaunchKernelGGL((ga::fit_select_kernel<1, true>), grid, block, 0, s, *a, hw);
    else hipLaunchKernelGGL((ga::fit_select_kernel<1, false>), grid, block, 0, s, *a, hw);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_fit_advance(const GaFitAdvanceArgs *a, void *stream)
{
    if (!a || !a->counter || !a->history) return GA_ERR_NULL_ARG;
    if ((a->photo_out && !a->w_photo) || (a->geo_out && !a->w_geo) || (a->status && !a->seen)) return GA_ERR_NULL_ARG;
    if (a->num_views < 1 || a->num_views > 65535 || a->max_steps < 1) return GA_ERR_BAD_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ga::fit_advance_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}
