// photo_loss.hip -- fused SSIM + L1 + L2 of two image batches, forward and backward (include/ga_loss.h).
//
// One workgroup of 256 lanes owns one 32 x 32 tile of one (n, c) plane.  It stages the 42 x 42 halo of its inputs in LDS (zero outside
// the image: the reference's zero padding), runs the 11-tap window over the rows into LDS and over the columns into registers.  Each
// lane of the row pass produces 4 adjacent columns from 14 staged values, each lane of the column pass 4 adjacent rows from 14 row
// results: 3.5 LDS reads per tap-sum and moment where the plain form needs 11.
//
// LDS images.  The halo has a row stride of 43 floats: the 32 lanes of a half wave in the row pass are 4 rows x 8 column groups, their
// addresses r * 43 + 4 g + j fall on 32 different banks (43 mod 4 = 3 walks the rows over the four residues).  The row results have a
// row stride of 32 floats, are written as one 16-byte store per lane and moment and read by 32 lanes of consecutive columns.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ga_loss.h"

namespace {

constexpr int kTile = 32;                 // output tile, both ways
constexpr int kTaps = GA_PHOTO_LOSS_WINDOW;
constexpr int kRad = kTaps / 2;
constexpr int kHalo = kTile + kTaps - 1;  // 42
constexpr int kHaloStride = kHalo + 1;    // 43: see 'LDS images'
constexpr int kThreads = 256;
constexpr int kRowItems = kHalo * (kTile / 4);   // row pass: (halo row, group of 4 columns)
constexpr float kC1 = 0.01f * 0.01f;
constexpr float kC2 = 0.03f * 0.03f;

#include "loss_reduce.h"   // block_sum3, loss_reduce_kernel (shared with geo_loss.hip)

struct Window {
    float w[kTaps];
};

// the reference's `gaussian(11, 1.5)`: the taps in double, rounded to fp32, divided by their fp32 sum.  torch's sum of these eleven
// values is the correctly rounded one (a lane-by-lane fp32 loop lands one ulp lower, which shifts every weight and biases the
// variances of a flat image), so the sum is taken in double and rounded once: the weights then have torch's bits.
Window make_window() {
    Window win;
    double sum = 0.0;
    for (int k = 0; k < kTaps; ++k) {
        win.w[k] = (float)exp(-(double)((k - kRad) * (k - kRad)) / (2.0 * 1.5 * 1.5));
        sum += (double)win.w[k];
    }
    for (int k = 0; k < kTaps; ++k) win.w[k] = win.w[k] / (float)sum;
    return win;
}

// the forward kernel's LDS, one object so that the plan can report its size
struct ForwardLds {
    __attribute__((aligned(16))) float rows[5][kHalo * kTile];   // row pass of x, y, x*x, y*y, x*y
    float hx[kHalo * kHaloStride];
    float hy[kHalo * kHaloStride];
    double red[3 * (kThreads / 64)];
};

struct TileCoord {
    size_t plane_off;  // first element of the (n, c) plane
    int image;         // n
    int y0, x0;        // first pixel of the tile
};

__device__ __forceinline__ TileCoord tile_coord(int C, int H, int W, int tiles_x, int tiles_y) {
    const unsigned tpp = (unsigned)(tiles_x * tiles_y);
    const unsigned wg = blockIdx.x;
    const unsigned plane = wg / tpp, t = wg - plane * tpp;
    TileCoord tc;
    tc.plane_off = (size_t)plane * (size_t)H * (size_t)W;
    tc.image = (int)(plane / (unsigned)C);
    tc.y0 = (int)(t / (unsigned)tiles_x) * kTile;
    tc.x0 = (int)(t % (unsigned)tiles_x) * kTile;
    return tc;
}

// halo of one plane into LDS, zero outside the image
__device__ __forceinline__ void stage_halo(float *dst, const float *__restrict__ src, const TileCoord &tc, int H, int W) {
    for (int i = threadIdx.x; i < kHalo * kHalo; i += kThreads) {
        const int r = i / kHalo, c = i - r * kHalo;
        const int gy = tc.y0 - kRad + r, gx = tc.x0 - kRad + c;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = src[tc.plane_off + (size_t)gy * W + gx];
        dst[r * kHaloStride + c] = v;
    }
}

// column pass of one moment for the lane's 4 rows: rowbuf is [kHalo][kTile]
__device__ __forceinline__ void column_pass(const float *rowbuf, int px, int py0, const Window &win, float out[4]) {
    float v[kTaps + 3];
#pragma unroll
    for (int i = 0; i < kTaps + 3; ++i) v[i] = rowbuf[(py0 + i) * kTile + px];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) a = fmaf(win.w[k], v[j + k], a);
        out[j] = a;
    }
}

struct PixelSsim {
    float S, d_mu, d_e11, d_e12;
};

// S and its derivatives from the five moments.  Contraction is off here: every product and sum is rounded on its own, so S has the
// same bits whether or not the derivative maps are wanted (a forward-only loss equals the one that is differentiated).
template <bool SAVE>
__device__ __forceinline__ PixelSsim pixel_ssim(float m1, float m2, float e11, float e22, float e12) {
#pragma clang fp contract(off)
    const float m1m2 = m1 * m2, m1sq = m1 * m1, m2sq = m2 * m2;
    const float s11 = e11 - m1sq, s22 = e22 - m2sq, s12 = e12 - m1m2;
    const float A1 = 2.f * m1m2 + kC1, A2 = 2.f * s12 + kC2;
    const float B1 = m1sq + m2sq + kC1, B2 = s11 + s22 + kC2;
    PixelSsim p;
    p.S = (A1 * A2) / (B1 * B2);
    p.d_mu = p.d_e11 = p.d_e12 = 0.f;
    if (SAVE) {
        const float inv = 1.f / (B1 * B2);
        const float a1_inv = A1 * inv;                 // A1 / (B1 B2)
        p.d_e11 = -(p.S / B2);
        p.d_e12 = 2.f * a1_inv;
        p.d_mu = 2.f * m2 * (A2 * inv - a1_inv) + 2.f * m1 * p.S * (1.f / B2 - 1.f / B1);
    }
    return p;
}

template <bool SAVE>
__global__ __launch_bounds__(kThreads) void photo_loss_forward_kernel(const float *__restrict__ img1, const float *__restrict__ img2,
                                                                      float *__restrict__ ssim_map, float *__restrict__ partials,
                                                                      float *__restrict__ d_mu, float *__restrict__ d_e11,
                                                                      float *__restrict__ d_e12, int C, int H, int W, int tiles_x,
                                                                      int tiles_y, Window win) {
    __shared__ ForwardLds lds;
    float *hx = lds.hx, *hy = lds.hy;
    float(*rows)[kHalo * kTile] = lds.rows;
    double *red = lds.red;

    const TileCoord tc = tile_coord(C, H, W, tiles_x, tiles_y);
    stage_halo(hx, img1, tc, H, W);
    stage_halo(hy, img2, tc, H, W);
    __syncthreads();

    // row pass: x, y, x*x, y*y, x*y
    for (int i = threadIdx.x; i < kRowItems; i += kThreads) {
        const int r = i >> 3, g = i & 7;
        float x[kTaps + 3], y[kTaps + 3];
#pragma unroll
        for (int k = 0; k < kTaps + 3; ++k) {
            x[k] = hx[r * kHaloStride + 4 * g + k];
            y[k] = hy[r * kHaloStride + 4 * g + k];
        }
        float m[5][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const float w = win.w[k], xv = x[j + k], yv = y[j + k];
                const float wx = w * xv, wy = w * yv;
                a0 += wx;
                a1 += wy;
                a2 = fmaf(wx, xv, a2);
                a3 = fmaf(wy, yv, a3);
                a4 = fmaf(wx, yv, a4);
            }
            m[0][j] = a0; m[1][j] = a1; m[2][j] = a2; m[3][j] = a3; m[4][j] = a4;
        }
#pragma unroll
        for (int q = 0; q < 5; ++q)
            *reinterpret_cast<float4 *>(&rows[q][r * kTile + 4 * g]) = make_float4(m[q][0], m[q][1], m[q][2], m[q][3]);
    }
    __syncthreads();

    // column pass and the per-pixel values: the lane owns column px, rows py0 .. py0 + 3 of the tile
    const int px = threadIdx.x & (kTile - 1), py0 = (threadIdx.x >> 5) * 4;
    float mu1[4], mu2[4], e11[4], e22[4], e12[4];
    column_pass(rows[0], px, py0, win, mu1);
    column_pass(rows[1], px, py0, win, mu2);
    column_pass(rows[2], px, py0, win, e11);
    column_pass(rows[3], px, py0, win, e22);
    column_pass(rows[4], px, py0, win, e12);

    float sum_s = 0.f, sum_l1 = 0.f, sum_l2 = 0.f;
    const int gx = tc.x0 + px;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gy = tc.y0 + py0 + j;
        if (gx < W && gy < H) {
            const size_t o = tc.plane_off + (size_t)gy * W + gx;
            const PixelSsim p = pixel_ssim<SAVE>(mu1[j], mu2[j], e11[j], e22[j], e12[j]);
            const float S = p.S;
            if (ssim_map) ssim_map[o] = S;
            if (SAVE) {
                d_e11[o] = p.d_e11;
                d_e12[o] = p.d_e12;
                d_mu[o] = p.d_mu;
            }
            const float d = hx[(py0 + j + kRad) * kHaloStride + px + kRad] - hy[(py0 + j + kRad) * kHaloStride + px + kRad];
            sum_s += S;
            sum_l1 += fabsf(d);
            sum_l2 = fmaf(d, d, sum_l2);
        }
    }
    double v[3] = {(double)sum_s, (double)sum_l1, (double)sum_l2};
    block_sum3(v, red);
    if (threadIdx.x == 0) {
        float *p = partials + (size_t)blockIdx.x * 3;
        p[0] = (float)v[0];
        p[1] = (float)v[1];
        p[2] = (float)v[2];
    }
}

__global__ __launch_bounds__(kThreads) void photo_loss_backward_kernel(const float *__restrict__ img1, const float *__restrict__ img2,
                                                                       const float *__restrict__ d_mu, const float *__restrict__ d_e11,
                                                                       const float *__restrict__ d_e12,
                                                                       const float *__restrict__ grad_out, float *__restrict__ grad_img1,
                                                                       int C, int H, int W, int tiles_x, int tiles_y, float inv_count,
                                                                       Window win) {
    __shared__ float halo[3][kHalo * kHaloStride];
    __shared__ __attribute__((aligned(16))) float rows[3][kHalo * kTile];

    const TileCoord tc = tile_coord(C, H, W, tiles_x, tiles_y);
    stage_halo(halo[0], d_mu, tc, H, W);
    stage_halo(halo[1], d_e11, tc, H, W);
    stage_halo(halo[2], d_e12, tc, H, W);
    __syncthreads();

    for (int i = threadIdx.x; i < kRowItems; i += kThreads) {
        const int r = i >> 3, g = i & 7;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float v[kTaps + 3];
#pragma unroll
            for (int k = 0; k < kTaps + 3; ++k) v[k] = halo[q][r * kHaloStride + 4 * g + k];
            float m[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < kTaps; ++k) a = fmaf(win.w[k], v[j + k], a);
                m[j] = a;
            }
            *reinterpret_cast<float4 *>(&rows[q][r * kTile + 4 * g]) = make_float4(m[0], m[1], m[2], m[3]);
        }
    }
    __syncthreads();

    const int px = threadIdx.x & (kTile - 1), py0 = (threadIdx.x >> 5) * 4;
    float c_mu[4], c_e11[4], c_e12[4];
    column_pass(rows[0], px, py0, win, c_mu);
    column_pass(rows[1], px, py0, win, c_e11);
    column_pass(rows[2], px, py0, win, c_e12);

    const float gs = grad_out[(size_t)tc.image * 3 + 0] * inv_count;
    const float g1 = grad_out[(size_t)tc.image * 3 + 1] * inv_count;
    const float g2 = grad_out[(size_t)tc.image * 3 + 2] * inv_count;
    const int gx = tc.x0 + px;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gy = tc.y0 + py0 + j;
        if (gx < W && gy < H) {
            const size_t o = tc.plane_off + (size_t)gy * W + gx;
            const float x = img1[o], y = img2[o];
            const float d = x - y;
            const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            const float ds = c_mu[j] + 2.f * x * c_e11[j] + y * c_e12[j];
            grad_img1[o] = gs * ds + g1 * sgn + g2 * (2.f * d);
        }
    }
}

bool shape_ok(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N < 1 || C < 1 || H < 1 || W < 1 || H > GA_PHOTO_LOSS_MAX_SIDE || W > GA_PHOTO_LOSS_MAX_SIDE) return false;
    const int64_t tiles = (int64_t)((H + kTile - 1) / kTile) * ((W + kTile - 1) / kTile);   // <= 2^22
    const int64_t planes = (int64_t)N * C;                                                  // < 2^62
    return planes < ((int64_t)1 << 31) && planes * tiles < ((int64_t)1 << 31);             // the grid; C * tiles is below it
}

size_t partial_bytes(const GaPhotoLossPlan &pl) { return ((size_t)pl.num_partials * 4 + 255) / 256 * 256; }

int check_args(const GaPhotoLossArgs *a, GaPhotoLossPlan *pl) {
    if (!a) return GA_ERR_NULL_ARG;
    if (a->flags & ~GA_PHOTO_LOSS_SAVE) return GA_ERR_BAD_FLAGS;
    const int rc = ga_photo_loss_plan(a->num_images, a->channels, a->height, a->width, pl);
    if (rc != GA_OK) return rc;
    if (!a->img1 || !a->img2 || !a->workspace) return GA_ERR_NULL_ARG;
    if (a->workspace_bytes < ga_photo_loss_workspace_bytes(a->num_images, a->channels, a->height, a->width, a->flags))
        return GA_ERR_WORKSPACE;
    return GA_OK;
}

}  // namespace

extern "C" int ga_photo_loss_plan(int32_t N, int32_t C, int32_t H, int32_t W, GaPhotoLossPlan *plan) {
    if (!plan) return GA_ERR_NULL_ARG;
    if (!shape_ok(N, C, H, W)) return GA_ERR_BAD_SHAPE;
    plan->tile_w = kTile;
    plan->tile_h = kTile;
    plan->threads = kThreads;
    plan->tiles_x = (W + kTile - 1) / kTile;
    plan->tiles_y = (H + kTile - 1) / kTile;
    plan->lds_bytes = (int32_t)sizeof(ForwardLds);
    plan->grid_x = (int64_t)N * C * plan->tiles_x * plan->tiles_y;
    plan->num_partials = plan->grid_x * 3;
    return GA_OK;
}

extern "C" size_t ga_photo_loss_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t flags) {
    GaPhotoLossPlan pl;
    if (ga_photo_loss_plan(N, C, H, W, &pl) != GA_OK) return 0;
    size_t bytes = partial_bytes(pl);
    if (flags & GA_PHOTO_LOSS_SAVE) bytes += (size_t)3 * 4 * (size_t)N * C * H * W;
    return bytes;
}

extern "C" int ga_photo_loss_forward(const GaPhotoLossArgs *a, void *stream_v) {
    GaPhotoLossPlan pl;
    const int rc = check_args(a, &pl);
    if (rc != GA_OK) return rc;
    if (!a->out) return GA_ERR_NULL_ARG;
    static const Window win = make_window();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    const size_t count = (size_t)a->num_images * a->channels * a->height * a->width;
    float *partials = reinterpret_cast<float *>(a->workspace);
    float *maps = reinterpret_cast<float *>(reinterpret_cast<char *>(a->workspace) + partial_bytes(pl));
    (void)hipGetLastError();
    if (a->flags & GA_PHOTO_LOSS_SAVE)
        hipLaunchKernelGGL(photo_loss_forward_kernel<true>, dim3((unsigned)pl.grid_x), dim3(kThreads), 0, s, a->img1, a->img2, a->ssim_map,
                           partials, maps, maps + count, maps + 2 * count, a->channels, a->height, a->width, pl.tiles_x, pl.tiles_y, win);
    else
        hipLaunchKernelGGL(photo_loss_forward_kernel<false>, dim3((unsigned)pl.grid_x), dim3(kThreads), 0, s, a->img1, a->img2, a->ssim_map,
                           partials, (float *)nullptr, (float *)nullptr, (float *)nullptr, a->channels, a->height, a->width, pl.tiles_x,
                           pl.tiles_y, win);
    const int per_image = a->channels * pl.tiles_x * pl.tiles_y;
    hipLaunchKernelGGL(loss_reduce_kernel, dim3((unsigned)a->num_images), dim3(kReduceThreads), 0, s, partials, a->out, per_image,
                       1.0 / ((double)a->channels * a->height * a->width));
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_photo_loss_backward(const GaPhotoLossArgs *a, void *stream_v) {
    GaPhotoLossPlan pl;
    const int rc = check_args(a, &pl);
    if (rc != GA_OK) return rc;
    if (!(a->flags & GA_PHOTO_LOSS_SAVE)) return GA_ERR_BAD_FLAGS;
    if (!a->grad_out || !a->grad_img1) return GA_ERR_NULL_ARG;
    static const Window win = make_window();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    const size_t count = (size_t)a->num_images * a->channels * a->height * a->width;
    const float *maps = reinterpret_cast<const float *>(reinterpret_cast<const char *>(a->workspace) + partial_bytes(pl));
    (void)hipGetLastError();
    hipLaunchKernelGGL(photo_loss_backward_kernel, dim3((unsigned)pl.grid_x), dim3(kThreads), 0, s, a->img1, a->img2, maps, maps + count,
                       maps + 2 * count, a->grad_out, a->grad_img1, a->channels, a->height, a->width, pl.tiles_x, pl.tiles_y,
                       (float)(1.0 / ((double)a->channels * a->height * a->width)), win);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}
