// geo_loss.hip -- geometry losses of a 2D-surfel render: pseudo surface normals of the depth map, the normal-consistency term, the mean
// of the distortion map and the L1 of alpha against a mask, forward and backward (include/ga_loss.h).
//
// One workgroup of 256 lanes owns one 32 x 32 tile of one view; a lane owns one column of the tile and 4 adjacent rows, so every global
// load and store of a wave is two runs of 32 consecutive floats.  The depth of the tile is staged in LDS with a halo of 1 (forward) or
// 2 (backward), zero outside the image; a normal needs the four neighbours of its pixel and never the centre.
//
// Backward.  The depth of pixel p enters the normals of its four neighbours.  Phase 1 walks the tile with a halo of 1 (34 x 34 pixels q),
// recomputes the cross product of q, pulls the gradient of q's normal back to q's four neighbour depths and leaves those four numbers
// in LDS; phase 2 lets p pick up the one number each neighbour holds for it, in a fixed order.  A gather: no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ga_loss.h"

namespace {

constexpr int kTile = 32;
constexpr int kThreads = 256;
constexpr int kFwdSide = kTile + 2;   // depth with a halo of 1
constexpr int kBwdSide = kTile + 4;   // depth with a halo of 2
constexpr int kPullSide = kTile + 2;  // pulled-back gradients with a halo of 1
constexpr float kEps = 1e-12f;        // F.normalize

#include "loss_reduce.h"   // block_sum3, loss_reduce_kernel (shared with photo_loss.hip)

enum Mode { kFromDepth = 0, kTarget = 1, kNormals = 2 };

struct Params {
    int H, W, tiles_x, tiles_y;
    float ifx, ify, half_w, half_h;   // 2 tanfov / W, 2 tanfov / H, W / 2, H / 2
    float inv_count;                  // 1 / (H W)
    const float *view, *rend_normal, *depth, *alpha, *dist, *target_normal, *mask, *grad_out;
    float *surf_normal_out, *partials, *grad_rend_normal, *grad_depth, *grad_dist, *grad_alpha;
};

struct ForwardLds {
    float depth[kFwdSide * kFwdSide];
    double red[3 * (kThreads / 64)];
};

struct BackwardLds {
    float depth[kBwdSide * kBwdSide];
    float pull[4][kPullSide * kPullSide];   // d loss / d depth of q's north, south, west, east neighbour through q's normal
};

struct TileCoord {
    size_t view_off;   // first pixel of the view in a one-channel map
    int view;
    int y0, x0;
};

__device__ __forceinline__ TileCoord tile_coord(const Params &p) {
    const unsigned tpv = (unsigned)(p.tiles_x * p.tiles_y);
    const unsigned wg = blockIdx.x;
    const unsigned v = wg / tpv, t = wg - v * tpv;
    TileCoord tc;
    tc.view = (int)v;
    tc.view_off = (size_t)v * (size_t)p.H * (size_t)p.W;
    tc.y0 = (int)(t / (unsigned)p.tiles_x) * kTile;
    tc.x0 = (int)(t % (unsigned)p.tiles_x) * kTile;
    return tc;
}

// depth of the tile with a halo of HALO into LDS, zero outside the image
template <int HALO>
__device__ __forceinline__ void stage_depth(float *dst, const Params &p, const TileCoord &tc) {
    constexpr int side = kTile + 2 * HALO;
    for (int i = threadIdx.x; i < side * side; i += kThreads) {
        const int r = i / side, c = i - r * side;
        const int gy = tc.y0 - HALO + r, gx = tc.x0 - HALO + c;
        float v = 0.f;
        if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) v = p.depth[tc.view_off + (size_t)gy * p.W + gx];
        dst[i] = v;
    }
}

struct Rot {
    float m[3][3];   // camera to world
};

__device__ __forceinline__ Rot load_rot(const float *view, int v) {
    Rot R;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R.m[i][j] = view[(size_t)v * 16 + 4 * i + j];
    return R;
}

// the cross product of pixel (gy, gx) from its four neighbour depths (ga_loss.h, 'cross') and what the backward needs of it
struct Cross {
    float dv, dh, p, q, u, v;   // differences, scaled sums, the pixel's ray
    float cx, cy, cz, len;
};

__device__ __forceinline__ Cross cross_at(float dN, float dS, float dW, float dE, int gy, int gx, const Params &p) {
    Cross k;
    k.u = ((float)gx - p.half_w) * p.ifx;
    k.v = ((float)gy - p.half_h) * p.ify;
    k.dv = dS - dN;
    k.dh = dE - dW;
    k.p = (dS + dN) * p.ify;
    k.q = (dE + dW) * p.ifx;
    k.cx = k.p * k.dh;
    k.cy = k.q * k.dv;
    k.cz = -(k.v * k.dv * k.q + k.u * k.dh * k.p + k.p * k.q);
    k.len = sqrtf(k.cx * k.cx + k.cy * k.cy + k.cz * k.cz);
    return k;
}

__device__ __forceinline__ void world_normal(const Cross &k, const Rot &R, float n[3]) {
    const float d = fmaxf(k.len, kEps);
    const float nx = k.cx / d, ny = k.cy / d, nz = k.cz / d;
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = R.m[i][0] * nx + R.m[i][1] * ny + R.m[i][2] * nz;
}

__device__ __forceinline__ bool interior(int gy, int gx, const Params &p) { return gy >= 1 && gy < p.H - 1 && gx >= 1 && gx < p.W - 1; }

// the s of the normal term at an in-image pixel: n alpha from the staged depth (centre at LDS row lr, column lc of a `side`-wide image),
// or target_normal mask
template <int MODE>
__device__ __forceinline__ void surf_normal_at(const float *lds_depth, int side, int lr, int lc, int gy, int gx, size_t pix, size_t o3,
                                               size_t hw, const Params &p, const Rot &R, float alpha, float s[3]) {
    if (MODE == kTarget) {
        const float m = p.mask ? p.mask[pix] : 1.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = p.target_normal[o3 + c * hw] * m;
        return;
    }
    s[0] = s[1] = s[2] = 0.f;
    if (interior(gy, gx, p)) {
        const Cross k = cross_at(lds_depth[(lr - 1) * side + lc], lds_depth[(lr + 1) * side + lc], lds_depth[lr * side + lc - 1],
                                 lds_depth[lr * side + lc + 1], gy, gx, p);
        world_normal(k, R, s);
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] *= alpha;
    }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void geo_loss_forward_kernel(Params p) {
    __shared__ ForwardLds lds;
    const TileCoord tc = tile_coord(p);
    Rot R = {};
    if (MODE != kTarget) {
        R = load_rot(p.view, tc.view);
        stage_depth<1>(lds.depth, p, tc);
        __syncthreads();
    }
    const int px = threadIdx.x & (kTile - 1), py0 = (threadIdx.x >> 5) * 4;
    const int gx = tc.x0 + px;
    const size_t hw = (size_t)p.H * (size_t)p.W;
    double sums[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gy = tc.y0 + py0 + j;
        if (gx < p.W && gy < p.H) {
            const size_t pix = tc.view_off + (size_t)gy * p.W + gx;              // one-channel maps
            const size_t o3 = 3 * tc.view_off + (size_t)gy * p.W + gx;           // channel 0 of the three-channel maps
            const float alpha = p.alpha ? p.alpha[pix] : 1.f;
            float s[3];
            surf_normal_at<MODE>(lds.depth, kFwdSide, py0 + j + 1, px + 1, gy, gx, pix, o3, hw, p, R, alpha, s);
            if (p.surf_normal_out) {
#pragma unroll
                for (int c = 0; c < 3; ++c) p.surf_normal_out[o3 + c * hw] = s[c];
            }
            if (MODE != kNormals) {
                float dot = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) dot += p.rend_normal[o3 + c * hw] * s[c];
                sums[0] += (double)(1.f - dot);
                sums[1] += (double)p.dist[pix];
                if (p.mask) sums[2] += (double)fabsf(alpha - p.mask[pix]);
            }
        }
    }
    if (MODE != kNormals) {
        block_sum3(sums, lds.red);
        if (threadIdx.x == 0) {
            float *o = p.partials + (size_t)blockIdx.x * 3;
            o[0] = (float)sums[0];
            o[1] = (float)sums[1];
            o[2] = (float)sums[2];
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void geo_loss_backward_kernel(Params p) {
    __shared__ BackwardLds lds;
    const TileCoord tc = tile_coord(p);
    const size_t hw = (size_t)p.H * (size_t)p.W;
    float coef_n = 1.f, g_dist = 0.f, g_alpha = 0.f;   // kNormals: the gradient of the map is taken as it is
    if (MODE != kNormals) {
        coef_n = -(p.grad_out[(size_t)tc.view * 3 + 0] * p.inv_count);
        g_dist = p.grad_out[(size_t)tc.view * 3 + 1] * p.inv_count;
        g_alpha = p.grad_out[(size_t)tc.view * 3 + 2] * p.inv_count;
    }
    Rot R = {};
    const bool pull_depth = MODE != kTarget && p.grad_depth != nullptr;   // the same for every lane of the grid
    if (MODE != kTarget) {
        R = load_rot(p.view, tc.view);
        stage_depth<2>(lds.depth, p, tc);
        __syncthreads();
    }
    if (pull_depth) {
        // phase 1: pixel q of the tile with a halo of 1 -> d loss / d (its four neighbour depths) through its normal
        for (int i = threadIdx.x; i < kPullSide * kPullSide; i += kThreads) {
            const int r = i / kPullSide, c = i - r * kPullSide;
            const int gy = tc.y0 - 1 + r, gx = tc.x0 - 1 + c;
            float gN = 0.f, gS = 0.f, gW = 0.f, gE = 0.f;
            if (interior(gy, gx, p)) {
                const int lr = r + 1, lc = c + 1;   // q in the staged depth
                const Cross k = cross_at(lds.depth[(lr - 1) * kBwdSide + lc], lds.depth[(lr + 1) * kBwdSide + lc],
                                         lds.depth[lr * kBwdSide + lc - 1], lds.depth[lr * kBwdSide + lc + 1], gy, gx, p);
                if (k.len >= kEps) {   // below: the gradient through this normal is zero (ga_loss.h)
                    const size_t pix = tc.view_off + (size_t)gy * p.W + gx;
                    const size_t o3 = 3 * tc.view_off + (size_t)gy * p.W + gx;
                    const float w = coef_n * (p.alpha ? p.alpha[pix] : 1.f);
                    const float *gsrc = MODE == kNormals ? p.grad_out : p.rend_normal;
                    const float G0 = w * gsrc[o3], G1 = w * gsrc[o3 + hw], G2 = w * gsrc[o3 + 2 * hw];   // d loss / d n (world)
                    // to camera space (R transposed), then through c / |c|
                    const float hx = R.m[0][0] * G0 + R.m[1][0] * G1 + R.m[2][0] * G2;
                    const float hy = R.m[0][1] * G0 + R.m[1][1] * G1 + R.m[2][1] * G2;
                    const float hz = R.m[0][2] * G0 + R.m[1][2] * G1 + R.m[2][2] * G2;
                    const float nx = k.cx / k.len, ny = k.cy / k.len, nz = k.cz / k.len;
                    const float along = nx * hx + ny * hy + nz * hz;
                    const float gcx = (hx - nx * along) / k.len, gcy = (hy - ny * along) / k.len, gcz = (hz - nz * along) / k.len;
                    // c = (p dh, q dv, -(v dv q + u dh p + p q))
                    const float g_dv = k.q * (gcy - gcz * k.v);
                    const float g_dh = k.p * (gcx - gcz * k.u);
                    const float g_sv = p.ify * (gcx * k.dh - gcz * (k.u * k.dh + k.q));   // through p = (dS + dN) ify
                    const float g_sh = p.ifx * (gcy * k.dv - gcz * (k.v * k.dv + k.p));   // through q = (dE + dW) ifx
                    gS = g_sv + g_dv;
                    gN = g_sv - g_dv;
                    gE = g_sh + g_dh;
                    gW = g_sh - g_dh;
                }
            }
            lds.pull[0][i] = gN;
            lds.pull[1][i] = gS;
            lds.pull[2][i] = gW;
            lds.pull[3][i] = gE;
        }
        __syncthreads();
    }

    // phase 2: the lane's pixels
    const int px = threadIdx.x & (kTile - 1), py0 = (threadIdx.x >> 5) * 4;
    const int gx = tc.x0 + px;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gy = tc.y0 + py0 + j;
        if (gx < p.W && gy < p.H) {
            const size_t pix = tc.view_off + (size_t)gy * p.W + gx;
            const size_t o3 = 3 * tc.view_off + (size_t)gy * p.W + gx;
            if (MODE != kNormals) {
                if (p.grad_dist) p.grad_dist[pix] = g_dist;
                const float alpha = p.alpha[pix];
                if (p.grad_alpha) {
                    float ga = 0.f;
                    if (p.mask) {
                        const float d = alpha - p.mask[pix];
                        ga = d > 0.f ? g_alpha : (d < 0.f ? -g_alpha : 0.f);
                    }
                    p.grad_alpha[pix] = ga;
                }
                if (p.grad_rend_normal) {
                    float s[3];
                    surf_normal_at<MODE>(lds.depth, kBwdSide, py0 + j + 2, px + 2, gy, gx, pix, o3, hw, p, R, alpha, s);
#pragma unroll
                    for (int c = 0; c < 3; ++c) p.grad_rend_normal[o3 + c * hw] = coef_n * s[c];
                }
            }
            if (p.grad_depth) {
                float gd = 0.f;
                if (MODE != kTarget) {
                    const int r = py0 + j + 1, c = px + 1;   // p in the pulled-back images
                    // p is the south neighbour of the pixel above it, the north one of the pixel below, the east one of the pixel to its
                    // left and the west one of the pixel to its right
                    gd = ((lds.pull[1][(r - 1) * kPullSide + c] + lds.pull[0][(r + 1) * kPullSide + c]) + lds.pull[3][r * kPullSide + c - 1]) +
                         lds.pull[2][r * kPullSide + c + 1];
                }
                p.grad_depth[pix] = gd;
            }
        }
    }
}

bool shape_ok(int32_t V, int32_t H, int32_t W) {
    if (V < 1 || H < 1 || W < 1 || H > GA_GEO_LOSS_MAX_SIDE || W > GA_GEO_LOSS_MAX_SIDE) return false;
    const int64_t tiles = (int64_t)((H + kTile - 1) / kTile) * ((W + kTile - 1) / kTile);   // <= 2^22
    return (int64_t)V * tiles < ((int64_t)1 << 31);                                          // the grid
}

int mode_of(int32_t flags) {
    if (flags == 0) return kFromDepth;
    if (flags == GA_GEO_LOSS_TARGET) return kTarget;
    if (flags == GA_GEO_LOSS_NORMALS) return kNormals;
    return -1;
}

// everything the host can see, for both directions -> mode
int check_args(const GaGeoLossArgs *a, GaGeoLossPlan *pl, int *mode) {
    if (!a) return GA_ERR_NULL_ARG;
    *mode = mode_of(a->flags);
    if (*mode < 0) return GA_ERR_BAD_FLAGS;
    const int rc = ga_geo_loss_plan(a->num_views, a->height, a->width, pl);
    if (rc != GA_OK) return rc;
    if (!(a->tanfov > 0.0) || !(a->tanfov < 1e30)) return GA_ERR_BAD_SHAPE;
    if (*mode == kNormals) {
        if (!a->view || !a->depth) return GA_ERR_NULL_ARG;
    } else {
        if (!a->rend_normal || !a->depth || !a->alpha || !a->dist) return GA_ERR_NULL_ARG;
        if (*mode == kTarget ? !a->target_normal : !a->view) return GA_ERR_NULL_ARG;
    }
    return GA_OK;
}

Params make_params(const GaGeoLossArgs *a, const GaGeoLossPlan &pl) {
    Params p;
    p.H = a->height;
    p.W = a->width;
    p.tiles_x = pl.tiles_x;
    p.tiles_y = pl.tiles_y;
    p.ifx = (float)(2.0 * a->tanfov / (double)a->width);
    p.ify = (float)(2.0 * a->tanfov / (double)a->height);
    p.half_w = 0.5f * (float)a->width;
    p.half_h = 0.5f * (float)a->height;
    p.inv_count = (float)(1.0 / ((double)a->height * (double)a->width));
    p.view = a->view;
    p.rend_normal = a->rend_normal;
    p.depth = a->depth;
    p.alpha = a->alpha;
    p.dist = a->dist;
    p.target_normal = a->target_normal;
    p.mask = a->mask;
    p.grad_out = a->grad_out;
    p.surf_normal_out = a->surf_normal_out;
    p.partials = reinterpret_cast<float *>(a->workspace);
    p.grad_rend_normal = a->grad_rend_normal;
    p.grad_depth = a->grad_depth;
    p.grad_dist = a->grad_dist;
    p.grad_alpha = a->grad_alpha;
    return p;
}

}  // namespace

extern "C" int ga_geo_loss_plan(int32_t V, int32_t H, int32_t W, GaGeoLossPlan *plan) {
    if (!plan) return GA_ERR_NULL_ARG;
    if (!shape_ok(V, H, W)) return GA_ERR_BAD_SHAPE;
    plan->tile_w = kTile;
    plan->tile_h = kTile;
    plan->threads = kThreads;
    plan->tiles_x = (W + kTile - 1) / kTile;
    plan->tiles_y = (H + kTile - 1) / kTile;
    plan->lds_bytes = (int32_t)sizeof(ForwardLds);
    plan->lds_bytes_backward = (int32_t)sizeof(BackwardLds);
    plan->reserved = 0;
    plan->grid_x = (int64_t)V * plan->tiles_x * plan->tiles_y;
    plan->num_partials = plan->grid_x * 3;
    return GA_OK;
}

extern "C" size_t ga_geo_loss_workspace_bytes(int32_t V, int32_t H, int32_t W) {
    GaGeoLossPlan pl;
    if (ga_geo_loss_plan(V, H, W, &pl) != GA_OK) return 0;
    return ((size_t)pl.num_partials * 4 + 255) / 256 * 256;
}

extern "C" int ga_geo_loss_forward(const GaGeoLossArgs *a, void *stream_v) {
    GaGeoLossPlan pl;
    int mode;
    const int rc = check_args(a, &pl, &mode);
    if (rc != GA_OK) return rc;
    if (mode == kNormals) {
        if (!a->surf_normal_out) return GA_ERR_NULL_ARG;
    } else {
        if (!a->out || !a->workspace) return GA_ERR_NULL_ARG;
        if (a->workspace_bytes < ga_geo_loss_workspace_bytes(a->num_views, a->height, a->width)) return GA_ERR_WORKSPACE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    Params p = make_params(a, pl);
    const dim3 grid((unsigned)pl.grid_x), block(kThreads);
    (void)hipGetLastError();
    if (mode == kNormals) {
        p.mask = nullptr;
        hipLaunchKernelGGL(geo_loss_forward_kernel<kNormals>, grid, block, 0, s, p);
        return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
    }
    if (mode == kTarget)
        hipLaunchKernelGGL(geo_loss_forward_kernel<kTarget>, grid, block, 0, s, p);
    else
        hipLaunchKernelGGL(geo_loss_forward_kernel<kFromDepth>, grid, block, 0, s, p);
    hipLaunchKernelGGL(loss_reduce_kernel, dim3((unsigned)a->num_views), dim3(kReduceThreads), 0, s, p.partials, a->out,
                       pl.tiles_x * pl.tiles_y, 1.0 / ((double)a->height * (double)a->width));
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_geo_loss_backward(const GaGeoLossArgs *a, void *stream_v) {
    GaGeoLossPlan pl;
    int mode;
    const int rc = check_args(a, &pl, &mode);
    if (rc != GA_OK) return rc;
    if (!a->grad_out) return GA_ERR_NULL_ARG;
    if (mode == kNormals && !a->grad_depth) return GA_ERR_NULL_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    const Params p = make_params(a, pl);
    const dim3 grid((unsigned)pl.grid_x), block(kThreads);
    (void)hipGetLastError();
    if (mode == kNormals)
        hipLaunchKernelGGL(geo_loss_backward_kernel<kNormals>, grid, block, 0, s, p);
    else if (mode == kTarget)
        hipLaunchKernelGGL(geo_loss_backward_kernel<kTarget>, grid, block, 0, s, p);
    else
        hipLaunchKernelGGL(geo_loss_backward_kernel<kFromDepth>, grid, block, 0, s, p);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}
