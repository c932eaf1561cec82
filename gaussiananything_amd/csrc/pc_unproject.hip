// pc_unproject.hip -- point clouds from posed depth views, for gfx950 (include/ga_pointcloud.h: GaUnprojectArgs, ga_pc_unproject).
//
// Built with -ffp-contract=off: every operation is rounded on its own, division and square root are hipcc's correctly rounded defaults,
// so the kernels are a function of their inputs alone and tests/_unproject_ref.py restates them in numpy float32 bit for bit.
//
// An ordered stream compaction whose output size is data dependent, three launches built from csrc/compact.h -- no workgroup waits for
// another one, there is no look-back, no spinning, no atomics:
//   1 flag     a workgroup owns a band of full rows of one view (band order = source order).  With erode > 0 the thresholded mask of the
//              band and an erode-wide halo is staged in LDS as bytes (outside the image: foreground) and a pixel is foreground when the
//              whole diamond |dx| + |dy| <= erode is: e iterations of the 3 x 3 cross.  kThreads consecutive pixels per trip, coalesced;
//              one flag byte per pixel and the band's count go to the workspace.
//   2 scan     ONE workgroup walks the band counts kThreads at a time (carry in a register), writes each band's exclusive offset in place,
//              the total behind them and to count[0], then the per-view differences to view_counts.
//   3 scatter  ranks the band's flags trip by trip (ballot + popcount inside a wave, the wave totals through LDS) and writes the rows of
//              its valid pixels; the point is computed again there (the same code on the same inputs gives the same bits) rather than
//              stored by the flag pass -- see the header.  Workgroups past the bands write the padding rows.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/ga_pointcloud.h"
#include "compact.h"

namespace {

using namespace gacompact;

constexpr int kThreads = GA_PC_UNPROJECT_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr int kTilePixels = GA_PC_UNPROJECT_TILE_PIXELS;
constexpr int kCam = GA_PC_CAMERA_FLOATS;

struct Shape {
    int rows_per_block, blocks_per_view, num_blocks;
};

__host__ __device__ inline Shape shape_of(int V, int H, int W) {
    Shape s;
    int r = kTilePixels / W;
    r = r < 1 ? 1 : r;
    s.rows_per_block = r > H ? H : r;
    s.blocks_per_view = (H + s.rows_per_block - 1) / s.rows_per_block;
    s.num_blocks = V * s.blocks_per_view;
    return s;
}

// the workspace: num_blocks + 1 int32 (band counts, then offsets and the total), padded to 16 bytes, then one flag byte per pixel
__host__ __device__ inline size_t flags_offset(const Shape &s) { return (((size_t)s.num_blocks + 1 + 3) / 4) * 16; }

// the point of pixel (x, y) with depth z; the operation order is the header's
__device__ __forceinline__ void lift(const float *__restrict__ cam, int x, int y, float z, float inv_w, float half_w, float inv_h,
                                     float half_h, int depth_kind, float clip, float &px, float &py, float &pz) {
    const float fx = cam[12], fy = cam[13], cx = cam[14], cy = cam[15], sk = cam[16];
    const float u = (float)x * inv_w + half_w;
    const float v = (float)y * inv_h + half_h;
    const float xl = (((u - cx) + (cy * sk) / fy) - (sk * v) / fy) / fx;
    const float yl = (v - cy) / fy;
    float dx = (cam[0] * xl + cam[1] * yl) + cam[2];
    float dy = (cam[3] * xl + cam[4] * yl) + cam[5];
    float dz = (cam[6] * xl + cam[7] * yl) + cam[8];
    if (depth_kind == GA_PC_DEPTH_RAY) {
        const float l = fmaxf(sqrtf((dx * dx + dy * dy) + dz * dz), 1e-12f);
        dx = dx / l; dy = dy / l; dz = dz / l;
    }
    px = cam[9] + z * dx;
    py = cam[10] + z * dy;
    pz = cam[11] + z * dz;
    if (clip > 0.f) {
        px = fminf(fmaxf(px, -clip), clip);
        py = fminf(fmaxf(py, -clip), clip);
        pz = fminf(fmaxf(pz, -clip), clip);
    }
}

__global__ __launch_bounds__(kThreads) void unproject_flag_kernel(GaUnprojectArgs a, Shape s, int halo) {
    extern __shared__ unsigned char fg[];   // (rows + 2 halo) x (W + 2 halo) thresholded mask bytes, when halo > 0
    __shared__ int wave_sum[kWaves];
    const int H = a.height, W = a.width;
    const int v = blockIdx.x / s.blocks_per_view, band = blockIdx.x - v * s.blocks_per_view;
    const int y0 = band * s.rows_per_block;
    const int rows = (H - y0) < s.rows_per_block ? (H - y0) : s.rows_per_block;
    const int64_t view0 = (int64_t)v * H * W;
    const int pitch = W + 2 * halo;
    if (halo > 0) {
        const int cells = (rows + 2 * halo) * pitch;
        for (int c = threadIdx.x; c < cells; c += kThreads) {
            const int ry = c / pitch, rx = c - ry * pitch;
            const int yy = y0 - halo + ry, xx = rx - halo;
            unsigned char f = 1;   // outside the image: never erodes anything
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) f = a.mask[view0 + (int64_t)yy * W + xx] >= a.mask_threshold ? 1 : 0;
            fg[c] = f;
        }
        __syncthreads();
    }
    const float *cam = a.cameras + (int64_t)v * kCam;
    const float inv_w = 1.f / (float)W, half_w = 0.5f / (float)W, inv_h = 1.f / (float)H, half_h = 0.5f / (float)H;
    unsigned char *flags = reinterpret_cast<unsigned char *>(a.workspace) + flags_offset(s);
    const int pixels = rows * W, st = a.pixel_stride;
    int mine = 0;
    for (int p = threadIdx.x; p < pixels; p += kThreads) {
        const int ry = p / W, x = p - ry * W, y = y0 + ry;
        const int64_t at = view0 + (int64_t)y * W + x;
        bool ok = (y % st == 0) && (x % st == 0);
        if (ok) {
            const float z = a.depth[at];
            ok = a.depth_min < z && z < a.depth_max;
            if (ok && a.mask) {
                if (halo > 0) {
                    const unsigned char *c = fg + (ry + halo) * pitch + (x + halo);
                    for (int dy = -halo; dy <= halo; ++dy) {
                        const int reach = halo - (dy < 0 ? -dy : dy);
                        for (int dx = -reach; dx <= reach; ++dx) ok = ok && c[dy * pitch + dx];
                    }
                } else {
                    ok = a.mask[at] >= a.mask_threshold;
                }
            }
            if (ok && (a.clip > 0.f || a.drop_zero)) {
                float px, py, pz;
                lift(cam, x, y, z, inv_w, half_w, inv_h, half_h, a.depth_kind, a.clip, px, py, pz);
                if (a.clip > 0.f) ok = !(fabsf(px) == a.clip || fabsf(py) == a.clip || fabsf(pz) == a.clip);
                if (a.drop_zero) ok = ok && !(px == 0.f || py == 0.f || pz == 0.f);
            }
        }
        flags[at] = ok ? 1 : 0;
        mine += ok ? 1 : 0;
    }
    const int total = block_sum<kWaves>(mine, wave_sum);
    if (threadIdx.x == 0) reinterpret_cast<int32_t *>(a.workspace)[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void unproject_scan_kernel(GaUnprojectArgs a, Shape s) {
    __shared__ int lds[kWaves];
    int32_t *sums = reinterpret_cast<int32_t *>(a.workspace);
    const int total = scan_counts_in_place<kThreads>(sums, s.num_blocks, lds);   // at most V * H * W < 2^31
    if (threadIdx.x == 0) a.count[0] = total;
    __syncthreads();   // the offsets this workgroup wrote are read back below
    for (int v = threadIdx.x; v < a.num_views; v += kThreads)
        a.view_counts[v] = sums[(v + 1) * s.blocks_per_view] - sums[v * s.blocks_per_view];
}

__global__ __launch_bounds__(kThreads) void unproject_scatter_kernel(GaUnprojectArgs a, Shape s) {
    __shared__ int wave_sum[kWaves];
    const int32_t *offs = reinterpret_cast<const int32_t *>(a.workspace);
    const int64_t cap = a.capacity;
    if ((int)blockIdx.x >= s.num_blocks) {   // padding: rows min(count, capacity) .. capacity - 1
        int64_t lo, hi;
        pad_range((int)blockIdx.x - s.num_blocks, offs[s.num_blocks], cap, lo, hi);
        for (int64_t r = lo + threadIdx.x; r < hi; r += kThreads) {
            a.points[3 * r] = 0.f; a.points[3 * r + 1] = 0.f; a.points[3 * r + 2] = 0.f;
            if (a.colors) { a.colors[3 * r] = 0.f; a.colors[3 * r + 1] = 0.f; a.colors[3 * r + 2] = 0.f; }
            if (a.normals) { a.normals[3 * r] = 0.f; a.normals[3 * r + 1] = 0.f; a.normals[3 * r + 2] = 0.f; }
            a.source[r] = -1;
        }
        return;
    }
    const int H = a.height, W = a.width;
    const int v = blockIdx.x / s.blocks_per_view, band = blockIdx.x - v * s.blocks_per_view;
    const int y0 = band * s.rows_per_block;
    const int rows = (H - y0) < s.rows_per_block ? (H - y0) : s.rows_per_block;
    const int64_t view0 = (int64_t)v * H * W, plane = (int64_t)H * W;
    const float *cam = a.cameras + (int64_t)v * kCam;
    const float inv_w = 1.f / (float)W, half_w = 0.5f / (float)W, inv_h = 1.f / (float)H, half_h = 0.5f / (float)H;
    const unsigned char *flags = reinterpret_cast<const unsigned char *>(a.workspace) + flags_offset(s);
    const int pixels = rows * W;
    int64_t row0 = offs[blockIdx.x];
    const int64_t row_end = offs[blockIdx.x + 1];
    for (int start = 0; start < pixels && row0 < row_end && row0 < cap; start += kThreads) {   // (uniform: the barriers are safe)
        const int p = start + (int)threadIdx.x;
        int ry = 0, x = 0;
        bool ok = false;
        if (p < pixels) {
            ry = p / W; x = p - ry * W;
            ok = flags[view0 + (int64_t)(y0 + ry) * W + x] != 0;
        }
        int all;
        const int64_t r = row0 + block_ballot_rank<kWaves>(ok, wave_sum, all);
        if (ok && r < cap) {
            const int y = y0 + ry;
            const int64_t at = view0 + (int64_t)y * W + x;
            float px, py, pz;
            lift(cam, x, y, a.depth[at], inv_w, half_w, inv_h, half_h, a.depth_kind, a.clip, px, py, pz);
            a.points[3 * r] = px; a.points[3 * r + 1] = py; a.points[3 * r + 2] = pz;
            a.source[r] = (int32_t)at;
            const int64_t c0 = 3 * view0 + (int64_t)y * W + x;   // [v, 0, y, x] of a [V,3,H,W] map
            if (a.colors) {
                float cr, cg, cb;
                if (a.color_kind == GA_PC_COLOR_U8) {
                    const unsigned char *c = reinterpret_cast<const unsigned char *>(a.color);
                    cr = (float)c[c0] / 255.f; cg = (float)c[c0 + plane] / 255.f; cb = (float)c[c0 + 2 * plane] / 255.f;
                } else {
                    const float *c = reinterpret_cast<const float *>(a.color);
                    cr = c[c0]; cg = c[c0 + plane]; cb = c[c0 + 2 * plane];
                }
                a.colors[3 * r] = cr; a.colors[3 * r + 1] = cg; a.colors[3 * r + 2] = cb;
            }
            if (a.normals) {
                float nx = a.normal[c0], ny = a.normal[c0 + plane], nz = a.normal[c0 + 2 * plane];
                const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
                if (l > 0.f) { nx = nx / l; ny = ny / l; nz = nz / l; } else { nx = 0.f; ny = 0.f; nz = 1.f; }
                a.normals[3 * r] = nx; a.normals[3 * r + 1] = ny; a.normals[3 * r + 2] = nz;
            }
        }
        row0 += all;
    }
}

bool unproject_shape_ok(int64_t V, int64_t H, int64_t W) {
    return V >= 1 && H >= 1 && W >= 1 && W <= GA_PC_UNPROJECT_MAX_WIDTH && V * H * W < (int64_t(1) << 31);
}

}  // namespace

extern "C" size_t ga_pc_unproject_workspace_bytes(int32_t num_views, int32_t height, int32_t width) {
    if (!unproject_shape_ok(num_views, height, width)) return 0;
    const Shape s = shape_of(num_views, height, width);
    return flags_offset(s) + (((size_t)num_views * height * width + 15) / 16) * 16;
}

extern "C" int ga_pc_unproject(const GaUnprojectArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaUnprojectArgs &a = *args;
    if (!unproject_shape_ok(a.num_views, a.height, a.width) || a.capacity < 1) return GA_ERR_BAD_SHAPE;
    if ((a.depth_kind != GA_PC_DEPTH_Z && a.depth_kind != GA_PC_DEPTH_RAY) || (a.color_kind != GA_PC_COLOR_F32 && a.color_kind != GA_PC_COLOR_U8) ||
        a.erode < 0 || a.erode > GA_PC_UNPROJECT_MAX_ERODE || (a.drop_zero != 0 && a.drop_zero != 1) || a.pixel_stride < 1 || a.reserved != 0)
        return GA_ERR_BAD_FLAGS;
    if (a.depth_min != a.depth_min || a.depth_max != a.depth_max || a.mask_threshold != a.mask_threshold ||
        !(a.clip >= 0.f && a.clip <= 3.0e38f))
        return GA_ERR_BAD_FLAGS;
    if (!a.depth || !a.cameras || !a.points || !a.source || !a.count || !a.view_counts || !a.workspace) return GA_ERR_NULL_ARG;
    if ((a.color != nullptr) != (a.colors != nullptr) || (a.normal != nullptr) != (a.normals != nullptr)) return GA_ERR_NULL_ARG;
    if (a.workspace_bytes < ga_pc_unproject_workspace_bytes(a.num_views, a.height, a.width) || (reinterpret_cast<uintptr_t>(a.workspace) & 15))
        return GA_ERR_WORKSPACE;
    const Shape s = shape_of(a.num_views, a.height, a.width);
    const int halo = a.mask ? a.erode : 0;
    // at most (1024 + 8) rows of 1 + 8 bytes, or 9 rows of 4096 + 8: under 37 KB
    const size_t lds = halo > 0 ? (size_t)(s.rows_per_block + 2 * halo) * (size_t)(a.width + 2 * halo) : 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    hipLaunchKernelGGL(unproject_flag_kernel, dim3(s.num_blocks), dim3(kThreads), lds, st, a, s, halo);
    hipLaunchKernelGGL(unproject_scan_kernel, dim3(1), dim3(kThreads), 0, st, a, s);
    hipLaunchKernelGGL(unproject_scatter_kernel, dim3((unsigned)s.num_blocks + pad_blocks(a.capacity)), dim3(kThreads), 0, st, a, s);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}
