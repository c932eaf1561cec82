// pc_filter.hip -- cross-view consistency filter and voxel thinning of a point cloud, for gfx950 (include/ga_pointcloud.h:
// GaFilterViewsArgs / ga_pc_filter_views, GaVoxelThinArgs / ga_pc_voxel_thin).
//
// Built with -ffp-contract=off: every operation is rounded on its own, division, square root and floor are exact or correctly rounded,
// so the kernels are a function of their inputs alone and tests/_pc_filter_ref.py restates them in numpy float32 bit for bit.
//
// Both calls end in the three-launch ordered compaction built from csrc/compact.h, here over bands of kBandRows consecutive ROWS:
//   flag     one flag byte per row and the band's count (filter_vote_kernel for the filter, voxel_flag_kernel for the thinning)
//   scan     ONE workgroup, kThreads band counts a trip with a register carry: exclusive offsets, count; view_counts zeroed
//   scatter  ballot + popcount ranks, copies the kept rows, adds them to view_counts; further workgroups write the padding
// The thinning puts two launches in front: table_clear_kernel and voxel_insert_kernel (an open-addressing table of key / rank / count
// that is touched through agent-scope integer atomics alone while it is being filled).  No workgroup waits for another, every probe
// loop is bounded by the table's size, phases are separate launches ordered by the stream.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/ga_pointcloud.h"
#include "compact.h"

namespace {

using namespace gacompact;

constexpr int kThreads = GA_PC_FILTER_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr int kBandRows = GA_PC_FILTER_BAND_ROWS;
constexpr int kTrips = kBandRows / kThreads;
constexpr int kCam = GA_PC_CAMERA_FLOATS;
constexpr unsigned long long kEmpty = ~0ull;   // no key (63 bits) and no rank of a row equals it

// what the compaction needs of either call
struct Compact {
    int rows, capacity, num_views, view_pixels, num_bands;
    const int32_t *in_count;
    const float *points, *colors, *normals;
    const int32_t *source;
    float *o_points, *o_colors, *o_normals;
    int32_t *o_source, *kept_rows, *count, *view_counts, *multiplicity;
    const int32_t *slot_of, *slot_count;   // the thinning's multiplicity: slot_count[slot_of[r]]
    int32_t *bands;                        // num_bands + 1: counts, then exclusive offsets and the total
    unsigned char *flags;                  // one byte per row
};

// the workspace: num_bands + 1 int32 padded to 16 bytes, one flag byte per row padded to 16 bytes; then, for the thinning, one int32
// slot per row padded to 16 bytes, table_slots keys, table_slots ranks, table_slots counts
__host__ __device__ inline int bands_of(int rows) { return (rows + kBandRows - 1) / kBandRows; }
inline size_t pad16(size_t n) { return (n + 15) / 16 * 16; }
inline size_t flags_offset(int rows) { return pad16(((size_t)bands_of(rows) + 1) * 4); }
inline size_t compact_bytes(int rows) { return flags_offset(rows) + pad16((size_t)rows); }

__device__ __forceinline__ int live_rows(const Compact &c) {
    int n = c.rows;
    if (c.in_count) {
        const int given = c.in_count[0];
        n = given < 0 ? 0 : (given < n ? given : n);
    }
    return n;
}

// ---- the filter's flag pass: one lane per row, every view votes ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void filter_vote_kernel(GaFilterViewsArgs a, Compact c) {
    __shared__ int wave_sum[kWaves];
    const int live = live_rows(c);
    const int H = a.height, W = a.width, V = a.num_views, win = a.window;
    const int plane = H * W;
    const float fw = (float)W, fh = (float)H;
    int mine = 0;
    for (int trip = 0; trip < kTrips; ++trip) {
        const int r = (int)blockIdx.x * kBandRows + trip * kThreads + (int)threadIdx.x;
        if (r >= c.rows) break;
        int support = 0, conflicts = 0;
        bool keep = false;
        if (r < live) {
            const float px = a.points[3 * (int64_t)r], py = a.points[3 * (int64_t)r + 1], pz = a.points[3 * (int64_t)r + 2];
            int own = -1;
            if (a.source) {
                const int s = a.source[r];
                if (s >= 0) own = s / plane;
            }
            for (int u = 0; u < V; ++u) {
                if (u == own) continue;
                const float *cam = a.cameras + (int64_t)u * kCam;
                const float ex = px - cam[9], ey = py - cam[10], ez = pz - cam[11];
                const float qx = (cam[0] * ex + cam[3] * ey) + cam[6] * ez;
                const float qy = (cam[1] * ex + cam[4] * ey) + cam[7] * ez;
                const float qz = (cam[2] * ex + cam[5] * ey) + cam[8] * ez;
                if (!(qz > 0.f)) continue;
                const float fx = cam[12], fy = cam[13], cx = cam[14], cy = cam[15], sk = cam[16];
                const float xl = qx / qz, yl = qy / qz;
                const float vv = yl * fy + cy;
                const float uu = ((xl * fx + cx) - (cy * sk) / fy) + (sk * vv) / fy;
                const float fa = uu * fw, fb = vv * fh;
                if (!(fa >= 0.f && fa < fw && fb >= 0.f && fb < fh)) continue;
                const int x = (int)fa, y = (int)fb;
                const float d = a.depth_kind == GA_PC_DEPTH_RAY ? sqrtf((qx * qx + qy * qy) + qz * qz) : qz;
                const int64_t view0 = (int64_t)u * plane;
                int inside = 0, surface = 0;
                bool centre = false;
                float zmin = 0.f, zmax = 0.f;
                for (int dy = -win; dy <= win; ++dy) {
                    const int yy = y + dy;
                    if (yy < 0 || yy >= H) continue;
                    for (int dx = -win; dx <= win; ++dx) {
                        const int xx = x + dx;
                        if (xx < 0 || xx >= W) continue;
                        const int64_t at = view0 + (int64_t)yy * W + xx;
                        const float z = a.depth[at];
                        bool ok = a.depth_min < z && z < a.depth_max;
                        if (ok && a.mask) ok = a.mask[at] >= a.mask_threshold;
                        ++inside;
                        if (ok) {
                            zmin = surface == 0 || z < zmin ? z : zmin;
                            zmax = surface == 0 || z > zmax ? z : zmax;
                            ++surface;
                            centre = centre || (dx == 0 && dy == 0);
                        }
                    }
                }
                if (surface > 0) {
                    const float lo = zmin - (a.tol_abs + a.tol_rel * zmin);
                    const float hi = zmax + (a.tol_abs + a.tol_rel * zmax);
                    if (centre && lo <= d && d <= hi) ++support;
                    if (surface == inside && d < lo) ++conflicts;
                } else if (a.carve) {
                    ++conflicts;
                }
            }
            keep = support >= a.min_support && conflicts <= a.max_conflicts;
        }
        if (a.support) a.support[r] = (uint8_t)(support > 255 ? 255 : support);
        if (a.conflicts) a.conflicts[r] = (uint8_t)(conflicts > 255 ? 255 : conflicts);
        c.flags[r] = keep ? 1 : 0;
        mine += keep ? 1 : 0;
    }
    const int total = block_sum<kWaves>(mine, wave_sum);
    if (threadIdx.x == 0) c.bands[blockIdx.x] = total;   // the band's count
}

// ---- the thinning's table ----------------------------------------------------------------------------------------------------------------
struct Table {
    unsigned long long *keys, *ranks;
    int32_t *counts, *slot_of;
    unsigned long long slots;   // a power of two
};

__global__ __launch_bounds__(kThreads) void table_clear_kernel(Table t, int32_t *dropped) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kThreads;
    for (unsigned long long s = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; s < t.slots; s += stride) {
        t.keys[s] = kEmpty;
        t.ranks[s] = kEmpty;
        t.counts[s] = 0;
    }
    if (dropped && blockIdx.x == 0 && threadIdx.x == 0) dropped[0] = 0;
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}

// One lane per row.  With GA_PC_VOXEL_WAVE_MERGE a run of neighbouring lanes of a wave that hold the same key (adjacent pixels share cells)
// is inserted once, by its first lane, with the run's smallest rank and its length; the slot goes back to the run by a shuffle.  The
// table ends up the same either way: min and add are associative, and no output depends on which lane did them.
__global__ __launch_bounds__(kThreads) void voxel_insert_kernel(GaVoxelThinArgs a, Table t, Compact c) {
    const int r = (int)blockIdx.x * kThreads + (int)threadIdx.x;   // (no early return: the shuffles below want whole waves)
    const int lane = threadIdx.x & 63;
    const bool live = r < live_rows(c);
    unsigned long long key = kEmpty, rank = 0;
    if (live) {
        const float vs = a.voxel_size;
        float p[3], fl[3];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = a.points[3 * (int64_t)r + k];
            const float g = (p[k] - a.origin[k]) / vs;
            fl[k] = floorf(g);
            ok = ok && fabsf(g) < __builtin_inff() && fabsf(fl[k]) <= (float)GA_PC_VOXEL_MAX_INDEX;
        }
        if (ok) {
            const unsigned long long bx = (unsigned long long)((int)fl[0] + (1 << 20)), by = (unsigned long long)((int)fl[1] + (1 << 20)),
                                     bz = (unsigned long long)((int)fl[2] + (1 << 20));
            key = (bx << 42) | (by << 21) | bz;
            rank = (unsigned long long)(unsigned)r;
            if (a.keep == GA_PC_VOXEL_CENTER) {
                const float dx = p[0] - ((fl[0] + 0.5f) * vs + a.origin[0]);
                const float dy = p[1] - ((fl[1] + 0.5f) * vs + a.origin[1]);
                const float dz = p[2] - ((fl[2] + 0.5f) * vs + a.origin[2]);
                const float dist2 = (dx * dx + dy * dy) + dz * dz;
                rank |= (unsigned long long)__float_as_uint(dist2) << 32;
            }
        }
    }
    bool mine = key != kEmpty;   // this lane inserts
    int members = 1, head = lane;
    if (a.flags & GA_PC_VOXEL_WAVE_MERGE) {
        const unsigned long long before = __shfl_up(key, 1, 64);
        const bool first = lane == 0 || key != before;
        const unsigned long long heads = __ballot(first);
        const unsigned long long upto = ~0ull >> (63 - lane);   // lanes 0 .. lane
        head = 63 - __clzll((long long)(heads & upto));
        const unsigned long long later = heads & ~upto;
        const int last = later ? __ffsll((long long)later) - 2 : 63;   // the lane in front of the next run's first
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {   // segmented min: a lane ends with the smallest rank of its run from itself on
            const unsigned long long other = __shfl_down(rank, d, 64);
            if (lane + d <= last && other < rank) rank = other;
        }
        members = last - head + 1;
        mine = mine && first;
    }
    int slot = -1;
    if (mine) {
        const unsigned long long mask = t.slots - 1;
        unsigned long long h = mix64(key) & mask;
        for (unsigned long long n = 0; n < t.slots; ++n) {   // bounded: never spins, an exhausted probe drops the row
            unsigned long long seen = kEmpty;
            __hip_atomic_compare_exchange_strong(&t.keys[h], &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen == kEmpty || seen == key) {
                slot = (int)h;
                break;
            }
            h = (h + 1) & mask;
        }
        if (slot >= 0) {
            __hip_atomic_fetch_min(&t.ranks[slot], rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&t.counts[slot], members, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (a.flags & GA_PC_VOXEL_WAVE_MERGE) slot = __shfl(slot, head, 64);
    if (live && slot < 0 && a.dropped) __hip_atomic_fetch_add(a.dropped, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r < c.rows) t.slot_of[r] = slot;
}

// a later launch: the table is complete and read with plain loads
__global__ __launch_bounds__(kThreads) void voxel_flag_kernel(Table t, Compact c) {
    __shared__ int wave_sum[kWaves];
    int mine = 0;
    for (int trip = 0; trip < kTrips; ++trip) {
        const int r = (int)blockIdx.x * kBandRows + trip * kThreads + (int)threadIdx.x;
        if (r >= c.rows) break;
        const int slot = t.slot_of[r];
        const bool keep = slot >= 0 && (unsigned)(t.ranks[slot] & 0xffffffffull) == (unsigned)r;
        c.flags[r] = keep ? 1 : 0;
        mine += keep ? 1 : 0;
    }
    const int total = block_sum<kWaves>(mine, wave_sum);
    if (threadIdx.x == 0) c.bands[blockIdx.x] = total;   // the band's count
}

// ---- scan and scatter ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void compact_scan_kernel(Compact c) {
    __shared__ int lds[kWaves];
    const int total = scan_counts_in_place<kThreads>(c.bands, c.num_bands, lds);   // at most rows <= 2^30
    if (threadIdx.x == 0) c.count[0] = total;
    if (c.view_counts)
        for (int v = threadIdx.x; v < c.num_views; v += kThreads) c.view_counts[v] = 0;   // the scatter launch adds to them
}

__global__ __launch_bounds__(kThreads) void compact_scatter_kernel(Compact c) {
    __shared__ int wave_sum[kWaves];
    const int64_t cap = c.capacity;
    if ((int)blockIdx.x >= c.num_bands) {   // padding: rows min(count, capacity) .. capacity - 1
        int64_t lo, hi;
        pad_range((int)blockIdx.x - c.num_bands, c.bands[c.num_bands], cap, lo, hi);
        for (int64_t r = lo + threadIdx.x; r < hi; r += kThreads) {
            c.o_points[3 * r] = 0.f; c.o_points[3 * r + 1] = 0.f; c.o_points[3 * r + 2] = 0.f;
            if (c.o_colors) { c.o_colors[3 * r] = 0.f; c.o_colors[3 * r + 1] = 0.f; c.o_colors[3 * r + 2] = 0.f; }
            if (c.o_normals) { c.o_normals[3 * r] = 0.f; c.o_normals[3 * r + 1] = 0.f; c.o_normals[3 * r + 2] = 0.f; }
            if (c.o_source) c.o_source[r] = -1;
            c.kept_rows[r] = -1;
            if (c.multiplicity) c.multiplicity[r] = 0;
        }
        return;
    }
    __shared__ int wave_view[kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int64_t row0 = c.bands[blockIdx.x];
    const int64_t row_end = c.bands[blockIdx.x + 1];
    int held_view = -1, held = 0;   // kept rows of one view this wave has counted and not yet added (the same in every lane)
    // (uniform: the barriers and the wave operations are safe; rows past the capacity still count for view_counts)
    for (int trip = 0; trip < kTrips && row0 < row_end && (row0 < cap || c.view_counts); ++trip) {
        const int64_t in = (int64_t)blockIdx.x * kBandRows + trip * kThreads + (int)threadIdx.x;
        const bool ok = in < c.rows && c.flags[in] != 0;
        int all;
        const int64_t r = row0 + block_ballot_rank<kWaves>(ok, wave_sum, all);
        int src = -1;
        if (ok && c.source) src = c.source[in];
        if (ok && r < cap) {
            c.o_points[3 * r] = c.points[3 * in]; c.o_points[3 * r + 1] = c.points[3 * in + 1]; c.o_points[3 * r + 2] = c.points[3 * in + 2];
            if (c.o_colors) {
                c.o_colors[3 * r] = c.colors[3 * in]; c.o_colors[3 * r + 1] = c.colors[3 * in + 1]; c.o_colors[3 * r + 2] = c.colors[3 * in + 2];
            }
            if (c.o_normals) {
                c.o_normals[3 * r] = c.normals[3 * in]; c.o_normals[3 * r + 1] = c.normals[3 * in + 1];
                c.o_normals[3 * r + 2] = c.normals[3 * in + 2];
            }
            if (c.o_source) c.o_source[r] = src;
            c.kept_rows[r] = (int32_t)in;
            if (c.multiplicity) c.multiplicity[r] = c.slot_count[c.slot_of[in]];
        }
        if (c.view_counts) {   // a wave whose kept rows share a view (an ordered cloud) counts in a register, a mixed one row by row
            int v = -1;
            if (src >= 0) {
                v = src / c.view_pixels;
                v = v < c.num_views ? v : -1;
            }
            const unsigned long long counted = __ballot(v >= 0);
            if (counted) {
                const int first = __ffsll((long long)counted) - 1;
                const int v0 = __shfl(v, first, 64);
                if (__ballot(v == v0) == counted) {
                    if (v0 != held_view) {
                        if (held > 0 && lane == 0) atomicAdd(&c.view_counts[held_view], held);
                        held_view = v0;
                        held = 0;
                    }
                    held += __popcll(counted);
                } else if (v >= 0) {
                    atomicAdd(&c.view_counts[v], 1);
                }
            }
        }
        row0 += all;
    }
    if (c.view_counts) {   // what the four waves hold: one integer atomic per view, most often one per workgroup
        if (lane == 0) {
            wave_view[wave] = held_view;
            wave_sum[wave] = held;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                int n = 0;
                bool first = true;   // a view is counted with the first wave that holds it
#pragma unroll
                for (int o = 0; o < kWaves; ++o) {
                    if (wave_view[o] != wave_view[w]) continue;
                    first = first && o >= w;
                    n += wave_sum[o];
                }
                if (first && n > 0) atomicAdd(&c.view_counts[wave_view[w]], n);
            }
        }
    }
}

bool rows_ok(int64_t rows) { return rows >= 1 && rows <= GA_PC_FILTER_MAX_ROWS; }

unsigned long long default_slots(int64_t rows) {
    unsigned long long s = 1;
    while (s < 2ull * (unsigned long long)rows) s <<= 1;
    return s;
}

// 0 for a table the call rejects
unsigned long long slots_of(int64_t rows, int64_t table_slots) {
    if (!rows_ok(rows)) return 0;
    if (table_slots == 0) return default_slots(rows);
    if (table_slots <= rows || table_slots > (int64_t(1) << 31) || (table_slots & (table_slots - 1))) return 0;
    return (unsigned long long)table_slots;
}

void launch_compaction(const Compact &c, hipStream_t st) {
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kThreads), 0, st, c);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3((unsigned)c.num_bands + pad_blocks(c.capacity)), dim3(kThreads), 0, st, c);
}

}  // namespace

extern "C" size_t ga_pc_filter_views_workspace_bytes(int32_t rows) { return rows_ok(rows) ? compact_bytes(rows) : 0; }

extern "C" size_t ga_pc_voxel_thin_workspace_bytes(int32_t rows, int64_t table_slots) {
    const unsigned long long slots = slots_of(rows, table_slots);
    if (!slots) return 0;
    return compact_bytes(rows) + pad16((size_t)rows * 4) + pad16((size_t)slots * 20);
}

extern "C" int ga_pc_filter_views(const GaFilterViewsArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaFilterViewsArgs &a = *args;
    if (!rows_ok(a.rows) || a.capacity < 1 || a.num_views < 1 || a.height < 1 || a.width < 1 ||
        (int64_t)a.num_views * a.height * a.width >= (int64_t(1) << 31))
        return GA_ERR_BAD_SHAPE;
    if ((a.depth_kind != GA_PC_DEPTH_Z && a.depth_kind != GA_PC_DEPTH_RAY) || (a.window != 0 && a.window != 1) || (a.carve != 0 && a.carve != 1) ||
        a.min_support < 0 || a.max_conflicts < 0 || a.reserved != 0)
        return GA_ERR_BAD_FLAGS;
    if (a.depth_min != a.depth_min || a.depth_max != a.depth_max || a.mask_threshold != a.mask_threshold ||
        !(a.tol_abs >= 0.f && a.tol_abs <= 3.0e38f) || !(a.tol_rel >= 0.f && a.tol_rel <= 3.0e38f))
        return GA_ERR_BAD_FLAGS;
    if (!a.points || !a.depth || !a.cameras || !a.out_points || !a.kept_rows || !a.count || !a.workspace) return GA_ERR_NULL_ARG;
    if ((a.colors != nullptr) != (a.out_colors != nullptr) || (a.normals != nullptr) != (a.out_normals != nullptr) ||
        (a.source != nullptr) != (a.out_source != nullptr) || (a.view_counts && !a.source))
        return GA_ERR_NULL_ARG;
    if (a.workspace_bytes < ga_pc_filter_views_workspace_bytes(a.rows) || (reinterpret_cast<uintptr_t>(a.workspace) & 15)) return GA_ERR_WORKSPACE;
    Compact c{};
    c.rows = a.rows; c.capacity = a.capacity; c.num_views = a.num_views; c.view_pixels = a.height * a.width; c.num_bands = bands_of(a.rows);
    c.in_count = a.in_count; c.points = a.points; c.colors = a.colors; c.normals = a.normals; c.source = a.source;
    c.o_points = a.out_points; c.o_colors = a.out_colors; c.o_normals = a.out_normals; c.o_source = a.out_source;
    c.kept_rows = a.kept_rows; c.count = a.count; c.view_counts = a.view_counts;
    c.bands = reinterpret_cast<int32_t *>(a.workspace);
    c.flags = reinterpret_cast<unsigned char *>(a.workspace) + flags_offset(a.rows);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    hipLaunchKernelGGL(filter_vote_kernel, dim3(c.num_bands), dim3(kThreads), 0, st, a, c);
    launch_compaction(c, st);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_pc_voxel_thin(const GaVoxelThinArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaVoxelThinArgs &a = *args;
    if (!rows_ok(a.rows) || a.capacity < 1) return GA_ERR_BAD_SHAPE;
    const unsigned long long slots = slots_of(a.rows, a.table_slots);
    if (!slots || (a.view_counts && (a.num_views < 1 || a.view_pixels < 1))) return GA_ERR_BAD_SHAPE;
    if ((a.keep != GA_PC_VOXEL_FIRST && a.keep != GA_PC_VOXEL_CENTER) || (a.flags & ~GA_PC_VOXEL_WAVE_MERGE)) return GA_ERR_BAD_FLAGS;
    if (!(a.voxel_size > 0.f && a.voxel_size <= 3.0e38f)) return GA_ERR_BAD_FLAGS;
    for (int k = 0; k < 3; ++k)
        if (!(a.origin[k] >= -3.0e38f && a.origin[k] <= 3.0e38f)) return GA_ERR_BAD_FLAGS;
    if (!a.points || !a.out_points || !a.kept_rows || !a.count || !a.workspace) return GA_ERR_NULL_ARG;
    if ((a.colors != nullptr) != (a.out_colors != nullptr) || (a.normals != nullptr) != (a.out_normals != nullptr) ||
        (a.source != nullptr) != (a.out_source != nullptr) || (a.view_counts && !a.source))
        return GA_ERR_NULL_ARG;
    if (a.workspace_bytes < ga_pc_voxel_thin_workspace_bytes(a.rows, a.table_slots) || (reinterpret_cast<uintptr_t>(a.workspace) & 15))
        return GA_ERR_WORKSPACE;
    unsigned char *ws = reinterpret_cast<unsigned char *>(a.workspace);
    Table t;
    t.slot_of = reinterpret_cast<int32_t *>(ws + compact_bytes(a.rows));
    t.keys = reinterpret_cast<unsigned long long *>(ws + compact_bytes(a.rows) + pad16((size_t)a.rows * 4));
    t.ranks = t.keys + slots;
    t.counts = reinterpret_cast<int32_t *>(t.ranks + slots);
    t.slots = slots;
    Compact c{};
    c.rows = a.rows; c.capacity = a.capacity; c.num_views = a.view_counts ? a.num_views : 0; c.view_pixels = a.view_counts ? a.view_pixels : 1;
    c.num_bands = bands_of(a.rows);
    c.in_count = a.in_count; c.points = a.points; c.colors = a.colors; c.normals = a.normals; c.source = a.source;
    c.o_points = a.out_points; c.o_colors = a.out_colors; c.o_normals = a.out_normals; c.o_source = a.out_source;
    c.kept_rows = a.kept_rows; c.count = a.count; c.view_counts = a.view_counts; c.multiplicity = a.multiplicity;
    c.slot_of = t.slot_of; c.slot_count = t.counts;
    c.bands = reinterpret_cast<int32_t *>(ws);
    c.flags = ws + flags_offset(a.rows);
    const unsigned long long clear_blocks = (slots + kThreads - 1) / kThreads;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    hipLaunchKernelGGL(table_clear_kernel, dim3((unsigned)(clear_blocks < 4096 ? clear_blocks : 4096)), dim3(kThreads), 0, st, t, a.dropped);
    hipLaunchKernelGGL(voxel_insert_kernel, dim3((unsigned)((a.rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a, t, c);
    hipLaunchKernelGGL(voxel_flag_kernel, dim3(c.num_bands), dim3(kThreads), 0, st, t, c);
    launch_compaction(c, st);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}
