// pointcloud.hip -- farthest point sampling and nearest point for gfx950 (include/ga_pointcloud.h).
//
// Built with -ffp-contract=off: the squared distance is dx*dx, + dy*dy, + dz*dz with every operation rounded on its own, so the
// results are a function of the inputs alone (tests/_pointcloud_ref.py restates them in numpy float32, bit for bit).
//
// FPS: one workgroup per cloud, K dependent iterations inside ONE launch; no workgroup waits for another.
//   (a) register-resident: lane `tid` keeps points tid, tid + T, tid + 2T, ... (x, y, z, closest) in VGPRs.  Per iteration: P distance
//       updates per lane, the in-lane argmax, a cross-lane argmax of the pair (distance, index) (DPP inside a row of 16, v_readlane
//       across the 4 rows), one LDS partial per wave -- written by the lane that OWNS the wave's winner, with the winner's coordinates
//       -- one __syncthreads(), and every wave scans the partials redundantly.  Two alternating LDS slots make the one barrier enough:
//       a wave that writes slot s again (iteration k + 2) has passed the barrier of iteration k + 1, which every wave reaches only
//       after it has read slot s in iteration k.
//   (b) streaming: the same iteration, the lane's points re-read from memory and `closest` kept in the workspace (each element is
//       only ever touched by the lane that owns it, so no barrier guards it).
//   The order everywhere is "greater distance, or equal distance and lower index"; lanes past the cloud's length carry distance -1
//   and an index >= n, so they never win against a real point (distance >= 0).
// Nearest: queries across lanes, targets staged in LDS in tiles of kNearestTile and read by broadcast (ds_read_b128 of a wave-uniform
//   address: four targets' x, y or z per read); strict `<` while walking targets upwards keeps the lowest index at ties.
// kNN: the same walk, with a sorted list of S = k_slots (distance, index) pairs per lane in registers (one kernel instance per S in
//   1, 2, 4, 8, 16, 32).  A target enters the list through a fully unrolled compare / select chain (compile-time register indices only)
//   that the wave runs only when `d < worst` holds for at least one of its lanes (a ballot: the branch is wave-uniform, the chain is
//   predicated per lane).  The chain places d behind every entry with distance <= d; targets arrive in ascending index, so equal
//   distances stay in index order and the k-th place keeps the lower index.
// kNN backward: query side one lane per query, k' ascending.  Target side one lane per TARGET: the workgroup walks the cloud's (i, k')
//   entries upwards in LDS tiles (index, 2 * grad, the query's coordinates) and a lane accumulates where the index is its own -- the
//   ascending order is the contract's, and no atomics are needed.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/ga_pointcloud.h"

namespace {

constexpr int kWave = 64;
constexpr int kFpsMaxPointsPerLane = 16;                             // 4 VGPRs a point: 64 of the 128 a lane has at 16 waves per CU
constexpr int kFpsStreamThreads = 1024;
constexpr int kFpsRegisterMaxN = 1024 * kFpsMaxPointsPerLane;        // 16384
constexpr int kNearestThreads = 256;
constexpr int kNearestTile = 1024;

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    float d = dx * dx;
    d = d + dy * dy;
    d = d + dz * dz;
    return d;
}

// (d, i) beats (bd, bi)
__device__ __forceinline__ bool beats(float d, int i, float bd, int bi) { return d > bd || (d == bd && i < bi); }

template <int CTRL>
__device__ __forceinline__ void dpp_step(float &d, int &i) {
    const float od = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d), CTRL, 0xf, 0xf, false));
    const int oi = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xf, 0xf, false);
    if (beats(od, oi, d, i)) { d = od; i = oi; }
}

// all-reduce of (distance, index) over the 64 lanes of a wave; every lane active.  The four DPP patterns (quad xor 1, quad xor 2,
// mirror within 8, mirror within 16) leave each row of 16 lanes holding its winner; the four rows are combined from SGPRs.
__device__ __forceinline__ void wave_argmax(float &d, int &i) {
    dpp_step<0xB1>(d, i);   // quad_perm [1,0,3,2]
    dpp_step<0x4E>(d, i);   // quad_perm [2,3,0,1]
    dpp_step<0x141>(d, i);  // row_half_mirror
    dpp_step<0x140>(d, i);  // row_mirror
    float bd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 0));
    int bi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        const float od = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 16 * r));
        const int oi = __builtin_amdgcn_readlane(i, 16 * r);
        if (beats(od, oi, bd, bi)) { bd = od; bi = oi; }
    }
    d = bd;
    i = bi;
}

struct FpsPartials {   // one entry per wave, two alternating slots
    float d[2][16];
    int i[2][16];
    float x[2][16], y[2][16], z[2][16];
};

// the part of an iteration both variants share: from every lane's candidate (bd, bi, bx, by, bz) to the workgroup's winner in all lanes
template <int W>
__device__ __forceinline__ void block_argmax(FpsPartials &lds, int slot, int wave, float &bd, int &bi, float &bx, float &by, float &bz) {
    float wd = bd;
    int wi = bi;
    wave_argmax(wd, wi);
    if (W == 1) {   // one wave: the owner's coordinates by v_readlane -- no LDS, no barrier
        const int owner = __builtin_ctzll(__ballot(bi == wi));
        bd = wd;
        bi = wi;
        bx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bx), owner));
        by = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(by), owner));
        bz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bz), owner));
        return;
    }
    if (bi == wi) {   // indices are unique per lane: exactly one owner
        lds.d[slot][wave] = wd;
        lds.i[slot][wave] = wi;
        lds.x[slot][wave] = bx;
        lds.y[slot][wave] = by;
        lds.z[slot][wave] = bz;
    }
    __syncthreads();
    bd = lds.d[slot][0]; bi = lds.i[slot][0]; bx = lds.x[slot][0]; by = lds.y[slot][0]; bz = lds.z[slot][0];
#pragma unroll
    for (int w = 1; w < W; ++w) {
        const float od = lds.d[slot][w];
        const int oi = lds.i[slot][w];
        if (beats(od, oi, bd, bi)) { bd = od; bi = oi; bx = lds.x[slot][w]; by = lds.y[slot][w]; bz = lds.z[slot][w]; }
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void fps_emit(int32_t *oi, float *op, int k, int sel, float sx, float sy, float sz) {
    oi[k] = sel;
    if (op) { op[3 * (size_t)k] = sx; op[3 * (size_t)k + 1] = sy; op[3 * (size_t)k + 2] = sz; }
}

__device__ __forceinline__ void fps_pad(int32_t *oi, float *op, int from, int K, int tid, int T) {
    for (int k = from + tid; k < K; k += T) {
        oi[k] = -1;
        if (op) { op[3 * (size_t)k] = 0.f; op[3 * (size_t)k + 1] = 0.f; op[3 * (size_t)k + 2] = 0.f; }
    }
}

// (a) register-resident: T lanes, P points a lane
template <int T, int P>
__global__ __launch_bounds__(T) void fps_register_kernel(const float *__restrict__ points, const int32_t *__restrict__ lengths,
                                                         const int32_t *__restrict__ start_idx, int N, int K,
                                                         int32_t *__restrict__ out_idx, float *__restrict__ out_points) {
    constexpr int W = T / kWave;
    __shared__ FpsPartials lds;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid / kWave;
    const int n = clampi(lengths ? lengths[b] : N, 0, N);
    const float *p = points + (size_t)b * N * 3;
    int32_t *oi = out_idx + (size_t)b * K;
    float *op = out_points ? out_points + (size_t)b * K * 3 : nullptr;
    const int m = K < n ? K : n;
    if (m > 0) {
        float x[P], y[P], z[P], c[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int i = j * T + tid;
            const bool live = i < n;
            x[j] = live ? p[3 * (size_t)i] : 0.f;
            y[j] = live ? p[3 * (size_t)i + 1] : 0.f;
            z[j] = live ? p[3 * (size_t)i + 2] : 0.f;
            c[j] = live ? __builtin_inff() : -1.f;
        }
        int sel = clampi(start_idx ? start_idx[b] : 0, 0, n - 1);
        float sx = p[3 * (size_t)sel], sy = p[3 * (size_t)sel + 1], sz = p[3 * (size_t)sel + 2];
        for (int k = 0;; ++k) {
            if (tid == 0) fps_emit(oi, op, k, sel, sx, sy, sz);
            if (k + 1 == m) break;
            float bd = -2.f, bx = 0.f, by = 0.f, bz = 0.f;
            int bi = tid;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const float d = dist2(x[j], y[j], z[j], sx, sy, sz);
                c[j] = c[j] < d ? c[j] : d;      // a dead slot stays -1: d >= 0
                if (c[j] > bd) { bd = c[j]; bi = j * T + tid; bx = x[j]; by = y[j]; bz = z[j]; }   // ascending index: `>` keeps the lowest
            }
            block_argmax<W>(lds, k & 1, wave, bd, bi, bx, by, bz);
            sel = bi; sx = bx; sy = by; sz = bz;
        }
    }
    fps_pad(oi, op, m, K, tid, T);
}

// (b) streaming: lane tid walks points tid, tid + T, ...; closest [B,N] in the workspace
__global__ __launch_bounds__(kFpsStreamThreads) void fps_stream_kernel(const float *__restrict__ points, const int32_t *__restrict__ lengths,
                                                                       const int32_t *__restrict__ start_idx, int N, int K,
                                                                       int32_t *__restrict__ out_idx, float *__restrict__ out_points,
                                                                       float *__restrict__ closest_all) {
    constexpr int T = kFpsStreamThreads, W = T / kWave;
    __shared__ FpsPartials lds;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid / kWave;
    const int n = clampi(lengths ? lengths[b] : N, 0, N);
    const float *p = points + (size_t)b * N * 3;
    float *closest = closest_all + (size_t)b * N;
    int32_t *oi = out_idx + (size_t)b * K;
    float *op = out_points ? out_points + (size_t)b * K * 3 : nullptr;
    const int m = K < n ? K : n;
    if (m > 0) {
        for (int i = tid; i < n; i += T) closest[i] = __builtin_inff();
        int sel = clampi(start_idx ? start_idx[b] : 0, 0, n - 1);
        float sx = p[3 * (size_t)sel], sy = p[3 * (size_t)sel + 1], sz = p[3 * (size_t)sel + 2];
        for (int k = 0;; ++k) {
            if (tid == 0) fps_emit(oi, op, k, sel, sx, sy, sz);
            if (k + 1 == m) break;
            float bd = -2.f, bx = 0.f, by = 0.f, bz = 0.f;
            int bi = N + tid;   // unique, past every real index
#pragma unroll 4
            for (int i = tid; i < n; i += T) {
                const float x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
                const float d = dist2(x, y, z, sx, sy, sz);
                float c = closest[i];
                c = c < d ? c : d;
                closest[i] = c;
                if (c > bd) { bd = c; bi = i; bx = x; by = y; bz = z; }
            }
            block_argmax<W>(lds, k & 1, wave, bd, bi, bx, by, bz);
            sel = bi; sx = bx; sy = by; sz = bz;
        }
    }
    fps_pad(oi, op, m, K, tid, T);
}

__global__ __launch_bounds__(kNearestThreads) void nearest_kernel(const float *__restrict__ query, const float *__restrict__ target,
                                                                  const int32_t *__restrict__ qlen, const int32_t *__restrict__ tlen,
                                                                  int Nq, int Nt, float *__restrict__ out_d, int32_t *__restrict__ out_i) {
    __shared__ __attribute__((aligned(16))) float tx[kNearestTile], ty[kNearestTile], tz[kNearestTile];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int q = blockIdx.x * kNearestThreads + tid;
    const int nq = clampi(qlen ? qlen[b] : Nq, 0, Nq), nt = clampi(tlen ? tlen[b] : Nt, 0, Nt);
    if (blockIdx.x * kNearestThreads >= nq) {   // the whole block is padding (block-uniform: no barrier is skipped by a part of it)
        if (q < Nq) { out_d[(size_t)b * Nq + q] = 0.f; out_i[(size_t)b * Nq + q] = -1; }
        return;
    }
    const float *qp = query + (size_t)b * Nq * 3, *tp = target + (size_t)b * Nt * 3;
    const bool live = q < nq;
    const float qx = live ? qp[3 * (size_t)q] : 0.f, qy = live ? qp[3 * (size_t)q + 1] : 0.f, qz = live ? qp[3 * (size_t)q + 2] : 0.f;
    float best = __builtin_inff();
    int besti = -1;
    for (int t0 = 0; t0 < nt; t0 += kNearestTile) {
        const int cnt = nt - t0 < kNearestTile ? nt - t0 : kNearestTile;
        __syncthreads();   // the previous tile has been read by every wave
        for (int j = tid; j < cnt; j += kNearestThreads) {
            const size_t g = 3 * (size_t)(t0 + j);
            tx[j] = tp[g]; ty[j] = tp[g + 1]; tz[j] = tp[g + 2];
        }
        __syncthreads();
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float d = dist2(qx, qy, qz, tx[j + u], ty[j + u], tz[j + u]);
                if (d < best) { best = d; besti = t0 + j + u; }
            }
        }
        for (; j < cnt; ++j) {
            const float d = dist2(qx, qy, qz, tx[j], ty[j], tz[j]);
            if (d < best) { best = d; besti = t0 + j; }
        }
    }
    if (q < Nq) {
        out_d[(size_t)b * Nq + q] = live ? best : 0.f;
        out_i[(size_t)b * Nq + q] = live ? besti : -1;
    }
}

constexpr int kKnnThreads = 256;
constexpr int kKnnTile = 1024;
constexpr int kKnnGradTile = 1024;   // (i, k') entries staged per tile of the target-side backward

// (d, t) into the ascending list behind every entry with distance <= d; a lane with d >= ld[S - 1] changes nothing.  Walking downwards,
// ld[s - 1] is still the old value when slot s is rewritten.  With ld[s - 1] <= ld[s] the new distance of slot s is the MEDIAN of
// (d, ld[s - 1], ld[s]) -- ld[s - 1] when d is below it (shift), d when it lies between, ld[s] otherwise: one v_med3_f32, which selects
// one of its operands and rounds nothing.  The index follows with one compare per slot (shared by two neighbouring slots) and two selects.
template <int S>
__device__ __forceinline__ void knn_insert(float (&ld)[S], int (&li)[S], float d, int t) {
    bool here = d < ld[S - 1];
#pragma unroll
    for (int s = S - 1; s >= 1; --s) {
        const bool shift = d < ld[s - 1];
        const int keep = here ? t : li[s];
        li[s] = shift ? li[s - 1] : keep;
        ld[s] = __builtin_amdgcn_fmed3f(d, ld[s - 1], ld[s]);
        here = shift;
    }
    li[0] = here ? t : li[0];
    ld[0] = here ? d : ld[0];
}

template <int S>
__device__ __forceinline__ void knn_offer(float (&ld)[S], int (&li)[S], float d, int t) {
    if (__ballot(d < ld[S - 1]) != 0) knn_insert<S>(ld, li, d, t);   // wave-uniform branch around the per-lane predicated chain
}

template <int S>
__global__ __launch_bounds__(kKnnThreads) void knn_kernel(const float *__restrict__ query, const float *__restrict__ target,
                                                          const int32_t *__restrict__ qlen, const int32_t *__restrict__ tlen, int Nq,
                                                          int Nt, int k, float *__restrict__ out_d, int32_t *__restrict__ out_i) {
    __shared__ __attribute__((aligned(16))) float tx[kKnnTile], ty[kKnnTile], tz[kKnnTile];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int q = blockIdx.x * kKnnThreads + tid;
    const int nq = clampi(qlen ? qlen[b] : Nq, 0, Nq), nt = clampi(tlen ? tlen[b] : Nt, 0, Nt);
    const size_t o = ((size_t)b * Nq + (size_t)q) * (size_t)k;
    if (blockIdx.x * kKnnThreads >= nq) {   // the whole block is padding (block-uniform: no barrier is skipped by a part of it)
        if (q < Nq)
            for (int s = 0; s < k; ++s) { out_d[o + s] = 0.f; out_i[o + s] = 0; }
        return;
    }
    const float *qp = query + (size_t)b * Nq * 3, *tp = target + (size_t)b * Nt * 3;
    const bool live = q < nq;
    const float qx = live ? qp[3 * (size_t)q] : 0.f, qy = live ? qp[3 * (size_t)q + 1] : 0.f, qz = live ? qp[3 * (size_t)q + 2] : 0.f;
    float ld[S];
    int li[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        ld[s] = live ? __builtin_inff() : -__builtin_inff();   // a dead lane never asks for the chain: no d is below -inf
        li[s] = 0;
    }
    for (int t0 = 0; t0 < nt; t0 += kKnnTile) {
        const int cnt = nt - t0 < kKnnTile ? nt - t0 : kKnnTile;
        __syncthreads();   // the previous tile has been read by every wave
        for (int j = tid; j < cnt; j += kKnnThreads) {
            const size_t g = 3 * (size_t)(t0 + j);
            tx[j] = tp[g]; ty[j] = tp[g + 1]; tz[j] = tp[g + 2];
        }
        __syncthreads();
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) knn_offer<S>(ld, li, dist2(qx, qy, qz, tx[j + u], ty[j + u], tz[j + u]), t0 + j + u);
        }
        for (; j < cnt; ++j) knn_offer<S>(ld, li, dist2(qx, qy, qz, tx[j], ty[j], tz[j]), t0 + j);
    }
    if (q < Nq) {
        const int m = live ? (k < nt ? k : nt) : 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (s < k) {
                out_d[o + s] = s < m ? ld[s] : 0.f;
                out_i[o + s] = s < m ? li[s] : 0;
            }
        }
    }
}

__global__ __launch_bounds__(kKnnThreads) void knn_grad_query_kernel(const float *__restrict__ query, const float *__restrict__ target,
                                                                     const int32_t *__restrict__ qlen, const int32_t *__restrict__ tlen,
                                                                     const int32_t *__restrict__ idx, const float *__restrict__ grad, int Nq,
                                                                     int Nt, int k, float *__restrict__ gq) {
    const int b = blockIdx.y, q = blockIdx.x * kKnnThreads + threadIdx.x;
    if (q >= Nq) return;
    const int nq = clampi(qlen ? qlen[b] : Nq, 0, Nq), nt = clampi(tlen ? tlen[b] : Nt, 0, Nt);
    const int m = k < nt ? k : nt;
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (q < nq) {
        const float *qp = query + ((size_t)b * Nq + (size_t)q) * 3, *tp = target + (size_t)b * Nt * 3;
        const size_t o = ((size_t)b * Nq + (size_t)q) * (size_t)k;
        const float qx = qp[0], qy = qp[1], qz = qp[2];
        for (int s = 0; s < m; ++s) {
            const int j = clampi(idx[o + s], 0, nt - 1);   // a valid pair's index is in range by contract; the clamp keeps a broken one inside the buffer
            const float c = 2.f * grad[o + s];
            ax = ax + c * (qx - tp[3 * (size_t)j]);
            ay = ay + c * (qy - tp[3 * (size_t)j + 1]);
            az = az + c * (qz - tp[3 * (size_t)j + 2]);
        }
    }
    float *out = gq + ((size_t)b * Nq + (size_t)q) * 3;
    out[0] = ax; out[1] = ay; out[2] = az;
}

__global__ __launch_bounds__(kKnnThreads) void knn_grad_target_kernel(const float *__restrict__ query, const float *__restrict__ target,
                                                                      const int32_t *__restrict__ qlen, const int32_t *__restrict__ tlen,
                                                                      const int32_t *__restrict__ idx, const float *__restrict__ grad, int Nq,
                                                                      int Nt, int k, float *__restrict__ gt) {
    __shared__ __attribute__((aligned(16))) int si[kKnnGradTile];
    __shared__ float sc[kKnnGradTile], sx[kKnnGradTile], sy[kKnnGradTile], sz[kKnnGradTile];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int j = blockIdx.x * kKnnThreads + tid;
    const int nq = clampi(qlen ? qlen[b] : Nq, 0, Nq), nt = clampi(tlen ? tlen[b] : Nt, 0, Nt);
    float *out = gt + ((size_t)b * Nt + (size_t)j) * 3;
    if (blockIdx.x * kKnnThreads >= nt) {   // the whole block is padding (block-uniform)
        if (j < Nt) { out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; }
        return;
    }
    const int m = k < nt ? k : nt;
    const float *qp = query + (size_t)b * Nq * 3, *tp = target + (size_t)b * Nt * 3;
    const int32_t *ip = idx + (size_t)b * Nq * (size_t)k;
    const float *gp = grad + (size_t)b * Nq * (size_t)k;
    const bool live = j < nt;
    const int mine = live ? j : -2;   // staged indices are >= -1: a dead lane matches nothing
    const float px = live ? tp[3 * (size_t)j] : 0.f, py = live ? tp[3 * (size_t)j + 1] : 0.f, pz = live ? tp[3 * (size_t)j + 2] : 0.f;
    float ax = 0.f, ay = 0.f, az = 0.f;
    const int total = nq * k;   // <= Nq * k < 2^31
    for (int e0 = 0; e0 < total; e0 += kKnnGradTile) {
        const int cnt = total - e0 < kKnnGradTile ? total - e0 : kKnnGradTile;
        const int cnt4 = (cnt + 3) & ~3;
        __syncthreads();   // the previous tile has been read by every wave
        for (int l = tid; l < cnt4; l += kKnnThreads) {
            const int e = e0 + l;
            const int i = e / k, s = e - i * k;
            const bool valid = l < cnt && s < m;   // validity from the lengths; the index of an invalid pair is not even read
            si[l] = valid ? ip[e] : -1;
            sc[l] = valid ? 2.f * gp[e] : 0.f;
            sx[l] = valid ? qp[3 * (size_t)i] : 0.f;
            sy[l] = valid ? qp[3 * (size_t)i + 1] : 0.f;
            sz[l] = valid ? qp[3 * (size_t)i + 2] : 0.f;
        }
        __syncthreads();
        for (int l = 0; l < cnt4; l += 4) {
            const int i0 = si[l], i1 = si[l + 1], i2 = si[l + 2], i3 = si[l + 3];
            if (__ballot(i0 == mine || i1 == mine || i2 == mine || i3 == mine) == 0) continue;   // wave-uniform
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if ((u == 0 ? i0 : u == 1 ? i1 : u == 2 ? i2 : i3) == mine) {
                    const float c = sc[l + u];
                    ax = ax + (-(c * (sx[l + u] - px)));
                    ay = ay + (-(c * (sy[l + u] - py)));
                    az = az + (-(c * (sz[l + u] - pz)));
                }
            }
        }
    }
    if (j < Nt) { out[0] = ax; out[1] = ay; out[2] = az; }
}

bool knn_shape_ok(int64_t B, int64_t Nq, int64_t Nt, int64_t k, int64_t kmax) {
    const int64_t lim = int64_t(1) << 31;
    return B > 0 && B <= GA_PC_MAX_BATCH && Nq > 0 && Nt > 0 && k >= 1 && k <= kmax && Nq * 3 < lim && Nt * 3 < lim && Nq * k < lim;
}

void knn_plan(int Nq, int k, GaKnnPlan &pl) {
    int S = 1;
    while (S < k) S *= 2;
    pl.k_slots = S;
    pl.threads = kKnnThreads;
    pl.tile = kKnnTile;
    pl.grid_x = (Nq + kKnnThreads - 1) / kKnnThreads;
    pl.grid_y = 1;
}

template <int S>
void launch_knn(const GaKnnArgs &a, const GaKnnPlan &pl, hipStream_t s) {
    hipLaunchKernelGGL((knn_kernel<S>), dim3(pl.grid_x, pl.grid_y * a.batch), dim3(pl.threads), 0, s, a.query, a.target, a.query_lengths,
                       a.target_lengths, a.num_query, a.num_target, a.k, a.out_dist2, a.out_idx);
}

bool fps_shape_ok(int64_t B, int64_t N, int64_t K) {
    return B > 0 && B <= GA_PC_MAX_BATCH && N > 0 && K > 0 && N * 3 < (int64_t(1) << 31);
}

void fps_plan(int N, GaFpsPlan &pl) {
    if (N > kFpsRegisterMaxN) {
        pl.variant = GA_FPS_VARIANT_STREAMING;
        pl.threads = kFpsStreamThreads;
        pl.points_per_lane = (N + kFpsStreamThreads - 1) / kFpsStreamThreads;
        return;
    }
    pl.variant = GA_FPS_VARIANT_REGISTER;
    // the smallest workgroup that holds the cloud at <= 16 points a lane: fewer waves make the per-iteration barrier and the scan of
    // the partials cheaper, and the distance updates are a small part of an iteration
    pl.threads = N <= 64 ? 64 : (N <= 256 * kFpsMaxPointsPerLane ? 256 : 1024);
    int P = 1;
    while (pl.threads * P < N) P *= 2;
    pl.points_per_lane = P;
}

template <int T, int P>
void launch_fps_register(const GaFpsArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((fps_register_kernel<T, P>), dim3(a.batch), dim3(T), 0, s, a.points, a.lengths, a.start_idx, a.num_points,
                       a.num_samples, a.out_idx, a.out_points);
}

}  // namespace

extern "C" int ga_pc_fps_plan(int32_t num_points, int32_t num_samples, GaFpsPlan *plan) {
    if (!plan) return GA_ERR_NULL_ARG;
    if (!fps_shape_ok(1, num_points, num_samples)) return GA_ERR_BAD_SHAPE;
    fps_plan(num_points, *plan);
    return GA_OK;
}

extern "C" size_t ga_pc_fps_workspace_bytes(int32_t batch, int32_t num_points, int32_t num_samples) {
    if (!fps_shape_ok(batch, num_points, num_samples)) return 0;
    GaFpsPlan pl;
    fps_plan(num_points, pl);
    return pl.variant == GA_FPS_VARIANT_STREAMING ? (size_t)batch * (size_t)num_points * sizeof(float) : 0;
}

extern "C" int ga_pc_fps(const GaFpsArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaFpsArgs &a = *args;
    if (!fps_shape_ok(a.batch, a.num_points, a.num_samples)) return GA_ERR_BAD_SHAPE;
    if (!a.points || !a.out_idx) return GA_ERR_NULL_ARG;
    const size_t need = ga_pc_fps_workspace_bytes(a.batch, a.num_points, a.num_samples);
    if (need > 0 && !a.workspace) return GA_ERR_NULL_ARG;
    if (a.workspace_bytes < need) return GA_ERR_WORKSPACE;
    GaFpsPlan pl;
    fps_plan(a.num_points, pl);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    if (pl.variant == GA_FPS_VARIANT_STREAMING) {
        hipLaunchKernelGGL(fps_stream_kernel, dim3(a.batch), dim3(kFpsStreamThreads), 0, s, a.points, a.lengths, a.start_idx,
                           a.num_points, a.num_samples, a.out_idx, a.out_points, static_cast<float *>(a.workspace));
    } else {
        switch (pl.threads * 100 + pl.points_per_lane) {
            case 64 * 100 + 1: launch_fps_register<64, 1>(a, s); break;
            case 256 * 100 + 1: launch_fps_register<256, 1>(a, s); break;
            case 256 * 100 + 2: launch_fps_register<256, 2>(a, s); break;
            case 256 * 100 + 4: launch_fps_register<256, 4>(a, s); break;
            case 256 * 100 + 8: launch_fps_register<256, 8>(a, s); break;
            case 256 * 100 + 16: launch_fps_register<256, 16>(a, s); break;
            case 1024 * 100 + 8: launch_fps_register<1024, 8>(a, s); break;
            case 1024 * 100 + 16: launch_fps_register<1024, 16>(a, s); break;
            default: return GA_ERR_BAD_SHAPE;   // unreachable: fps_plan yields only the instances above
        }
    }
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_pc_nearest(const GaNearestArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaNearestArgs &a = *args;
    if (a.batch <= 0 || a.batch > GA_PC_MAX_BATCH || a.num_query <= 0 || a.num_target <= 0 ||
        (int64_t)a.num_query * 3 >= (int64_t(1) << 31) || (int64_t)a.num_target * 3 >= (int64_t(1) << 31))
        return GA_ERR_BAD_SHAPE;
    if (!a.query || !a.target || !a.out_dist2 || !a.out_idx) return GA_ERR_NULL_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    const unsigned blocks = (unsigned)((a.num_query + kNearestThreads - 1) / kNearestThreads);
    hipLaunchKernelGGL(nearest_kernel, dim3(blocks, a.batch), dim3(kNearestThreads), 0, s, a.query, a.target, a.query_lengths,
                       a.target_lengths, a.num_query, a.num_target, a.out_dist2, a.out_idx);
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_pc_knn_plan(int32_t num_query, int32_t num_target, int32_t k, GaKnnPlan *plan) {
    if (!plan) return GA_ERR_NULL_ARG;
    if (!knn_shape_ok(1, num_query, num_target, k, GA_PC_KNN_MAX_K)) return GA_ERR_BAD_SHAPE;
    knn_plan(num_query, k, *plan);
    return GA_OK;
}

extern "C" int ga_pc_knn(const GaKnnArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaKnnArgs &a = *args;
    if (!knn_shape_ok(a.batch, a.num_query, a.num_target, a.k, GA_PC_KNN_MAX_K)) return GA_ERR_BAD_SHAPE;
    if (!a.query || !a.target || !a.out_dist2 || !a.out_idx) return GA_ERR_NULL_ARG;
    GaKnnPlan pl;
    knn_plan(a.num_query, a.k, pl);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    switch (pl.k_slots) {
        case 1: launch_knn<1>(a, pl, s); break;
        case 2: launch_knn<2>(a, pl, s); break;
        case 4: launch_knn<4>(a, pl, s); break;
        case 8: launch_knn<8>(a, pl, s); break;
        case 16: launch_knn<16>(a, pl, s); break;
        case 32: launch_knn<32>(a, pl, s); break;
        default: return GA_ERR_BAD_SHAPE;   // unreachable: knn_plan yields only the instances above
    }
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}

extern "C" int ga_pc_knn_backward(const GaKnnBackwardArgs *args, void *stream_v) {
    if (!args) return GA_ERR_NULL_ARG;
    const GaKnnBackwardArgs &a = *args;
    if (!knn_shape_ok(a.batch, a.num_query, a.num_target, a.k, INT32_MAX)) return GA_ERR_BAD_SHAPE;
    if (!a.query || !a.target || !a.idx || !a.grad_dist2) return GA_ERR_NULL_ARG;
    if (!a.grad_query && !a.grad_target) return GA_OK;   // nothing asked for
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_v);
    (void)hipGetLastError();
    if (a.grad_query) {
        const unsigned blocks = (unsigned)((a.num_query + kKnnThreads - 1) / kKnnThreads);
        hipLaunchKernelGGL(knn_grad_query_kernel, dim3(blocks, a.batch), dim3(kKnnThreads), 0, s, a.query, a.target, a.query_lengths,
                           a.target_lengths, a.idx, a.grad_dist2, a.num_query, a.num_target, a.k, a.grad_query);
    }
    if (a.grad_target) {
        const unsigned blocks = (unsigned)((a.num_target + kKnnThreads - 1) / kKnnThreads);
        hipLaunchKernelGGL(knn_grad_target_kernel, dim3(blocks, a.batch), dim3(kKnnThreads), 0, s, a.query, a.target, a.query_lengths,
                           a.target_lengths, a.idx, a.grad_dist2, a.num_query, a.num_target, a.k, a.grad_target);
    }
    return hipGetLastError() == hipSuccess ? GA_OK : GA_ERR_LAUNCH;
}
