// dit_attention_short.hip -- attention forward for SHORT key lists (Lk <= 128), head_dim 64, bf16 MFMA, gfx950.
//
// The cross-attention of the text denoisers (/root/reference/dit/dit_models_xformers.py:357-376 on 77 caption tokens): 768 queries x 77
// keys per head.  attention_fwd_kernel (dit_attention.hip) picks its configuration by Lq alone and walks such a list with key groups, a
// three-slot ring, a running maximum with rescale and an LDS merge -- machinery for key lists that do not fit LDS.  Here the whole list
// does:
//   * a workgroup = 4 waves x 16 queries of one (batch, head); grid (heads * batch, ceil(Lq / 64)) head-major as in dit_attention.hip;
//   * K and V^T of the head (at most two 64-key tiles each, 32 KiB) are staged ONCE by LDS-DMA, requested before anything else, in the
//     swizzled row-major image of dit_attention.hip (the fragment reads and lane <-> element maps are the same code:
//     dit_attention_common.h);
//   * one S^T = K Q^T pass over at most 8 key fragments (key columns >= Lk masked), ONE-PASS softmax with the true row maximum -- no
//     rescale, no merge --, then O^T = V^T P^T;
//   * q is either given or projected inside the workgroup (GaAttentionArgs.qp_*) by the code attention_fwd_kernel<4,3> projects it
//     with (QProjection, dit_attention_common.h: fp32 accumulation over the slices in order, row scale, per-head RMSNorm, rounded to
//     bf16 as the projection GEMM would have stored it, then the softmax scale); this kernel's own part is how the slices arrive: A /
//     W K-slices staged by LDS-DMA into a three-slot ring behind the K / V^T tiles (two slices ahead, one counted vmcnt + one raw
//     barrier per slice), every wave taking every slice.
// vmcnt accounting: every wave issues its K / V^T DMA instructions first (4 per key tile: 4 or 8), then 4 per K-slice of the projection;
// waiting for slice t with slice t + 1 in flight is vmcnt(4) -- the counter retires in order, so everything older than the 4
// instructions of slice t + 1, the K / V^T pieces included, has landed by the first such wait.
// LDS: the K / V^T tiles of the instantiation (16 KiB per key tile) and, only where q is projected inside (QP), the 48 KiB ring.
#include <algorithm>

#include "dit_attention_common.h"

namespace gadit {
namespace {

constexpr int SQ = 64, MAXT = 2;

// workgroups behind the attention grid (y slices >= y0) that pull weight ranges towards the Infinity Cache (dit_common.h: PrefetchJob) on
// the CUs the grid leaves idle; nwgs == 0: none
struct ShortTail {
    PrefetchJob pf;
    int y0, nwgs;
};

template <int NT, bool QP>   // key tiles: 1 (Lk <= 64) or 2; QP: q projected inside (a.qp_a != nullptr)
__global__ __launch_bounds__(256) void attention_short_kernel(GaAttentionArgs a, ShortTail tail)
{
    if (tail.nwgs > 0 && (int)blockIdx.y >= tail.y0) {   // workgroup-uniform
        prefetch_block(tail.pf, ((int)blockIdx.y - tail.y0) * (int)gridDim.x + (int)blockIdx.x, tail.nwgs);
        return;
    }
    // K[NT][key][d] | V^T[NT][d][key] | QP: ring of the q projection, 3 x (W slice [64 head rows][64], A slice [64 queries][64])
    __shared__ __attribute__((aligned(16))) uint16_t smem[(2 * NT + (QP ? 6 : 0)) * TILE];
    uint16_t *sK = smem, *sV = smem + NT * TILE, *sR = smem + 2 * NT * TILE;
    (void)sR;
    const int tid = threadIdx.x, lane = tid & 63, wq = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    const int b = blockIdx.x / a.heads, h = blockIdx.x - b * a.heads, q0 = blockIdx.y * SQ + wq * 16;
    const int Lq = a.Lq, Lk = a.Lk;
    const int nfull = Lk / KB;
    const uint16_t *vt_base = a.vt + ((size_t)b * a.heads + h) * HD * a.vt_ld;
    const uint16_t *k_base = a.k + (size_t)b * Lk * a.k_stride + h * HD;

    // ---- K / V^T of the head, once: piece p (0..15) of a tile is 8 rows (p < 8: K rows 8p .., else V^T rows 8(p-8) ..); wave wq moves
    // pieces 4 wq .. 4 wq + 3 of every tile; lane l -> row 8p + (l>>3), LDS slot l&7 <- global chunk slot ^ swz
#pragma unroll
    for (int tile = 0; tile < NT; ++tile)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = wq * 4 + i, r8 = (p & 7) * 8, row = r8 + (lane >> 3), chunk = (lane & 7) ^ swz_of(row);
            if (p < 8) {     // wave-uniform.  Rows behind the last key re-read it (masked below)
                const int key = min(tile * KB + row, Lk - 1);
                glds16(k_base + (size_t)key * a.k_stride + chunk * 8, sK + tile * TILE + r8 * 64);
            } else {
                glds16(vt_base + (size_t)row * a.vt_ld + tile * KB + chunk * 8, sV + tile * TILE + r8 * 64);
            }
        }

    // ---- Q fragments (B operand of S^T = K Q^T): lane holds Q[q0 + c16][kk*32 + g*8 .. +7], normalised, scaled
    bf16x8 qf[2];
    if constexpr (QP) {   // the q projection inside the workgroup (QProjection, dit_attention_common.h), slice by slice through a ring of its own
        QProjection qp;
        qp.setup(a, b, h, q0, wq, lane);
        auto dma_q = [&](int sl_raw, int slot) {
            uint16_t *dw = sR + slot * 2 * TILE;
            qp.issue(sl_raw, dw, dw + TILE);
        };
        f32x4 acc[4];
#pragma unroll
        for (int kf = 0; kf < 4; ++kf) acc[kf] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int krow = 8 * (c16 >> 2) + (c16 & 3);
        int s0 = 0, s1 = 1, s2 = 2;
        dma_q(0, 0);
        dma_q(1, 1);
        for (int t = 0; t < qp.nsl; ++t) {
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // my pieces of slice t (and of K / V^T, issued before); slice t + 1 may be in flight
            __builtin_amdgcn_s_barrier();                        // everyone's pieces have landed, everyone has left slice t - 1
            __builtin_amdgcn_sched_barrier(0);
            const uint16_t *bk = sR + s0 * 2 * TILE, *bx = bk + TILE;
            bf16x8 frag[4][2], xf[2];      // (the slice step, as in attention_fwd_kernel's projection: not a shared helper, see dit_attention_common.h)
#pragma unroll
            for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
                    frag[kf][kk] = *reinterpret_cast<const bf16x8 *>(bk + swz((kf >> 1) * 32 + (kf & 1) * 4 + krow, kk * 4 + g));
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) xf[kk] = *reinterpret_cast<const bf16x8 *>(bx + swz(wq * 16 + c16, kk * 4 + g));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int kf = 0; kf < 4; ++kf) acc[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag[kf][kk], xf[kk], acc[kf], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            dma_q(t + 2, s2);     // the slot slice t - 1 left (everybody is past this step's barrier)
            __builtin_amdgcn_sched_barrier(0);
            const int r = s0; s0 = s1; s1 = s2; s2 = r;
        }
        qp.finish(a, acc, qf);
    } else {
        q_frags_from_memory(a, b, h, min(q0 + c16, Lq - 1), g, qf);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // K / V^T (and the projection's last re-fetches: no DMA outlives the workgroup's LDS)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    // ---- S^T = K Q^T : s[tile][kf][r] <-> key 64 tile + (kf>>1)*32 + g*8 + (kf&1)*4 + r, query c16
    f32x4 s[NT][4];
#pragma unroll
    for (int tile = 0; tile < NT; ++tile) {
        bf16x8 frag[4][2];
        kq_frags(sK + tile * TILE, c16, g, frag);
#pragma unroll
        for (int kf = 0; kf < 4; ++kf) s[tile][kf] = f32x4{0.f, 0.f, 0.f, 0.f};
        kq_mfma(frag, qf, s[tile]);
        if (tile >= nfull) {     // kernel-uniform: the ragged tile
            const int kbase = tile * KB + g * 8;
#pragma unroll
            for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kbase + (kf >> 1) * 32 + (kf & 1) * 4 + r >= Lk) s[tile][kf][r] = -1e30f;
        }
    }
    // the V^T fragments land while the softmax runs
    bf16x8 vf[NT][4][2];
#pragma unroll
    for (int tile = 0; tile < NT; ++tile)
#pragma unroll
        for (int df = 0; df < 4; ++df)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) vf[tile][df][kb] = *reinterpret_cast<const bf16x8 *>(sV + tile * TILE + swz(df * 16 + c16, kb * 4 + g));
    // ---- one-pass softmax with the true row maximum (key 0 always exists: the maximum is a real score)
    float m = s[0][0][0];
#pragma unroll
    for (int tile = 0; tile < NT; ++tile)
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
#pragma unroll
            for (int r = 0; r < 4; ++r) m = fmaxf(m, s[tile][kf][r]);
    m = group_max(m);
    bf16x8 pf[NT][2];
    float l = 0.f;
#pragma unroll
    for (int tile = 0; tile < NT; ++tile)
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(s[tile][kf][r] - m);
                l += p;
                pf[tile][kf >> 1][(kf & 1) * 4 + r] = (short)f32_to_bf16(p);
            }
    // ---- O^T = V^T P^T : o[df][r] = O[q = c16][d = df*16 + g*4 + r]; the lane's 8 P of block kb are keys 64 tile + 32 kb + 8 g ..
    f32x4 o[4];
#pragma unroll
    for (int df = 0; df < 4; ++df) o[df] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tile = 0; tile < NT; ++tile)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int df = 0; df < 4; ++df) o[df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[tile][df][kb], pf[tile][kb], o[df], 0, 0, 0);
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    const int row = q0 + c16;
    if (row < Lq) {
        uint16_t *op = a.out + ((size_t)b * Lq + row) * a.out_stride + h * HD + g * 4;
#pragma unroll
        for (int df = 0; df < 4; ++df) {
            const uint2 p = make_uint2(pack_bf16x2(o[df][0] * inv, o[df][1] * inv), pack_bf16x2(o[df][2] * inv, o[df][3] * inv));
            *reinterpret_cast<uint2 *>(op + df * 16) = p;
        }
    }
}

// argument validation + the launch geometry: what ga_attention_short_bf16 returns before it launches
int short_plan(const GaAttentionArgs *a, GaAttentionShortPlan *pl)
{
    if (!a || (!a->q && !a->qp_a) || !a->k || !a->vt || !a->out) return GA_DIT_ERR_NULL_ARG;
    if (a->k_norm_weight) return GA_DIT_ERR_BAD_SHAPE;      // K arrives normalised (once per conditioning, in the projection GEMM)
    const int rc = attention_args_check(a);
    if (rc != GA_DIT_OK) return rc;
    if (a->Lk > MAXT * KB || (int64_t)a->heads * a->batch > INT32_MAX) return GA_DIT_ERR_BAD_SHAPE;
    *pl = GaAttentionShortPlan{};
    pl->queries_per_wg = SQ;
    pl->key_tiles = (a->Lk + KB - 1) / KB;
    pl->fuses_q = a->qp_a != nullptr;
    pl->grid_x = a->heads * a->batch; pl->grid_y = (a->Lq + SQ - 1) / SQ; pl->grid_z = 1;
    pl->lds_bytes = (2 * pl->key_tiles + (pl->fuses_q ? 6 : 0)) * TILE * (int)sizeof(uint16_t);
    return GA_DIT_OK;
}

int launch_short(const GaAttentionArgs *a, void *stream, const PrefetchJob *pf, int pf_wgs)
{
    GaAttentionShortPlan pl;
    const int rc = short_plan(a, &pl);
    if (rc != GA_DIT_OK) return rc;
    dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y, 1);
    ShortTail tail{};
    if (pf && pf_wgs > 0) {
        tail.pf = *pf; tail.y0 = pl.grid_y;
        const int slices = (pf_wgs + pl.grid_x - 1) / pl.grid_x;
        grid.y += slices; tail.nwgs = slices * pl.grid_x;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (pl.key_tiles == 1 && pl.fuses_q) hipLaunchKernelGGL((attention_short_kernel<1, true>), grid, dim3(256), 0, s, *a, tail);
    else if (pl.key_tiles == 1) hipLaunchKernelGGL((attention_short_kernel<1, false>), grid, dim3(256), 0, s, *a, tail);
    else if (pl.fuses_q) hipLaunchKernelGGL((attention_short_kernel<2, true>), grid, dim3(256), 0, s, *a, tail);
    else hipLaunchKernelGGL((attention_short_kernel<2, false>), grid, dim3(256), 0, s, *a, tail);
    return hipGetLastError() == hipSuccess ? GA_DIT_OK : GA_DIT_ERR_LAUNCH;
}

}  // namespace

// ga_dit_forward: the launch with prefetch tail workgroups behind its grid, and the grid's size (a tail only pays while it leaves CUs idle)
int attention_short_with_tail(const GaAttentionArgs *a, void *stream, const PrefetchJob *pf, int pf_wgs)
{
    const int rc = attention_tail_check(nullptr, pf);
    return rc != GA_DIT_OK ? rc : launch_short(a, stream, pf, pf_wgs);
}
int attention_short_workgroups(const GaAttentionArgs *a)
{
    return (int)std::min<int64_t>((int64_t)a->heads * a->batch * ((a->Lq + SQ - 1) / SQ), INT32_MAX);
}
}  // namespace gadit

extern "C" int ga_attention_short_plan(const GaAttentionArgs *a, GaAttentionShortPlan *plan)
{
    if (!plan) return GA_DIT_ERR_NULL_ARG;
    GaAttentionShortPlan pl;
    const int rc = gadit::short_plan(a, &pl);
    if (rc == GA_DIT_OK) *plan = pl;
    return rc;
}

extern "C" int ga_attention_short_bf16(const GaAttentionArgs *a, void *stream) { return gadit::launch_short(a, stream, nullptr, 0); }
