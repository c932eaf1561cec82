// dit_attention_common.h -- what the attention kernels share (gfx950 only): the tile constants and the swizzled LDS image of the
// head-64 kernels, the LDS-DMA instruction, the lane-group maximum, the Q fragments read from memory, the ring-independent pieces of
// the Q projection inside the workgroup (GaAttentionArgs.qp_*), and the argument checks of the two head-64 plans.
//
// attention_fwd_kernel (dit_attention.hip) and attention_short_kernel (dit_attention_short.hip) are two walks over ONE formulation:
// the same fragment reads, the same lane <-> element maps, the same projection arithmetic in the same order.  Everything here is a
// straight-line body, force-inlined; the loops, the rings, the counted vmcnt waits and the barriers around these bodies belong to the
// kernels.  dit_attention_hd.hip takes group_max only.
#pragma once
#include "dit_common.h"

namespace gadit {

constexpr int KB = 64, HD = 64;
constexpr int TILE = KB * HD;  // elements of one staged tile (8 KiB)

// Rows are 128 bytes; the DMA writes LDS in lane order, so the bank-conflict-free image is made on the SOURCE side: slot s of row r
// holds global 16-byte chunk s ^ swz_of(r)
__device__ __forceinline__ int swz_of(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }
__device__ __forceinline__ int swz(int row, int chunk) { return row * 64 + ((chunk ^ swz_of(row)) * 8); }

__device__ __forceinline__ void glds16(const uint16_t *gsrc, uint16_t *lds_wave_base)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                     (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

// max over the four lane groups that hold one query's keys (lanes l, l^16, l^32, l^48): two VALU lane swaps instead of two
// LDS round trips (ds_bpermute) on the tile's critical path
__device__ __forceinline__ float group_max(float t)
{
    const unsigned u = __float_as_uint(t);
    const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const float m = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const unsigned v = __float_as_uint(m);
    const auto c = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return fmaxf(__uint_as_float(c[0]), __uint_as_float(c[1]));
}

// ---- S^T = K Q^T for one 64-key tile at `bk`: the K fragment of MFMA row i reads key row 32 (kf>>1) + 8 (i>>2) + 4 (kf&1) + (i&3), so
// s[kf][r] <-> key (kf>>1)*32 + g*8 + (kf&1)*4 + r of the tile, query c16 (g = lane >> 4, c16 = lane & 15)
__device__ __forceinline__ void kq_frags(const uint16_t *bk, int c16, int g, bf16x8 (&frag)[4][2])
{
    const int krow = 8 * (c16 >> 2) + (c16 & 3);
#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
            frag[kf][kk] = *reinterpret_cast<const bf16x8 *>(bk + swz((kf >> 1) * 32 + (kf & 1) * 4 + krow, kk * 4 + g));
}
__device__ __forceinline__ void kq_mfma(const bf16x8 (&frag)[4][2], const bf16x8 (&qf)[2], f32x4 (&s)[4])
{
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int kf = 0; kf < 4; ++kf) s[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag[kf][kk], qf[kk], s[kf], 0, 0, 0);
}

// ---- Q fragments (B operand of S^T = K Q^T) read from memory: the lane holds Q[row][kk*32 + g*8 .. +7] of head h (row = q0 + c16,
// clamped by the caller), RMS-normalised by the 4 lane groups that hold a row's fragments when q_norm_weight is given; the softmax
// scale and log2(e) are folded in so the exponentials are bare v_exp_f32.
// (The argument block goes to the helpers BY VALUE: a helper is optimised on its own before it is inlined, and with the block behind a
//  reference the kernels came out with other register counts than with this text in their own bodies.)
__device__ __forceinline__ void q_frags_from_memory(const GaAttentionArgs a, int b, int h, int row, int g, bf16x8 (&qf)[2])
{
    const uint16_t *qp = a.q + ((size_t)b * a.Lq + row) * a.q_stride + h * HD;
    float qv[16];
    float ss = 0.f;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(qp + kk * 32 + g * 8);
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            qv[kk * 8 + 2 * e] = __uint_as_float(w[e] << 16);
            qv[kk * 8 + 2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) ss += qv[e] * qv[e];
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    float rs = 0.125f * 1.4426950408889634f;  // 64^-1/2 * log2(e)
    if (a.q_norm_weight) rs *= rsqrtf(ss * (1.0f / HD) + 1e-5f);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = qv[kk * 8 + e];
            if (a.q_norm_weight) v *= a.q_norm_weight[kk * 32 + g * 8 + e];
            qf[kk][e] = (short)f32_to_bf16(v * rs);
        }
}

// ---- THE Q PROJECTION INSIDE THE WORKGROUP (GaAttentionArgs.qp_*): Q[64 queries x 64] of this head = A rows x W_head^T over K = qp_k,
// instead of a GEMM launch of its own in front of the attention.  A 64-wide K-slice of W_head is 64 rows x 128 bytes -- the shape of a
// K tile -- and so is the slice of the workgroup's 64 A rows: both are staged by the key walk's LDS-DMA pattern (piece p = 8 rows; wave
// wq of four moves pieces 2 wq, 2 wq + 1 of each), W read with the K walk's permuted fragment rows, A with the V^T walk's natural rows,
// which leaves the accumulators of S^T = W_slice A_slice^T in exactly the lanes the Q fragments live in:
// acc[kf][r] <-> Q[q0 + c16][32 (kf >> 1) + 8 g + 4 (kf & 1) + r].  Everything is DMA: no compiler-managed load sits in the pipeline
// (with the A fragments as register loads hipcc put s_waitcnt vmcnt(0) in front of every DMA issue of the loop).
// Which slices a wave takes, where their tiles lie and when they are waited for is the kernel's business.  So is the slice step itself
// (10 fragment reads, 8 MFMAs, once in each kernel's loop): as a helper here it cost both kernels ~1 % of their time -- the compiler
// forms the LDS addresses of the reads another way when it first sees them outside the loop (profiles/attention_shared_header.txt).
struct QProjection {
    int wq;
    int nsl;             // 64-wide K-slices
    float tot;           // RMSNorm row scale folded out of the A operand: the row's sum of squares (used in finish)
    float qnw[16];       // per-head norm weights of my 16 head columns, requested in front of the DMA stream (a load behind it would wait for all of it)
    // a lane's byte offsets once (32 bits), a slice's address = wave-uniform base + offset
    uint32_t qw_off[2], qa_off[2];
    bool w_tiled;        // (issue derives the slice step from it: a multiplier it can see is a power of two becomes the shift the kernels had)
    const char *qw_base[2], *qa_base;

    // q0: first query row of the wave (the workgroup's is q0 - 16 wq)
    __device__ __forceinline__ void setup(const GaAttentionArgs a, int b, int h, int q0, int wq_, int lane)
    {
        wq = wq_;
        const int c16 = lane & 15, g = lane >> 4;
        nsl = a.qp_k >> 6;
        const int Lq = a.Lq, qbase = q0 - wq * 16;
        tot = 0.f;
        if (a.qp_row_ss) {   // (same summation order as the GEMM consumer)
            const float *rp = a.qp_row_ss + ((size_t)b * Lq + min(q0 + c16, Lq - 1)) * a.qp_row_ss_tiles;
            for (int t4 = 0; t4 < a.qp_row_ss_tiles; t4 += 4) {
                const float4 q4 = *reinterpret_cast<const float4 *>(rp + t4);
                tot += (q4.x + q4.y) + (q4.z + q4.w);
            }
        }
        {
            float4 w4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) w4[i] = make_float4(1.f, 1.f, 1.f, 1.f);
            if (a.q_norm_weight) {   // kernel-uniform
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    w4[2 * kk] = *reinterpret_cast<const float4 *>(a.q_norm_weight + kk * 32 + g * 8);
                    w4[2 * kk + 1] = *reinterpret_cast<const float4 *>(a.q_norm_weight + kk * 32 + g * 8 + 4);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) { qnw[4 * i] = w4[i].x; qnw[4 * i + 1] = w4[i].y; qnw[4 * i + 2] = w4[i].z; qnw[4 * i + 3] = w4[i].w; }
        }
        qa_base = reinterpret_cast<const char *>(a.qp_a + (size_t)b * Lq * a.qp_lda);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = wq * 2 + i, r8 = p * 8, row = r8 + (lane >> 3), chunk = (lane & 7) ^ swz_of(row);
            if (a.qp_w_tiled) {    // kernel-uniform
                qw_base[i] = reinterpret_cast<const char *>(a.qp_w + (size_t)(h * 8 + p) * nsl * 512);
                qw_off[i] = (uint32_t)((lane >> 3) * 64 + chunk * 8) * 2u;
            } else {
                qw_base[i] = reinterpret_cast<const char *>(a.qp_w + (size_t)h * 64 * a.qp_k);
                qw_off[i] = ((uint32_t)row * (uint32_t)a.qp_k + (uint32_t)chunk * 8u) * 2u;
            }
            qa_off[i] = ((uint32_t)min(qbase + row, Lq - 1) * (uint32_t)a.qp_lda + (uint32_t)chunk * 8u) * 2u;
        }
        w_tiled = a.qp_w_tiled != 0;
    }

    // the wave's four DMA instructions of slice sl_raw: two W pieces into the tile at `dw`, two A pieces into the tile at `da`
    __device__ __forceinline__ void issue(int sl_raw, uint16_t *dw, uint16_t *da) const
    {
        const int sl = min(sl_raw, nsl - 1);   // past the end: a harmless re-fetch (keeps the kernels' vmcnt arithmetic exact)
        const uint32_t qw_step = w_tiled ? 1024u : 128u;     // bytes from one 64-wide K-slice of W to the next
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(reinterpret_cast<const uint16_t *>(qw_base[i] + (size_t)sl * qw_step + qw_off[i]), dw + (wq * 2 + i) * 8 * 64);
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(reinterpret_cast<const uint16_t *>(qa_base + (size_t)sl * 128 + qa_off[i]), da + (wq * 2 + i) * 8 * 64);
    }

    // row scale, per-head RMSNorm, bf16 as the projection GEMM would have stored it, then the softmax scale as in q_frags_from_memory
    __device__ __forceinline__ void finish(const GaAttentionArgs a, const f32x4 (&acc)[4], bf16x8 (&qf)[2]) const
    {
        const float rsc = a.qp_row_ss ? rsqrtf(tot * (1.0f / (float)a.qp_row_ss_dim) + a.qp_row_ss_eps) : 1.f;
        float xv[16];
        float ss = 0.f;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = acc[2 * kk + (e >> 2)][e & 3] * rsc;
                xv[kk * 8 + e] = v;
                ss += v * v;
            }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        const float rn = rsqrtf(ss * (1.0f / HD) + 1e-5f);
        const float rs = 0.125f * 1.4426950408889634f;  // 64^-1/2 * log2(e)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = xv[kk * 8 + e];
                if (a.q_norm_weight) v *= rn * qnw[kk * 8 + e];
                qf[kk][e] = (short)f32_to_bf16(bf16_to_f32(f32_to_bf16(v)) * rs);
            }
    }
};

// ---- the argument checks attention_plan and short_plan share (behind each one's own NULL and k_norm_weight answers): the qp_* block,
// shapes and strides, 16-byte accesses (vector loads of q, LDS-DMA of k / vt / qp_a / qp_w) and the 8-byte stores of out
static inline int attention_args_check(const GaAttentionArgs *a)
{
    if (a->qp_a) {   // the q projection inside the workgroup: 16-byte aligned operands, K in 64-wide slices
        if (!a->qp_w) return GA_DIT_ERR_NULL_ARG;
        if (a->qp_k < 64 || a->qp_k % 64 || a->qp_lda % 8 || a->qp_lda < a->qp_k || ((uintptr_t)a->qp_a | (uintptr_t)a->qp_w) % 16 != 0 ||
            (a->qp_row_ss && (a->qp_row_ss_tiles <= 0 || a->qp_row_ss_tiles % 4 != 0 || a->qp_row_ss_dim <= 0 || (uintptr_t)a->qp_row_ss % 16 != 0)))
            return GA_DIT_ERR_BAD_SHAPE;
    }
    if (a->batch <= 0 || a->heads <= 0 || a->Lq <= 0 || a->Lk <= 0 || a->q_stride % 8 || a->k_stride % 8 || a->vt_ld % 8 ||
        a->vt_ld < ((a->Lk + KB - 1) / KB) * KB || a->out_stride % 4)
        return GA_DIT_ERR_BAD_SHAPE;
    if (((a->qp_a ? 0 : (uintptr_t)a->q) | (uintptr_t)a->k | (uintptr_t)a->vt) % 16 != 0 || (uintptr_t)a->out % 8 != 0) return GA_DIT_ERR_BAD_SHAPE;
    return GA_DIT_OK;
}

}  // namespace gadit
