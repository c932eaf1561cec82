// compact.h -- what the ordered stream compactions share (gfx950, wave64 only; integers only, so the including file's -ffp-contract
// setting cannot reach anything here).  DESIGN.md section 13 describes the pattern: three launches ordered by the stream -- flag / count,
// ONE workgroup scanning the per-block counts with a register carry, scatter with in-block ranks -- no look-back, no spinning, no
// atomics.  Used by surfel_densify.hip, pc_unproject.hip, pc_filter.hip and tsdf.hip.
//
// Everything is force-inlined and is called by every lane of the workgroup (the barriers inside are uniform).  The flag and scatter
// bodies, the launches and the workspace layouts belong to the files.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace gacompact {

constexpr int kPadRows = 1024;   // padding rows per trailing workgroup of a scatter launch

// inclusive scan over the 64 lanes of a wave; T is int or long long
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T x)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// inclusive scan over the kWaves waves of the workgroup (the wave totals through LDS); `total` is the workgroup's sum.  `lds` holds
// kWaves words; two barriers, the second one leaves `lds` free on return, so calls may follow each other on one array
template <int kWaves, typename T>
__device__ __forceinline__ T block_inclusive_scan(T x, T *lds, T &total)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const T incl = wave_inclusive_scan(x);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const T s = lds[w];
        before += w < wave ? s : 0;
        all += s;
    }
    __syncthreads();
    total = all;
    return incl + before;
}

// the workgroup's sum of x, valid in thread 0 alone.  One barrier; `lds` (kWaves words) is in use until the next one
template <int kWaves, typename T>
__device__ __forceinline__ T block_sum(T x, T *lds)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    T total = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kWaves; ++w) total += lds[w];
    }
    return total;
}

// one trip of an ordered scatter: the rank of a lane with `ok` among the trip's kept lanes (ballot + popcount inside a wave, the wave
// totals through LDS) and the trip's total.  Two barriers, `lds` (kWaves words) is free on return
template <int kWaves>
__device__ __forceinline__ int block_ballot_rank(bool ok, int *lds, int &all)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long vote = __ballot(ok);
    if (lane == 0) lds[wave] = __popcll(vote);
    __syncthreads();
    int before = 0;
    all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int t = lds[w];
        before += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();
    return before + __popcll(vote & ((1ull << lane) - 1ull));
}

// the scan launch, ONE workgroup of kThreads lanes: every count sums[0 .. n - 1] becomes its exclusive offset in place, kThreads of them
// a trip with the carry in a register (the caller bounds the total below 2^31); the total goes to sums[n] and is returned in every lane
template <int kThreads>
__device__ __forceinline__ int scan_counts_in_place(int32_t *sums, int n, int *lds)
{
    int carry = 0;
    for (int start = 0; start < n; start += kThreads) {   // (every lane takes every trip: the barriers are uniform)
        const int b = start + (int)threadIdx.x;
        const int c = b < n ? sums[b] : 0;
        int all;
        const int incl = block_inclusive_scan<kThreads / 64>(c, lds, all);
        if (b < n) sums[b] = carry + (incl - c);
        carry += all;
    }
    if (threadIdx.x == 0) sums[n] = carry;
    return carry;
}

// the trailing workgroups of a scatter launch write the padding rows min(total, capacity) .. capacity - 1, kPadRows apiece: the rows
// lo .. hi - 1 of the pad_block-th of them (none when lo >= hi)
inline unsigned pad_blocks(int64_t capacity) { return (unsigned)((capacity + kPadRows - 1) / kPadRows); }

__device__ __forceinline__ void pad_range(int pad_block, int64_t total, int64_t capacity, int64_t &lo, int64_t &hi)
{
    const int64_t first = (int64_t)pad_block * kPadRows;
    lo = total < capacity ? total : capacity;
    lo = lo > first ? lo : first;
    hi = first + kPadRows < capacity ? first + kPadRows : capacity;
}

}  // namespace gacompact
