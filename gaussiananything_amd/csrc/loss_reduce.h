// loss_reduce.h -- the fixed-order reduction both loss translation units (photo_loss.hip, geo_loss.hip) end on: three sums per workgroup,
// then one workgroup per image / view over that image's partials.  fp64 across lanes, waves and workgroups, no atomics: two calls on the
// same input give the same bits.  Included inside each unit's anonymous namespace, after its kThreads.
#ifndef GA_LOSS_REDUCE_H
#define GA_LOSS_REDUCE_H

constexpr int kReduceThreads = 256;

// fixed-order sum of three doubles per lane over the workgroup; the result is valid in thread 0
__device__ __forceinline__ void block_sum3(double v[3], double *red /* [3][waves] */) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
    }
    const int wave = threadIdx.x >> 6, waves = kThreads / 64;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) red[q * waves + wave] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            double s = red[q * waves];
            for (int w = 1; w < waves; ++w) s += red[q * waves + w];
            v[q] = s;
        }
    }
}

// one workgroup per image (or view): its partials are contiguous ([per_image] x 3); fixed order: lane-strided, then a tree
__global__ __launch_bounds__(kReduceThreads) void loss_reduce_kernel(const float *__restrict__ partials, float *__restrict__ out,
                                                                     int per_image, double inv_count) {
    __shared__ double red[3][kReduceThreads];
    const float *p = partials + (size_t)blockIdx.x * (size_t)per_image * 3;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < per_image; i += kReduceThreads) {
        s0 += (double)p[(size_t)i * 3 + 0];
        s1 += (double)p[(size_t)i * 3 + 1];
        s2 += (double)p[(size_t)i * 3 + 2];
    }
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int off = kReduceThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            red[0][threadIdx.x] += red[0][threadIdx.x + off];
            red[1][threadIdx.x] += red[1][threadIdx.x + off];
            red[2][threadIdx.x] += red[2][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) out[(size_t)blockIdx.x * 3 + threadIdx.x] = (float)(red[threadIdx.x][0] * inv_count);
}

#endif
