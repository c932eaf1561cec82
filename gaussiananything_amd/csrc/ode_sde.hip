// ode_sde.hip -- the steps of the reference's SDE sampler, resident on the device (gfx950).
//
// The reference's Sampler.sample_sde (/root/reference/transport/transport.py:322-382) runs the stepper class `sde`
// (/root/reference/transport/integrators.py:8-75): Euler-Maruyama or Heun over a fixed grid, the noise of every step drawn on the host,
// then one "last step" (transport.py:290-320).  For a velocity model on the GVP / Linear path its drift is
//     drift(x, t) = v + w(t) * score,   score = (r(t) * v - x) / var(t)                   (path.py:70-84, transport.py:282-284)
// with v the model output at (x, t): ONE evaluation serves drift and score.  Here a step is a short chain of launches around
// ga_dit_forward(step.velocity) that reads everything that changes from step to step -- the step index, the coefficients of the
// interval, the seed -- from DEVICE memory, so one step captured into a HIP graph is replayed for the whole trajectory and every replay
// draws fresh noise.  Phases (GaSdeStep / ga_sde_step in include/ga_dit.h), one launch over the n floats of the state each:
//   EM            score, drift, mean = x + drift dt, x = mean + g (xi sqrt_dt); traj[counter] = x
//   HEUN_PERTURB  xhat = x + g (xi sqrt_dt)                                     (the first evaluation's input)
//   HEUN_PREDICT  k1 = drift(xhat, v, t); x = xhat + dt k1; timesteps = t + dt  (the second evaluation's input)
//   HEUN_CORRECT  x = xhat + (0.5 dt) (k1 + drift(x, v, t + dt)); traj[counter] = x
//   LAST_*        the last step into traj[num_intervals]
//   ADVANCE       one thread: ++counter, timesteps = t of the next coefficient row
// This translation unit is compiled with -ffp-contract=off: every product, quotient and sum below is rounded on its own, in the order
// written -- the same numbers as the eager torch loop of transport/sampler.py and the numpy restatement of the tests, bit for bit.
//
// Noise: Philox4x32-10 (Salmon et al., SC'11), key = the 64-bit seed, counter = (draw index / 4, step counter READ FROM THE DEVICE,
// stream id of the phase, 0); the four words give four normals by two Box-Muller pairs (the transform is written out in ga_dit.h).
// A thread computes the block of its element and keeps the one normal it needs: the stream is a function of (seed, step, element)
// alone, never of the grid.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ga_dit.h"
#include "philox.h"

namespace gasde {

// the normal of draw index j at step `step` (ga_dit.h: "noise of ga_sde_step")
__device__ __forceinline__ float normal_of(uint64_t seed, uint32_t step, uint32_t stream, int64_t j)
{
    uint32_t w[4];
    gaphilox::philox4x32_10((uint32_t)(j >> 2), step, stream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const int lane = (int)(j & 3), pair = lane >> 1;
    return gaphilox::box_muller(w[2 * pair], w[2 * pair + 1], lane & 1);
}

__global__ __launch_bounds__(256) void step_kernel(GaSdeStep s, int phase)
{
    const int64_t n = s.n;
    const int64_t ndraw = s.cfg_pairs ? n / 2 : n;
    const bool last = phase >= GA_SDE_LAST_MEAN;
    int c = *s.counter;
    c = c < 0 ? 0 : (c > s.num_intervals - 1 ? s.num_intervals - 1 : c);      // a replay past the end stays inside every buffer
    const int row = last ? s.num_intervals : c;
    const float *co = s.coef + (size_t)row * GA_SDE_COEF_STRIDE;
    const float dt = co[GA_SDE_C_DT], sqrt_dt = co[GA_SDE_C_SQRT_DT], w = co[GA_SDE_C_W], g = co[GA_SDE_C_G], r = co[GA_SDE_C_R],
                var = co[GA_SDE_C_VAR];
    if (phase == GA_SDE_HEUN_PREDICT && blockIdx.x == 0 && (int)threadIdx.x < s.batch) s.timesteps[threadIdx.x] = co[GA_SDE_C_T2];
    const bool draws = phase == GA_SDE_EM || phase == GA_SDE_HEUN_PERTURB;
    const uint64_t seed = (draws && !s.noise) ? *s.seed : 0;
    float *slot = s.traj + (size_t)row * n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float xi = 0.0f;
        if (draws) {
            const int64_t j = i < ndraw ? i : i - ndraw;       // cfg_pairs: both halves of the doubled state take the same normal
            xi = s.noise ? s.noise[(size_t)c * ndraw + j] : normal_of(seed, (uint32_t)c, (uint32_t)phase, j);
            if (s.noise_out && i < ndraw) s.noise_out[i] = xi;
        }
        switch (phase) {
        case GA_SDE_EM: {
            const float x = s.state[i], v = s.velocity[i];
            const float score = (r * v - x) / var;
            const float drift = v + w * score;
            const float mean = x + drift * dt;
            const float xn = mean + g * (xi * sqrt_dt);
            s.state[i] = xn;
            slot[i] = xn;
        } break;
        case GA_SDE_HEUN_PERTURB:
            s.xhat[i] = s.state[i] + g * (xi * sqrt_dt);
            break;
        case GA_SDE_HEUN_PREDICT: {
            const float xh = s.xhat[i], v = s.velocity[i];
            const float score = (r * v - xh) / var;
            const float k1 = v + w * score;
            s.k1[i] = k1;
            s.state[i] = xh + dt * k1;
        } break;
        case GA_SDE_HEUN_CORRECT: {
            const float xp = s.state[i], v = s.velocity[i];
            const float score = (co[GA_SDE_C_R2] * v - xp) / co[GA_SDE_C_VAR2];
            const float k2 = v + co[GA_SDE_C_W2] * score;
            const float xn = s.xhat[i] + co[GA_SDE_C_HALF_DT] * (s.k1[i] + k2);
            s.state[i] = xn;
            slot[i] = xn;
        } break;
        case GA_SDE_LAST_MEAN: {
            const float x = s.state[i], v = s.velocity[i];
            const float score = (r * v - x) / var;
            const float drift = v + w * score;
            slot[i] = x + drift * dt;                              // (dt of the last row = last_step_size)
        } break;
        case GA_SDE_LAST_TWEEDIE: {
            const float x = s.state[i], v = s.velocity[i];
            const float score = (r * v - x) / var;
            slot[i] = x / co[GA_SDE_C_ALPHA] + co[GA_SDE_C_SIG2A] * score;
        } break;
        case GA_SDE_LAST_EULER:
            slot[i] = s.state[i] + s.velocity[i] * dt;
            break;
        default:   // GA_SDE_LAST_NONE
            slot[i] = s.state[i];
            break;
        }
    }
}

__global__ __launch_bounds__(64) void advance_kernel(int32_t *__restrict__ counter, const float *__restrict__ coef, int num_intervals,
                                                     float *__restrict__ timesteps, int batch)
{
    int c = *counter + 1;
    c = c < 0 ? 0 : (c > num_intervals ? num_intervals : c);      // the last row carries t1, the time of the last step
    const float t = coef[(size_t)c * GA_SDE_COEF_STRIDE + GA_SDE_C_T];
    __syncthreads();                                               // every lane has read the counter before lane 0 moves it
    if ((int)threadIdx.x < batch) timesteps[threadIdx.x] = t;
    if (threadIdx.x == 0) *counter = c;
}

}  // namespace gasde

extern "C" {

int ga_sde_step_check(const GaSdeStep *s, int32_t phase)
{
    if (!s) return GA_DIT_ERR_NULL_ARG;
    if (phase < GA_SDE_EM || phase > GA_SDE_ADVANCE) return GA_DIT_ERR_BAD_SHAPE;
    if (s->n <= 0 || s->n > INT32_MAX || s->batch <= 0 || s->batch > 64 || s->num_intervals <= 0) return GA_DIT_ERR_BAD_SHAPE;
    if (s->cfg_pairs && (s->n & 1)) return GA_DIT_ERR_BAD_SHAPE;
    if (!s->counter || !s->coef) return GA_DIT_ERR_NULL_ARG;
    if (phase == GA_SDE_ADVANCE) return s->timesteps ? GA_DIT_OK : GA_DIT_ERR_NULL_ARG;
    if (!s->state) return GA_DIT_ERR_NULL_ARG;
    if (phase != GA_SDE_HEUN_PERTURB && phase != GA_SDE_LAST_NONE && !s->velocity) return GA_DIT_ERR_NULL_ARG;
    if (phase != GA_SDE_HEUN_PERTURB && phase != GA_SDE_HEUN_PREDICT && !s->traj) return GA_DIT_ERR_NULL_ARG;
    if (phase >= GA_SDE_HEUN_PERTURB && phase <= GA_SDE_HEUN_CORRECT && !s->xhat) return GA_DIT_ERR_NULL_ARG;
    if ((phase == GA_SDE_HEUN_PREDICT || phase == GA_SDE_HEUN_CORRECT) && !s->k1) return GA_DIT_ERR_NULL_ARG;
    if (phase == GA_SDE_HEUN_PREDICT && !s->timesteps) return GA_DIT_ERR_NULL_ARG;
    if ((phase == GA_SDE_EM || phase == GA_SDE_HEUN_PERTURB) && !s->noise && !s->seed) return GA_DIT_ERR_NULL_ARG;
    return GA_DIT_OK;
}

int ga_sde_step(const GaSdeStep *s, int32_t phase, void *stream)
{
    using namespace gasde;
    const int rc = ga_sde_step_check(s, phase);
    if (rc != GA_DIT_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (phase == GA_SDE_ADVANCE) {
        hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, st, s->counter, s->coef, s->num_intervals, s->timesteps, s->batch);
    } else {
        const int64_t blocks = (s->n + 255) / 256;
        hipLaunchKernelGGL(step_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, *s, (int)phase);
    }
    return hipGetLastError() == hipSuccess ? GA_DIT_OK : GA_DIT_ERR_LAUNCH;
}

}  // extern "C"
