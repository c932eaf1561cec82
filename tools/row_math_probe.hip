// Relative error of the fp32 math-library functions the row kernels call (dit_ops.hip, decode_ops.hip: tanhf, sinf, cosf, expf, log1pf,
// sqrtf), each evaluated ALONE on a dense grid over the argument range the cases of tests/_row_cases.py use, against the host's double
// function of the same fp32 argument.  The constants of tests/_bounds.py are twice the worst relative error printed here (a grid can
// miss the worst argument); profiles/row_math_error.txt holds the output.  Compiled as the library is (csrc/Makefile: -O3 -ffp-contract=fast).
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=fast tools/row_math_probe.hip -o tools/_build/row_math_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

enum Fn { TANH, SIN, COS, EXP, LOG1P, SQRT };

template <int FN>
__global__ void eval(const float *x, float *y, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    y[i] = FN == TANH ? tanhf(v) : FN == SIN ? sinf(v) : FN == COS ? cosf(v) : FN == EXP ? expf(v) : FN == LOG1P ? log1pf(v) : sqrtf(v);
}

static double ref(int fn, double v)
{
    switch (fn) {
    case TANH: return std::tanh(v);
    case SIN: return std::sin(v);
    case COS: return std::cos(v);
    case EXP: return std::exp(v);
    case LOG1P: return std::log1p(v);
    default: return std::sqrt(v);
    }
}

#define CHECK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

// linear grid of n points over [lo, hi] (log == 0) or geometric grid over [lo, hi], lo > 0, mirrored to negative arguments when sym
static int run(const char *name, int fn, double lo, double hi, int n, bool log, bool sym)
{
    std::vector<float> x(n), y(n);
    for (int i = 0; i < n; ++i) {
        const double f = (double)i / (n - 1);
        double v = log ? lo * std::pow(hi / lo, f) : lo + (hi - lo) * f;
        if (sym && (i & 1)) v = -v;
        x[i] = (float)v;
    }
    float *dx, *dy;
    CHECK(hipMalloc(&dx, n * sizeof(float)));
    CHECK(hipMalloc(&dy, n * sizeof(float)));
    CHECK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    const dim3 grid((n + 255) / 256), block(256);
    switch (fn) {
    case TANH: hipLaunchKernelGGL(eval<TANH>, grid, block, 0, 0, dx, dy, n); break;
    case SIN: hipLaunchKernelGGL(eval<SIN>, grid, block, 0, 0, dx, dy, n); break;
    case COS: hipLaunchKernelGGL(eval<COS>, grid, block, 0, 0, dx, dy, n); break;
    case EXP: hipLaunchKernelGGL(eval<EXP>, grid, block, 0, 0, dx, dy, n); break;
    case LOG1P: hipLaunchKernelGGL(eval<LOG1P>, grid, block, 0, 0, dx, dy, n); break;
    default: hipLaunchKernelGGL(eval<SQRT>, grid, block, 0, 0, dx, dy, n); break;
    }
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(y.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost));
    CHECK(hipFree(dx));
    CHECK(hipFree(dy));
    double worst = 0, worst_abs = 0, at = 0, at_abs = 0;
    long bad = 0;
    for (int i = 0; i < n; ++i) {
        const double r = ref(fn, (double)x[i]), e = std::fabs((double)y[i] - r);
        if (!std::isfinite((double)y[i])) { ++bad; continue; }
        if (e > worst_abs) { worst_abs = e; at_abs = x[i]; }
        if (r != 0 && e / std::fabs(r) > worst) { worst = e / std::fabs(r); at = x[i]; }
    }
    printf("%-6s %s grid of %d points over [%g, %g]%s: worst relative error %.4e = %.3f u (u = 2^-24) at x = %.9g; worst absolute error %.4e at x = %.9g; "
           "%ld non-finite\n", name, log ? "geometric" : "linear", n, lo, hi, sym ? ", both signs" : "", worst, worst * 16777216.0, at, worst_abs, at_abs, bad);
    return 0;
}

int main()
{
    const int N = 1 << 24;
    int rc = 0;
    rc |= run("tanhf", TANH, -32.0, 32.0, N, false, false);
    rc |= run("tanhf", TANH, 1e-30, 32.0, N, true, true);
    rc |= run("sinf", SIN, 0.0, 1024.0, N, false, false);
    rc |= run("sinf", SIN, 1e-30, 1024.0, N, true, false);
    rc |= run("cosf", COS, 0.0, 1024.0, N, false, false);
    rc |= run("cosf", COS, 1e-30, 1024.0, N, true, false);
    rc |= run("expf", EXP, -40.0, 40.0, N, false, false);
    rc |= run("expf", EXP, 1e-30, 40.0, N, true, true);
    rc |= run("expf", EXP, -9.25, 0.0, N, false, false);      // the timestep frequencies: exp(-ln(10000) j / 128), j < 128
    rc |= run("log1pf", LOG1P, 1e-18, 1e18, N, true, false);
    rc |= run("log1pf", LOG1P, 0.0, 64.0, N, false, false);
    rc |= run("sqrtf", SQRT, 1e-30, 1e10, N, true, false);
    rc |= run("sqrtf", SQRT, 0.0, 4096.0, N, false, false);
    return rc;
}
