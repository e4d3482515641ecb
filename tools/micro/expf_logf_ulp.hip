// How far are the device's expf and logf from float64 exp / log over the arguments the small-kernel tests use?
// tests/small_kernel_cases.py counts an expf (softmax_k) or a logf (sum_log) as EXPF_ROUNDINGS / LOGF_ROUNDINGS float32 roundings; those
// figures are the worst errors found here, in units of u |result| (u = 2^-24: a correctly rounded function stays <= 1), rounded up.
// Every float32 of the range is tried: expf on [-87, -0] (results in the normal range), logf on [1e-9, 1].  The reference is the
// device's float64 function (a few 2^-53: nothing at this scale).  Compiled with the library's flags:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/micro/expf_logf_ulp.hip -o tools/micro/expf_logf_ulp && tools/micro/expf_logf_ulp
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

constexpr int BLOCKS = 4096;

template <int FN>   // 0: expf, 1: logf
__global__ __launch_bounds__(256) void worst_kernel(unsigned lo_bits, unsigned count, double* __restrict__ worst_u, double* __restrict__ worst_ulp,
                                                    unsigned* __restrict__ worst_arg) {
    __shared__ double su[256], sl[256];
    __shared__ unsigned sa[256];
    double wu = 0.0, wl = 0.0;
    unsigned wa = lo_bits;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < count; i += BLOCKS * 256u) {
        const unsigned bits = lo_bits + i;
        const float x = __builtin_bit_cast(float, bits);
        const float f = FN == 0 ? expf(x) : logf(x);
        const double r = FN == 0 ? exp((double)x) : log((double)x);
        if (r == 0.0) {                                   // log(1): nothing to scale by; anything but 0 counts as infinitely wrong
            if (f != 0.0f) { wu = wl = 1e300; wa = bits; }
            continue;
        }
        int e;
        frexp(r, &e);                                     // |r| in [2^(e-1), 2^e): ulp = 2^(e-1-23)
        const double err = fabs((double)f - r), u = err / (fabs(r) * 0x1p-24), l = err / ldexp(1.0, e - 24);
        if (u > wu) { wu = u; wa = bits; }
        if (l > wl) wl = l;
    }
    su[threadIdx.x] = wu; sl[threadIdx.x] = wl; sa[threadIdx.x] = wa;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < 256; ++t) {
            if (su[t] > wu) { wu = su[t]; wa = sa[t]; }
            if (sl[t] > wl) wl = sl[t];
        }
        worst_u[blockIdx.x] = wu; worst_ulp[blockIdx.x] = wl; worst_arg[blockIdx.x] = wa;
    }
}

static unsigned bits_of(float v) { unsigned b; memcpy(&b, &v, 4); return b; }

template <int FN>
static int run(const char* name, float from, float to) {
    // both ends have one sign, so the bit patterns between them are the floats between them
    const unsigned a = bits_of(from), b = bits_of(to), lo = a < b ? a : b, count = (a < b ? b - a : a - b) + 1u;
    double *du, *dl;
    unsigned* da;
    if (hipMalloc(&du, BLOCKS * sizeof(double)) != hipSuccess || hipMalloc(&dl, BLOCKS * sizeof(double)) != hipSuccess ||
        hipMalloc(&da, BLOCKS * sizeof(unsigned)) != hipSuccess) return 1;
    hipLaunchKernelGGL(worst_kernel<FN>, dim3(BLOCKS), dim3(256), 0, 0, lo, count, du, dl, da);
    std::vector<double> hu(BLOCKS), hl(BLOCKS);
    std::vector<unsigned> ha(BLOCKS);
    if (hipMemcpy(hu.data(), du, BLOCKS * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (hipMemcpy(hl.data(), dl, BLOCKS * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (hipMemcpy(ha.data(), da, BLOCKS * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    double wu = 0.0, wl = 0.0;
    unsigned wa = lo;
    for (int i = 0; i < BLOCKS; ++i) {
        if (hu[i] > wu) { wu = hu[i]; wa = ha[i]; }
        if (hl[i] > wl) wl = hl[i];
    }
    float arg;
    memcpy(&arg, &wa, 4);
    printf("%s on [%g, %g]: %u arguments, worst %.4f u |result| (at %.9g), worst %.4f ulp -> %d roundings\n", name, from, to, count, wu, arg, wl, (int)ceil(wu));
    hipFree(du); hipFree(dl); hipFree(da);
    return 0;
}

int main() {
    if (run<0>("expf", -0.0f, -87.0f)) return 1;
    if (run<1>("logf", 1e-9f, 1.0f)) return 1;
    return 0;
}
