// wgrad_plan_record.h -- records what the weight-gradient launchers WOULD launch, without a GPU (tests/golden/make_wgrad_plan_golden.py).
//
// The generator builds one translation unit per source file:
//     #include <hip/hip_runtime.h>
//     #include "wgrad_plan_record.h"            part 1: hipLaunchKernelGGL becomes a recorder, hipGetLastError() is hipSuccess
//     #include ".../conv_wgrad.hip"             (or wgrad_f16k.hip) of the commit being recorded, unmodified
//     #define WGRAD_RECORD_DRIVER 1             (2 for wgrad_f16k.hip)
//     #include "wgrad_plan_record.h"            part 2: main() -- reads cases from stdin, calls the entry points with dummy pointers
// and links it with misc.hip (masic_set_error).  Nothing is launched.
//
// stdin, one case per line:
//   driver 1:  22 integers = masic_conv_desc_t, then flags (MASIC_WGRAD_DET 1, _IN16 2, _CLEAN 4)
//   driver 2:  kind (3, 5, 1), then  B Cin Cout H W flags  (kind 3 / 5)  or  bias_of B CA CQ HW flags  (kind 1)
// stdout per case:  "# <return code> <launches>", then per launch  "kernel | pretty function | gx,gy,gz | block | lds".
#ifndef WGRAD_PLAN_RECORD_H
#define WGRAD_PLAN_RECORD_H
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

struct WgradRecord { std::string kernel, where; dim3 grid, block; size_t lds; };
static std::vector<WgradRecord> wgrad_records;
template <class... Args>
static void wgrad_record(const char* kernel, const char* where, dim3 grid, dim3 block, size_t lds, hipStream_t, const Args&...) {
    wgrad_records.push_back({kernel, where, grid, block, lds});
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, st, ...) wgrad_record(#kernel, __PRETTY_FUNCTION__, dim3(grid), dim3(block), (size_t)(lds), st, ##__VA_ARGS__)
#define hipGetLastError() hipSuccess

#elif defined(WGRAD_RECORD_DRIVER)
int main() {
    static float dummy[4];
    void* p = dummy;
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        int v[24], n = 0, used = 0, pos = 0;
        while (n < 24 && sscanf(line + pos, "%d%n", &v[n], &used) == 1) { pos += used; ++n; }
        if (n == 0) continue;
        wgrad_records.clear();
        int rc = -100;
#if WGRAD_RECORD_DRIVER == 1
        masic_conv_desc_t d;
        static_assert(sizeof d == 22 * sizeof(int), "descriptor of 22 integers");
        if (n != 23) { fprintf(stderr, "bad case: %s", line); return 2; }
        memcpy(&d, v, sizeof d);
        const int flags = v[22], det = flags & 1, in16 = flags & 2, clean = (flags & 4) ? 1 : 0;
        if (det && clean) rc = -101;     // (no such entry point)
        else if (det) rc = in16 ? masic_conv2d_wgrad_bf16in_det(p, p, dummy, p, &d, nullptr) : masic_conv2d_wgrad_det(dummy, dummy, dummy, p, &d, nullptr);
        else rc = in16 ? masic_conv2d_wgrad_bf16in(p, p, dummy, p, &d, clean, nullptr) : masic_conv2d_wgrad_ws(dummy, dummy, dummy, p, &d, clean, nullptr);
#else
        if (n != 7) { fprintf(stderr, "bad case: %s", line); return 2; }
        const int kind = v[0], flags = v[6], det = flags & 1, clean = (flags & 4) ? 1 : 0;
        if ((det && clean) || (kind == 1 && clean)) rc = -101;
        else if (kind == 3) rc = det ? masic_conv3x3_wgrad_f16k_det(p, p, dummy, p, v[1], v[2], v[3], v[4], v[5], nullptr)
                                     : masic_conv3x3_wgrad_f16k_ws(p, p, dummy, p, v[1], v[2], v[3], v[4], v[5], clean, nullptr);
        else if (kind == 5) rc = det ? masic_conv5x5_wgrad_f16k_det(p, p, dummy, p, v[1], v[2], v[3], v[4], v[5], nullptr)
                                     : masic_conv5x5_wgrad_f16k_ws(p, p, dummy, p, v[1], v[2], v[3], v[4], v[5], clean, nullptr);
        else rc = det ? masic_gemm_wgrad_bias_f16k_det(p, p, dummy, p, v[1], v[2], v[3], v[4], v[5], nullptr)
                      : masic_gemm_wgrad_bias_f16k(p, p, dummy, v[1], v[2], v[3], v[4], v[5], nullptr);
#endif
        if (rc != 0) wgrad_records.clear();
        printf("# %d %zu\n", rc, wgrad_records.size());
        for (const WgradRecord& r : wgrad_records)
            printf("%s | %s | %u,%u,%u | %u | %zu\n", r.kernel.c_str(), r.where.c_str(), r.grid.x, r.grid.y, r.grid.z, r.block.x, r.lds);
    }
    return 0;
}
#endif
