// conv_plan_record.h -- records what the NCHW convolution launcher of conv.hip WOULD launch, without a GPU
// (tests/golden/make_conv_plan_golden.py; the sibling of wgrad_plan_record.h).
//
// The generator builds one translation unit:
//     #include <hip/hip_runtime.h>
//     #include "conv_plan_record.h"             part 1: hipLaunchKernelGGL becomes a recorder, hipGetLastError() is hipSuccess
//     #include ".../conv.hip"                   of the commit being recorded, unmodified
//     #define CONV_RECORD_DRIVER 1
//     #include "conv_plan_record.h"             part 2: main() -- reads cases from stdin, calls the entry points with dummy pointers
// and links it with misc.hip (masic_set_error).  Nothing is launched.
//
// stdin, one case per line: 22 integers = masic_conv_desc_t, then the form (MASIC_CONV_GATE 1, _RES1 2, _RES2 4, _F16K_OUT 8).
// stdout per case:  "# <return code> <launches>", then per launch  "kernel | gx,gy,gz | block | lds | integers", the integers read from
// the by-value argument struct the kernel is handed (the recorder keeps its bytes; the driver, which sees the struct definitions of
// conv.hip, decodes them):
//     conv_igemm_*          Cin_pad Cout_pad KC TW TH SR PH PW PSZ buf_sz vec4 nphase
//     conv_direct_f32       nphase
//     deconv5s2_small_cout  Cin_pad tiles_w
//     conv5s1_small         tiles_w
#ifndef CONV_PLAN_RECORD_H
#define CONV_PLAN_RECORD_H
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

struct ConvRecord { std::string kernel; dim3 grid, block; size_t lds; std::vector<char> arg0; };
static std::vector<ConvRecord> conv_records;
template <class A0, class... Rest>
static void conv_record(const char* kernel, dim3 grid, dim3 block, size_t lds, hipStream_t, const A0& a0, const Rest&...) {
    const char* b = reinterpret_cast<const char*>(&a0);
    conv_records.push_back({kernel, grid, block, lds, std::vector<char>(b, b + sizeof a0)});
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, st, ...) conv_record(#kernel, dim3(grid), dim3(block), (size_t)(lds), st, __VA_ARGS__)
#define hipGetLastError() hipSuccess

#elif defined(CONV_RECORD_DRIVER)
template <class A> static A conv_record_args(const ConvRecord& r) {
    A a;
    if (r.arg0.size() != sizeof a) { fprintf(stderr, "%s: argument struct of %zu bytes\n", r.kernel.c_str(), r.arg0.size()); exit(3); }
    memcpy((void*)&a, r.arg0.data(), sizeof a);
    return a;
}

int main() {
    static float dummy[4];
    void* p = dummy;
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        int v[24], n = 0, used = 0, pos = 0;
        while (n < 24 && sscanf(line + pos, "%d%n", &v[n], &used) == 1) { pos += used; ++n; }
        if (n == 0) continue;
        if (n != 23) { fprintf(stderr, "bad case: %s", line); return 2; }
        conv_records.clear();
        masic_conv_desc_t d;
        static_assert(sizeof d == 22 * sizeof(int), "descriptor of 22 integers");
        memcpy(&d, v, sizeof d);
        const int form = v[22];
        int rc;
        if (form & 8) rc = (form & 7) ? -101 : masic_conv2d_f16k_out_fwd(dummy, p, dummy, p, &d, nullptr);      // (no such entry point)
        else rc = masic_conv2d_fwd_ex(dummy, p, dummy, (form & 1) ? dummy : nullptr, (form & 2) ? dummy : nullptr, (form & 4) ? dummy : nullptr,
                                      dummy, &d, nullptr);
        if (rc != 0) conv_records.clear();
        printf("# %d %zu\n", rc, conv_records.size());
        for (const ConvRecord& r : conv_records) {
            printf("%s | %u,%u,%u | %u | %zu |", r.kernel.c_str(), r.grid.x, r.grid.y, r.grid.z, r.block.x, r.lds);
            if (r.kernel.find("conv_igemm") != std::string::npos) {
                const IgemmArgs a = conv_record_args<IgemmArgs>(r);
                printf(" %d %d %d %d %d %d %d %d %d %d %d %d", a.Cin_pad, a.Cout_pad, a.KC, a.TW, a.TH, a.SR, a.PH, a.PW, a.PSZ, a.buf_sz, a.vec4, a.nphase);
            } else if (r.kernel.find("conv_direct") != std::string::npos) {
                printf(" %d", conv_record_args<DirectArgs>(r).nphase);
            } else if (r.kernel.find("deconv5s2") != std::string::npos) {
                const Deconv4Args a = conv_record_args<Deconv4Args>(r);
                printf(" %d %d", a.Cin_pad, a.tiles_w);
            } else if (r.kernel.find("conv5s1_small") != std::string::npos) {
                printf(" %d", conv_record_args<Conv5s1Args>(r).tiles_w);
            } else {
                fprintf(stderr, "unknown kernel %s\n", r.kernel.c_str());
                return 3;
            }
            printf("\n");
        }
    }
    return 0;
}
#endif
