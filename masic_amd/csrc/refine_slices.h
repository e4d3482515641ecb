// refine_slices.h -- the one launch shape of the latent refinement's elementwise kernels (refine.hip, refine_budget.hip).
//
// A launch covers up to six tensors of B pairs each: block (x, t, b) walks pair b's slice of tensor t, n[t] floats that start at float
// b * n[t] of the tensor -- on a 16-byte boundary only when that product is a multiple of 4.  The slice is cut into a head of single
// floats up to the next 16-byte boundary, nvec float4 pieces and a tail of single floats; where the arrays of one operation are not
// aligned alike the head is the whole slice.  The grid is bounded (GRID_CAP workgroups) and every loop is a grid-stride loop.  No
// atomics, no grid-wide synchronisation, nothing read by the host.
#pragma once
#include "common.h"

namespace {

constexpr int MAX_PAIRS = 65535;               // the pair is gridDim.z
constexpr int GRID_CAP = 8192;                 // workgroups of a launch at most
constexpr int NT = 6;                          // tensors of a launch at most

struct Span { size_t head, nvec, tail0; };

// the cut of a slice of n floats; mis[k] = float index of array k's slice start within its 16-byte line
template <int K>
__device__ __forceinline__ Span span_of(size_t n, const uintptr_t (&addr)[K]) {
    const unsigned mis = (unsigned)(addr[0] >> 2) & 3u;
    bool alike = (addr[0] & 3u) == 0;
#pragma unroll
    for (int k = 1; k < K; ++k) alike = alike && (addr[k] & 15u) == (addr[0] & 15u);
    size_t head = (4u - mis) & 3u;
    if (!alike || head > n) head = n;
    Span s;
    s.head = head;
    s.nvec = (n - head) / 4;
    s.tail0 = head + s.nvec * 4;
    return s;
}

// grid (gx, tensors, B).  Op: n(t) elements per pair; begin(t, b) -> false to skip the slice, sets the op's slice pointers and returns the
// span through `s`; one(i) handles float i of the slice, four(i) the aligned floats i .. i + 3.
template <class Op>
__global__ __launch_bounds__(256) void slices_kernel(Op op) {
    const int t = blockIdx.y, b = blockIdx.z;
    const size_t n = op.n[t];
    Span s;
    if (n == 0 || !op.begin(t, b, n, s)) return;
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = first; i < s.nvec; i += stride) op.four(s.head + 4 * i);
    for (size_t i = first; i < s.head; i += stride) op.one(i);
    for (size_t i = s.tail0 + first; i < n; i += stride) op.one(i);
}

template <class Op>
void launch_slices(const Op& op, int nt, int B, hipStream_t st) {
    size_t nmax = 1;
    for (int t = 0; t < nt; ++t) nmax = op.n[t] > nmax ? op.n[t] : nmax;
    size_t gx = (nmax / 4 + 255) / 256;
    const size_t cap = (size_t)(GRID_CAP / (nt * B) > 0 ? GRID_CAP / (nt * B) : 1);
    gx = gx > cap ? cap : (gx == 0 ? 1 : gx);
    hipLaunchKernelGGL(slices_kernel<Op>, dim3((unsigned)gx, nt, B), dim3(256), 0, st, op);
}

bool four_ok(const void* const* a, const size_t* n) {
    if (!a || !n) return false;
    for (int k = 0; k < 4; ++k)
        if (!a[k] || n[k] == 0) return false;
    return true;
}

}  // namespace
