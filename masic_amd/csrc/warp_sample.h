// warp_sample.h -- where the perspective warp samples: one destination pixel -> the source cell and its bilinear weights.
//
// Shared by warp.hip (warp_kernel, the forward) and warp_bwd_matrix.hip (the gradient with respect to the sampling matrix), so
// that the derivative is taken in the cell the forward sampled: the same float32 operations in the same order (explicit
// __fmul_rn / __fadd_rn: no FMA contraction), the same floorf, the same saturating int conversion, the same `finite` test.
// warp_kernel's output bits are pinned by goldens; a change here changes them.
#pragma once
#include "common.h"

struct WarpSample {
    float gx, gy;                  // the normalised destination grid point
    float X, Y, Z, scale;          // [X Y Z]^T = minv [gx gy 1]^T; scale = 1 / (Z + eps), 1 where |Z| <= eps
    float fx, fy;                  // the sampling position in source pixels
    float wx, wy, ex, ey;          // fractional position inside the cell, and 1 - it
    int x0, y0;                    // the cell's north-west corner

    __device__ __forceinline__ bool divides() const { return fabsf(Z) > 1e-8f; }
    __device__ __forceinline__ bool finite() const { return (fx == fx) && (fy == fy); }          // neither coordinate is NaN
    // which of the cell's columns / rows lie inside a source of Hs x Ws
    __device__ __forceinline__ bool vx0(int Ws) const { return x0 >= 0 && x0 < Ws; }
    __device__ __forceinline__ bool vx1(int Ws) const { return x0 + 1 >= 0 && x0 + 1 < Ws; }
    __device__ __forceinline__ bool vy0(int Hs) const { return y0 >= 0 && y0 < Hs; }
    __device__ __forceinline__ bool vy1(int Hs) const { return y0 + 1 >= 0 && y0 + 1 < Hs; }
};

// create_meshgrid(normalized) -> transform_points -> convert_points_from_homogeneous(eps = 1e-8) -> grid_sample's unnormalisation
__device__ __forceinline__ WarpSample masic_warp_sample(const float* __restrict__ m, int ox, int oy, int Hs, int Ws, int Hd, int Wd,
                                                        int align_corners) {
    WarpSample s;
    // create_meshgrid(normalized_coordinates=True): (i / (n-1) - 0.5) * 2
    s.gx = __fmul_rn(__fsub_rn(__fdiv_rn((float)ox, (float)(Wd - 1)), 0.5f), 2.0f);
    s.gy = __fmul_rn(__fsub_rn(__fdiv_rn((float)oy, (float)(Hd - 1)), 0.5f), 2.0f);
    s.X = __fadd_rn(__fadd_rn(__fmul_rn(s.gx, m[0]), __fmul_rn(s.gy, m[1])), m[2]);
    s.Y = __fadd_rn(__fadd_rn(__fmul_rn(s.gx, m[3]), __fmul_rn(s.gy, m[4])), m[5]);
    s.Z = __fadd_rn(__fadd_rn(__fmul_rn(s.gx, m[6]), __fmul_rn(s.gy, m[7])), m[8]);
    s.scale = fabsf(s.Z) > 1e-8f ? __fdiv_rn(1.0f, __fadd_rn(s.Z, 1e-8f)) : 1.0f;
    const float nx = __fmul_rn(s.X, s.scale), ny = __fmul_rn(s.Y, s.scale);
    s.fx = masic_grid_unnormalize(nx, Ws, align_corners);
    s.fy = masic_grid_unnormalize(ny, Hs, align_corners);
    const float x0f = floorf(s.fx), y0f = floorf(s.fy);
    s.wx = __fsub_rn(s.fx, x0f);
    s.wy = __fsub_rn(s.fy, y0f);
    s.ex = __fsub_rn(1.0f, s.wx);
    s.ey = __fsub_rn(1.0f, s.wy);
    // float -> int with saturation so that far-away samples stay out of range instead of wrapping
    const float lim = 1.0e9f;
    s.x0 = (int)fminf(fmaxf(x0f, -lim), lim);
    s.y0 = (int)fminf(fmaxf(y0f, -lim), lim);
    return s;
}
