// warp_bwd_matrix.hip -- the perspective warp differentiated with respect to its 3 x 3 matrix (gfx950).
//
// The reference's four warps (coremasic/mywork/MASIC.py:638,644,781,821/833) are kornia.warp_perspective, which is differentiable
// in h_matrix; warp.hip / backward.hip carry the gradient with respect to the source image only.  Here:
//
//   masic_warp_perspective_bwd_matrix   d loss / d minv_norm of dst = warp(src; minv_norm) from an arbitrary incoming gradient on a
//                                       C-channel destination (src NULL: the all-ones source of the mask warp), as per-workgroup
//                                       partial sums in float64;
//   masic_warp_matrix_bwd               the adjoint of warp_matrix_kernel: those partials (of the forward chain, of the
//                                       invert_first chain, or both) -> d loss / d M;
//   masic_homography_from_corners_bwd   the adjoint of homography_from_corners_kernel: d loss / d h_matrix -> d loss / d delta.
//
// The sampling coordinates are recomputed by warp_sample.h, the code warp_kernel itself runs, so the bilinear derivative is taken
// in the cell the forward sampled.  Everything after the coordinates is float64.  No float atomics and no cross-workgroup
// combine inside a launch: every workgroup stores nine sums into a slot of its own, an item's slots depend on that item's pixels
// only, and whoever adds the slots does so in a fixed order (slot_sum) -- results are bit-reproducible and do not depend on the batch an item
// is part of (the pattern of udh_train.hip: udh_photo_loss_bwd_kernel / udh_photo_matrix_bwd_kernel).
#include "common.h"
#include "homography_math.h"
#include "warp_sample.h"

namespace {

constexpr int WBM_PIX = 1024;          // destination pixels per workgroup: four per lane, 256 lanes apart

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// part[b][block][9]: sum over the block's pixels of (dL/dX, dL/dY, dL/dZ) (x) (gx, gy, 1), [X Y Z]^T = minv_norm [gx gy 1]^T
__global__ __launch_bounds__(256) void warp_bwd_matrix_kernel(const float* __restrict__ src, const float* __restrict__ minv, const float* __restrict__ g_dst,
                                                              double* __restrict__ part, int C, int Hs, int Ws, int Hd, int Wd, int align_corners) {
    __shared__ double red[4][9];
    const int b = blockIdx.y;
    const int npix = Hd * Wd;
    const size_t splane = (size_t)Hs * Ws, dplane = (size_t)npix;
    // source pixels per unit of the normalised coordinate (masic_grid_unnormalize)
    const double ux = align_corners ? 0.5 * (double)(Ws - 1) : 0.5 * (double)Ws;
    const double uy = align_corners ? 0.5 * (double)(Hs - 1) : 0.5 * (double)Hs;
    double g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = 0.0;
    for (int j = 0; j < WBM_PIX / 256; ++j) {
        const int pix = blockIdx.x * WBM_PIX + j * 256 + threadIdx.x;
        if (pix >= npix) break;
        const int oy = pix / Wd, ox = pix - oy * Wd;
        const WarpSample s = masic_warp_sample(minv + b * 9, ox, oy, Hs, Ws, Hd, Wd, align_corners);
        if (!s.finite()) continue;        // the forward stored 0 whatever the matrix
        const bool vx0 = s.vx0(Ws), vx1 = s.vx1(Ws), vy0 = s.vy0(Hs), vy1 = s.vy1(Hs);
        const bool v_nw = vx0 && vy0, v_ne = vx1 && vy0, v_sw = vx0 && vy1, v_se = vx1 && vy1;
        if (!(v_nw || v_ne || v_sw || v_se)) continue;
        const double wx = (double)s.wx, wy = (double)s.wy, ex = (double)s.ex, ey = (double)s.ey;
        const long o_n = (long)s.y0 * Ws + s.x0, o_s = o_n + Ws;          // read only where the tap is in range
        double dfx = 0.0, dfy = 0.0;      // dL / d(source x), dL / d(source y) in pixels
        if (src == nullptr) {
            const double nw = v_nw ? 1.0 : 0.0, ne = v_ne ? 1.0 : 0.0, sw = v_sw ? 1.0 : 0.0, se = v_se ? 1.0 : 0.0;
            const double gd = (double)g_dst[(size_t)b * dplane + pix];
            dfx = gd * ((ne - nw) * ey + (se - sw) * wy);
            dfy = gd * ((sw - nw) * ex + (se - ne) * wx);
        } else {
            const float* sc = src + (size_t)b * C * splane;
            const float* gc = g_dst + (size_t)b * C * dplane + pix;
            for (int c = 0; c < C; ++c, sc += splane, gc += dplane) {
                const double nw = v_nw ? (double)sc[o_n] : 0.0, ne = v_ne ? (double)sc[o_n + 1] : 0.0;
                const double sw = v_sw ? (double)sc[o_s] : 0.0, se = v_se ? (double)sc[o_s + 1] : 0.0;
                const double gd = (double)gc[0];
                dfx += gd * ((ne - nw) * ey + (se - sw) * wy);
                dfy += gd * ((sw - nw) * ex + (se - ne) * wx);
            }
        }
        const double gnx = dfx * ux, gny = dfy * uy;
        const double sc_ = (double)s.scale;
        const double gX = gnx * sc_, gY = gny * sc_;
        const double gZ = s.divides() ? -(gnx * (double)s.X + gny * (double)s.Y) * sc_ * sc_ : 0.0;
        const double px = (double)s.gx, py = (double)s.gy;
        g[0] += gX * px; g[1] += gX * py; g[2] += gX;
        g[3] += gY * px; g[4] += gY * py; g[5] += gY;
        g[6] += gZ * px; g[7] += gZ * py; g[8] += gZ;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double t = wave_sum(g[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int k = threadIdx.x;
        part[((size_t)b * gridDim.x + blockIdx.x) * 9 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// Entry k of item b's slots [slots][9], added by one wave in a fixed order: lane l adds slots l, l + 64, l + 128, ... in index order,
// then the 64 partial sums go through the butterfly of wave_sum.  Every lane returns the same value; it depends on the item's own
// slots only, and with a single slot it is that slot exactly.
template <typename T>
__device__ __forceinline__ double slot_sum(const T* __restrict__ g, int b, int slots, int k) {
    const T* p = g + (size_t)b * slots * 9 + k;
    double s = 0.0;
    for (int j = threadIdx.x; j < slots; j += 64) s += (double)p[(size_t)j * 9];
    return wave_sum(s);
}

// g_minv[b][k] = slot_sum of item b (one wave per item), rounded once to float32 (what an autograd node hands on)
__global__ __launch_bounds__(64) void warp_bwd_matrix_finish_kernel(const double* __restrict__ part, float* __restrict__ g_minv, int slots) {
    const int b = blockIdx.x;
    for (int k = 0; k < 9; ++k) {
        const double s = slot_sum<double>(part, b, slots, k);
        if (threadIdx.x == 0) g_minv[b * 9 + k] = (float)s;
    }
}

// adjoint of S = inverse(N_dst A N_src^-1) given g_S: g_A.  false for a singular chain.
__device__ bool chain_bwd(const double* a, const double* nd, const double* nsi, const double* g_s, double* g_a) {
    double t[9], u[9], s[9], g_u[9];
    mul3(a, nsi, t);
    mul3(nd, t, u);
    if (!inv3(u, s)) return false;
    inv3_bwd(s, g_s, g_u);
    mul3_tn(nd, g_u, t);              // U = N_dst A N_src^-1: g_A = N_dst^T g_U N_src^-T
    mul3_nt(t, nsi, g_a);
    return true;
}

// The adjoint of warp_matrix_kernel, one wave per item (the wave adds the slots, lane 0 does the 3 x 3 algebra): g_M = adjoint of inverse(N_dst M N_src^-1) applied to the forward chain's
// slots + adjoint of inverse(N_dst inverse(M) N_src^-1) applied to the invert_first chain's (either may be absent).
__global__ __launch_bounds__(64) void warp_matrix_bwd_kernel(const float* __restrict__ M, const void* __restrict__ g_fwd, int slots_fwd,
                                                             const void* __restrict__ g_inv, int slots_inv, int f64, float* __restrict__ g_M, int B,
                                                             int Hs, int Ws, int Hd, int Wd) {
    const int b = blockIdx.x;
    double m[9], nd[9], nsi[9], out[9], gf[9], gi[9], ga[9];
    for (int k = 0; k < 9; ++k) {          // (uniform branches: every lane of the wave takes part in the sums)
        gf[k] = g_fwd == nullptr ? 0.0 : (f64 ? slot_sum((const double*)g_fwd, b, slots_fwd, k) : slot_sum((const float*)g_fwd, b, slots_fwd, k));
        gi[k] = g_inv == nullptr ? 0.0 : (f64 ? slot_sum((const double*)g_inv, b, slots_inv, k) : slot_sum((const float*)g_inv, b, slots_inv, k));
    }
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 9; ++k) { m[k] = (double)M[b * 9 + k]; out[k] = 0.0; }
    normal_transforms(Hs, Ws, Hd, Wd, nd, nsi);
    bool ok = true;
    if (g_fwd != nullptr) {
        ok = chain_bwd(m, nd, nsi, gf, ga);
        for (int k = 0; k < 9; ++k) out[k] += ga[k];
    }
    if (g_inv != nullptr && ok) {
        double mi[9], gm[9];
        ok = inv3(m, mi) && chain_bwd(mi, nd, nsi, gi, ga);
        if (ok) {
            inv3_bwd(mi, ga, gm);
            for (int k = 0; k < 9; ++k) out[k] += gm[k];
        }
    }
    for (int k = 0; k < 9; ++k) g_M[b * 9 + k] = ok ? (float)out[k] : __builtin_nanf("");
}

// The adjoint of homography_from_corners_kernel (warp.hip), one lane per pair: h_adjust's four scalings, the cofactor inverse,
// and the 8 x 8 direct-linear-transform solve by implicit differentiation (A x = b: lambda = A^-T g_x, g_A = -lambda x^T,
// g_b = lambda), as udh_photo_matrix_bwd_kernel does it.
__global__ __launch_bounds__(64) void homography_from_corners_bwd_kernel(const float* __restrict__ corners, const float* __restrict__ delta,
                                                                         const float* __restrict__ g_h, float* __restrict__ g_delta, int B, float a, float b) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B) return;
    double px[4], py[4], qx[4], qy[4];
    double A[8][9], x[8];
    for (int k = 0; k < 4; ++k) {
        px[k] = corners[(i * 4 + k) * 2];
        py[k] = corners[(i * 4 + k) * 2 + 1];
        qx[k] = (double)(corners[(i * 4 + k) * 2] + delta[(i * 4 + k) * 2]);            // corners_hat is formed in float32
        qy[k] = (double)(corners[(i * 4 + k) * 2 + 1] + delta[(i * 4 + k) * 2 + 1]);
    }
    auto rows = [&](double (&R)[8][9]) {
        for (int k = 0; k < 4; ++k) {
            double* rx = R[2 * k];
            double* ry = R[2 * k + 1];
            rx[0] = px[k]; rx[1] = py[k]; rx[2] = 1; rx[3] = 0; rx[4] = 0; rx[5] = 0; rx[6] = -px[k] * qx[k]; rx[7] = -py[k] * qx[k]; rx[8] = qx[k];
            ry[0] = 0; ry[1] = 0; ry[2] = 0; ry[3] = px[k]; ry[4] = py[k]; ry[5] = 1; ry[6] = -px[k] * qy[k]; ry[7] = -py[k] * qy[k]; ry[8] = qy[k];
        }
    };
    rows(A);
    bool ok = solve8(A, x);
    double lam[8];
    if (ok) {
        double H[9], h[9], gr[9], gH[9];
        for (int k = 0; k < 8; ++k) H[k] = x[k];
        H[8] = 1.0;
        ok = inv3(H, h);
        if (ok) {
            // h_adjust in the forward's order and float32 factors: row 0 by a, column 0 by 1/a, row 1 by b, column 1 by 1/b
            const double ia = (double)(1.0f / a), ib = (double)(1.0f / b);
            const double rs[3] = {(double)a, (double)b, 1.0}, cs[3] = {ia, ib, 1.0};
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) gr[3 * r + c] = (double)g_h[(size_t)i * 9 + 3 * r + c] * rs[r] * cs[c];
            inv3_bwd(h, gr, gH);          // entry 8 of H is the constant 1: its gradient is dropped
            double At[8][9];
            rows(A);
            for (int r = 0; r < 8; ++r) {
                for (int k = 0; k < 8; ++k) At[r][k] = A[k][r];
                At[r][8] = gH[r];
            }
            ok = solve8(At, lam);
        }
    }
    for (int k = 0; k < 4; ++k) {
        float gu = __builtin_nanf(""), gv = gu;
        if (ok) {
            // u enters row 2k through b and the entries -x u, -y u (columns 6, 7); v the same in row 2k + 1
            const double f = 1.0 + px[k] * x[6] + py[k] * x[7];
            gu = (float)(lam[2 * k] * f);
            gv = (float)(lam[2 * k + 1] * f);
        }
        g_delta[(size_t)i * 8 + 2 * k] = gu;
        g_delta[(size_t)i * 8 + 2 * k + 1] = gv;
    }
}

}  // namespace

extern "C" int masic_warp_matrix_slots(int Hd, int Wd) { return Hd > 0 && Wd > 0 && (long)Hd * Wd <= (1L << 30) ? ceil_div(Hd * Wd, WBM_PIX) : 0; }

extern "C" int masic_warp_perspective_bwd_matrix(const float* src, const float* minv_norm, const float* g_dst, double* part, float* g_minv,
                                                 int B, int C, int Hs, int Ws, int Hd, int Wd, void* stream) {
    MASIC_REQUIRE(minv_norm && g_dst && part, MASIC_ERR_ARG, "warp_perspective_bwd_matrix: null pointer");
    MASIC_REQUIRE(src != nullptr || C == 1, MASIC_ERR_ARG, "warp_perspective_bwd_matrix: ones-source needs C == 1");
    const int slots = masic_warp_matrix_slots(Hd, Wd);
    MASIC_REQUIRE(B > 0 && B <= 65535 && C > 0 && Hs > 0 && Ws > 0 && slots > 0 && (long)Hs * Ws <= (1L << 30) && (long)B * slots <= (1L << 26),
                  MASIC_ERR_SHAPE, "warp_perspective_bwd_matrix: B %d, C %d, %d x %d -> %d x %d", B, C, Hs, Ws, Hd, Wd);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(warp_bwd_matrix_kernel, dim3(slots, B), dim3(256), 0, st, src, minv_norm, g_dst, part, C, Hs, Ws, Hd, Wd,
                       masic_warp_align_corners_value());
    if (g_minv != nullptr)
        hipLaunchKernelGGL(warp_bwd_matrix_finish_kernel, dim3(B), dim3(64), 0, st, (const double*)part, g_minv, slots);
    return masic_launch_status("warp_perspective_bwd_matrix");
}

extern "C" int masic_warp_matrix_bwd(const float* M, const void* g_fwd, int slots_fwd, const void* g_inv, int slots_inv, int slots_f64, float* g_M,
                                     int B, int Hs, int Ws, int Hd, int Wd, void* stream) {
    MASIC_REQUIRE(M && g_M && (g_fwd || g_inv), MASIC_ERR_ARG, "warp_matrix_bwd: null pointer");
    MASIC_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && (!g_fwd || slots_fwd > 0) && (!g_inv || slots_inv > 0), MASIC_ERR_SHAPE,
                  "warp_matrix_bwd: B %d, slots %d / %d", B, slots_fwd, slots_inv);
    hipLaunchKernelGGL(warp_matrix_bwd_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, M, g_fwd, slots_fwd, g_inv, slots_inv,
                       slots_f64, g_M, B, Hs, Ws, Hd, Wd);
    return masic_launch_status("warp_matrix_bwd");
}

extern "C" int masic_homography_from_corners_bwd(const float* corners, const float* delta, const float* g_h, float* g_delta, int B, float scale_a,
                                                 float scale_b, void* stream) {
    MASIC_REQUIRE(corners && delta && g_h && g_delta, MASIC_ERR_ARG, "homography_from_corners_bwd: null pointer");
    MASIC_REQUIRE(B > 0 && scale_a > 0.0f && scale_b > 0.0f, MASIC_ERR_SHAPE, "homography_from_corners_bwd: B=%d, scales %g %g", B, (double)scale_a,
                  (double)scale_b);
    hipLaunchKernelGGL(homography_from_corners_bwd_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, corners, delta, g_h, g_delta, B,
                       scale_a, scale_b);
    return masic_launch_status("homography_from_corners_bwd");
}
