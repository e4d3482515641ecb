// homography_math.h -- float64 3 x 3 and 8 x 8 pieces shared by the adjoints of the homography chains (udh_train.hip:
// udh_photo_matrix_bwd_kernel; warp_bwd_matrix.hip: warp_matrix_bwd_kernel, homography_from_corners_bwd_kernel).
#pragma once
#include "common.h"

// Gaussian elimination with partial pivoting of an 8 x 8 system; false if a pivot is exactly zero.
__device__ inline bool solve8(double (&A)[8][9], double (&x)[8]) {
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        for (int r = c + 1; r < 8; ++r)
            if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
        if (A[piv][c] == 0.0 || A[piv][c] != A[piv][c]) return false;
        if (piv != c)
            for (int k = 0; k < 9; ++k) { const double t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; }
        for (int r = c + 1; r < 8; ++r) {
            const double f = A[r][c] / A[c][c];
            for (int k = c; k < 9; ++k) A[r][k] -= f * A[c][k];
        }
    }
    for (int c = 7; c >= 0; --c) {
        double s = A[c][8];
        for (int k = c + 1; k < 8; ++k) s -= A[c][k] * x[k];
        x[c] = s / A[c][c];
    }
    return true;
}

__device__ inline bool inv3(const double* a, double* r) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    if (det == 0.0 || det != det) return false;
    const double id = 1.0 / det;
    r[0] = c00 * id; r[1] = (a[2] * a[7] - a[1] * a[8]) * id; r[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    r[3] = c01 * id; r[4] = (a[0] * a[8] - a[2] * a[6]) * id; r[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    r[6] = c02 * id; r[7] = (a[1] * a[6] - a[0] * a[7]) * id; r[8] = (a[0] * a[4] - a[1] * a[3]) * id;
    return true;
}

__device__ inline void mul3(const double* a, const double* b, double* c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__device__ inline void mul3_tn(const double* a, const double* b, double* c) {      // a^T b
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}
__device__ inline void mul3_nt(const double* a, const double* b, double* c) {      // a b^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}

// adjoint of R = inverse(A) given R: g_A = -R^T g_R R^T
__device__ inline void inv3_bwd(const double* r, const double* g_r, double* g_a) {
    double t[9];
    mul3_tn(r, g_r, t);
    mul3_nt(t, r, g_a);
    for (int k = 0; k < 9; ++k) g_a[k] = -g_a[k];
}

// N(h, w) = [[2/(w-1), 0, -1], [0, 2/(h-1), -1], [0, 0, 1]] of the destination and N^-1 of the source (kornia: a size-1 axis
// divides by 1e-14)
__device__ inline void normal_transforms(int Hs, int Ws, int Hd, int Wd, double* nd, double* nsi) {
    const double sxs = Ws == 1 ? 1e-14 : (double)(Ws - 1), sys = Hs == 1 ? 1e-14 : (double)(Hs - 1);
    const double sxd = Wd == 1 ? 1e-14 : (double)(Wd - 1), syd = Hd == 1 ? 1e-14 : (double)(Hd - 1);
    for (int k = 0; k < 9; ++k) nd[k] = nsi[k] = 0.0;
    nd[0] = 2.0 / sxd; nd[2] = -1.0; nd[4] = 2.0 / syd; nd[5] = -1.0; nd[8] = 1.0;
    nsi[0] = sxs / 2.0; nsi[2] = sxs / 2.0; nsi[4] = sys / 2.0; nsi[5] = sys / 2.0; nsi[8] = 1.0;
}
