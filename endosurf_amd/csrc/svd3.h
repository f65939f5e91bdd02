// The singular value decomposition of a 3 x 3 matrix in fp64 registers by a fixed number of one-sided (Hestenes) Jacobi sweeps, and
// what register.hip builds on it: the proper rotation that best maps one weighted point set onto another (Kabsch).  The one-sided
// form works on the matrix itself, not on S^T S, so a second singular value far below the first keeps its relative accuracy: the
// rank test of the rigid fit (1e-12) needs that; sym3.h's eigenvalues of S^T S would resolve it to 1e-8 only.
#pragma once
#include <hip/hip_runtime.h>

#include "sym3.h"

namespace es {

constexpr int SVD3_SWEEPS = 12;          // three column pairs a sweep; orthogonal to fp64 rounding after 5 - 6, the count is fixed

__device__ __forceinline__ double dot3r(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3r(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// One plane rotation that makes the columns ai, aj orthogonal; the same rotation is applied to vi, vj (sym3.h's choice of the
// smaller angle).
__device__ __forceinline__ void hestenes_rot(double (&ai)[3], double (&aj)[3], double (&vi)[3], double (&vj)[3]) {
    const double alpha = dot3r(ai, ai), beta = dot3r(aj, aj), gamma = dot3r(ai, aj);
    if (gamma == 0.0) return;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));          // (zeta^2 = inf: t = 0)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = ai[k], y = aj[k], vx = vi[k], vy = vj[k];
        ai[k] = c * x - s * y;
        aj[k] = s * x + c * y;
        vi[k] = c * vx - s * vy;
        vj[k] = s * vx + c * vy;
    }
}

// S (row-major) = U diag(sigma) V^T: on return column k of S V is a[k] = sigma[k] u_k and v[k] is column k of V; no order.
__device__ __forceinline__ void svd3_columns(const double (&S)[9], double (&a)[3][3], double (&v)[3][3], double (&sigma)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[k][r] = S[3 * r + k];
            v[k][r] = r == k ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < SVD3_SWEEPS; ++sweep) {
        hestenes_rot(a[0], a[1], v[0], v[1]);
        hestenes_rot(a[0], a[2], v[0], v[2]);
        hestenes_rot(a[1], a[2], v[1], v[2]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) sigma[k] = sqrt(dot3r(a[k], a[k]));
}

// The proper rotation R (row-major) that maximises trace(R S) for S = sum w p q^T (centred): with u_1, u_2 and v_1, v_2 the singular
// vectors of the two largest singular values, R = v_1 u_1^T + v_2 u_2^T + (v_1 x v_2) (u_1 x u_2)^T -- Kabsch's V diag(1, 1, det) U^T
// without a determinant: the third pair is built, so R is proper by construction and a planar set (sigma_3 = 0) needs no special
// case.  false, and R untouched, where sigma_2 <= rank_rel sigma_1 (coincident or collinear points: no rotation is determined).
__device__ __forceinline__ bool kabsch_rotation(const double (&S)[9], double rank_rel, double (&R)[9]) {
    double a[3][3], v[3][3], sg[3];
    svd3_columns(S, a, v, sg);
    int i0 = 0, i1 = 1, i2 = 2, t;          // descending order of sigma, ties by index
    if (sg[i1] > sg[i0]) { t = i0; i0 = i1; i1 = t; }
    if (sg[i2] > sg[i1]) { t = i1; i1 = i2; i2 = t; }
    if (sg[i1] > sg[i0]) { t = i0; i0 = i1; i1 = t; }
    double s1 = 0.0, s2 = 0.0, u1[3], u2[3], v1[3], v2[3], u3[3], v3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {          // (selects, not dynamic indexing: the arrays stay in registers)
        if (k == i0) { s1 = sg[k]; for (int r = 0; r < 3; ++r) { u1[r] = a[k][r]; v1[r] = v[k][r]; } }
        if (k == i1) { s2 = sg[k]; for (int r = 0; r < 3; ++r) { u2[r] = a[k][r]; v2[r] = v[k][r]; } }
    }
    if (!(s2 > rank_rel * s1)) return false;
#pragma unroll
    for (int r = 0; r < 3; ++r) { u1[r] /= s1; u2[r] /= s2; }
    cross3r(u1, u2, u3);
    cross3r(v1, v2, v3);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (v1[i] * u1[j] + v2[i] * u2[j]) + v3[i] * u3[j];
    return true;
}

}  // namespace es
