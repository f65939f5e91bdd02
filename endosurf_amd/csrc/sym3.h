// 3 x 3 algebra in fp64 registers for the kernels that work row by row (k_strain_rows, strain.hip; k_kinematics_rows, kinematics.hip):
// determinant, cofactors, and the eigenvalues of a symmetric matrix by a fixed number of cyclic Jacobi sweeps -- the trigonometric
// closed form of the cubic loses ~sqrt(eps) where eigenvalues coincide, which is the common case (F ~ I, a strain rate ~ 0).
#pragma once
#include <hip/hip_runtime.h>

namespace es {

constexpr int JACOBI_SWEEPS = 8;          // a 3 x 3 symmetric matrix is diagonal to fp64 rounding after 4 - 5; the count is fixed

struct Sym3 { double a00, a11, a22, a01, a02, a12; };

// One Jacobi rotation in the (p, q) plane: app, aqq the diagonal entries, apq the entry it annihilates, arp, arq the two entries of
// the third row.  (Rutishauser's update: the diagonal moves by t * apq.)
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));          // (theta^2 = inf: t = 0)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
}

// eigenvalues of a symmetric 3 x 3 matrix, descending
__device__ __forceinline__ void eig_sym3(Sym3 m, double (&w)[3]) {
#pragma unroll 1
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        jacobi_rot(m.a00, m.a11, m.a01, m.a02, m.a12);
        jacobi_rot(m.a00, m.a22, m.a02, m.a01, m.a12);
        jacobi_rot(m.a11, m.a22, m.a12, m.a01, m.a02);
    }
    double a = m.a00, b = m.a11, c = m.a22, t;
    if (a < b) { t = a; a = b; b = t; }
    if (b < c) { t = b; b = c; c = t; }
    if (a < b) { t = a; a = b; b = t; }
    w[0] = a; w[1] = b; w[2] = c;
}

__device__ __forceinline__ double det3(const double (&m)[9]) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// cofactor matrix: cof(m)^T = adj(m), m^-1 = adj(m) / det(m)
__device__ __forceinline__ void cof3(const double (&m)[9], double (&c)[9]) {
    c[0] = m[4] * m[8] - m[5] * m[7]; c[1] = m[5] * m[6] - m[3] * m[8]; c[2] = m[3] * m[7] - m[4] * m[6];
    c[3] = m[2] * m[7] - m[1] * m[8]; c[4] = m[0] * m[8] - m[2] * m[6]; c[5] = m[1] * m[6] - m[0] * m[7];
    c[6] = m[1] * m[5] - m[2] * m[4]; c[7] = m[2] * m[3] - m[0] * m[5]; c[8] = m[0] * m[4] - m[1] * m[3];
}

}  // namespace es
