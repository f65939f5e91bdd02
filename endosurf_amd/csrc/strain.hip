// Strain of the tracked map between two times, row by row (endosurf_amd/strain.py strain_rows is the specification and the fp64
// twin):  F = J_to^-1 J_from  from the deformation Jacobians at the two ends of a track, its determinant (the volume
// ratio), its singular values (the principal stretches) and, with a unit normal n of the surface at the "from" end, the area ratio
// |cof(F) n| (Nanson) and the two singular values of F restricted to the tangent plane.  One thread per row, fp64 arithmetic in
// registers, fp32 results, plain loads and stores, no atomics: the same bits from call to call.  The inverse goes by adjugate and
// determinant; the singular values are the square roots of the eigenvalues of F^T F (and of P F^T F P, P = I - n n^T, the two largest)
// by a fixed number of cyclic Jacobi sweeps -- the trigonometric closed form of the cubic loses ~sqrt(eps) where eigenvalues
// coincide, which is the common case F ~ I.
#include <cfloat>

#include "host.h"
#include "launch.h"
#include "sym3.h"

namespace es {

__global__ __launch_bounds__(256) void k_strain_rows(const float* __restrict__ jac_from, const float* __restrict__ jac_to,
                                                     const float* __restrict__ normals, int M, float* __restrict__ F_out,
                                                     float* __restrict__ det_out, float* __restrict__ stretch_out,
                                                     float* __restrict__ area_out, float* __restrict__ surface_out,
                                                     unsigned char* __restrict__ valid_out) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (size_t)M) return;
    double Ja[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, Jb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        Jb[k] = (double)jac_to[9 * r + k];
        if (jac_from) Ja[k] = (double)jac_from[9 * r + k];
    }
    const double da = det3(Ja), db = det3(Jb);
    bool valid = da > 0.0 && db > 0.0;          // (false for NaN)
    double n[3] = {0.0, 0.0, 0.0};
    if (normals) {
        const double n0 = (double)normals[3 * r], n1 = (double)normals[3 * r + 1], n2 = (double)normals[3 * r + 2];
        const double len = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
        const bool n_ok = len > 0.0 && len <= DBL_MAX;          // a finite positive length (false for NaN)
        valid = valid && n_ok;
        if (n_ok) { n[0] = n0 / len; n[1] = n1 / len; n[2] = n2 / len; }
    }
    double F[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double det = 0.0, w[3] = {0.0, 0.0, 0.0}, area = 0.0, ws[3] = {0.0, 0.0, 0.0};
    if (valid) {
        double cb[9];
        cof3(Jb, cb);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)          // adj(Jb) = cof(Jb)^T
                F[3 * i + j] = (cb[i] * Ja[j] + cb[3 + i] * Ja[3 + j] + cb[6 + i] * Ja[6 + j]) / db;
        det = da / db;
        Sym3 C;
        C.a00 = F[0] * F[0] + F[3] * F[3] + F[6] * F[6];
        C.a11 = F[1] * F[1] + F[4] * F[4] + F[7] * F[7];
        C.a22 = F[2] * F[2] + F[5] * F[5] + F[8] * F[8];
        C.a01 = F[0] * F[1] + F[3] * F[4] + F[6] * F[7];
        C.a02 = F[0] * F[2] + F[3] * F[5] + F[6] * F[8];
        C.a12 = F[1] * F[2] + F[4] * F[5] + F[7] * F[8];
        eig_sym3(C, w);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = sqrt(fmax(w[k], 0.0));
        if (normals) {
            double cf[9];
            cof3(F, cf);
            const double g0 = cf[0] * n[0] + cf[1] * n[1] + cf[2] * n[2], g1 = cf[3] * n[0] + cf[4] * n[1] + cf[5] * n[2],
                         g2 = cf[6] * n[0] + cf[7] * n[1] + cf[8] * n[2];
            area = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
            // P C P with P = I - n n^T:  C - n (Cn)^T - (Cn) n^T + (n^T C n) n n^T
            const double c0 = C.a00 * n[0] + C.a01 * n[1] + C.a02 * n[2], c1 = C.a01 * n[0] + C.a11 * n[1] + C.a12 * n[2],
                         c2 = C.a02 * n[0] + C.a12 * n[1] + C.a22 * n[2];
            const double q = c0 * n[0] + c1 * n[1] + c2 * n[2];
            Sym3 S;
            S.a00 = C.a00 - 2.0 * n[0] * c0 + q * n[0] * n[0];
            S.a11 = C.a11 - 2.0 * n[1] * c1 + q * n[1] * n[1];
            S.a22 = C.a22 - 2.0 * n[2] * c2 + q * n[2] * n[2];
            S.a01 = C.a01 - n[0] * c1 - c0 * n[1] + q * n[0] * n[1];
            S.a02 = C.a02 - n[0] * c2 - c0 * n[2] + q * n[0] * n[2];
            S.a12 = C.a12 - n[1] * c2 - c1 * n[2] + q * n[1] * n[2];
            eig_sym3(S, ws);          // the third eigenvalue is the 0 of the direction n
#pragma unroll
            for (int k = 0; k < 2; ++k) ws[k] = sqrt(fmax(ws[k], 0.0));
        }
    }
    if (F_out)
#pragma unroll
        for (int k = 0; k < 9; ++k) F_out[9 * r + k] = (float)F[k];
    if (det_out) det_out[r] = (float)det;
    if (stretch_out) { stretch_out[3 * r] = (float)w[0]; stretch_out[3 * r + 1] = (float)w[1]; stretch_out[3 * r + 2] = (float)w[2]; }
    if (area_out) area_out[r] = (float)area;
    if (surface_out) { surface_out[2 * r] = (float)ws[0]; surface_out[2 * r + 1] = (float)ws[1]; }
    if (valid_out) valid_out[r] = valid ? 1 : 0;
}

int strain_rows(const float* jac_from, const float* jac_to, const float* normals, int M, float* F_out, float* det_out, float* stretch_out,
                float* area_out, float* surface_out, unsigned char* valid_out, hipStream_t st) {
    if (M <= 0) return ST_OK;
    const dim3 grid((M - 1) / 256 + 1), block(256);
    hipLaunchKernelGGL(k_strain_rows, grid, block, 0, st, jac_from, jac_to, normals, M, F_out, det_out, stretch_out, area_out, surface_out,
                       valid_out);
    return hip_last("strain_rows");
}

}  // namespace es
