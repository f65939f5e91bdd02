// Velocity and strain rate of the tissue at a point, row by row (endosurf_amd/kinematics.py kinematics_rows is the specification and
// the fp64 twin, in its diagonal form with d_xt = 0).  A material point satisfies y + D(y, t) = c, so with J = I + dD/dx,
// D_t = dD/dt and dd[i][k] = d2 D_i / d x_k^2 (the mixed second derivatives of the network vanish):
//     v = -J^-1 D_t,        L_ik = -(J^-1)_il dd_lk v_k        (dF/dt = L F),
// d = sym L the strain rate, its eigenvalues the principal rates, tr L the rate of ln(volume), the axial vector of L - L^T the
// vorticity and, with a unit normal n of the surface in the current configuration, tr d - n.d.n the rate of ln(area) and the
// eigenvalues of d restricted to the plane normal to n.  One thread per row, fp64 arithmetic in registers, fp32 results, plain loads
// and stores, no atomics: the same bits from call to call.  The inverse goes by adjugate and determinant, the eigenvalues of d by
// k_strain_rows' Jacobi sweeps (sym3.h), those of the 2 x 2 restriction in closed form (mean +- hypot, as k_curvature_rows).
#include <cfloat>

#include "host.h"
#include "launch.h"
#include "sym3.h"

namespace es {

__global__ __launch_bounds__(256) void k_kinematics_rows(const float* __restrict__ jac, const float* __restrict__ d_t,
                                                         const float* __restrict__ dd, const float* __restrict__ normals, int M,
                                                         float* __restrict__ vel_out, float* __restrict__ speed_out, float* __restrict__ L_out,
                                                         float* __restrict__ rate_out, float* __restrict__ principal_out,
                                                         float* __restrict__ div_out, float* __restrict__ vort_out,
                                                         float* __restrict__ area_out, float* __restrict__ surface_out,
                                                         unsigned char* __restrict__ valid_out) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (size_t)M) return;
    double J[9], H[9], dt[3];
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        J[k] = (double)jac[9 * r + k];
        H[k] = (double)dd[9 * r + k];
        valid = valid && fabs(J[k]) <= DBL_MAX && fabs(H[k]) <= DBL_MAX;          // finite (false for NaN)
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        dt[k] = (double)d_t[3 * r + k];
        valid = valid && fabs(dt[k]) <= DBL_MAX;
    }
    const double det = det3(J);
    valid = valid && det > 0.0;
    double n[3] = {0.0, 0.0, 0.0};
    if (normals) {
        const double n0 = (double)normals[3 * r], n1 = (double)normals[3 * r + 1], n2 = (double)normals[3 * r + 2];
        const double len = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
        const bool n_ok = len > 0.0 && len <= DBL_MAX;          // a finite positive length (false for NaN)
        valid = valid && n_ok;
        if (n_ok) { n[0] = n0 / len; n[1] = n1 / len; n[2] = n2 / len; }
    }
    double v[3] = {0.0, 0.0, 0.0}, L[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
    double speed = 0.0, div = 0.0, area = 0.0, s1 = 0.0, s2 = 0.0;
    Sym3 d = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (valid) {
        double cf[9];
        cof3(J, cf);          // (J^-1)_il = cof_li / det
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = -(cf[i] * dt[0] + cf[3 + i] * dt[1] + cf[6 + i] * dt[2]) / det;
        speed = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) L[3 * i + k] = -((cf[i] * H[k] + cf[3 + i] * H[3 + k] + cf[6 + i] * H[6 + k]) / det) * v[k];
        div = L[0] + L[4] + L[8];
        d.a00 = L[0]; d.a11 = L[4]; d.a22 = L[8];
        d.a01 = 0.5 * (L[1] + L[3]); d.a02 = 0.5 * (L[2] + L[6]); d.a12 = 0.5 * (L[5] + L[7]);
        eig_sym3(d, w);
        if (normals) {
            // T: n x e for the axis e the normal is furthest from, normalised, and n x that (as k_curvature_rows builds it)
            const double a0 = fabs(n[0]), a1 = fabs(n[1]), a2 = fabs(n[2]);
            const int e = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);          // the first smallest, as numpy.argmin
            double t1[3];
            if (e == 0) { t1[0] = 0.0; t1[1] = n[2]; t1[2] = -n[1]; }
            else if (e == 1) { t1[0] = -n[2]; t1[1] = 0.0; t1[2] = n[0]; }
            else { t1[0] = n[1]; t1[1] = -n[0]; t1[2] = 0.0; }
            const double l1 = sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
            t1[0] /= l1; t1[1] /= l1; t1[2] /= l1;
            const double t2[3] = {n[1] * t1[2] - n[2] * t1[1], n[2] * t1[0] - n[0] * t1[2], n[0] * t1[1] - n[1] * t1[0]};
            const double h1[3] = {d.a00 * t1[0] + d.a01 * t1[1] + d.a02 * t1[2], d.a01 * t1[0] + d.a11 * t1[1] + d.a12 * t1[2],
                                  d.a02 * t1[0] + d.a12 * t1[1] + d.a22 * t1[2]};
            const double h2[3] = {d.a00 * t2[0] + d.a01 * t2[1] + d.a02 * t2[2], d.a01 * t2[0] + d.a11 * t2[1] + d.a12 * t2[2],
                                  d.a02 * t2[0] + d.a12 * t2[1] + d.a22 * t2[2]};
            const double hn[3] = {d.a00 * n[0] + d.a01 * n[1] + d.a02 * n[2], d.a01 * n[0] + d.a11 * n[1] + d.a12 * n[2],
                                  d.a02 * n[0] + d.a12 * n[1] + d.a22 * n[2]};
            area = (d.a00 + d.a11 + d.a22) - (n[0] * hn[0] + n[1] * hn[1] + n[2] * hn[2]);
            const double a = t1[0] * h1[0] + t1[1] * h1[1] + t1[2] * h1[2];
            const double b = t1[0] * h2[0] + t1[1] * h2[1] + t1[2] * h2[2];
            const double c = t2[0] * h2[0] + t2[1] * h2[1] + t2[2] * h2[2];
            const double mean = 0.5 * (a + c), rad = hypot(0.5 * (a - c), b);
            s1 = mean + rad; s2 = mean - rad;
        }
    }
    if (vel_out) { vel_out[3 * r] = (float)v[0]; vel_out[3 * r + 1] = (float)v[1]; vel_out[3 * r + 2] = (float)v[2]; }
    if (speed_out) speed_out[r] = (float)speed;
    if (L_out)
#pragma unroll
        for (int k = 0; k < 9; ++k) L_out[9 * r + k] = (float)L[k];
    if (rate_out) {
        rate_out[9 * r] = (float)d.a00; rate_out[9 * r + 1] = (float)d.a01; rate_out[9 * r + 2] = (float)d.a02;
        rate_out[9 * r + 3] = (float)d.a01; rate_out[9 * r + 4] = (float)d.a11; rate_out[9 * r + 5] = (float)d.a12;
        rate_out[9 * r + 6] = (float)d.a02; rate_out[9 * r + 7] = (float)d.a12; rate_out[9 * r + 8] = (float)d.a22;
    }
    if (principal_out) { principal_out[3 * r] = (float)w[0]; principal_out[3 * r + 1] = (float)w[1]; principal_out[3 * r + 2] = (float)w[2]; }
    if (div_out) div_out[r] = (float)div;
    if (vort_out) { vort_out[3 * r] = (float)(L[7] - L[5]); vort_out[3 * r + 1] = (float)(L[2] - L[6]); vort_out[3 * r + 2] = (float)(L[3] - L[1]); }
    if (area_out) area_out[r] = (float)area;
    if (surface_out) { surface_out[2 * r] = (float)s1; surface_out[2 * r + 1] = (float)s2; }
    if (valid_out) valid_out[r] = valid ? 1 : 0;
}

int kinematics_rows(const float* jac, const float* d_t, const float* dd, const float* normals, int M, float* vel_out, float* speed_out,
                    float* L_out, float* rate_out, float* principal_out, float* div_out, float* vort_out, float* area_out,
                    float* surface_out, unsigned char* valid_out, hipStream_t st) {
    if (M <= 0) return ST_OK;
    const dim3 grid((M - 1) / 256 + 1), block(256);
    hipLaunchKernelGGL(k_kinematics_rows, grid, block, 0, st, jac, d_t, dd, normals, M, vel_out, speed_out, L_out, rate_out, principal_out,
                       div_out, vort_out, area_out, surface_out, valid_out);
    return hip_last("kinematics_rows");
}

}  // namespace es
