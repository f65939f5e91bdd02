// Curvature of the level sets of  sdf(x + D(x, t)), row by row (endosurf_amd/curvature.py compose_hessian / curvature_rows are the
// specification and the fp64 twin).  From the canonical gradient g_c and Hessian H_c of the SDF network, the Jacobian J
// of the deformation and the curvature of its encodings dd = CURV(g_c) (ES_WS_CURV):
//     g_o = J^T g_c,        H_o = J^T H_c J - diag(dd),
// and with n = g_o / |g_o| (towards increasing SDF), T = [t1 t2] an orthonormal basis of the plane normal to n and the shape operator
// S = T^T H_o T / |g_o| = [[a, b], [b, c]]:  mean = (a + c) / 2,  gauss = a c - b^2,  principal = mean +- hypot((a - c) / 2, b).
// A sphere |x| - R seen from outside has both curvatures +1/R.  T as strain.hip's twin builds it: t1 = n x e normalised for the axis e
// the normal is furthest from, t2 = n x t1.  One thread per row, fp64 arithmetic in registers, fp32 results, plain loads and stores,
// no atomics: the same bits from call to call.
#include <cfloat>

#include "host.h"
#include "launch.h"

namespace es {

__global__ __launch_bounds__(256) void k_curvature_rows(const float* __restrict__ grad_c, const float* __restrict__ hess_c,
                                                        const float* __restrict__ jac, const float* __restrict__ dd, int M,
                                                        float* __restrict__ grad_o, float* __restrict__ hess_o, float* __restrict__ mean_out,
                                                        float* __restrict__ gauss_out, float* __restrict__ principal_out,
                                                        unsigned char* __restrict__ valid_out) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (size_t)M) return;
    double g[3], H[9], J[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, d[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        H[k] = (double)hess_c[9 * r + k];
        if (jac) J[k] = (double)jac[9 * r + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g[k] = (double)grad_c[3 * r + k];
        if (dd) d[k] = (double)dd[3 * r + k];
    }
    double go[3], HJ[9], Ho[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) go[j] = J[j] * g[0] + J[3 + j] * g[1] + J[6 + j] * g[2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) HJ[3 * i + j] = H[3 * i] * J[j] + H[3 * i + 1] * J[3 + j] + H[3 * i + 2] * J[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Ho[3 * i + j] = J[i] * HJ[j] + J[3 + i] * HJ[3 + j] + J[6 + i] * HJ[6 + j] - (i == j ? d[i] : 0.0);
    const double len = sqrt(go[0] * go[0] + go[1] * go[1] + go[2] * go[2]);
    bool valid = len > 0.0 && len <= DBL_MAX;          // a finite positive length (false for NaN)
#pragma unroll
    for (int k = 0; k < 9; ++k) valid = valid && fabs(Ho[k]) <= DBL_MAX;
    double mean = 0.0, gauss = 0.0, k1 = 0.0, k2 = 0.0;
    if (valid) {
        const double n[3] = {go[0] / len, go[1] / len, go[2] / len};
        const double a0 = fabs(n[0]), a1 = fabs(n[1]), a2 = fabs(n[2]);
        const int e = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);          // the first smallest, as numpy.argmin
        double t1[3];          // n x e_e
        if (e == 0) { t1[0] = 0.0; t1[1] = n[2]; t1[2] = -n[1]; }
        else if (e == 1) { t1[0] = -n[2]; t1[1] = 0.0; t1[2] = n[0]; }
        else { t1[0] = n[1]; t1[1] = -n[0]; t1[2] = 0.0; }
        const double l1 = sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
        t1[0] /= l1; t1[1] /= l1; t1[2] /= l1;
        const double t2[3] = {n[1] * t1[2] - n[2] * t1[1], n[2] * t1[0] - n[0] * t1[2], n[0] * t1[1] - n[1] * t1[0]};
        double h1[3], h2[3];          // H_o t1, H_o t2
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            h1[i] = Ho[3 * i] * t1[0] + Ho[3 * i + 1] * t1[1] + Ho[3 * i + 2] * t1[2];
            h2[i] = Ho[3 * i] * t2[0] + Ho[3 * i + 1] * t2[1] + Ho[3 * i + 2] * t2[2];
        }
        const double a = (t1[0] * h1[0] + t1[1] * h1[1] + t1[2] * h1[2]) / len;
        const double b = (t1[0] * h2[0] + t1[1] * h2[1] + t1[2] * h2[2]) / len;
        const double c = (t2[0] * h2[0] + t2[1] * h2[1] + t2[2] * h2[2]) / len;
        mean = 0.5 * (a + c);
        gauss = a * c - b * b;
        const double rad = hypot(0.5 * (a - c), b);
        k1 = mean + rad; k2 = mean - rad;
    }
    if (grad_o) { grad_o[3 * r] = (float)go[0]; grad_o[3 * r + 1] = (float)go[1]; grad_o[3 * r + 2] = (float)go[2]; }
    if (hess_o)
#pragma unroll
        for (int k = 0; k < 9; ++k) hess_o[9 * r + k] = (float)Ho[k];
    if (mean_out) mean_out[r] = (float)mean;
    if (gauss_out) gauss_out[r] = (float)gauss;
    if (principal_out) { principal_out[2 * r] = (float)k1; principal_out[2 * r + 1] = (float)k2; }
    if (valid_out) valid_out[r] = valid ? 1 : 0;
}

int curvature_rows(const float* grad_c, const float* hess_c, const float* jac, const float* dd, int M, float* grad_o, float* hess_o,
                   float* mean_out, float* gauss_out, float* principal_out, unsigned char* valid_out, hipStream_t st) {
    if (M <= 0) return ST_OK;
    const dim3 grid((M - 1) / 256 + 1), block(256);
    hipLaunchKernelGGL(k_curvature_rows, grid, block, 0, st, grad_c, hess_c, jac, dd, M, grad_o, hess_o, mean_out, gauss_out, principal_out,
                       valid_out);
    return hip_last("curvature_rows");
}

}  // namespace es
