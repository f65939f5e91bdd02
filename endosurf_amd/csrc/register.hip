// Rigid registration (endosurf_amd/registration.py is the specification and the fp64 host twin): the least-squares
// rigid motion between corresponding rows (Kabsch) and iterative closest point against the triangles of a mesh, whose closest
// triangles es_surf_query finds.  Rows are fp32, every sum and every solve is fp64.
//
//   k_reg_partials<Rows>   one workgroup per (batch, REG_CHUNK rows): thread t adds rows chunk0 + t, + 256, + 512, + 768 -- a fixed
//                          set, in index order -- into Rows::K fp64 registers (MomentRows: the 17 moments of a rigid fit; PlaneRows:
//                          the 29 sums of a point-to-plane step); block_sum combines the 256 threads by a fixed tree (shuffles down
//                          the 64 lanes, then the 4 wavefronts in order); one partial row of K per workgroup
//   k_reg_total<K>         one workgroup per batch: the batch's partial rows added in index order (thread t owns a contiguous run,
//                          the runs are combined by block_sum) -> out[b][K]
//   k_rigid_solve          one thread per batch: moments -> rotation, translation, weight, valid (svd3.h)
//   k_rigid_apply          one thread per row: R p + t in fp64, rounded to fp32; with q the residual q - (R p + t) and its length
//   k_rigid_rmse           one thread per batch: sqrt(the last moment of (R p + t, q) / W)
//   k_icp_update           one thread: the sums of an iteration -> the next transform in the state record, or nothing once done
//
// No atomics at all: a partial is written by exactly one workgroup and read by a later launch, so two calls give the same bits whatever
// the scratch held before (metrics.hip's scheme).  No workgroup waits for another.  Every device loop is bounded by an argument or a
// constant.  Every index read from ``triangle`` / ``triangles`` is checked against T / V before it is used.  The host side refuses
// sizes whose products leave int32.  The library is compiled with contraction, so a w * p + acc here is one fma where the twin rounds
// twice: the device is held to the twin within a tolerance, bit-exact only from call to call (and where every sum is exact).
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"
#include "svd3.h"

namespace es {

namespace {

constexpr int REG_PER_THREAD = 4;
constexpr int REG_CHUNK = 256 * REG_PER_THREAD;          // rows per workgroup of k_reg_partials (registration.MOMENT_CHUNK)
constexpr int REG_MOMENTS = 17, REG_PLANE = 29;
constexpr long long REG_MAX_COUNT = 1ll << 31;
constexpr double REG_RANK_REL = 1e-12, REG_PIVOT_REL = 1e-12;          // registration.RANK_REL, PIVOT_REL
constexpr int ICP_CONVERGED = 0, ICP_MAX_ITERS = 1, ICP_DEGENERATE = 2, ICP_POINT = 0, ICP_PLANE = 1;
constexpr int ICP_STATE_DOUBLES = 16;          // R[9], t[3], step, then int32 status, iterations, done, (pad)

inline long long reg_chunks(long long N) { return (N + REG_CHUNK - 1) / REG_CHUNK; }
__device__ __forceinline__ bool finite3(const float* x) { return fabsf(x[0]) <= FLT_MAX && fabsf(x[1]) <= FLT_MAX && fabsf(x[2]) <= FLT_MAX; }

// The workgroup's sum of each acc[k], in a fixed order: down the lanes of each wavefront (32, 16, .. 1), then the four wavefronts one
// after the other.  Thread k < K leaves with the sum of entry k in ``mine``.
template <int K>
__device__ __forceinline__ double block_sum(double (&acc)[K], double (&lds)[4][K]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) lds[wv][k] = v;
    }
    __syncthreads();
    double mine = 0.0;
    if (threadIdx.x < K) mine = ((lds[0][threadIdx.x] + lds[1][threadIdx.x]) + lds[2][threadIdx.x]) + lds[3][threadIdx.x];
    return mine;
}

// The 17 moments of rigid_fit: W, sum w p, sum w q, sum w p q^T (row-major), sum w |p - q|^2.
struct MomentRows {
    static constexpr int K = REG_MOMENTS;
    const float* p; const float* q; const float* w;
    long long N;
    int w_per_batch;
    __device__ __forceinline__ void add(int b, long long i, double (&acc)[K]) const {
        const size_t row = (size_t)b * (size_t)N + (size_t)i;
        const float* pr = p + 3 * row;
        const float* qr = q + 3 * row;
        const float wf = w ? w[w_per_batch ? row : (size_t)i] : 1.f;
        if (!(wf > 0.f && wf <= FLT_MAX && finite3(pr) && finite3(qr))) return;
        const double wd = (double)wf;
        const double pd[3] = {(double)pr[0], (double)pr[1], (double)pr[2]}, qd[3] = {(double)qr[0], (double)qr[1], (double)qr[2]};
        acc[0] += wd;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double wp = wd * pd[a];
            acc[1 + a] += wp;
            acc[4 + a] += wd * qd[a];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[7 + 3 * a + c] += wp * qd[c];
        }
        const double d[3] = {pd[0] - qd[0], pd[1] - qd[1], pd[2] - qd[2]};
        acc[16] += wd * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    }
};

// The 29 sums of a point-to-plane step (registration.normal_equations).
struct PlaneRows {
    static constexpr int K = REG_PLANE;
    const float* x; const float* closest; const int* triangle; const float* dist; const float* verts; const int* tris;
    long long V, T, N;
    double max_distance;          // negative: none
    __device__ __forceinline__ void add(int, long long i, double (&acc)[K]) const {
        const long long t = triangle[i];
        if (t < 0 || t >= T) return;
        if (max_distance >= 0.0 && !((double)dist[i] <= max_distance)) return;
        const float* xr = x + 3 * (size_t)i;
        const float* cr = closest + 3 * (size_t)i;
        if (!(finite3(xr) && finite3(cr))) return;
        const long long i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
        if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return;
        double v0[3], e1[3], e2[3], n[3], xd[3], a[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v0[k] = (double)verts[3 * i0 + k];
            e1[k] = (double)verts[3 * i1 + k] - v0[k];
            e2[k] = (double)verts[3 * i2 + k] - v0[k];
            xd[k] = (double)xr[k];
        }
        cross3r(e1, e2, n);
        const double n2 = dot3r(n, n);
        if (!(n2 > 0.0 && n2 <= DBL_MAX)) return;
        const double len = sqrt(n2);
#pragma unroll
        for (int k = 0; k < 3; ++k) a[3 + k] = n[k] / len;
        const double nn[3] = {a[3], a[4], a[5]}, d[3] = {xd[0] - (double)cr[0], xd[1] - (double)cr[1], xd[2] - (double)cr[2]};
        double m[3];
        cross3r(xd, nn, m);
        a[0] = m[0]; a[1] = m[1]; a[2] = m[2];
        const double r = dot3r(d, nn);
        int at = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int c = p; c < 6; ++c) acc[at++] += a[p] * a[c];
#pragma unroll
        for (int p = 0; p < 6; ++p) acc[21 + p] -= a[p] * r;
        acc[27] += r * r;
        acc[28] += 1.0;
    }
};

template <class Rows>
__global__ __launch_bounds__(256) void k_reg_partials(Rows rows, long long nchunk, double* __restrict__ part) {
    constexpr int K = Rows::K;
    __shared__ double lds[4][K];
    const int b = (int)(blockIdx.x / nchunk);
    const long long chunk = blockIdx.x % nchunk;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int j = 0; j < REG_PER_THREAD; ++j) {
        const long long i = chunk * REG_CHUNK + j * 256 + threadIdx.x;
        if (i < rows.N) rows.add(b, i, acc);
    }
    const double mine = block_sum<K>(acc, lds);
    if (threadIdx.x < K) part[(size_t)blockIdx.x * K + threadIdx.x] = mine;
}

template <int K>
__global__ __launch_bounds__(256) void k_reg_total(const double* __restrict__ part, long long nchunk, double* __restrict__ out) {
    __shared__ double lds[4][K];
    const long long per = (nchunk + 255) / 256, c0 = threadIdx.x * per, c1 = c0 + per < nchunk ? c0 + per : nchunk;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (long long c = c0; c < c1; ++c) {
        const double* row = part + ((size_t)blockIdx.x * (size_t)nchunk + (size_t)c) * K;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += row[k];
    }
    const double mine = block_sum<K>(acc, lds);
    if (threadIdx.x < K) out[(size_t)blockIdx.x * K + threadIdx.x] = mine;
}

template <class Rows>
inline int reduce_rows(const Rows& rows, int B, double* part, double* out, hipStream_t st, const char* what) {
    const long long nchunk = reg_chunks(rows.N);
    if (nchunk > 0) hipLaunchKernelGGL(k_reg_partials<Rows>, dim3((unsigned)(B * nchunk)), dim3(256), 0, st, rows, nchunk, part);
    hipLaunchKernelGGL(k_reg_total<Rows::K>, dim3((unsigned)B), dim3(256), 0, st, part, nchunk, out);
    return hip_last(what);
}

// registration.solve_moments: one row of moments -> R (row-major), t, the weight; false where the fit is not valid.
__device__ __forceinline__ bool solve_moments(const double* m, double (&R)[9], double (&t)[3], double& W) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    t[0] = t[1] = t[2] = 0.0;
    W = m[0];
    if (!(W > 0.0)) { W = 0.0; return false; }
    double pm[3], qm[3], S[9];
#pragma unroll
    for (int a = 0; a < 3; ++a) { pm[a] = m[1 + a] / W; qm[a] = m[4 + a] / W; }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) S[3 * a + c] = m[7 + 3 * a + c] - (m[1 + a] * m[4 + c]) / W;
    const bool valid = kabsch_rotation(S, REG_RANK_REL, R);
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = qm[a] - ((R[3 * a] * pm[0] + R[3 * a + 1] * pm[1]) + R[3 * a + 2] * pm[2]);
    return valid;
}

__global__ __launch_bounds__(64) void k_rigid_solve(const double* __restrict__ moments, int B, double* __restrict__ rotation,
                                                    double* __restrict__ translation, double* __restrict__ weight,
                                                    unsigned char* __restrict__ valid) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double R[9], t[3], W;
    const bool ok = solve_moments(moments + (size_t)b * REG_MOMENTS, R, t, W);
#pragma unroll
    for (int k = 0; k < 9; ++k) rotation[9 * (size_t)b + k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) translation[3 * (size_t)b + k] = t[k];
    if (weight) weight[b] = W;
    if (valid) valid[b] = ok ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_rigid_rmse(const double* __restrict__ moments, int B, double* __restrict__ rmse) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double W = moments[(size_t)b * REG_MOMENTS], s = moments[(size_t)b * REG_MOMENTS + 16];
    rmse[b] = W > 0.0 ? sqrt(s / W) : 0.0;
}

__global__ __launch_bounds__(256) void k_rigid_apply(const double* __restrict__ rotation, const double* __restrict__ translation,
                                                     const float* __restrict__ p, long long N, size_t n, long long p_stride,
                                                     float* __restrict__ out_points, const float* __restrict__ q,
                                                     float* __restrict__ out_residual, float* __restrict__ out_norm) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t b = i / (size_t)N, r = i % (size_t)N;
        const double* R = rotation + 9 * b;
        const double* t = translation + 3 * b;
        const float* pr = p + b * (size_t)p_stride + 3 * r;
        const double x[3] = {(double)pr[0], (double)pr[1], (double)pr[2]};
        double y[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) y[a] = ((R[3 * a] * x[0] + R[3 * a + 1] * x[1]) + R[3 * a + 2] * x[2]) + t[a];
        if (out_points) {
#pragma unroll
            for (int a = 0; a < 3; ++a) out_points[3 * i + a] = (float)y[a];
        }
        if (q) {
            const double d[3] = {(double)q[3 * i] - y[0], (double)q[3 * i + 1] - y[1], (double)q[3 * i + 2] - y[2]};
            if (out_residual) {
#pragma unroll
                for (int a = 0; a < 3; ++a) out_residual[3 * i + a] = (float)d[a];
            }
            if (out_norm) out_norm[i] = (float)sqrt(dot3r(d, d));
        }
    }
}

// registration.solve_normal_equations: Cholesky of the 6 x 6 with the pivot rule; false where the system is degenerate.
__device__ __forceinline__ bool solve_plane(const double* s, double (&z)[6]) {
    if (!(s[28] > 0.0)) return false;
    double A[6][6], L[6][6], y[6];
    int at = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int c = p; c < 6; ++c) { A[p][c] = s[at]; A[c][p] = s[at]; ++at; }
    double dmax = A[0][0];
#pragma unroll
    for (int p = 1; p < 6; ++p) dmax = fmax(dmax, A[p][p]);
    const double floor_ = REG_PIVOT_REL * dmax;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > floor_)) return false;
        L[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double e = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) e -= L[i][k] * L[j][k];
            L[i][j] = e / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double e = s[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) e -= L[i][k] * y[k];
        y[i] = e / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double e = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) e -= L[k][i] * z[k];
        z[i] = e / L[i][i];
    }
    return true;
}

// registration.rodrigues: I + a K + b K^2, a = sin(th) / th, b = (sin(th / 2) / (th / 2))^2 / 2.
__device__ __forceinline__ void rodrigues(const double (&w)[3], double th, double (&R)[9]) {
    const double half = 0.5 * th;
    const double a = th > 0.0 ? sin(th) / th : 1.0, sh = th > 0.0 ? sin(half) / half : 1.0, b = 0.5 * (sh * sh);
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
            R[3 * i + j] = ((i == j ? 1.0 : 0.0) + a * K[3 * i + j]) + b * kk;
        }
}

__global__ __launch_bounds__(64) void k_icp_update(const double* __restrict__ sums, int method, double tol, double* __restrict__ state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int* word = reinterpret_cast<int*>(state + 13);          // status, iterations, done
    if (word[2]) return;                                     // once done, nothing changes: any number of further launches
    double dR[9], dt[3], angle;
    bool ok;
    if (method == ICP_PLANE) {
        double z[6];
        ok = solve_plane(sums, z);
        if (ok) {
            const double w[3] = {z[0], z[1], z[2]};
            angle = sqrt(dot3r(w, w));
            rodrigues(w, angle, dR);
            dt[0] = z[3]; dt[1] = z[4]; dt[2] = z[5];
        }
    } else {
        double W;
        ok = solve_moments(sums, dR, dt, W);
        if (ok) {
            const double v[3] = {0.5 * (dR[7] - dR[5]), 0.5 * (dR[2] - dR[6]), 0.5 * (dR[3] - dR[1])};
            angle = atan2(sqrt(dot3r(v, v)), 0.5 * (((dR[0] + dR[4]) + dR[8]) - 1.0));
        }
    }
    if (!ok) {
        word[0] = ICP_DEGENERATE;
        word[2] = 1;
        return;
    }
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (dR[3 * i] * state[j] + dR[3 * i + 1] * state[3 + j]) + dR[3 * i + 2] * state[6 + j];
        t[i] = ((dR[3 * i] * state[9] + dR[3 * i + 1] * state[10]) + dR[3 * i + 2] * state[11]) + dt[i];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) state[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) state[9 + k] = t[k];
    const double step = fmax(angle, sqrt(dot3r(dt, dt)));
    state[12] = step;
    word[1] += 1;
    if (step < tol) {
        word[0] = ICP_CONVERGED;
        word[2] = 1;
    }
}

int reg_sizes(int B, long long N) {
    ES_REQUIRE(B >= 0 && N >= 0, "negative count (B, N)");
    ES_REQUIRE(N < REG_MAX_COUNT && (long long)B * N <= (REG_MAX_COUNT - 1) / 3, "2^31 coordinates or more in one call");
    ES_REQUIRE((long long)(B > 0 ? B : 1) * (reg_chunks(N) > 0 ? reg_chunks(N) : 1) < REG_MAX_COUNT, "2^31 workgroups or more in one call");
    return ST_OK;
}

}  // namespace

}  // namespace es

using namespace es;

#define REG_ALIGNED8(p, what) ES_REQUIRE(p && reinterpret_cast<uintptr_t>(p) % 8 == 0, what " must be an 8-byte aligned device buffer")

extern "C" {

int64_t es_rigid_scratch_bytes(int B, long long N) {
    if (reg_sizes(B, N) != ST_OK) return -1;
    const long long nchunk = reg_chunks(N);
    return up16(8ll * REG_PLANE * (B > 0 ? B : 1) * (nchunk > 0 ? nchunk : 1));
}

int es_rigid_moments(const float* p, const float* q, const float* w, int B, long long N, int w_per_batch, void* scratch, double* out,
                     void* stream) {
    if (const int s = reg_sizes(B, N)) return s;
    if (B == 0) return ST_OK;
    ES_REQUIRE((p && q) || N == 0, "es_rigid_moments: null buffer (p, q)");
    REG_ALIGNED8(scratch, "es_rigid_moments: scratch");
    REG_ALIGNED8(out, "es_rigid_moments: out");
    const MomentRows rows{p, q, w, N, w_per_batch != 0};
    return reduce_rows(rows, B, static_cast<double*>(scratch), out, static_cast<hipStream_t>(stream), "es_rigid_moments");
}

int es_rigid_solve(const double* moments, int B, double* rotation, double* translation, double* weight, unsigned char* valid, void* stream) {
    ES_REQUIRE(B >= 0, "es_rigid_solve: negative count (B)");
    if (B == 0) return ST_OK;
    ES_REQUIRE(moments && rotation && translation, "es_rigid_solve: null buffer (moments, rotation, translation)");
    hipLaunchKernelGGL(k_rigid_solve, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), moments, B, rotation,
                       translation, weight, valid);
    return hip_last("es_rigid_solve");
}

int es_rigid_rmse(const double* moments, int B, double* rmse, void* stream) {
    ES_REQUIRE(B >= 0, "es_rigid_rmse: negative count (B)");
    if (B == 0) return ST_OK;
    ES_REQUIRE(moments && rmse, "es_rigid_rmse: null buffer (moments, rmse)");
    hipLaunchKernelGGL(k_rigid_rmse, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), moments, B, rmse);
    return hip_last("es_rigid_rmse");
}

int es_rigid_apply(const double* rotation, const double* translation, const float* p, int B, long long N, long long p_batch_stride,
                   float* out_points, const float* q, float* out_residual, float* out_norm, void* stream) {
    if (const int s = reg_sizes(B, N)) return s;
    ES_REQUIRE(p_batch_stride == 0 || p_batch_stride == 3 * N, "es_rigid_apply: p_batch_stride must be 0 (one shared p) or 3 N");
    if (B == 0 || N == 0) return ST_OK;
    ES_REQUIRE(out_points || out_residual || out_norm, "es_rigid_apply: no output requested");
    ES_REQUIRE(q || !(out_residual || out_norm), "es_rigid_apply: residual and norm need q");
    ES_REQUIRE(rotation && translation && p, "es_rigid_apply: null buffer (rotation, translation, p)");
    ES_REQUIRE(reinterpret_cast<uintptr_t>(rotation) % 8 == 0 && reinterpret_cast<uintptr_t>(translation) % 8 == 0,
               "es_rigid_apply: rotation and translation must be 8-byte aligned");
    const size_t n = (size_t)B * (size_t)N;
    hipLaunchKernelGGL(k_rigid_apply, dim3(grid_for((long long)n)), dim3(256), 0, static_cast<hipStream_t>(stream), rotation, translation, p, N,
                       n, p_batch_stride, out_points, q, out_residual, out_norm);
    return hip_last("es_rigid_apply");
}

int es_icp_normal_equations(const float* x, const float* closest, const int* triangle, const float* dist, const float* vertices,
                            const int* triangles, long long V, long long T, long long N, double max_distance, void* scratch, double* out,
                            void* stream) {
    if (const int s = reg_sizes(1, N)) return s;
    ES_REQUIRE(V >= 0 && T >= 0, "es_icp_normal_equations: negative count (V, T)");
    ES_REQUIRE(V < REG_MAX_COUNT && T < REG_MAX_COUNT, "es_icp_normal_equations: 2^31 vertices or triangles or more");
    ES_REQUIRE(!std::isnan(max_distance), "es_icp_normal_equations: max_distance is NaN (negative means none)");
    ES_REQUIRE((x && closest && triangle && dist) || N == 0, "es_icp_normal_equations: null buffer (x, closest, triangle, dist)");
    ES_REQUIRE((vertices || V == 0) && (triangles || T == 0), "es_icp_normal_equations: null buffer (vertices, triangles)");
    REG_ALIGNED8(scratch, "es_icp_normal_equations: scratch");
    REG_ALIGNED8(out, "es_icp_normal_equations: out");
    const PlaneRows rows{x, closest, triangle, dist, vertices, triangles, V, T, N, max_distance};
    return reduce_rows(rows, 1, static_cast<double*>(scratch), out, static_cast<hipStream_t>(stream), "es_icp_normal_equations");
}

int es_icp_update(const double* sums, int method, double tol, double* state, void* stream) {
    ES_REQUIRE(method == ICP_POINT || method == ICP_PLANE, "es_icp_update: unknown method (0 = point, 1 = plane)");
    ES_REQUIRE(!std::isnan(tol), "es_icp_update: tol is NaN");
    ES_REQUIRE(sums, "es_icp_update: null buffer (sums)");
    REG_ALIGNED8(state, "es_icp_update: state");
    static_assert(ICP_STATE_DOUBLES * 8 >= 13 * 8 + 4 * 4, "the state record holds its three words");
    hipLaunchKernelGGL(k_icp_update, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), sums, method, tol, state);
    return hip_last("es_icp_update");
}

}  // extern "C"
