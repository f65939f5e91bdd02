// Geodesic distance on triangle meshes (endosurf_amd/geodesic.py is the specification and the fp64 host twin): a
// first-order eikonal solver, the triangle update of Kimmel and Sethian with an edge fallback, as double-buffered Jacobi sweeps.
// One thread per (triangle, field); a field b < B = F S reads frame b / S of the vertices.  The fields are fp64 values kept as their
// unsigned 64-bit patterns: non-negative doubles (and +inf) order as unsigned integers, so atomicMin on unsigned long long is the
// minimum, which is exact and commutative: the same bits from call to call, whatever the order the threads arrive in.  No float
// atomics, no LDS.
//
// Rounding.  The library is built with -ffp-contract=fast, which would fuse the twin's products into its sums (nn_grid.h tells why
// the pragma does not help).  Every product of corner_geometry, corner_value and the read-out's straight distance goes through mul(), whose
// empty asm statement makes it a value the optimiser cannot look through: each line below rounds where geodesic.corner_update's
// docstring says.  Sums, quotients and square roots are single IEEE operations.  The device still does not promise the twin's fp64
// bits (its sqrt is the device's); it promises them to one fp32 ulp after rounding.
#include <cfloat>

#include "host.h"
#include "launch.h"

namespace es {

namespace {

typedef unsigned long long u64;
constexpr u64 GEO_INF = 0x7FF0000000000000ull;          // +inf
constexpr double GEO_DET_REL = 0x1p-40;                 // geodesic.DET_REL
constexpr int GEO_MAX_Y = 32768;                        // grid.y; a kernel strides over what is beyond

__device__ __forceinline__ double mul(double a, double b) {
    double p = a * b;
    asm("" : "+v"(p));
    return p;
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (mul(a[0], b[0]) + mul(a[1], b[1])) + mul(a[2], b[2]); }
__device__ __forceinline__ double as_f64(u64 x) { return __longlong_as_double((long long)x); }
__device__ __forceinline__ u64 as_u64(double x) { return (u64)__double_as_longlong(x); }
__device__ __forceinline__ bool below_inf(double x) { return x <= DBL_MAX; }          // finite and not NaN, for x >= 0

// What corner_update needs of a corner and does not depend on the values (geodesic.corner_geometry).
struct Corner {
    double l1, l2, q11, q12, q22;
    bool ok;
};

__device__ __forceinline__ Corner corner_geometry(const double* c, const double* a, const double* b) {
    const double e1[3] = {a[0] - c[0], a[1] - c[1], a[2] - c[2]}, e2[3] = {b[0] - c[0], b[1] - c[1], b[2] - c[2]};
    const double g11 = dot3(e1, e1), g12 = dot3(e1, e2), g22 = dot3(e2, e2);
    const double det = mul(g11, g22) - mul(g12, g12);
    Corner g;
    g.l1 = sqrt(g11);
    g.l2 = sqrt(g22);
    g.ok = det > mul(mul(GEO_DET_REL, g11), g22);
    g.q11 = g.ok ? g22 / det : 0.0;
    g.q12 = g.ok ? -g12 / det : 0.0;
    g.q22 = g.ok ? g11 / det : 0.0;
    return g;
}

// geodesic.corner_update, line by line.
__device__ __forceinline__ double corner_value(const Corner& g, double ua, double ub) {
    const double edge = fmin(ua + g.l1, ub + g.l2);
    if (!(g.ok && below_inf(ua) && below_inf(ub))) return edge;
    const double r1 = g.q11 + g.q12, r2 = g.q12 + g.q22, A = r1 + r2;
    const double B = mul(r1, ua) + mul(r2, ub);
    const double s1 = mul(g.q11, ua) + mul(g.q12, ub), s2 = mul(g.q12, ua) + mul(g.q22, ub);
    const double C = (mul(ua, s1) + mul(ub, s2)) - 1.0;
    const double disc = mul(B, B) - mul(A, C);
    if (!(disc >= 0.0)) return edge;
    double t = (B + sqrt(disc)) / A;
    const double da = ua - t, db = ub - t;
    const double w1 = mul(g.q11, da) + mul(g.q12, db), w2 = mul(g.q12, da) + mul(g.q22, db);
    if (!(w1 <= 0.0 && w2 <= 0.0)) return edge;
    t = fmax(fmax(t, ua), ub);
    return fmin(t, edge);
}

// The triangle's indices if they are distinct and in [0, V) (nothing else is ever dereferenced with them).
__device__ __forceinline__ bool load_indices(const int* __restrict__ tris, long long t, long long V, int* idx) {
    idx[0] = tris[3 * t];
    idx[1] = tris[3 * t + 1];
    idx[2] = tris[3 * t + 2];
    const bool in = idx[0] >= 0 && idx[0] < V && idx[1] >= 0 && idx[1] < V && idx[2] >= 0 && idx[2] < V;
    return in && idx[0] != idx[1] && idx[1] != idx[2] && idx[0] != idx[2];
}
// Its corners in the frame ``vf`` [V,3]; false if one is not finite.
__device__ __forceinline__ bool load_corners(const float* __restrict__ vf, const int* idx, double p[3][3]) {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float x = vf[3 * (size_t)idx[k] + d];
            finite = finite && fabsf(x) <= FLT_MAX;
            p[k][d] = (double)x;
        }
    return finite;
}

__global__ __launch_bounds__(256) void k_geodesic_fill(u64* __restrict__ a, u64* __restrict__ b, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        a[i] = GEO_INF;
        b[i] = GEO_INF;
    }
}

// One thread per (triangle, seed): a seed takes effect iff its vertex is a corner of a triangle that is valid in its field's frame.
__global__ __launch_bounds__(256) void k_geodesic_seed(const float* __restrict__ vertices, const int* __restrict__ tris, long long V, long long T,
                                                       int S, int B, const int* __restrict__ seed_field, const int* __restrict__ seed_vertex,
                                                       const double* __restrict__ seed_value, long long n_seeds, u64* __restrict__ cur,
                                                       u64* __restrict__ next) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int idx[3];
    if (!load_indices(tris, t, V, idx)) return;
    for (long long j = blockIdx.y; j < n_seeds; j += gridDim.y) {
        const int b = seed_field[j], vtx = seed_vertex[j];
        const double val = seed_value[j];
        if (b < 0 || b >= B || !(val >= 0.0 && below_inf(val))) continue;
        if (vtx != idx[0] && vtx != idx[1] && vtx != idx[2]) continue;
        double p[3][3];
        if (!load_corners(vertices + 3 * (size_t)(b / S) * (size_t)V, idx, p)) continue;
        const size_t at = (size_t)b * (size_t)V + (size_t)vtx;
        atomicMin(cur + at, as_u64(fabs(val)));          // (fabs: -0.0 would not order as an unsigned integer)
        atomicMin(next + at, as_u64(fabs(val)));
    }
}

// One sweep: next[c] = min(next[c], cur[c], the corner updates of this triangle computed from cur).  ``next`` holds the field of the
// sweep before ``cur``, which is nowhere below cur (values only fall), so after the launch next = min(cur, every update): the two
// buffers change places without a copy.  The plain read of next[c] only saves atomics: what it sees was stored at some time, so it is
// never below the final value.
__global__ __launch_bounds__(256) void k_geodesic_sweep(const float* __restrict__ vertices, const int* __restrict__ tris, long long V,
                                                        long long T, int S, int B, const u64* __restrict__ cur, u64* next, int* changed) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int idx[3];
    if (!load_indices(tris, t, V, idx)) return;
    bool lowered = false;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const size_t row = (size_t)b * (size_t)V;
        const double u[3] = {as_f64(cur[row + idx[0]]), as_f64(cur[row + idx[1]]), as_f64(cur[row + idx[2]])};
        if (!below_inf(u[0]) && !below_inf(u[1]) && !below_inf(u[2])) continue;          // the front has not arrived
        double p[3][3];
        if (!load_corners(vertices + 3 * (size_t)(b / S) * (size_t)V, idx, p)) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int ia = (k + 1) % 3, ib = (k + 2) % 3;
            if (!below_inf(u[ia]) && !below_inf(u[ib])) continue;
            const double cand = corner_value(corner_geometry(p[k], p[ia], p[ib]), u[ia], u[ib]);
            lowered = lowered || cand < u[k];
            const double m = fmin(cand, u[k]);
            u64* dst = next + row + idx[k];
            if (m < as_f64(*dst)) atomicMin(dst, as_u64(m));
        }
    }
    if (lowered && changed) *changed = 1;
}

// One thread per (field, target): geodesic.mesh_geodesic's read-out.
__global__ __launch_bounds__(256) void k_geodesic_read(const u64* __restrict__ field, const float* __restrict__ vertices,
                                                       const int* __restrict__ tris, long long V, long long T, int S, long long Q, size_t n,
                                                       const int* __restrict__ target_tri, const double* __restrict__ target_pt,
                                                       const int* __restrict__ source_tri, const double* __restrict__ source_pt,
                                                       float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t b = i / (size_t)Q, q = i % (size_t)Q, f = b / (size_t)S, s = b % (size_t)S;
        const long long t = target_tri[q];
        double best = as_f64(GEO_INF);
        int idx[3];
        double p[3][3];
        const double* x = target_pt + 3 * (f * (size_t)Q + q);
        const bool finite = fabs(x[0]) <= DBL_MAX && fabs(x[1]) <= DBL_MAX && fabs(x[2]) <= DBL_MAX;
        if (t >= 0 && t < T && finite && load_indices(tris, t, V, idx) && load_corners(vertices + 3 * f * (size_t)V, idx, p)) {
            const size_t row = b * (size_t)V;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int ia = k, ib = (k + 1) % 3;
                const Corner g = corner_geometry(x, p[ia], p[ib]);
                best = fmin(best, corner_value(g, as_f64(field[row + idx[ia]]), as_f64(field[row + idx[ib]])));
            }
            if (source_tri && source_pt && source_tri[s] == t) {
                const double* y = source_pt + 3 * (f * (size_t)S + s);
                const double d[3] = {y[0] - x[0], y[1] - x[1], y[2] - x[2]};
                const double straight = sqrt(dot3(d, d));
                if (below_inf(straight)) best = fmin(best, straight);
            }
        }
        out[i] = (float)best;
    }
}

__global__ __launch_bounds__(256) void k_geodesic_finish(const u64* __restrict__ field, size_t n, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (float)as_f64(field[i]);
}

inline dim3 tri_grid(long long T, long long ny) { return dim3((unsigned)((T - 1) / 256 + 1), (unsigned)(ny < GEO_MAX_Y ? ny : GEO_MAX_Y)); }

}  // namespace

int geodesic_seed(const float* vertices, const int* tris, int F, long long V, long long T, int S, const int* seed_field,
                  const int* seed_vertex, const double* seed_value, long long n_seeds, unsigned long long* cur, unsigned long long* next,
                  hipStream_t st) {
    const size_t n = (size_t)F * (size_t)S * (size_t)V;
    if (n == 0) return ST_OK;
    hipLaunchKernelGGL(k_geodesic_fill, dim3(grid_for((long long)n)), dim3(256), 0, st, cur, next, n);
    if (T > 0 && n_seeds > 0)
        hipLaunchKernelGGL(k_geodesic_seed, tri_grid(T, n_seeds), dim3(256), 0, st, vertices, tris, V, T, S, F * S, seed_field, seed_vertex,
                           seed_value, n_seeds, cur, next);
    return hip_last("geodesic_seed");
}

int geodesic_sweep(const float* vertices, const int* tris, int F, long long V, long long T, int S, const unsigned long long* cur,
                   unsigned long long* next, int* changed, hipStream_t st) {
    if (changed) ES_HIP(hipMemsetAsync(changed, 0, sizeof(int), st));
    if (F == 0 || V == 0 || T == 0) return ST_OK;
    hipLaunchKernelGGL(k_geodesic_sweep, tri_grid(T, (long long)F * S), dim3(256), 0, st, vertices, tris, V, T, S, F * S, cur, next, changed);
    return hip_last("geodesic_sweep");
}

int geodesic_read(const unsigned long long* field, const float* vertices, const int* tris, int F, long long V, long long T, int S,
                  const int* target_tri, const double* target_pt, long long Q, const int* source_tri, const double* source_pt, float* out,
                  hipStream_t st) {
    const size_t n = (size_t)F * (size_t)S * (size_t)Q;
    if (n == 0) return ST_OK;
    hipLaunchKernelGGL(k_geodesic_read, dim3(grid_for((long long)n)), dim3(256), 0, st, field, vertices, tris, V, T, S, Q, n, target_tri,
                       target_pt, source_tri, source_pt, out);
    return hip_last("geodesic_read");
}

int geodesic_finish(const unsigned long long* field, long long n, float* out, hipStream_t st) {
    if (n == 0) return ST_OK;
    hipLaunchKernelGGL(k_geodesic_finish, dim3(grid_for(n)), dim3(256), 0, st, field, (size_t)n, out);
    return hip_last("geodesic_finish");
}

}  // namespace es
