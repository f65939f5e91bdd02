// Exact distance from a point to a triangle mesh on the device (additive to ABI v14).  Numpy twin and specification:
// endosurf_amd/meshing.py point_to_mesh.  Contract: DESIGN.md 7f.
//
//   k_surf_prepare       one thread per triangle: its centroid (fp64 mean of the corners, rounded to fp32; NaN for a triangle that takes
//                        no part), its radius (fp64: the largest distance from the ROUNDED centroid to a corner, rounded up to fp32) and
//                        the largest radius R of the mesh, one integer atomicMax per wave on the bits of the non-negative float
//   es_nn_build          (csrc/mesh.hip) the uniform grid of the nearest-neighbour search over the centroids; a NaN centroid is in no cell
//   k_surf_query         one thread per query: Chebyshev shells of cells around the query's (clamped) cell as in k_nn_query; every record
//                        names a triangle, which is loaded by its index and measured in fp64 by the rule below
//
// The rule (all of it in fp64 on the fp32 inputs).  A triangle takes part iff its indices are distinct and in [0, V) and its corners
// finite.  Edge (i, j): oriented from the smaller index a to the larger b, l2 = |b - a|^2, t = l2 > 0 ? (q - a).(b - a) / l2 : 0,
// c = a (t <= 0), b (t >= 1), else a + t (b - a); d2 = |q - c|^2: two triangles that share an edge evaluate the same expression on the
// same operands (the edge loop below is not unrolled, so it is the same instructions too).  Face: n = (v1 - v0) x (v2 - v0), only if
// n.n > 0: p = q - ((q - v0).n / n.n) n counts iff ((vb - va) x (p - va)).n > 0 for the three sides; d2 = |q - p|^2.  Per triangle the
// smallest d2, the face first, then v0v1, v1v2, v2v0; per query the smallest (d2, triangle index).
//
// Stop rule.  As in k_nn_query, after shells 0 .. r a centroid c not yet seen has |c - q|^2 >= (r h)^2 + |q - q'|^2 (q' = q clamped into
// the box of the centroids, h = h_safe), and every point x of its triangle has |x - c| <= R, so |x - q| >= sqrt((r h)^2 + |q - q'|^2) - R.
// The walk stops once best < D^2 with D = sqrt((r h)^2 + |q - q'|^2) (1 - 2^-16) - R (1 + 2^-16) > 0: the two factors cover the fp32
// cell function's slack (already in h_safe), the rounding of R and of this fp64 evaluation many times over, and the comparison is
// strict, so an unseen triangle cannot win, not even a tie.  r never exceeds the largest grid dimension - 1.
// Cull.  A record carries its triangle's (rounded) centroid c, the point R was measured from, so the triangle is no nearer than
// |c - q| - R: once |c - q|^2 > (sqrt(best) + R)^2 (1 + 2^-15) it is skipped before its corners are loaded.  The comparison is strict and
// padded, so a triangle that could win or tie is always measured; a NaN on either side measures it too.
// Known limit: one huge triangle makes R large, and every query then reads most of the grid: correct, bounded by T, slow.
//
// One kind of atomic, the integer maximum on R's bits (and the integer atomics of es_nn_build, whose order only permutes the records
// of a cell, which the (d2, index) minimum does not see): two calls give the same bits.  No workgroup waits for another; every device
// loop is bounded by an argument or by the grid's dimensions; a record's triangle index and a triangle's vertex indices are checked
// against T and V before they address memory, whatever the scratch holds.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"
#include "nn_grid.h"

namespace es {

struct SurfScratch {
    unsigned* rbits;         // [4] the bits of R, the largest triangle radius (fp32 >= 0); 3 words unused
    float* cent;             // [T][3] triangle centroids, NaN for a triangle that takes no part
    void* nn;                // es_nn_scratch_bytes(T): the grid over the centroids
    long long bytes;
};
static SurfScratch surf_layout(const void* scratch, long long T) {          // a null scratch measures only
    Carver c(scratch);
    SurfScratch s;
    s.rbits = c.take<unsigned>(4);
    s.cent = c.take<float>(3 * T);
    s.nn = c.take<char>(nn_layout(nullptr, T).bytes);
    s.bytes = c.off;
    return s;
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 sub(const D3& a, const D3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(const D3& a, const D3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross(const D3& a, const D3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// the corners of triangle t if it takes part; no vertex is read before its index is known to lie in [0, V)
__device__ __forceinline__ bool surf_tri_load(const float* __restrict__ verts, const int* __restrict__ tris, long long t, int V, int& i0, int& i1,
                                              int& i2, D3& v0, D3& v1, D3& v2) {
    i0 = tris[3 * t]; i1 = tris[3 * t + 1]; i2 = tris[3 * t + 2];
    if (!(in_range(i0, V) && in_range(i1, V) && in_range(i2, V) && i0 != i1 && i1 != i2 && i0 != i2)) return false;
    const float* a = verts + 3 * (size_t)i0;
    const float* b = verts + 3 * (size_t)i1;
    const float* c = verts + 3 * (size_t)i2;
    const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
    if (!(finite3(ax, ay, az) && finite3(bx, by, bz) && finite3(cx, cy, cz))) return false;
    v0 = {(double)ax, (double)ay, (double)az};
    v1 = {(double)bx, (double)by, (double)bz};
    v2 = {(double)cx, (double)cy, (double)cz};
    return true;
}

__global__ __launch_bounds__(256) void k_surf_prepare(const float* __restrict__ verts, const int* __restrict__ tris, int V, long long T,
                                                      float* __restrict__ cent, unsigned* rbits) {
    const int lane = threadIdx.x & 63;
    float rmax = 0.f;
    for (long long base = blockIdx.x * 256ll; base < T; base += gridDim.x * 256ll) {          // (wave-uniform trip count)
        const long long t = base + threadIdx.x;
        if (t >= T) continue;
        int i0, i1, i2;
        D3 v0, v1, v2;
        float cx = NAN, cy = NAN, cz = NAN;
        if (surf_tri_load(verts, tris, t, V, i0, i1, i2, v0, v1, v2)) {
            cx = (float)(((v0.x + v1.x) + v2.x) / 3.0);          // (|mean| <= the largest |corner|: finite in fp32)
            cy = (float)(((v0.y + v1.y) + v2.y) / 3.0);
            cz = (float)(((v0.z + v1.z) + v2.z) / 3.0);
            const D3 c = {(double)cx, (double)cy, (double)cz};
            const D3 e0 = sub(v0, c), e1 = sub(v1, c), e2 = sub(v2, c);
            const double r = sqrt(fmax(fmax(dot(e0, e0), dot(e1, e1)), dot(e2, e2)));
            float rf = (float)r;
            if ((double)rf < r) rf = __uint_as_float(__float_as_uint(rf) + 1u);          // rounded up (inf stays: it is not < r)
            rmax = fmaxf(rmax, rf);
        }
        cent[3 * t] = cx; cent[3 * t + 1] = cy; cent[3 * t + 2] = cz;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, o, 64));
    if (lane == 0 && rmax > 0.f) atomicMax(rbits, __float_as_uint(rmax));          // (the bits of floats >= 0 order like the floats)
}

// one oriented edge: the closest point c of segment (a, b) to q and its squared distance
__device__ __forceinline__ void surf_edge(const D3& q, D3 a, D3 b, int ia, int ib, double& d2, D3& c) {
    if (ia > ib) { const D3 s = a; a = b; b = s; }
    const D3 e = sub(b, a);
    const double l2 = dot(e, e);
    const double t = l2 > 0.0 ? dot(sub(q, a), e) / l2 : 0.0;
    if (t <= 0.0) c = a;
    else if (t >= 1.0) c = b;
    else c = {a.x + t * e.x, a.y + t * e.y, a.z + t * e.z};
    const D3 d = sub(q, c);
    d2 = dot(d, d);
}

// the triangles of the records of cells [c0, c1] of one (x, y) column (contiguous: z fastest), each measured by the rule above
__device__ __forceinline__ void surf_scan_run(const float4* __restrict__ rec, const int* __restrict__ start, const float* __restrict__ verts,
                                              const int* __restrict__ tris, int V, long long T, int c0, int c1, const D3& q, double R, double& best,
                                              double& reach2, int& arg, D3& at, int& n_eval) {
    long long s = start[c0], e = start[c1 + 1];
    s = s < 0 ? 0 : s;
    e = e > T ? T : e;
    for (long long i = s; i < e; ++i) {
        const float4 rc = rec[i];
        const int t = __float_as_int(rc.w);
        if (!in_range(t, (int)T)) continue;
        const D3 dc = sub(q, D3{(double)rc.x, (double)rc.y, (double)rc.z});
        if (dot(dc, dc) > reach2) continue;          // farther than sqrt(best) + R from the centroid: it cannot win, nor tie
        int i0, i1, i2;
        D3 v0, v1, v2;
        if (!surf_tri_load(verts, tris, t, V, i0, i1, i2, v0, v1, v2)) continue;
        ++n_eval;
        double tb = INFINITY;
        D3 tc = q;
        const D3 n = cross(sub(v1, v0), sub(v2, v0));
        const double n2 = dot(n, n);
        if (n2 > 0.0) {
            const double sc = dot(sub(q, v0), n) / n2;
            const D3 p = {q.x - sc * n.x, q.y - sc * n.y, q.z - sc * n.z};
            const double s0 = dot(cross(sub(v1, v0), sub(p, v0)), n);
            const double s1 = dot(cross(sub(v2, v1), sub(p, v1)), n);
            const double s2 = dot(cross(sub(v0, v2), sub(p, v2)), n);
            if (s0 > 0.0 && s1 > 0.0 && s2 > 0.0) {
                const D3 d = sub(q, p);
                tb = dot(d, d);
                tc = p;
            }
        }
        // v0v1, v1v2, v2v0: one body, the corners rotated, so that every edge of every triangle runs the same instructions
#pragma unroll 1
        for (int k = 0; k < 3; ++k) {
            double d2;
            D3 c;
            surf_edge(q, v0, v1, i0, i1, d2, c);
            if (d2 < tb) { tb = d2; tc = c; }
            const D3 vs = v0;
            const int is = i0;
            v0 = v1; v1 = v2; v2 = vs;
            i0 = i1; i1 = i2; i2 = is;
        }
        if (tb < best || (tb == best && t < arg)) {
            best = tb; arg = t; at = tc;
            const double reach = sqrt(tb) + R;
            reach2 = reach * reach * (1.0 + 1.0 / 32768.0);          // (inf for R = inf: nothing is culled)
        }
    }
}

__global__ __launch_bounds__(256) void k_surf_query(const float* __restrict__ query, long long Q, const float* __restrict__ verts,
                                                    const int* __restrict__ tris, int V, long long T, const NnHeader* __restrict__ head,
                                                    const int* __restrict__ start, const float4* __restrict__ rec,
                                                    const unsigned* __restrict__ rbits, float* __restrict__ dist, int* __restrict__ triangle,
                                                    float* __restrict__ closest, int* __restrict__ work) {
    const NnHeader h = *head;
    const bool ok = nn_head_ok(h, T) && h.n_finite > 0;
    const int nx = h.n[0], ny = h.n[1], nz = h.n[2];
    const unsigned rb = rbits[0];
    const double R = rb <= 0x7f800000u ? (double)__uint_as_float(rb) : (double)INFINITY;          // (bits no build wrote: never stop early)
    const double hs = h.h_safe > 0.f ? (double)h.h_safe : 0.0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < Q; i += gridDim.x * 256ll) {
        const float qx = query[3 * i], qy = query[3 * i + 1], qz = query[3 * i + 2];
        double best = INFINITY, reach2 = INFINITY;
        int arg = -1, n_shell = 0, n_eval = 0;
        D3 at = {0.0, 0.0, 0.0};
        if (ok && finite3(qx, qy, qz)) {
            const D3 q = {(double)qx, (double)qy, (double)qz};
            const float cx_ = fminf(fmaxf(qx, h.lo[0]), h.hi[0]), cy_ = fminf(fmaxf(qy, h.lo[1]), h.hi[1]), cz_ = fminf(fmaxf(qz, h.lo[2]), h.hi[2]);
            const double ox = q.x - (double)cx_, oy = q.y - (double)cy_, oz = q.z - (double)cz_;
            const double out2 = (ox * ox + oy * oy) + oz * oz;
            const int cx = nn_cell1(cx_, h.lo[0], h.inv_h[0], nx), cy = nn_cell1(cy_, h.lo[1], h.inv_h[1], ny), cz = nn_cell1(cz_, h.lo[2], h.inv_h[2], nz);
            const int rmax = max(max(max(cx, nx - 1 - cx), max(cy, ny - 1 - cy)), max(cz, nz - 1 - cz));
            for (int r = 0; r <= rmax; ++r) {
                const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
                const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
                for (int x = x0; x <= x1; ++x) {
                    const bool xface = x == cx - r || x == cx + r;
                    for (int y = y0; y <= y1; ++y) {
                        const int col = (x * ny + y) * nz;
                        if (xface || y == cy - r || y == cy + r) {
                            surf_scan_run(rec, start, verts, tris, V, T, col + z0, col + z1, q, R, best, reach2, arg, at, n_eval);
                        } else {
                            if (cz - r >= 0) surf_scan_run(rec, start, verts, tris, V, T, col + cz - r, col + cz - r, q, R, best, reach2, arg, at, n_eval);
                            if (cz + r < nz && r > 0) surf_scan_run(rec, start, verts, tris, V, T, col + cz + r, col + cz + r, q, R, best, reach2, arg, at, n_eval);
                        }
                    }
                }
                ++n_shell;
                const double reach = (double)r * hs;
                const double D = sqrt(reach * reach + out2) * (1.0 - 1.0 / 65536.0) - R * (1.0 + 1.0 / 65536.0);
                if (D > 0.0 && best < D * D) break;
            }
        }
        const bool hit = arg >= 0;
        dist[i] = hit ? (float)sqrt(best) : INFINITY;
        triangle[i] = arg;
        closest[3 * i] = hit ? (float)at.x : NAN;
        closest[3 * i + 1] = hit ? (float)at.y : NAN;
        closest[3 * i + 2] = hit ? (float)at.z : NAN;
        if (work) { work[2 * i] = n_shell; work[2 * i + 1] = n_eval; }
    }
}

static int surf_check(long long V, long long T, long long Q) {
    ES_REQUIRE(V >= 0 && T >= 0 && Q >= 0, "surface: negative vertex, triangle or query count");
    ES_REQUIRE(V < MESH_MAX && T < MESH_MAX && Q < MESH_MAX, "surface: 2^31 vertices, triangles or queries or more (indices are int32)");
    return ST_OK;
}

}  // namespace es

using namespace es;

extern "C" {

int64_t es_surf_scratch_bytes(long long n_verts, long long n_tris) {
    if (surf_check(n_verts, n_tris, 0) != ST_OK) return -1;
    return surf_layout(nullptr, n_tris).bytes;
}

int es_surf_build(const float* verts, const int* tris, long long V, long long T, void* scratch, void* stream) {
    if (const int s = surf_check(V, T, 0)) return s;
    ES_REQUIRE((verts || V == 0) && (tris || T == 0), "es_surf_build needs verts and tris");
    ES_SCRATCH_OK(scratch, "surface scratch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SurfScratch s = surf_layout(scratch, T);
    ES_HIP(hipMemsetAsync(s.rbits, 0, 4 * sizeof(unsigned), st));
    if (T > 0) hipLaunchKernelGGL(k_surf_prepare, dim3(grid_for(T)), dim3(256), 0, st, verts, tris, (int)V, T, s.cent, s.rbits);
    if (const int e = hip_last("es_surf_build")) return e;
    return es_nn_build(s.cent, T, s.nn, stream);
}

int es_surf_query(const float* query, long long Q, const float* verts, const int* tris, long long V, long long T, const void* scratch, float* dist,
                  int* triangle, float* closest, int* work, void* stream) {
    if (const int s = surf_check(V, T, Q)) return s;
    if (Q == 0) return ST_OK;
    ES_REQUIRE(query && dist && triangle && closest, "es_surf_query needs query, dist, triangle and closest");
    ES_REQUIRE((verts || V == 0) && (tris || T == 0), "es_surf_query needs verts and tris");
    ES_SCRATCH_OK(scratch, "surface scratch");
    const SurfScratch s = surf_layout(scratch, T);
    const NnScratch g = nn_layout(s.nn, T);
    hipLaunchKernelGGL(k_surf_query, dim3(grid_for(Q)), dim3(256), 0, static_cast<hipStream_t>(stream), query, Q, verts, tris, (int)V, T, g.head,
                       g.start, g.rec, s.rbits, dist, triangle, closest, work);
    return hip_last("es_surf_query");
}

}  // extern "C"
