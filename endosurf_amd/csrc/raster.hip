// Mesh rasteriser (ABI v12): an indexed triangle mesh as depth / triangle-id / barycentric / interpolated-attribute images of a pinhole
// camera -- what the reference's demo gets from Open3D's Visualizer (vis_mesh: the "Mesh / Texture / Normal" panels), which needs an
// OpenGL window a compute node does not have.  Numpy twins: endosurf_amd/meshing.py project_vertices / rasterize_projected, which are
// the specification.  Contract: DESIGN.md 7c.
//
//   k_rast_project      one thread per vertex: x_cam = R^T (x - t), (u, v) through the intrinsics in fp64 -> xy = rint(256 (u, v)) clamped
//                       to +-2^22 (1/256-pixel fixed point, snapped per VERTEX: triangles that share a vertex share its position, so the
//                       raster is watertight), zc = camera z (NaN for a non-finite vertex)
//   k_rast_setup        one thread per triangle: the rejection tests, the pixel box clamped to the image -> count[t] = the number of
//                       8 x 8-pixel tiles the box touches, or -reason for a rejected triangle
//   k_rast_blocksum / k_rast_scan_blocks / k_rast_offsets
//                       the three-launch exclusive scan of scan.h over count -> offset[t], totals = {work items, rejected by reason}.
//                       Kernels of raster's own: one sequence is scanned, the five reasons are only summed in the same launches
//   k_rast_fill         one thread per work item (its triangle by binary search in offset): the at most 64 pixel centres of box and
//                       tile; coverage by three int64 edge functions with a top-left rule for the value 0; depth from fp64
//                       barycentrics of the exact integers; one atomicMin of (bits of float32(z) << 32 | t) on zbuf[i W + j]
//   k_rast_resolve      one thread per pixel: decodes the key, recomputes the weights of the winner with the function k_rast_fill
//                       used, writes depth (from the key), triangle, bary, attributes; per-workgroup covered-pixel counts
//   k_rast_covered      one workgroup: their sum -> totals[6]
//
// Atomics: one kind, the 64-bit integer atomicMin on a pixel's key (a native global_atomic_umin_x2, no compare-and-swap loop).  The
// minimum of a set of keys does not depend on the order in which they arrive, and a key names depth and triangle together (equal depths
// go to the smaller index), so two calls give bit-identical images and a shuffled triangle list the same picture.  The plain read in
// front of the atomic only skips keys that cannot win: a key in zbuf never grows, so a stale value is an upper bound.  No float atomics.
// No workgroup waits for another one and nothing spins on a flag.  Every device loop is bounded by an argument or by 64 (the binary
// search by 32).  Every index read from a buffer (a triangle's corners, offset[], the triangle of a key) is range-checked before it
// addresses memory and every pixel comes out of a box clamped to the image: an uninitialised scratch gives a wrong image, not a fault.
// The depth arithmetic has no multiply that feeds an add, so the contraction the library is compiled with has nothing to fuse there.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"
#include "scan.h"

namespace es {

constexpr int RAST_SUB = 256;                                // fixed-point units per pixel
constexpr int RAST_GUARD = 1 << 22;                          // |fixed-point coordinate| <= this
constexpr int RAST_MAX_SIZE = 8192;                          // largest image side
constexpr int RAST_MAX_ATTRS = 8;
constexpr long long RAST_MAX_COUNT = 1ll << 31;              // int32 indices
constexpr unsigned long long RAST_EMPTY = ~0ull;             // the key of a pixel nothing covers
constexpr int RAST_TOTALS = 8;                               // work items, invalid, near, zero area, culled, off screen, covered pixels, 0
enum { RAST_INVALID = 1, RAST_NEAR = 2, RAST_AREA = 3, RAST_CULLED = 4, RAST_OFFSCREEN = 5 };

struct RastCamera {
    double R[9];                     // rotation of the camera-to-world pose, row-major
    double t[3];
    double k00, k01, k02, k11, k12;
};
struct RastView {
    int V, T, H, W, cull;
    double near;
};
struct RastScratch {
    unsigned long long* zbuf;        // [H W] keys
    int* count;                      // [T] tiles of the triangle's box, or -reason
    int* offset;                     // [T] exclusive scan of max(count, 0)
    long long* bsum;                 // [nchunk][6] work items and the five reasons per chunk
    long long* boff;                 // [nchunk] exclusive scan of the work items
    int* cov;                        // [ncov] covered pixels per workgroup of k_rast_resolve
    int nchunk, ncov;
    long long bytes;
};
static RastScratch rast_layout(const void* scratch, long long T, int H, int W) {          // a null scratch measures only
    Carver c(scratch);
    RastScratch s;
    s.nchunk = (int)scan_chunks(T);
    s.ncov = (int)(((long long)H * W + 255) / 256);
    s.zbuf = c.take<unsigned long long>((long long)H * W);
    s.count = c.take<int>(T);
    s.offset = c.take<int>(T);
    s.bsum = c.take<long long>(6ll * s.nchunk);
    s.boff = c.take<long long>(s.nchunk);
    s.cov = c.take<int>(s.ncov);
    s.bytes = c.off;
    return s;
}

__device__ __forceinline__ int rast_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int rast_max(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int rast_snap(double u) {
    double q = u * (double)RAST_SUB;
    if (q != q) q = 0.0;
    q = fmin(fmax(q, -(double)RAST_GUARD), (double)RAST_GUARD);
    return (int)rint(q);
}

__global__ __launch_bounds__(256) void k_rast_project(const float* __restrict__ verts, int V, RastCamera c, int* __restrict__ xy,
                                                      float* __restrict__ zc) {
    for (int v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256) {
        const float fx = verts[3 * (size_t)v], fy = verts[3 * (size_t)v + 1], fz = verts[3 * (size_t)v + 2];
        const double dx = (double)fx - c.t[0], dy = (double)fy - c.t[1], dz = (double)fz - c.t[2];
        const double x = (c.R[0] * dx + c.R[3] * dy) + c.R[6] * dz;
        const double y = (c.R[1] * dx + c.R[4] * dy) + c.R[7] * dz;
        const double z = (c.R[2] * dx + c.R[5] * dy) + c.R[8] * dz;
        const double pu = (c.k00 * x + c.k01 * y) / z + c.k02, pv = c.k11 * y / z + c.k12;
        xy[2 * (size_t)v] = rast_snap(pu);
        xy[2 * (size_t)v + 1] = rast_snap(pv);
        const bool ok = isfinite(fx) && isfinite(fy) && isfinite(fz) && isfinite(z);
        zc[v] = ok ? (float)z : __builtin_nanf("");
    }
}

// A triangle as the fill and resolve kernels see it.
struct RastTri {
    long long x[3], y[3];            // snapped corners
    double z[3];                     // their camera depths
    long long area;                  // (p1 - p0) x (p2 - p0): negative for a triangle seen from its front (the image's y axis points down)
    int jmin, jmax, imin, imax;      // pixel centres inside the box of the corners, clamped to the image
};
__device__ __forceinline__ int rast_ceil_div(int a) { return (a + RAST_SUB - 1) >> 8; }          // ceil(a / 256), a > -2^30
// 0 = drawn (``tr`` filled; its box may still be empty: RAST_OFFSCREEN), else the reason of the rejection.  Nothing outside
// [0, V) is dereferenced.
__device__ __forceinline__ int rast_setup(const int* __restrict__ tris, const int* __restrict__ xy, const float* __restrict__ zc, const RastView& g,
                                          int t, RastTri& tr) {
    const int a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
    if (a < 0 || b < 0 || c < 0 || a >= g.V || b >= g.V || c >= g.V || a == b || b == c || a == c) return RAST_INVALID;
    const int id[3] = {a, b, c};
    bool near_ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int px = xy[2 * (size_t)id[k]], py = xy[2 * (size_t)id[k] + 1];
        px = rast_min(rast_max(px, -RAST_GUARD), RAST_GUARD);          // (the projection's own clamp again: xy is a caller's buffer)
        py = rast_min(rast_max(py, -RAST_GUARD), RAST_GUARD);
        tr.x[k] = px; tr.y[k] = py;
        tr.z[k] = (double)zc[id[k]];
        near_ok = near_ok && tr.z[k] > g.near;          // (false for NaN)
    }
    if (!near_ok) return RAST_NEAR;
    tr.area = (tr.x[1] - tr.x[0]) * (tr.y[2] - tr.y[0]) - (tr.y[1] - tr.y[0]) * (tr.x[2] - tr.x[0]);
    if (tr.area == 0) return RAST_AREA;
    if ((g.cull == 1 && tr.area > 0) || (g.cull == 2 && tr.area < 0)) return RAST_CULLED;
    const int x0 = (int)tr.x[0], x1 = (int)tr.x[1], x2 = (int)tr.x[2], y0 = (int)tr.y[0], y1 = (int)tr.y[1], y2 = (int)tr.y[2];
    tr.jmin = rast_max(rast_ceil_div(rast_min(x0, rast_min(x1, x2))), 0);
    tr.jmax = rast_min(rast_max(x0, rast_max(x1, x2)) >> 8, g.W - 1);
    tr.imin = rast_max(rast_ceil_div(rast_min(y0, rast_min(y1, y2))), 0);
    tr.imax = rast_min(rast_max(y0, rast_max(y1, y2)) >> 8, g.H - 1);
    return 0;
}
__device__ __forceinline__ int rast_tiles(const RastTri& tr) {
    if (tr.jmin > tr.jmax || tr.imin > tr.imax) return 0;
    return ((tr.jmax >> 3) - (tr.jmin >> 3) + 1) * ((tr.imax >> 3) - (tr.imin >> 3) + 1);
}
// Edge functions of the pixel centre (256 j, 256 i): E[k] belongs to the edge opposite corner k; E[0] + E[1] + E[2] = area.  True when
// the centre is covered: s E[k] > 0, or E[k] == 0 on a left edge (dy < 0) or a top edge (dy == 0, dx > 0) of d = s (b - a).
__device__ __forceinline__ bool rast_edges(const RastTri& tr, int i, int j, long long (&E)[3]) {
    const long long px = (long long)j * RAST_SUB, py = (long long)i * RAST_SUB;
    const long long s = tr.area > 0 ? 1 : -1;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ia = (k + 1) % 3, ib = (k + 2) % 3;
        const long long dx = tr.x[ib] - tr.x[ia], dy = tr.y[ib] - tr.y[ia];
        E[k] = dx * (py - tr.y[ia]) - dy * (px - tr.x[ia]);
        const bool owns = s * dy < 0 || (dy == 0 && s * dx > 0);
        in = in && (s * E[k] > 0 || (E[k] == 0 && owns));
    }
    return in;
}
// w_k = (E_k / A) / z_k, z = 1 / ((w_0 + w_1) + w_2): quotients and sums only (the perspective-correct weights are w_k z).
__device__ __forceinline__ double rast_depth(const RastTri& tr, const long long (&E)[3], double (&w)[3]) {
    const double A = (double)tr.area;
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = ((double)E[k] / A) / tr.z[k];
    return 1.0 / ((w[0] + w[1]) + w[2]);
}

__global__ __launch_bounds__(256) void k_rast_setup(const int* __restrict__ tris, const int* __restrict__ xy, const float* __restrict__ zc, RastView g,
                                                    int* __restrict__ count) {
    for (int t = blockIdx.x * 256 + threadIdx.x; t < g.T; t += gridDim.x * 256) {
        RastTri tr;
        const int reason = rast_setup(tris, xy, zc, g, t, tr);
        count[t] = reason ? -reason : rast_tiles(tr);
    }
}

// a thread's 16 consecutive triangles: v[0] = their work items, v[1..5] = how many were rejected for each reason (5: an empty box)
__device__ __forceinline__ void rast_chunk_counts(const int* __restrict__ count, int T, int t0, long long (&v)[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = 0;
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {
        const int t = t0 + i;
        if (t >= T) continue;
        const int c = count[t];
        if (c > 0) v[0] += c;
        else if (c == 0) v[RAST_OFFSCREEN] += 1;
        else if (c >= -RAST_CULLED) v[-c] += 1;
    }
}

__global__ __launch_bounds__(256) void k_rast_blocksum(const int* __restrict__ count, int T, long long* __restrict__ bsum) {
    __shared__ long long part[4][2];
    long long v[6], total[2];
    rast_chunk_counts(count, T, blockIdx.x * SCAN_CHUNK + threadIdx.x * SCAN_PER_THREAD, v);
#pragma unroll
    for (int k = 0; k < 6; k += 2) {
        block_scan2(v[k], v[k + 1], part, total);
        if (threadIdx.x == 0) { bsum[6 * (size_t)blockIdx.x + k] = total[0]; bsum[6 * (size_t)blockIdx.x + k + 1] = total[1]; }
    }
}

// One workgroup: thread i owns a contiguous run of chunks.
__global__ __launch_bounds__(256) void k_rast_scan_blocks(const long long* __restrict__ bsum, int nchunk, long long* __restrict__ boff,
                                                          long long* __restrict__ totals) {
    __shared__ long long part[4][2];
    const int per = (nchunk + 255) / 256, c0 = threadIdx.x * per, c1 = c0 + per < nchunk ? c0 + per : nchunk;
    long long v[6] = {0, 0, 0, 0, 0, 0}, total[2];
    for (int c = c0; c < c1; ++c) {
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] += bsum[6 * (size_t)c + k];
    }
#pragma unroll
    for (int k = 0; k < 6; k += 2) {
        block_scan2(v[k], v[k + 1], part, total);
        if (threadIdx.x == 0) { totals[k] = total[0]; totals[k + 1] = total[1]; }
    }
    long long run = v[0];          // (exclusive: the work items of the chunks in front of this thread's run)
    for (int c = c0; c < c1; ++c) { boff[c] = run; run += bsum[6 * (size_t)c]; }
    if (threadIdx.x == 0) { totals[6] = 0; totals[7] = 0; }
}

__global__ __launch_bounds__(256) void k_rast_offsets(const int* __restrict__ count, int T, const long long* __restrict__ boff, int* __restrict__ offset) {
    __shared__ long long part[4][2];
    const int t0 = blockIdx.x * SCAN_CHUNK + threadIdx.x * SCAN_PER_THREAD;
    long long v[6], total[2], none = 0;
    rast_chunk_counts(count, T, t0, v);
    block_scan2(v[0], none, part, total);
    long long run = v[0] + boff[blockIdx.x];
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {
        const int t = t0 + i;
        if (t >= T) continue;
        offset[t] = (int)run;          // (below 2^31 whenever the host goes on to k_rast_fill)
        const int c = count[t];
        run += c > 0 ? c : 0;
    }
}

__global__ __launch_bounds__(256) void k_rast_fill(const int* __restrict__ tris, const int* __restrict__ xy, const float* __restrict__ zc, RastView g,
                                                   const int* __restrict__ offset, long long n_work, unsigned long long* zbuf) {
    for (long long w = blockIdx.x * 256ll + threadIdx.x; w < n_work; w += gridDim.x * 256ll) {
        int lo = 0, hi = g.T;          // the last triangle with offset <= w: the one with work items there
        for (int it = 0; it < 32 && hi - lo > 1; ++it) {
            const int mid = (lo + hi) >> 1;
            if (offset[mid] <= w) lo = mid; else hi = mid;
        }
        RastTri tr;
        if (rast_setup(tris, xy, zc, g, lo, tr)) continue;
        const long long local = w - offset[lo];
        if (local < 0 || local >= rast_tiles(tr)) continue;
        const int ntx = (tr.jmax >> 3) - (tr.jmin >> 3) + 1;
        const int tx = (tr.jmin >> 3) + (int)(local % ntx), ty = (tr.imin >> 3) + (int)(local / ntx);
        const int j0 = rast_max(tx * 8, tr.jmin), j1 = rast_min(tx * 8 + 7, tr.jmax);
        const int i0 = rast_max(ty * 8, tr.imin), i1 = rast_min(ty * 8 + 7, tr.imax);
        const int nj = j1 - j0 + 1, n = nj * (i1 - i0 + 1);          // 1..64
        for (int e = 0; e < 64 && e < n; ++e) {
            const int i = i0 + e / nj, j = j0 + e % nj;
            long long E[3];
            if (!rast_edges(tr, i, j, E)) continue;
            double wk[3];
            const float z = (float)rast_depth(tr, E, wk);
            const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)lo;
            unsigned long long* cell = zbuf + ((size_t)i * g.W + j);
            if (key < *cell) atomicMin(cell, key);
        }
    }
}

__global__ __launch_bounds__(256) void k_rast_resolve(const int* __restrict__ tris, const int* __restrict__ xy, const float* __restrict__ zc,
                                                      const float* __restrict__ attrs, int C, RastView g, const unsigned long long* __restrict__ zbuf,
                                                      float* __restrict__ depth, int* __restrict__ triangle, float* __restrict__ bary,
                                                      float* __restrict__ attr_out, int* __restrict__ cov) {
    __shared__ int part[4][2];
    const long long p = blockIdx.x * 256ll + threadIdx.x, P = (long long)g.H * g.W;
    int hit = 0, none = 0;
    if (p < P) {
        const unsigned long long key = zbuf[p];
        const unsigned t = (unsigned)(key & 0xFFFFFFFFull);
        const int i = (int)(p / g.W), j = (int)(p % g.W);
        RastTri tr;
        long long E[3];
        double w[3] = {0.0, 0.0, 0.0};
        double z = 0.0;
        if (key != RAST_EMPTY && t < (unsigned)g.T && rast_setup(tris, xy, zc, g, (int)t, tr) == 0 && rast_edges(tr, i, j, E)) {
            z = rast_depth(tr, E, w);
            hit = 1;
        }
        const float b0 = (float)(w[0] * z), b1 = (float)(w[1] * z), b2 = (float)(w[2] * z);
        depth[p] = hit ? __uint_as_float((unsigned)(key >> 32)) : __builtin_inff();
        triangle[p] = hit ? (int)t : -1;
        bary[3 * (size_t)p] = b0; bary[3 * (size_t)p + 1] = b1; bary[3 * (size_t)p + 2] = b2;
        if (C > 0) {
            const int a = hit ? tris[3 * (size_t)t] : 0, b = hit ? tris[3 * (size_t)t + 1] : 0, c = hit ? tris[3 * (size_t)t + 2] : 0;
            for (int k = 0; k < RAST_MAX_ATTRS && k < C; ++k) {
                float o = 0.f;
                if (hit) o = (b0 * attrs[(size_t)a * C + k] + b1 * attrs[(size_t)b * C + k]) + b2 * attrs[(size_t)c * C + k];
                attr_out[(size_t)p * C + k] = o;
            }
        }
    }
    int total[2];
    block_scan2(hit, none, part, total);
    if (threadIdx.x == 0) cov[blockIdx.x] = total[0];
}

__global__ __launch_bounds__(256) void k_rast_covered(const int* __restrict__ cov, int ncov, long long* __restrict__ totals) {
    __shared__ long long part[4][2];
    long long s = 0, none = 0, total[2];
    for (int c = threadIdx.x; c < ncov; c += 256) s += cov[c];
    block_scan2(s, none, part, total);
    if (threadIdx.x == 0) totals[6] = total[0];
}

static int rast_check(long long V, long long T, int H, int W) {
    ES_REQUIRE(V >= 0 && T >= 0, "negative vertex or triangle count");
    ES_REQUIRE(V < RAST_MAX_COUNT && T < RAST_MAX_COUNT, "2^31 vertices or triangles or more (indices are int32)");
    ES_REQUIRE(H >= 1 && H <= RAST_MAX_SIZE && W >= 1 && W <= RAST_MAX_SIZE, "image height and width must be 1..8192");
    return ST_OK;
}
static int rast_view(long long V, long long T, int H, int W, double near, int cull, RastView& g) {
    if (const int s = rast_check(V, T, H, W)) return s;
    ES_REQUIRE(near >= 0.0 && std::isfinite(near), "near must be finite and >= 0");
    ES_REQUIRE(cull >= 0 && cull <= 2, "cull must be 0 (none), 1 (back) or 2 (front)");
    g.V = (int)V; g.T = (int)T; g.H = H; g.W = W; g.cull = cull; g.near = near;
    return ST_OK;
}

}  // namespace es

using namespace es;

extern "C" {

int64_t es_rast_scratch_bytes(long long n_verts, long long n_tris, int height, int width) {
    if (rast_check(n_verts, n_tris, height, width) != ST_OK) return -1;
    return rast_layout(nullptr, n_tris, height, width).bytes;
}

int es_rast_project(const float* verts, long long V, const double* camera, int* xy, float* zc, void* stream) {
    ES_REQUIRE(V >= 0, "negative vertex or triangle count");
    ES_REQUIRE(V < RAST_MAX_COUNT, "2^31 vertices or triangles or more (indices are int32)");
    ES_REQUIRE(camera, "es_rast_project needs camera (17 doubles on the host)");
    RastCamera c;
    for (int k = 0; k < 17; ++k) ES_REQUIRE(std::isfinite(camera[k]), "camera parameters must be finite");
    for (int k = 0; k < 9; ++k) c.R[k] = camera[k];
    for (int k = 0; k < 3; ++k) c.t[k] = camera[9 + k];
    c.k00 = camera[12]; c.k01 = camera[13]; c.k02 = camera[14]; c.k11 = camera[15]; c.k12 = camera[16];
    ES_REQUIRE(c.k00 > 0.0 && c.k11 > 0.0, "focal lengths must be positive");
    if (V == 0) return ST_OK;
    ES_REQUIRE(verts && xy && zc, "es_rast_project needs verts, xy and zc");
    hipLaunchKernelGGL(k_rast_project, dim3(grid_for(V)), dim3(256), 0, static_cast<hipStream_t>(stream), verts, (int)V, c, xy, zc);
    return hip_last("es_rast_project");
}

int es_rast_count(const int* tris, long long V, long long T, const int* xy, const float* zc, int height, int width, double near, int cull,
                  void* scratch, long long* totals, void* stream) {
    RastView g;
    if (const int s = rast_view(V, T, height, width, near, cull, g)) return s;
    ES_REQUIRE(totals, "es_rast_count needs totals");
    ES_REQUIRE(T == 0 || tris, "es_rast_count needs tris");
    ES_REQUIRE(V == 0 || (xy && zc), "es_rast_count needs xy and zc");
    ES_SCRATCH_OK(scratch, "raster scratch");
    const RastScratch s = rast_layout(scratch, T, height, width);
    hipStream_t st = static_cast<hipStream_t>(stream);
    ES_HIP(hipMemsetAsync(s.zbuf, 0xFF, 8ull * height * width, st));
    if (T == 0) {
        ES_HIP(hipMemsetAsync(totals, 0, 8 * RAST_TOTALS, st));
        return ST_OK;
    }
    hipLaunchKernelGGL(k_rast_setup, dim3(grid_for(T)), dim3(256), 0, st, tris, xy, zc, g, s.count);
    hipLaunchKernelGGL(k_rast_blocksum, dim3((unsigned)s.nchunk), dim3(256), 0, st, s.count, g.T, s.bsum);
    hipLaunchKernelGGL(k_rast_scan_blocks, dim3(1), dim3(256), 0, st, s.bsum, s.nchunk, s.boff, totals);
    hipLaunchKernelGGL(k_rast_offsets, dim3((unsigned)s.nchunk), dim3(256), 0, st, s.count, g.T, s.boff, s.offset);
    return hip_last("es_rast_count");
}

int es_rast_fill(const int* tris, long long V, long long T, const int* xy, const float* zc, int height, int width, double near, int cull,
                 void* scratch, long long n_work, void* stream) {
    RastView g;
    if (const int s = rast_view(V, T, height, width, near, cull, g)) return s;
    ES_REQUIRE(n_work >= 0, "negative work item count");
    ES_REQUIRE(n_work < RAST_MAX_COUNT, "2^31 work items or more: too many large triangles for one call");
    if (n_work == 0 || T == 0) return ST_OK;
    ES_REQUIRE(tris && xy && zc, "es_rast_fill needs tris, xy and zc");
    ES_SCRATCH_OK(scratch, "raster scratch");
    const RastScratch s = rast_layout(scratch, T, height, width);
    hipLaunchKernelGGL(k_rast_fill, dim3(grid_for(n_work)), dim3(256), 0, static_cast<hipStream_t>(stream), tris, xy, zc, g, s.offset, n_work, s.zbuf);
    return hip_last("es_rast_fill");
}

int es_rast_resolve(const int* tris, long long V, long long T, const int* xy, const float* zc, const float* attrs, int n_attrs, int height,
                    int width, double near, int cull, void* scratch, float* depth, int* triangle, float* bary, float* attr_out, long long* totals,
                    void* stream) {
    RastView g;
    if (const int s = rast_view(V, T, height, width, near, cull, g)) return s;
    ES_REQUIRE(n_attrs >= 0 && n_attrs <= RAST_MAX_ATTRS, "n_attrs must be 0..8");
    ES_REQUIRE(depth && triangle && bary && totals, "es_rast_resolve needs depth, triangle, bary and totals");
    ES_REQUIRE(n_attrs == 0 || attr_out, "es_rast_resolve needs attr_out");
    ES_REQUIRE(T == 0 || (tris && (V == 0 || (xy && zc))), "es_rast_resolve needs tris, xy and zc");
    ES_REQUIRE(n_attrs == 0 || V == 0 || T == 0 || attrs, "es_rast_resolve needs attrs");
    ES_SCRATCH_OK(scratch, "raster scratch");
    const RastScratch s = rast_layout(scratch, T, height, width);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_rast_resolve, dim3((unsigned)s.ncov), dim3(256), 0, st, tris, xy, zc, attrs, n_attrs, g, s.zbuf, depth, triangle, bary,
                       attr_out, s.cov);
    hipLaunchKernelGGL(k_rast_covered, dim3(1), dim3(256), 0, st, s.cov, s.ncov, totals);
    return hip_last("es_rast_resolve");
}

}  // extern "C"
