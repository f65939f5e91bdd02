// Narrow-band field assembly (ABI v10): the device half of a block-sparse mesh extraction.  A dense field u[nx][ny][nz] is built from
// evaluations of the caller's sampler near the level set only, such that es_iso_count / es_iso_emit (iso.hip, unchanged) produce from it
// the mesh they produce from the densely sampled field.  The host drives the rounds (Engine.band_field; numpy twin: meshing.band_field):
//
//   blocks of B cells per axis, ceil((n - 1) / B) per axis, edge blocks shorter; block corners are lattice points (min(i B, n - 1))
//   k_band_lattice_points  coordinates of a run of lattice points (stride 1: the lattice itself; stride B: the coarse lattice)
//   k_band_seed            round[b] = 1 for a seed block (corner flags differ | a NaN corner | no corner farther than ``margin`` from the
//                          level), else 0; fill[b] = the corner value farthest from the level
//   scan.h's three         the blocks with round[b] == r in ascending order -> ids[], exclusive point offsets poff[], totals (BandSrc:
//                          the scan over blocks, its store pass compacting)
//   k_band_fill            field[p] = fill[block of p]
//   k_band_points          coordinates of points [m0, m0 + count) of the listed blocks (closed ranges: shared faces are listed twice)
//   k_band_scatter         their values -> field
//   k_band_grow            an inactive block next to a block evaluated in round r whose shared face holds a value of the other sign than
//                          the block's fill value gets round[b] = r + 1
//
// No atomics, no hand-off between workgroups: within k_band_grow a block only ever turns from 0 to r + 1 while its neighbours look for
// == r, and duplicated face points scatter the same value.  Every loop over rounds is on the host.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"
#include "scan.h"

namespace es {

constexpr long long BAND_MAX_POINTS = 1ll << 31;             // int32 indices

struct BandGeom {
    int nx, ny, nz, B, nbx, nby, nbz;
    int NB;                  // blocks
    long long N;             // lattice points
};
struct BandScratch {
    int* round;              // [NB] 0 = inactive, r = activated in round r (1 = seed)
    float* fill;             // [NB] the corner value farthest from the level
    int* ids;                // [NB] the current list: block ids, ascending
    int* poff;               // [NB] first point of each listed block
    int* bsum;               // [nchunk][2] listed blocks / their points per chunk
    int* boff;               // [nchunk][2] exclusive scan of bsum
    long long nchunk, bytes;
};
static inline BandGeom band_geom(int nx, int ny, int nz, int B) {
    BandGeom g;
    g.nx = nx; g.ny = ny; g.nz = nz; g.B = B;
    g.nbx = (nx - 2 + B) / B; g.nby = (ny - 2 + B) / B; g.nbz = (nz - 2 + B) / B;
    g.NB = g.nbx * g.nby * g.nbz;
    g.N = (long long)nx * ny * nz;
    return g;
}
static BandScratch band_layout(const void* scratch, const BandGeom& g) {          // a null scratch measures only
    Carver c(scratch);
    BandScratch s;
    s.nchunk = scan_chunks(g.NB);
    s.round = c.take<int>(g.NB);          // (first: Engine.band_field reads it from the head of the scratch)
    s.fill = c.take<float>(g.NB);
    s.ids = c.take<int>(g.NB);
    s.poff = c.take<int>(g.NB);
    s.bsum = c.take<int>(2 * s.nchunk);
    s.boff = c.take<int>(2 * s.nchunk);
    s.bytes = c.off;
    return s;
}

__device__ __forceinline__ bool band_inside(float u, double thr) { return (double)u < thr; }          // iso.hip is_inside
__device__ __forceinline__ int band_min(int a, int b) { return a < b ? a : b; }
// cells of block coordinate b along an axis of n points
__device__ __forceinline__ int band_extent(int b, int B, int n) { return band_min(B, n - 1 - b * B); }
__device__ __forceinline__ void band_coords(const BandGeom& g, int b, int& bi, int& bj, int& bk) {
    bk = b % g.nbz; bj = (b / g.nbz) % g.nby; bi = b / g.nbz / g.nby;
}
__device__ __forceinline__ int band_block_points(const BandGeom& g, int b) {
    int bi, bj, bk;
    band_coords(g, b, bi, bj, bk);
    return (band_extent(bi, g.B, g.nx) + 1) * (band_extent(bj, g.B, g.ny) + 1) * (band_extent(bk, g.B, g.nz) + 1);
}

// Point p0 + e of the lattice of (cx, cy, cz) points with index min(i stride, n - 1) along each axis.
__global__ __launch_bounds__(256) void k_band_lattice_points(const float* __restrict__ ax, const float* __restrict__ ay, const float* __restrict__ az,
                                                             int nx, int ny, int nz, int cx, int cy, int cz, int stride, long long p0, long long count,
                                                             float* __restrict__ x) {
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < count; e += gridDim.x * 256ll) {
        const long long p = p0 + e;
        const int k = (int)(p % cz), j = (int)((p / cz) % cy), i = (int)(p / cz / cy);
        if (i >= cx) continue;
        float* o = x + 3 * (size_t)e;
        o[0] = ax[band_min(i * stride, nx - 1)];
        o[1] = ay[band_min(j * stride, ny - 1)];
        o[2] = az[band_min(k * stride, nz - 1)];
    }
}

// uc: the coarse lattice [nbx + 1][nby + 1][nbz + 1]
__global__ __launch_bounds__(256) void k_band_seed(const float* __restrict__ uc, BandGeom g, double thr, double margin, int* __restrict__ round,
                                                   float* __restrict__ fill) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b < g.NB; b += gridDim.x * 256) {
        int bi, bj, bk;
        band_coords(g, b, bi, bj, bk);
        double best = -1.0;
        float val = 0.f;
        int n_in = 0;
        bool nan = false;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float u = uc[((size_t)(bi + (c >> 2)) * (g.nby + 1) + (bj + ((c >> 1) & 1))) * (g.nbz + 1) + (bk + (c & 1))];
            const double d = fabs((double)u - thr);
            nan |= u != u;
            n_in += band_inside(u, thr) ? 1 : 0;
            if (d > best) { best = d; val = u; }          // (a NaN distance never wins: the first farthest corner, as numpy's argmax)
        }
        const bool seed = (n_in != 0 && n_in != 8) || nan || !(best > margin);
        round[b] = seed ? 1 : 0;
        fill[b] = val;
    }
}

// the scan's source: the blocks with round == sel, in ascending order -> ids[], poff[]
struct BandSrc {
    using sum_t = int;
    using items_t = unsigned;          // bit i: block b0 + i is listed
    const int* round;
    BandGeom g;
    int sel;
    int *ids, *poff;
    // a thread's 16 consecutive blocks: how many are listed and the points of those
    __device__ __forceinline__ void load(long long b0, unsigned& mask, int& cnt, int& pts) const {
        cnt = 0; pts = 0; mask = 0;
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) {
            const int b = (int)b0 + i;
            if (b < g.NB && round[b] == sel) { ++cnt; pts += band_block_points(g, b); mask |= 1u << i; }
        }
    }
    __device__ __forceinline__ void store(long long b0, const unsigned& mask, int cnt, int pts) const {
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) {
            if (!((mask >> i) & 1u)) continue;
            if (cnt >= 0 && cnt < g.NB) { ids[cnt] = (int)b0 + i; poff[cnt] = pts; }
            ++cnt; pts += band_block_points(g, (int)b0 + i);
        }
    }
};

__global__ __launch_bounds__(256) void k_band_fill(BandGeom g, const float* __restrict__ fill, float* __restrict__ field) {
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < g.N; p += gridDim.x * 256ll) {
        const int k = (int)(p % g.nz), j = (int)((p / g.nz) % g.ny), i = (int)(p / g.nz / g.ny);
        const int bi = band_min(i / g.B, g.nbx - 1), bj = band_min(j / g.B, g.nby - 1), bk = band_min(k / g.B, g.nbz - 1);
        field[p] = fill[(bi * g.nby + bj) * g.nbz + bk];
    }
}

// Point m of the current list -> its lattice indices.  False (nothing may be read or written for it) when the list, whatever it holds,
// does not place m inside the lattice.
__device__ __forceinline__ bool band_locate(const BandGeom& g, const int* __restrict__ ids, const int* __restrict__ poff, int n_list, long long m,
                                            int& i, int& j, int& k) {
    int lo = 0, hi = n_list;          // the last entry with poff <= m
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (poff[mid] <= m) lo = mid; else hi = mid;
    }
    const int b = ids[lo];
    const long long local = m - poff[lo];
    if (b < 0 || b >= g.NB || local < 0) return false;
    int bi, bj, bk;
    band_coords(g, b, bi, bj, bk);
    const int ey = band_extent(bj, g.B, g.ny) + 1, ez = band_extent(bk, g.B, g.nz) + 1, ex = band_extent(bi, g.B, g.nx) + 1;
    if (local >= (long long)ex * ey * ez) return false;
    const int l = (int)local;
    i = bi * g.B + l / (ey * ez); j = bj * g.B + (l / ez) % ey; k = bk * g.B + l % ez;
    return true;
}

__global__ __launch_bounds__(256) void k_band_points(const float* __restrict__ ax, const float* __restrict__ ay, const float* __restrict__ az, BandGeom g,
                                                     const int* __restrict__ ids, const int* __restrict__ poff, int n_list, long long m0, long long count,
                                                     float* __restrict__ x) {
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < count; e += gridDim.x * 256ll) {
        int i = 0, j = 0, k = 0;
        float* o = x + 3 * (size_t)e;
        // a slot the list does not cover still gets a point of the lattice: the sampler reads all ``count`` rows
        band_locate(g, ids, poff, n_list, m0 + e, i, j, k);
        o[0] = ax[i]; o[1] = ay[j]; o[2] = az[k];
    }
}

__global__ __launch_bounds__(256) void k_band_scatter(const float* __restrict__ vals, BandGeom g, const int* __restrict__ ids,
                                                      const int* __restrict__ poff, int n_list, long long m0, long long count, float* __restrict__ field) {
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < count; e += gridDim.x * 256ll) {
        int i, j, k;
        if (band_locate(g, ids, poff, n_list, m0 + e, i, j, k)) field[((size_t)i * g.ny + j) * g.nz + k] = vals[e];
    }
}

// One wavefront per block.  The face shared with a neighbour along ``axis`` lies in the lattice plane max(b, q) B of that axis and spans
// the block's closed ranges along the other two (the higher of them runs fastest: z whenever the face is not a z plane).
__global__ __launch_bounds__(256) void k_band_grow(const float* __restrict__ field, BandGeom g, double thr, int r, int* round,
                                                   const float* __restrict__ fill) {
    const int lane = threadIdx.x & 63;
    for (int b = blockIdx.x * 4 + (threadIdx.x >> 6); b < g.NB; b += gridDim.x * 4) {
        if (round[b] != 0) continue;          // (wave-uniform)
        int ci, cj, ck;
        band_coords(g, b, ci, cj, ck);
        const int ei = band_extent(ci, g.B, g.nx) + 1, ej = band_extent(cj, g.B, g.ny) + 1, ek = band_extent(ck, g.B, g.nz) + 1;
        const bool in_b = band_inside(fill[b], thr);
        bool hit = false;
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            const int axis = f >> 1, side = (f & 1) ? 1 : -1;
            const int ca = axis == 0 ? ci : (axis == 1 ? cj : ck), qa = ca + side;
            if (hit || qa < 0 || qa >= (axis == 0 ? g.nbx : (axis == 1 ? g.nby : g.nbz))) continue;
            const int q = ((axis == 0 ? qa : ci) * g.nby + (axis == 1 ? qa : cj)) * g.nbz + (axis == 2 ? qa : ck);
            if (round[q] != r) continue;
            const int plane = (side > 0 ? qa : ca) * g.B;
            const int e1 = axis == 0 ? ej : ei, e2 = axis == 2 ? ej : ek;          // extents along the lower / higher remaining axis
            bool differs = false;
            for (int e = lane; e < e1 * e2; e += 64) {
                const int u = e / e2, v = e % e2;
                const int i = axis == 0 ? plane : ci * g.B + u;
                const int j = axis == 1 ? plane : cj * g.B + (axis == 0 ? u : v);
                const int k = axis == 2 ? plane : ck * g.B + v;
                differs |= band_inside(field[((size_t)i * g.ny + j) * g.nz + k], thr) != in_b;
            }
            hit = __any(differs);
        }
        if (hit && lane == 0) round[b] = r + 1;
    }
}

static int band_check(int nx, int ny, int nz, int block) {
    ES_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "band lattice needs at least 2 points per axis");
    ES_REQUIRE(block >= 2 && block <= 32, "band block must be 2..32 cells");
    ES_REQUIRE((long long)nx * ny * nz < BAND_MAX_POINTS, "band lattice has 2^31 points or more (int32 indices)");
    const long long nb = (long long)((nx - 2 + block) / block) * ((ny - 2 + block) / block) * ((nz - 2 + block) / block);
    ES_REQUIRE(nb * (block + 1) * (block + 1) * (block + 1) < BAND_MAX_POINTS, "band blocks hold 2^31 points or more (int32 indices)");
    return ST_OK;
}
// the list of the blocks with round == sel (ids, poff) and its totals
static void band_list(const BandGeom& g, const BandScratch& s, int sel, long long* totals, hipStream_t st) {
    scan_launch(BandSrc{s.round, g, sel, s.ids, s.poff}, s.nchunk, s.bsum, s.boff, totals, st);
}

}  // namespace es

using namespace es;

extern "C" {

int64_t es_band_scratch_bytes(int nx, int ny, int nz, int block) {
    if (band_check(nx, ny, nz, block) != ST_OK) return -1;
    return band_layout(nullptr, band_geom(nx, ny, nz, block)).bytes;
}

int es_band_lattice_points(const float* ax, const float* ay, const float* az, int nx, int ny, int nz, int stride, long long p0, long long count,
                           float* x, void* stream) {
    ES_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "band lattice needs at least 2 points per axis");
    ES_REQUIRE((long long)nx * ny * nz < BAND_MAX_POINTS, "band lattice has 2^31 points or more (int32 indices)");
    ES_REQUIRE(stride >= 1 && stride <= 32, "es_band_lattice_points: stride must be 1..32");
    const int cx = stride == 1 ? nx : (nx - 2 + stride) / stride + 1, cy = stride == 1 ? ny : (ny - 2 + stride) / stride + 1,
              cz = stride == 1 ? nz : (nz - 2 + stride) / stride + 1;
    ES_REQUIRE(p0 >= 0 && count >= 0 && p0 + count <= (long long)cx * cy * cz, "es_band_lattice_points: point range outside the lattice");
    if (count == 0) return ST_OK;
    ES_REQUIRE(ax && ay && az && x, "es_band_lattice_points needs the three axes and x");
    hipLaunchKernelGGL(k_band_lattice_points, dim3(grid_for(count)), dim3(256), 0, static_cast<hipStream_t>(stream), ax, ay, az, nx, ny, nz, cx, cy, cz,
                       stride, p0, count, x);
    return hip_last("es_band_lattice_points");
}

int es_band_seed(const float* coarse, int nx, int ny, int nz, int block, double threshold, double margin, void* scratch, long long* totals,
                 void* stream) {
    if (const int s = band_check(nx, ny, nz, block)) return s;
    ES_REQUIRE(coarse && totals, "es_band_seed needs coarse and totals");
    ES_SCRATCH_OK(scratch, "band scratch");
    const BandGeom g = band_geom(nx, ny, nz, block);
    const BandScratch s = band_layout(scratch, g);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_band_seed, dim3(grid_for(g.NB)), dim3(256), 0, st, coarse, g, threshold, margin, s.round, s.fill);
    band_list(g, s, 1, totals, st);
    return hip_last("es_band_seed");
}

int es_band_fill(int nx, int ny, int nz, int block, const void* scratch, float* field, void* stream) {
    if (const int s = band_check(nx, ny, nz, block)) return s;
    ES_REQUIRE(field, "es_band_fill needs field");
    ES_SCRATCH_OK(scratch, "band scratch");
    const BandGeom g = band_geom(nx, ny, nz, block);
    const BandScratch s = band_layout(scratch, g);
    hipLaunchKernelGGL(k_band_fill, dim3(grid_for(g.N)), dim3(256), 0, static_cast<hipStream_t>(stream), g, s.fill, field);
    return hip_last("es_band_fill");
}

int es_band_points(const float* ax, const float* ay, const float* az, int nx, int ny, int nz, int block, const void* scratch, long long n_list,
                   long long m0, long long count, float* x, void* stream) {
    if (const int s = band_check(nx, ny, nz, block)) return s;
    ES_SCRATCH_OK(scratch, "band scratch");
    const BandGeom g = band_geom(nx, ny, nz, block);
    ES_REQUIRE(n_list >= 1 && n_list <= g.NB && m0 >= 0 && count >= 0 && m0 + count < BAND_MAX_POINTS, "es_band_points: list or point range out of range");
    if (count == 0) return ST_OK;
    ES_REQUIRE(ax && ay && az && x, "es_band_points needs the three axes and x");
    const BandScratch s = band_layout(scratch, g);
    hipLaunchKernelGGL(k_band_points, dim3(grid_for(count)), dim3(256), 0, static_cast<hipStream_t>(stream), ax, ay, az, g, s.ids, s.poff, (int)n_list, m0,
                       count, x);
    return hip_last("es_band_points");
}

int es_band_scatter(const float* values, int nx, int ny, int nz, int block, const void* scratch, long long n_list, long long m0, long long count,
                    float* field, void* stream) {
    if (const int s = band_check(nx, ny, nz, block)) return s;
    ES_SCRATCH_OK(scratch, "band scratch");
    const BandGeom g = band_geom(nx, ny, nz, block);
    ES_REQUIRE(n_list >= 1 && n_list <= g.NB && m0 >= 0 && count >= 0 && m0 + count < BAND_MAX_POINTS, "es_band_scatter: list or point range out of range");
    if (count == 0) return ST_OK;
    ES_REQUIRE(values && field, "es_band_scatter needs values and field");
    const BandScratch s = band_layout(scratch, g);
    hipLaunchKernelGGL(k_band_scatter, dim3(grid_for(count)), dim3(256), 0, static_cast<hipStream_t>(stream), values, g, s.ids, s.poff, (int)n_list, m0,
                       count, field);
    return hip_last("es_band_scatter");
}

int es_band_grow(const float* field, int nx, int ny, int nz, int block, double threshold, int round, void* scratch, long long* totals, void* stream) {
    if (const int s = band_check(nx, ny, nz, block)) return s;
    ES_REQUIRE(field && totals, "es_band_grow needs field and totals");
    ES_REQUIRE(round >= 1 && round < (1 << 30), "es_band_grow: round must be >= 1");
    ES_SCRATCH_OK(scratch, "band scratch");
    const BandGeom g = band_geom(nx, ny, nz, block);
    const BandScratch s = band_layout(scratch, g);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_band_grow, dim3(grid_for(g.NB, 4)), dim3(256), 0, st, field, g, threshold, round, s.round, s.fill);
    band_list(g, s, round + 1, totals, st);
    return hip_last("es_band_grow");
}

}  // extern "C"
