// Cube triangulation of an iso-surface on the device: a field u[nx][ny][nz] -> the welded, oriented triangle mesh of u == threshold with
// the case table of endosurf_amd/meshing.py marching_cubes (this project's own table, rendered into cubes_table.h by
// tools/gen_cubes_table.py).  The scheme is iso.hip's with one table row per cell instead of 6 tetrahedra:
//
// a mesh vertex sits on an axis edge from a grid point p to p + e_axis, so it has exactly one owner slot (p, axis) and welding is
// indexing: vertex id = (exclusive scan of the owners' crossing-edge counts)[p] + rank of the axis inside p's 3-bit mask (z, y, x).
// Five launches, no atomics, no hand-off between workgroups inside a launch (bit-identical from call to call):
//   k_cubes_classify   code[p] = mask of crossing owned edges | triangles of cell p << 3 | case of cell p << 8   (signs through an LDS tile)
//   scan.h's three     exclusive scan of the vertex and triangle counts of the codes -> voff[p], toff[p], totals (CubesSrc)
//   k_cubes_emit       vertices (iso.hip's fp64 interpolation, stored fp32), their end points, triangles
// Vertex order = ascending (linear id of the owner point, direction code 4 dx + 2 dy + dz); triangle order = ascending (cell, table row).
// A point of the last plane, row or column owns no edge that leaves the grid and anchors no cell: its mask bits and its case are 0.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "cubes_table.h"
#include "launch.h"
#include "scan.h"

namespace es {

constexpr int CUBES_TX = 4, CUBES_TY = 8, CUBES_TZ = 64;      // classify tile (z fastest, one wave per x row)
constexpr long long CUBES_MAX_POINTS = 1ll << 31;             // int32 indices

struct CubesScratch {
    int* voff;               // [N] first vertex id owned by point p
    int* toff;               // [N] first triangle id of cell p
    int* bsum;               // [nblk][2] vertex / triangle count of a chunk
    int* boff;               // [nblk][2] exclusive scan of bsum
    unsigned short* code;    // [N] classify output
    long long* totals;       // [2] the counts es_cubes_count found: es_cubes_emit checks its capacities against them
    long long N, nblk, bytes;
};
static CubesScratch cubes_layout(const void* scratch, long long N) {          // a null scratch measures only
    Carver c(scratch);
    CubesScratch s;
    s.N = N;
    s.nblk = scan_chunks(N);
    s.voff = c.take<int>(N);
    s.toff = c.take<int>(N);
    s.bsum = c.take<int>(2 * s.nblk);
    s.boff = c.take<int>(2 * s.nblk);
    s.code = c.take<unsigned short>(N);
    s.totals = c.take<long long>(2);
    s.bytes = c.off;
    return s;
}

__device__ __forceinline__ bool cubes_inside(float u, double thr) { return (double)u < thr; }          // NaN and u == thr are outside
// bit k: the edge from a point along axis k (0 = z, 1 = y, 2 = x) stays inside the grid
__device__ __forceinline__ unsigned axis_valid_mask(bool vx, bool vy, bool vz) { return (unsigned)vz | (unsigned)vy << 1 | (unsigned)vx << 2; }
// cm: bit c = corner c of the cell at p is inside.  Crossing axis edges owned by p: corners 1 (z), 2 (y), 4 (x) differ from corner 0.
__device__ __forceinline__ unsigned axis_edge_mask(unsigned cm, unsigned valid) {
    return ((((cm >> 1) & 1u) | ((cm >> 2) & 1u) << 1 | ((cm >> 4) & 1u) << 2) ^ (0u - (cm & 1u))) & 7u & valid;
}

__global__ __launch_bounds__(256) void k_cubes_classify(const float* __restrict__ u, int nx, int ny, int nz, double thr, int tiles_z, int tiles_y,
                                                        long long ntiles, unsigned short* __restrict__ code) {
    __shared__ unsigned char in[CUBES_TX + 1][CUBES_TY + 1][CUBES_TZ + 4];
    const int tid = threadIdx.x, lane = tid & 63, lx = tid >> 6;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int z0 = (int)(tile % tiles_z) * CUBES_TZ, y0 = (int)((tile / tiles_z) % tiles_y) * CUBES_TY, x0 = (int)(tile / tiles_z / tiles_y) * CUBES_TX;
        for (int e = tid; e < (CUBES_TX + 1) * (CUBES_TY + 1) * (CUBES_TZ + 1); e += 256) {
            const int ez = e % (CUBES_TZ + 1), r = e / (CUBES_TZ + 1), ey = r % (CUBES_TY + 1), ex = r / (CUBES_TY + 1);
            const int gx = x0 + ex, gy = y0 + ey, gz = z0 + ez;
            unsigned char v = 0;
            if (gx < nx && gy < ny && gz < nz) v = cubes_inside(u[((size_t)gx * ny + gy) * nz + gz], thr) ? 1 : 0;
            in[ex][ey][ez] = v;
        }
        __syncthreads();
        const int gx = x0 + lx, gz = z0 + lane;
        if (gx < nx && gz < nz) {
#pragma unroll
            for (int ly = 0; ly < CUBES_TY; ++ly) {
                const int gy = y0 + ly;
                if (gy >= ny) break;
                unsigned cm = 0;
#pragma unroll
                for (int c = 0; c < 8; ++c) cm |= (unsigned)in[lx + (c >> 2)][ly + ((c >> 1) & 1)][lane + (c & 1)] << c;
                const bool vx = gx + 1 < nx, vy = gy + 1 < ny, vz = gz + 1 < nz;
                const unsigned m = axis_edge_mask(cm, axis_valid_mask(vx, vy, vz));
                const unsigned cs = (vx && vy && vz) ? cm : 0u;          // (a point that anchors no cell: case 0, no triangle)
                code[((size_t)gx * ny + gy) * nz + gz] = (unsigned short)(m | (unsigned)CUBES_TRI[cs][15] << 3 | cs << 8);
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int cubes_code_verts(unsigned c) { return __popc(c & 7u); }
__device__ __forceinline__ int cubes_code_tris(unsigned c) { return (int)((c >> 3) & 7u); }
// the scan's source: the codes -> voff[p], toff[p]
struct CubesSrc {
    using sum_t = int;
    using items_t = unsigned short[SCAN_PER_THREAD];
    const unsigned short* code;
    long long N;
    int *voff, *toff;
    // the 16 codes of a thread's consecutive points (0 beyond the grid) -> its vertex and triangle counts
    __device__ __forceinline__ void load(long long p0, items_t& c, int& nv, int& nt) const {
        if (p0 + SCAN_PER_THREAD <= N) {
            const uint4* q = reinterpret_cast<const uint4*>(code + p0);          // 32-byte aligned: code is 16-byte aligned, p0 a multiple of 16
            uint4 w[2] = {q[0], q[1]};
            __builtin_memcpy(c, w, sizeof(c));
        } else {
#pragma unroll
            for (int i = 0; i < SCAN_PER_THREAD; ++i) c[i] = p0 + i < N ? code[p0 + i] : (unsigned short)0;
        }
        nv = 0; nt = 0;
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) { nv += cubes_code_verts(c[i]); nt += cubes_code_tris(c[i]); }
    }
    __device__ __forceinline__ void store(long long p0, const items_t& c, int nv, int nt) const {
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) {
            if (p0 + i < N) { voff[p0 + i] = nv; toff[p0 + i] = nt; }
            nv += cubes_code_verts(c[i]); nt += cubes_code_tris(c[i]);
        }
    }
};

// One thread per grid point: the vertices it owns and the triangles of its cell.  Every read is inside the grid whatever ``code`` /
// ``voff`` / ``toff`` hold (validity comes from the coordinates, the case is 8 bits, a table row ends at its 0xff), every write is
// checked against the capacity of the output buffers.
__global__ __launch_bounds__(256) void k_cubes_emit(const float* __restrict__ u, int nx, int ny, int nz, double thr, const unsigned short* __restrict__ code,
                                                    const int* __restrict__ voff, const int* __restrict__ toff, int cap_v, int cap_t,
                                                    float* __restrict__ verts, int* __restrict__ ends, int* __restrict__ tris) {
    const unsigned N = (unsigned)nx * (unsigned)ny * (unsigned)nz, p = blockIdx.x * 256u + threadIdx.x;
    if (p >= N) return;
    const unsigned cd = code[p];
    if (cd == 0) return;
    const int z = (int)(p % (unsigned)nz), y = (int)((p / (unsigned)nz) % (unsigned)ny), x = (int)(p / (unsigned)nz / (unsigned)ny);
    const bool vx = x + 1 < nx, vy = y + 1 < ny, vz = z + 1 < nz;
    const unsigned sx = (unsigned)ny * (unsigned)nz, sy = (unsigned)nz;
    const unsigned m = cd & 7u & axis_valid_mask(vx, vy, vz);
    if (m) {
        const float up = u[p];
        const bool pin = cubes_inside(up, thr);
        int vid = voff[p];
#pragma unroll
        for (int k = 0; k < 3; ++k) {          // z, y, x: ascending direction code
            if (!((m >> k) & 1u)) continue;
            const int dx = k == 2, dy = k == 1, dz = k == 0;
            const unsigned q = p + dx * sx + dy * sy + dz;
            const float uq = u[q];
            // a: the inside end, b: the outside end; w in fp64 as on the host (the expression of k_iso_emit)
            const double ua = pin ? up : uq, ub = pin ? uq : up;
            const double w = (thr - ua) / (ub - ua), sgn = pin ? 1.0 : -1.0;
            if (vid >= 0 && vid < cap_v) {
                float* v = verts + 3 * (size_t)vid;
                v[0] = (float)((double)(pin ? x : x + dx) + w * (sgn * dx));
                v[1] = (float)((double)(pin ? y : y + dy) + w * (sgn * dy));
                v[2] = (float)((double)(pin ? z : z + dz) + w * (sgn * dz));
                ends[2 * (size_t)vid] = (int)(pin ? p : q);
                ends[2 * (size_t)vid + 1] = (int)(pin ? q : p);
            }
            ++vid;
        }
    }
    if (((cd >> 3) & 7u) && vx && vy && vz) {
        const unsigned char* row = CUBES_TRI[(cd >> 8) & 0xffu];
        int tid = toff[p];
        for (int k = 0; k < 5 && row[3 * k] != 0xff; ++k, ++tid) {
            if (tid < 0 || tid >= cap_t) continue;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned e = row[3 * k + j], oc = e >> 3, d = e & 7u;
                const unsigned o = p + (oc >> 2) * sx + ((oc >> 1) & 1u) * sy + (oc & 1u);          // the owner: a corner of this cell
                tris[3 * (size_t)tid + j] = voff[o] + __popc(code[o] & (d - 1u));          // bits below the axis bit (d = 1, 2, 4)
            }
        }
    }
}

static int cubes_check_dims(int nx, int ny, int nz) {
    ES_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "iso-surface grid needs at least 2 points per axis");
    ES_REQUIRE((long long)nx * ny * nz < CUBES_MAX_POINTS, "iso-surface grid has 2^31 points or more (int32 indices)");
    return ST_OK;
}

}  // namespace es

using namespace es;

extern "C" {

int64_t es_cubes_scratch_bytes(int nx, int ny, int nz) {
    if (cubes_check_dims(nx, ny, nz) != ST_OK) return -1;
    return cubes_layout(nullptr, (long long)nx * ny * nz).bytes;
}

int es_cubes_count(const float* field, int nx, int ny, int nz, double threshold, void* scratch, long long* totals, void* stream) {
    if (const int s = cubes_check_dims(nx, ny, nz)) return s;
    ES_REQUIRE(field && scratch && totals, "es_cubes_count needs field, scratch and totals");
    ES_SCRATCH_OK(scratch, "iso-surface scratch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CubesScratch s = cubes_layout(scratch, (long long)nx * ny * nz);
    const int tiles_z = (nz + CUBES_TZ - 1) / CUBES_TZ, tiles_y = (ny + CUBES_TY - 1) / CUBES_TY, tiles_x = (nx + CUBES_TX - 1) / CUBES_TX;
    const long long ntiles = (long long)tiles_z * tiles_y * tiles_x;
    const unsigned grid = (unsigned)(ntiles < (1ll << 20) ? ntiles : (1ll << 20));
    hipLaunchKernelGGL(k_cubes_classify, dim3(grid), dim3(256), 0, st, field, nx, ny, nz, threshold, tiles_z, tiles_y, ntiles, s.code);
    scan_launch(CubesSrc{s.code, s.N, s.voff, s.toff}, s.nblk, s.bsum, s.boff, s.totals, st);
    ES_HIP(hipMemcpyAsync(totals, s.totals, 2 * sizeof(long long), hipMemcpyDeviceToDevice, st));
    return hip_last("es_cubes_count");
}

int es_cubes_emit(const float* field, int nx, int ny, int nz, double threshold, const void* scratch, long long n_verts, long long n_tris, float* verts,
                  int* edge_ends, int* tris, void* stream) {
    if (const int s = cubes_check_dims(nx, ny, nz)) return s;
    ES_REQUIRE(field && scratch, "es_cubes_emit needs field and scratch");
    ES_SCRATCH_OK(scratch, "iso-surface scratch");
    ES_REQUIRE(n_verts >= 0 && n_tris >= 0 && n_verts < CUBES_MAX_POINTS && n_tris < CUBES_MAX_POINTS, "mesh does not fit int32 indices");
    if (n_verts == 0 && n_tris == 0) return ST_OK;
    ES_REQUIRE((n_verts == 0 || (verts && edge_ends)) && (n_tris == 0 || tris), "es_cubes_emit needs verts, edge_ends and tris");
    const long long N = (long long)nx * ny * nz;
    const CubesScratch s = cubes_layout(scratch, N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long found[2] = {0, 0};          // (the caller has read the totals already: this copy waits for nothing but itself)
    ES_HIP(hipMemcpyAsync(found, s.totals, sizeof(found), hipMemcpyDeviceToHost, st));
    ES_HIP(hipStreamSynchronize(st));
    ES_REQUIRE(found[0] <= n_verts && found[1] <= n_tris, "es_cubes_emit: the mesh es_cubes_count found exceeds the capacity of the output buffers");
    hipLaunchKernelGGL(k_cubes_emit, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, field, nx, ny, nz, threshold,
                       s.code, s.voff, s.toff, (int)n_verts, (int)n_tris, verts, edge_ends, tris);
    return hip_last("es_cubes_emit");
}

}  // extern "C"
