// Iso-surface extraction on the device (ABI v9): a field u[nx][ny][nz] -> the welded, oriented triangle mesh of u == threshold, with the
// triangulation of endosurf_amd/meshing.py marching_tetrahedra (6 tetrahedra per cell around the 0-7 diagonal, tables derived from that
// module by tools/gen_iso_table.py).
//
// Every tetrahedron edge runs from a grid point p to p + d with d one of the 7 non-zero binary vectors, so a mesh vertex has exactly one
// owner slot (p, d) and welding is indexing: vertex id = (exclusive scan of the owners' crossing-edge counts)[p] + rank of d inside p's
// 7-bit mask.  Five launches, no atomics, no hand-off between workgroups inside a launch (bit-identical from call to call):
//   k_iso_classify     code[p] = mask of crossing owned edges | triangles of cell p << 8   (corner signs through an LDS tile)
//   scan.h's three     exclusive scan of the vertex and triangle counts of the codes -> voff[p], toff[p], totals (IsoSrc)
//   k_iso_emit         vertices (fp64 interpolation, stored fp32), their end points, triangles
// Vertex order = ascending (linear id of the owner point, d); triangle order = ascending (cell, tetrahedron, table order).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "iso_table.h"
#include "launch.h"
#include "scan.h"

namespace es {

constexpr int ISO_TX = 4, ISO_TY = 8, ISO_TZ = 64;          // classify tile (z fastest, one wave per x row)
constexpr long long ISO_MAX_POINTS = 1ll << 31;             // int32 indices

struct IsoScratch {
    int* voff;               // [N] first vertex id owned by point p
    int* toff;               // [N] first triangle id of cell p
    int* bsum;               // [nblk][2] vertex / triangle count of a chunk
    int* boff;               // [nblk][2] exclusive scan of bsum
    unsigned short* code;    // [N] classify output
    long long N, nblk, bytes;
};
static IsoScratch iso_layout(const void* scratch, long long N) {          // a null scratch measures only
    Carver c(scratch);
    IsoScratch s;
    s.N = N;
    s.nblk = scan_chunks(N);
    s.voff = c.take<int>(N);
    s.toff = c.take<int>(N);
    s.bsum = c.take<int>(2 * s.nblk);
    s.boff = c.take<int>(2 * s.nblk);
    s.code = c.take<unsigned short>(N);
    s.bytes = c.off;
    return s;
}

// bit d-1: the edge from a point to point + d (d = 4 dx + 2 dy + dz) stays inside the grid
__device__ __forceinline__ unsigned dir_valid_mask(bool vx, bool vy, bool vz) {
    unsigned m = 0;
#pragma unroll
    for (int d = 1; d < 8; ++d) m |= (unsigned)((!(d & 4) || vx) && (!(d & 2) || vy) && (!(d & 1) || vz)) << (d - 1);
    return m;
}
// cm: bit c = corner c of the cell at p is inside.  Crossing edges owned by p: corner d differs from corner 0.
__device__ __forceinline__ unsigned edge_mask(unsigned cm, unsigned valid) { return ((cm >> 1) ^ (0u - (cm & 1u))) & 0x7fu & valid; }
__device__ __forceinline__ unsigned tet_case(unsigned cm, int t) {
    return ((cm >> ISO_TETS[t][0]) & 1u) | ((cm >> ISO_TETS[t][1]) & 1u) << 1 | ((cm >> ISO_TETS[t][2]) & 1u) << 2 | ((cm >> ISO_TETS[t][3]) & 1u) << 3;
}
__device__ __forceinline__ unsigned tri_count(unsigned cm) {
    unsigned n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int k = __popc(tet_case(cm, t));
        n += (k == 0 || k == 4) ? 0u : (k == 2 ? 2u : 1u);
    }
    return n;
}
__device__ __forceinline__ bool is_inside(float u, double thr) { return (double)u < thr; }          // NaN and u == thr are outside

__global__ __launch_bounds__(256) void k_iso_classify(const float* __restrict__ u, int nx, int ny, int nz, double thr, int tiles_z, int tiles_y,
                                                      long long ntiles, unsigned short* __restrict__ code) {
    __shared__ unsigned char in[ISO_TX + 1][ISO_TY + 1][ISO_TZ + 4];
    const int tid = threadIdx.x, lane = tid & 63, lx = tid >> 6;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int z0 = (int)(tile % tiles_z) * ISO_TZ, y0 = (int)((tile / tiles_z) % tiles_y) * ISO_TY, x0 = (int)(tile / tiles_z / tiles_y) * ISO_TX;
        for (int e = tid; e < (ISO_TX + 1) * (ISO_TY + 1) * (ISO_TZ + 1); e += 256) {
            const int ez = e % (ISO_TZ + 1), r = e / (ISO_TZ + 1), ey = r % (ISO_TY + 1), ex = r / (ISO_TY + 1);
            const int gx = x0 + ex, gy = y0 + ey, gz = z0 + ez;
            unsigned char v = 0;
            if (gx < nx && gy < ny && gz < nz) v = is_inside(u[((size_t)gx * ny + gy) * nz + gz], thr) ? 1 : 0;
            in[ex][ey][ez] = v;
        }
        __syncthreads();
        const int gx = x0 + lx, gz = z0 + lane;
        if (gx < nx && gz < nz) {
#pragma unroll
            for (int ly = 0; ly < ISO_TY; ++ly) {
                const int gy = y0 + ly;
                if (gy >= ny) break;
                unsigned cm = 0;
#pragma unroll
                for (int c = 0; c < 8; ++c) cm |= (unsigned)in[lx + (c >> 2)][ly + ((c >> 1) & 1)][lane + (c & 1)] << c;
                const bool vx = gx + 1 < nx, vy = gy + 1 < ny, vz = gz + 1 < nz;
                const unsigned m = edge_mask(cm, dir_valid_mask(vx, vy, vz));
                const unsigned tc = (vx && vy && vz) ? tri_count(cm) : 0u;
                code[((size_t)gx * ny + gy) * nz + gz] = (unsigned short)(m | tc << 8);
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int code_verts(unsigned c) { return __popc(c & 0x7fu); }
__device__ __forceinline__ int code_tris(unsigned c) { return (int)((c >> 8) & 15u); }
// the scan's source: the codes -> voff[p], toff[p]
struct IsoSrc {
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
        for (int i = 0; i < SCAN_PER_THREAD; ++i) { nv += code_verts(c[i]); nt += code_tris(c[i]); }
    }
    __device__ __forceinline__ void store(long long p0, const items_t& c, int nv, int nt) const {
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) {
            if (p0 + i < N) { voff[p0 + i] = nv; toff[p0 + i] = nt; }
            nv += code_verts(c[i]); nt += code_tris(c[i]);
        }
    }
};

// One thread per grid point: the vertices it owns and the triangles of its cell.  Every read is inside the grid whatever ``code`` /
// ``voff`` / ``toff`` hold (validity comes from the coordinates), every write is checked against the capacity of the output buffers.
__global__ __launch_bounds__(256) void k_iso_emit(const float* __restrict__ u, int nx, int ny, int nz, double thr, const unsigned short* __restrict__ code,
                                                  const int* __restrict__ voff, const int* __restrict__ toff, int cap_v, int cap_t,
                                                  float* __restrict__ verts, int* __restrict__ ends, int* __restrict__ tris) {
    const unsigned N = (unsigned)nx * (unsigned)ny * (unsigned)nz, p = blockIdx.x * 256u + threadIdx.x;
    if (p >= N) return;
    const unsigned cd = code[p];
    if (cd == 0) return;
    const int z = (int)(p % (unsigned)nz), y = (int)((p / (unsigned)nz) % (unsigned)ny), x = (int)(p / (unsigned)nz / (unsigned)ny);
    const bool vx = x + 1 < nx, vy = y + 1 < ny, vz = z + 1 < nz;
    const unsigned sx = (unsigned)ny * (unsigned)nz, sy = (unsigned)nz;
    const unsigned m = cd & 0x7fu & dir_valid_mask(vx, vy, vz);
    if (m) {
        const float up = u[p];
        const bool pin = is_inside(up, thr);
        int vid = voff[p];
        for (int d = 1; d < 8; ++d) {
            if (!((m >> (d - 1)) & 1u)) continue;
            const int dx = d >> 2, dy = (d >> 1) & 1, dz = d & 1;
            const unsigned q = p + dx * sx + dy * sy + dz;
            const float uq = u[q];
            // a: the inside end, b: the outside end; w in fp64 as on the host
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
    if (((cd >> 8) & 15u) && vx && vy && vz) {
        unsigned cm = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) cm |= (unsigned)is_inside(u[p + (c >> 2) * sx + ((c >> 1) & 1) * sy + (c & 1)], thr) << c;
        int tid = toff[p];
        for (int t = 0; t < 6; ++t) {
            const unsigned char* tab = ISO_TRI[t][tet_case(cm, t)];
            for (int k = 0; k < 2 && tab[3 * k] != 0xff; ++k, ++tid) {
                if (tid < 0 || tid >= cap_t) continue;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const unsigned e = tab[3 * k + j], oc = e >> 3, d = e & 7u;
                    const unsigned o = p + (oc >> 2) * sx + ((oc >> 1) & 1u) * sy + (oc & 1u);          // the owner: a corner of this cell
                    tris[3 * (size_t)tid + j] = voff[o] + __popc(code[o] & ((1u << (d - 1)) - 1u));
                }
            }
        }
    }
}

static int iso_check_dims(int nx, int ny, int nz) {
    ES_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "iso-surface grid needs at least 2 points per axis");
    ES_REQUIRE((long long)nx * ny * nz < ISO_MAX_POINTS, "iso-surface grid has 2^31 points or more (int32 indices)");
    return ST_OK;
}

}  // namespace es

using namespace es;

extern "C" {

int64_t es_iso_scratch_bytes(int nx, int ny, int nz) {
    if (iso_check_dims(nx, ny, nz) != ST_OK) return -1;
    return iso_layout(nullptr, (long long)nx * ny * nz).bytes;
}

int es_iso_count(const float* field, int nx, int ny, int nz, double threshold, void* scratch, long long* totals, void* stream) {
    if (const int s = iso_check_dims(nx, ny, nz)) return s;
    ES_REQUIRE(field && scratch && totals, "es_iso_count needs field, scratch and totals");
    ES_SCRATCH_OK(scratch, "iso-surface scratch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const IsoScratch s = iso_layout(scratch, (long long)nx * ny * nz);
    const int tiles_z = (nz + ISO_TZ - 1) / ISO_TZ, tiles_y = (ny + ISO_TY - 1) / ISO_TY, tiles_x = (nx + ISO_TX - 1) / ISO_TX;
    const long long ntiles = (long long)tiles_z * tiles_y * tiles_x;
    const unsigned grid = (unsigned)(ntiles < (1ll << 20) ? ntiles : (1ll << 20));
    hipLaunchKernelGGL(k_iso_classify, dim3(grid), dim3(256), 0, st, field, nx, ny, nz, threshold, tiles_z, tiles_y, ntiles, s.code);
    scan_launch(IsoSrc{s.code, s.N, s.voff, s.toff}, s.nblk, s.bsum, s.boff, totals, st);
    return hip_last("es_iso_count");
}

int es_iso_emit(const float* field, int nx, int ny, int nz, double threshold, const void* scratch, long long n_verts, long long n_tris, float* verts,
                int* edge_ends, int* tris, void* stream) {
    if (const int s = iso_check_dims(nx, ny, nz)) return s;
    ES_REQUIRE(field && scratch, "es_iso_emit needs field and scratch");
    ES_SCRATCH_OK(scratch, "iso-surface scratch");
    ES_REQUIRE(n_verts >= 0 && n_tris >= 0 && n_verts < ISO_MAX_POINTS && n_tris < ISO_MAX_POINTS, "mesh does not fit int32 indices");
    if (n_verts == 0 && n_tris == 0) return ST_OK;
    ES_REQUIRE((n_verts == 0 || (verts && edge_ends)) && (n_tris == 0 || tris), "es_iso_emit needs verts, edge_ends and tris");
    const long long N = (long long)nx * ny * nz;
    const IsoScratch s = iso_layout(scratch, N);
    hipLaunchKernelGGL(k_iso_emit, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), field, nx, ny, nz, threshold,
                       s.code, s.voff, s.toff, (int)n_verts, (int)n_tris, verts, edge_ends, tris);
    return hip_last("es_iso_emit");
}

}  // extern "C"
