// Mesh export on the device (ABI v14): what the reference's demo does to an extracted mesh through Open3D before it writes its PLY files
// (trainer_endosurf.py:435-466 compute_vertex_normals, the painted normals, write_triangle_mesh), plus vertex clustering, as three
// primitives.  Numpy twins: endosurf_amd/meshing.py vertex_normals / cluster_vertices, endosurf_amd/data.py ply_body.  Contract: DESIGN.md 7e.
// (The fourth, the removal of degenerate and duplicate triangles, shares the component filter's compaction: mesh.hip.)
//
// Vertex normals (the fp64 sum of a vertex's un-normalised face cross products in the order of numpy's np.add.at loop -- corner 0 of
// every triangle in triangle order, then corner 1, then corner 2 --, normalised, rounded to fp32):
//   k_vn_count           count[v] = corners that name v (integer adds)
//   scan.h's three (VnSrc)   start[0 .. V] = the exclusive scan
//   (the caller orders the 3 T corners e = k T + t by (vertex, e): one stable sort; this is the fill)
//   k_vn_gather          one thread per vertex: its run of corners, added in that order
// Vertex clustering (a vertex's cell = floor((double(v) - origin) / cell) per axis, each in [-2^20, 2^20), as one 63-bit key):
//   k_cluster_keys       key[v], -1 for a cell out of range or a coordinate that is not finite
//   (the caller orders the vertices by (key, index): one stable sort)
//   scan.h's three (ClusterSrc)   cell number of each place of that order, first place of each cell; totals: cells, keys of -1
//   k_cluster_sizes      the largest member count (integer maximum)
//   k_cluster_emit       one thread per cell: the fp64 sums of its members' positions and attribute channels in ascending old index,
//                        divided by the member count, rounded to fp32; vertex_cluster[old] = cell
//   k_cluster_remap      triangle corners -> cell numbers
// PLY body (binary_little_endian 1.0):
//   k_ply_pack           one thread per record: a vertex (x y z [nx ny nz] [r g b]) or a face (3, a, b, c); a 4-byte value that does
//                        not start on a 4-byte boundary is stored byte by byte
//
// Integer atomics only (counts, a maximum): no result depends on their order.  No float atomics: every sum has one thread that adds
// in index order, so the results are bit-identical from call to call.  Every product of the cross product and of the length is rounded on
// its own (mul_rn below); the cell quotient and the mean have no product that feeds a sum.  No workgroup waits for another; every device loop is bounded
// by an argument or by a range read from the scratch and clamped to it; every index read from a buffer is range-checked before it
// addresses memory, whatever the scratch holds.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"
#include "scan.h"

namespace es {

constexpr long long EXPORT_MAX = 1ll << 31;                  // int32 indices
constexpr int CLUSTER_MAX_ATTRS = 8;
constexpr double CLUSTER_HALF = 1048576.0;                   // cell coordinates lie in [-2^20, 2^20)

__device__ __forceinline__ bool idx_ok(long long i, long long n) { return i >= 0 && i < n; }

// ---- vertex normals ---------------------------------------------------------------------------------------------------------------------

struct VnScratch {
    int* count;              // [V + 1] corners per vertex
    int* start;              // [V + 1] first corner of each vertex in the sorted order; start[V] = counted corners
    int* bsum;               // [nblk][2]
    int* boff;               // [nblk][2]
    long long nblk, bytes;
};
static VnScratch vn_layout(const void* scratch, long long V) {          // a null scratch measures only
    Carver c(scratch);
    VnScratch s;
    s.nblk = scan_chunks(V + 1);
    s.count = c.take<int>(V + 1);
    s.start = c.take<int>(V + 1);
    s.bsum = c.take<int>(2 * s.nblk);
    s.boff = c.take<int>(2 * s.nblk);
    s.bytes = c.off;
    return s;
}

// corner_vertex[k T + t] = corner k of triangle t (the sort key), V for an index that is no vertex; count[] of the others
__global__ __launch_bounds__(256) void k_vn_count(const int* __restrict__ tris, int V, long long T, int* __restrict__ corner_vertex, int* count) {
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < 3 * T; e += gridDim.x * 256ll) {
        const long long k = e / T, t = e - k * T;
        const int v = tris[3 * t + k];
        const bool ok = (unsigned)v < (unsigned)V;
        corner_vertex[e] = ok ? v : V;
        if (ok) atomicAdd(count + v, 1);
    }
}

// the scan's source: count[0 .. n) -> start[] (one sequence; the second stays 0)
struct VnSrc {
    using sum_t = int;
    using items_t = int[SCAN_PER_THREAD];
    const int* count;
    long long n;
    int* start;
    __device__ __forceinline__ void load(long long i0, items_t& c, int& s, int& none) const {
        s = 0; none = 0;
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) { c[i] = i0 + i < n ? count[i0 + i] : 0; s += c[i]; }
    }
    __device__ __forceinline__ void store(long long i0, const items_t& c, int s, int) const {
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) {
            if (i0 + i < n) start[i0 + i] = s;
            s += c[i];
        }
    }
};

// a b rounded on its own.  The library is built with -ffp-contract=fast, under which the compiler fuses a product into the sum that
// uses it whatever a contraction pragma says (checked in the assembly); an explicit fma with a zero addend is a product it leaves alone.
// (a b = -0 comes out as +0: the sums below start from +0, which absorbs either.)
__device__ __forceinline__ double mul_rn(double a, double b) { return __builtin_fma(a, b, 0.0); }

// (p1 - p0) x (p2 - p0) in fp64, every product and difference rounded on its own, as numpy's np.cross
__device__ __forceinline__ void face_cross(const float* __restrict__ verts, int a, int b, int c, double (&n)[3]) {
    double p[3], q[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double o = (double)verts[3 * (size_t)a + j];
        p[j] = (double)verts[3 * (size_t)b + j] - o;
        q[j] = (double)verts[3 * (size_t)c + j] - o;
    }
    n[0] = mul_rn(p[1], q[2]) - mul_rn(p[2], q[1]);
    n[1] = mul_rn(p[2], q[0]) - mul_rn(p[0], q[2]);
    n[2] = mul_rn(p[0], q[1]) - mul_rn(p[1], q[0]);
}

__global__ __launch_bounds__(256) void k_vn_gather(const float* __restrict__ verts, const int* __restrict__ tris, int V, long long T,
                                                   const int* __restrict__ start, const long long* __restrict__ order, float* __restrict__ normals) {
    for (long long v = blockIdx.x * 256ll + threadIdx.x; v < V; v += gridDim.x * 256ll) {
        long long s = start[v], e = start[v + 1];
        s = s < 0 ? 0 : s;
        e = e > 3 * T ? 3 * T : e;
        double acc[3] = {0.0, 0.0, 0.0};
        for (long long i = s; i < e; ++i) {
            const long long c = order[i];
            if (!idx_ok(c, 3 * T)) continue;
            const long long t = c % T;
            const int a = tris[3 * t], b = tris[3 * t + 1], d = tris[3 * t + 2];
            if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)d >= (unsigned)V) continue;
            double n[3];
            face_cross(verts, a, b, d, n);
            acc[0] += n[0]; acc[1] += n[1]; acc[2] += n[2];
        }
        {
            const double len = sqrt((mul_rn(acc[0], acc[0]) + mul_rn(acc[1], acc[1])) + mul_rn(acc[2], acc[2]));
            const double den = (len > 1e-30 || len != len) ? len : 1e-30;          // numpy's maximum(len, 1e-30): a NaN stays
            normals[3 * v] = (float)(acc[0] / den);
            normals[3 * v + 1] = (float)(acc[1] / den);
            normals[3 * v + 2] = (float)(acc[2] / den);
        }
    }
}

// ---- vertex clustering -------------------------------------------------------------------------------------------------------------------

struct ClusterScratch {
    int* cid;                // [V] cell number of each place of the sorted order
    int* start;              // [V + 1] first place of each cell; start[cells] = V
    int* bsum;               // [nblk][2]
    int* boff;               // [nblk][2]
    long long nblk, bytes;
};
static ClusterScratch cluster_layout(const void* scratch, long long V) {          // a null scratch measures only
    Carver c(scratch);
    ClusterScratch s;
    s.nblk = V > 0 ? scan_chunks(V) : 1;
    s.cid = c.take<int>(V);
    s.start = c.take<int>(V + 1);
    s.bsum = c.take<int>(2 * s.nblk);
    s.boff = c.take<int>(2 * s.nblk);
    s.bytes = c.off;
    return s;
}

// floor((x - origin) / cell) + 2^20 when it lies in [0, 2^21), else -1
__device__ __forceinline__ long long cluster_coord(float x, double origin, double cell) {
    const double d = (double)x - origin;
    const double f = floor(d / cell);
    if (!(f >= -CLUSTER_HALF && f < CLUSTER_HALF)) return -1;
    return (long long)f + (long long)CLUSTER_HALF;
}

__global__ __launch_bounds__(256) void k_cluster_keys(const float* __restrict__ verts, long long V, double cell, double ox, double oy, double oz,
                                                      long long* __restrict__ key) {
    for (long long v = blockIdx.x * 256ll + threadIdx.x; v < V; v += gridDim.x * 256ll) {
        const long long ix = cluster_coord(verts[3 * v], ox, cell), iy = cluster_coord(verts[3 * v + 1], oy, cell),
                        iz = cluster_coord(verts[3 * v + 2], oz, cell);
        key[v] = (ix < 0 || iy < 0 || iz < 0) ? -1 : ((ix << 42) | (iy << 21) | iz);
    }
}

// the scan's source: sequence 0 = "this place opens a cell", sequence 1 = "this key is -1" -> cid[], start[]
struct ClusterSrc {
    using sum_t = int;
    struct items_t { unsigned char head[SCAN_PER_THREAD]; };
    const long long* key;          // sorted
    long long V;
    int *cid, *start;
    __device__ __forceinline__ void load(long long i0, items_t& c, int& nh, int& nbad) const {
        nh = 0; nbad = 0;
        long long prev = i0 > 0 && i0 - 1 < V ? key[i0 - 1] : 0;
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) {
            const long long p = i0 + i;
            const long long k = p < V ? key[p] : 0;
            c.head[i] = p < V && (p == 0 || k != prev) ? 1 : 0;
            nh += c.head[i];
            nbad += p < V && k < 0 ? 1 : 0;
            prev = k;
        }
    }
    __device__ __forceinline__ void store(long long i0, const items_t& c, int nh, int) const {
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) {
            const long long p = i0 + i;
            if (p >= V) break;
            nh += c.head[i];                                          // cells opened up to and including this place, >= 1
            const int id = nh - 1;
            cid[p] = id;
            if (c.head[i] && idx_ok(id, V)) start[id] = (int)p;
            if (p == V - 1 && idx_ok(id + 1, V + 1)) start[id + 1] = (int)V;
        }
    }
};

__global__ __launch_bounds__(256) void k_cluster_sizes(const int* __restrict__ start, long long V, unsigned long long* totals) {
    __shared__ int part[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long cells = (long long)totals[0] < V ? (long long)totals[0] : V;
    int mx = 0;
    for (long long c = blockIdx.x * 256ll + threadIdx.x; c < cells; c += gridDim.x * 256ll) mx = max(mx, start[c + 1] - start[c]);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) part[wv] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int m = max(max(part[0], part[1]), max(part[2], part[3]));
        if (m > 0) atomicMax(totals + 2, (unsigned long long)m);
    }
}

__global__ __launch_bounds__(256) void k_cluster_emit(const float* __restrict__ verts, const float* __restrict__ attrs, int C, long long V,
                                                      const long long* __restrict__ order, const int* __restrict__ start, long long cells,
                                                      float* __restrict__ verts_out, float* __restrict__ attrs_out, int* __restrict__ vertex_cluster) {
    for (long long c = blockIdx.x * 256ll + threadIdx.x; c < cells; c += gridDim.x * 256ll) {
        long long s = start[c], e = start[c + 1];
        s = s < 0 ? 0 : s;
        e = e > V ? V : e;
        double acc[3 + CLUSTER_MAX_ATTRS];
#pragma unroll
        for (int j = 0; j < 3 + CLUSTER_MAX_ATTRS; ++j) acc[j] = 0.0;
        long long n = 0;
        for (long long i = s; i < e; ++i) {
            const long long v = order[i];
            if (!idx_ok(v, V)) continue;
            ++n;
            acc[0] += (double)verts[3 * v]; acc[1] += (double)verts[3 * v + 1]; acc[2] += (double)verts[3 * v + 2];
#pragma unroll
            for (int j = 0; j < CLUSTER_MAX_ATTRS; ++j)
                if (j < C) acc[3 + j] += (double)attrs[(size_t)C * v + j];
            vertex_cluster[v] = (int)c;
        }
        const double cnt = (double)(n > 0 ? n : 1);
        verts_out[3 * c] = (float)(acc[0] / cnt); verts_out[3 * c + 1] = (float)(acc[1] / cnt); verts_out[3 * c + 2] = (float)(acc[2] / cnt);
#pragma unroll
        for (int j = 0; j < CLUSTER_MAX_ATTRS; ++j)
            if (j < C) attrs_out[(size_t)C * c + j] = (float)(acc[3 + j] / cnt);
    }
}

__global__ __launch_bounds__(256) void k_cluster_remap(const int* __restrict__ tris, long long V, long long T, const int* __restrict__ vertex_cluster,
                                                       int* __restrict__ tris_out) {
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < 3 * T; e += gridDim.x * 256ll) {
        const int v = tris[e];
        tris_out[e] = idx_ok(v, V) ? vertex_cluster[v] : -1;
    }
}

// ---- PLY body ------------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void put4(unsigned char* p, unsigned int w) {
    if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<unsigned int*>(p) = w;
    } else {
        p[0] = (unsigned char)(w & 255u); p[1] = (unsigned char)((w >> 8) & 255u);
        p[2] = (unsigned char)((w >> 16) & 255u); p[3] = (unsigned char)(w >> 24);
    }
}
// data.to8b: 255 clip(x, 0, 1) in fp32, truncated; NaN gives 0
__device__ __forceinline__ unsigned char ply_8b(float x) {
    const float c = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;          // (NaN fails x > 0)
    return (unsigned char)(int)(255.f * c);
}

__global__ __launch_bounds__(256) void k_ply_pack(const float* __restrict__ verts, const float* __restrict__ normals, const float* __restrict__ colors,
                                                  const int* __restrict__ tris, long long V, long long T, int vbytes, unsigned char* __restrict__ out) {
    for (long long r = blockIdx.x * 256ll + threadIdx.x; r < V + T; r += gridDim.x * 256ll) {
        if (r < V) {
            unsigned char* p = out + r * vbytes;
#pragma unroll
            for (int j = 0; j < 3; ++j) put4(p + 4 * j, __float_as_uint(verts[3 * r + j]));
            p += 12;
            if (normals) {
#pragma unroll
                for (int j = 0; j < 3; ++j) put4(p + 4 * j, __float_as_uint(normals[3 * r + j]));
                p += 12;
            }
            if (colors) {
#pragma unroll
                for (int j = 0; j < 3; ++j) p[j] = ply_8b(colors[3 * r + j]);
            }
        } else {
            const long long t = r - V;
            unsigned char* p = out + V * vbytes + 13 * t;
            p[0] = 3;
#pragma unroll
            for (int j = 0; j < 3; ++j) put4(p + 1 + 4 * j, (unsigned int)tris[3 * t + j]);
        }
    }
}

static int export_check(long long V, long long T, const char* what) {
    if (!(V >= 0 && T >= 0)) return fail(ST_BAD_ARG, what, "negative vertex or triangle count");
    if (!(V < EXPORT_MAX && T < EXPORT_MAX)) return fail(ST_BAD_ARG, what, "2^31 vertices or triangles or more (indices are int32)");
    return ST_OK;
}
static inline int ply_vertex_bytes(bool normals, bool colors) { return 12 + (normals ? 12 : 0) + (colors ? 3 : 0); }

}  // namespace es

using namespace es;

extern "C" {

int64_t es_vn_scratch_bytes(long long n_verts) {
    if (export_check(n_verts, 0, "es_vn_scratch_bytes") != ST_OK) return -1;
    return vn_layout(nullptr, n_verts).bytes;
}

int es_vn_count(const int* tris, long long V, long long T, int* corner_vertex, void* scratch, void* stream) {
    if (const int s = export_check(V, T, "es_vn_count")) return s;
    ES_REQUIRE(T == 0 || (tris && corner_vertex), "es_vn_count needs tris and corner_vertex");
    ES_SCRATCH_OK(scratch, "normals scratch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const VnScratch s = vn_layout(scratch, V);
    ES_HIP(hipMemsetAsync(s.count, 0, 4 * (V + 1), st));
    if (T > 0) hipLaunchKernelGGL(k_vn_count, dim3(grid_for(3 * T)), dim3(256), 0, st, tris, (int)V, T, corner_vertex, s.count);
    scan_launch(VnSrc{s.count, V + 1, s.start}, s.nblk, s.bsum, s.boff, nullptr, st);
    return hip_last("es_vn_count");
}

int es_vn_gather(const float* verts, const int* tris, long long V, long long T, const long long* order, const void* scratch, float* normals,
                 void* stream) {
    if (const int s = export_check(V, T, "es_vn_gather")) return s;
    if (V == 0) return ST_OK;
    ES_REQUIRE(verts && normals && (T == 0 || (tris && order)), "es_vn_gather needs verts, normals, tris and order");
    ES_SCRATCH_OK(scratch, "normals scratch");
    const VnScratch s = vn_layout(scratch, V);
    hipLaunchKernelGGL(k_vn_gather, dim3(grid_for(V)), dim3(256), 0, static_cast<hipStream_t>(stream), verts, tris, (int)V, T, s.start, order, normals);
    return hip_last("es_vn_gather");
}

int64_t es_cluster_scratch_bytes(long long n_verts) {
    if (export_check(n_verts, 0, "es_cluster_scratch_bytes") != ST_OK) return -1;
    return cluster_layout(nullptr, n_verts).bytes;
}

int es_cluster_keys(const float* verts, long long V, double cell, double ox, double oy, double oz, long long* key, void* stream) {
    if (const int s = export_check(V, 0, "es_cluster_keys")) return s;
    ES_REQUIRE(cell > 0.0 && std::isfinite(cell) && std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz),
               "es_cluster_keys: cell must be finite and positive, origin finite");
    if (V == 0) return ST_OK;
    ES_REQUIRE(verts && key, "es_cluster_keys needs verts and key");
    hipLaunchKernelGGL(k_cluster_keys, dim3(grid_for(V)), dim3(256), 0, static_cast<hipStream_t>(stream), verts, V, cell, ox, oy, oz, key);
    return hip_last("es_cluster_keys");
}

int es_cluster_count(const long long* sorted_key, long long V, void* scratch, long long* totals, void* stream) {
    if (const int s = export_check(V, 0, "es_cluster_count")) return s;
    ES_REQUIRE(totals && (V == 0 || sorted_key), "es_cluster_count needs sorted_key and totals");
    ES_SCRATCH_OK(scratch, "cluster scratch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ClusterScratch s = cluster_layout(scratch, V);
    ES_HIP(hipMemsetAsync(totals, 0, 3 * sizeof(long long), st));
    if (V == 0) return ST_OK;
    scan_launch(ClusterSrc{sorted_key, V, s.cid, s.start}, s.nblk, s.bsum, s.boff, totals, st);
    hipLaunchKernelGGL(k_cluster_sizes, dim3(grid_for(V)), dim3(256), 0, st, s.start, V, reinterpret_cast<unsigned long long*>(totals));
    return hip_last("es_cluster_count");
}

int es_cluster_emit(const float* verts, const float* attrs, int n_attrs, long long V, const long long* order, const void* scratch, long long n_cells,
                    long long n_out_of_range, float* verts_out, float* attrs_out, int* vertex_cluster, void* stream) {
    if (const int s = export_check(V, 0, "es_cluster_emit")) return s;
    ES_REQUIRE(n_attrs >= 0 && n_attrs <= CLUSTER_MAX_ATTRS, "es_cluster_emit: at most 8 attribute channels");
    ES_REQUIRE(n_out_of_range == 0, "cluster: a vertex's cell coordinate lies outside [-2^20, 2^20) (or the vertex is not finite): use a larger cell");
    ES_REQUIRE(n_cells >= 0 && n_cells <= V && (n_cells > 0) == (V > 0), "es_cluster_emit: cell count outside 1..V");
    ES_SCRATCH_OK(scratch, "cluster scratch");
    if (V == 0) return ST_OK;
    ES_REQUIRE(verts && order && verts_out && vertex_cluster && (n_attrs == 0 || (attrs && attrs_out)),
               "es_cluster_emit needs verts, order, verts_out, vertex_cluster and attrs / attrs_out with channels");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ClusterScratch s = cluster_layout(scratch, V);
    ES_HIP(hipMemsetAsync(vertex_cluster, 0, 4 * V, st));
    hipLaunchKernelGGL(k_cluster_emit, dim3(grid_for(n_cells)), dim3(256), 0, st, verts, attrs, n_attrs, V, order, s.start, n_cells, verts_out,
                       attrs_out, vertex_cluster);
    return hip_last("es_cluster_emit");
}

int es_cluster_remap(const int* tris, long long V, long long T, const int* vertex_cluster, int* tris_out, void* stream) {
    if (const int s = export_check(V, T, "es_cluster_remap")) return s;
    if (T == 0) return ST_OK;
    ES_REQUIRE(tris && tris_out && vertex_cluster, "es_cluster_remap needs tris, vertex_cluster and tris_out");
    hipLaunchKernelGGL(k_cluster_remap, dim3(grid_for(3 * T)), dim3(256), 0, static_cast<hipStream_t>(stream), tris, V, T, vertex_cluster, tris_out);
    return hip_last("es_cluster_remap");
}

int64_t es_ply_body_bytes(long long V, long long T, int has_normals, int has_colors) {
    if (export_check(V, T, "es_ply_body_bytes") != ST_OK) return -1;
    return V * ply_vertex_bytes(has_normals != 0, has_colors != 0) + 13 * T;
}

int es_ply_pack(const float* verts, const float* normals, const float* colors, const int* tris, long long V, long long T, unsigned char* out,
                void* stream) {
    if (const int s = export_check(V, T, "es_ply_pack")) return s;
    if (V == 0 && T == 0) return ST_OK;
    ES_REQUIRE(out && (V == 0 || verts) && (T == 0 || tris), "es_ply_pack needs verts, tris and out");
    hipLaunchKernelGGL(k_ply_pack, dim3(grid_for(V + T)), dim3(256), 0, static_cast<hipStream_t>(stream), verts, normals, colors, tris, V, T,
                       ply_vertex_bytes(normals != nullptr, colors != nullptr), out);
    return hip_last("es_ply_pack");
}

}  // extern "C"
