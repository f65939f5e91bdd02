// Mesh clean-up and geometric error on the device (ABI v11): what the reference's demo does to an extracted mesh through Open3D on the
// host (trainer_endosurf.py:436-447 cluster_connected_triangles + remove_triangles_by_mask, :418 / :452ff point-cloud distance), as two
// primitives.  Numpy twins: endosurf_amd/meshing.py mesh_components / keep_components / nearest.  Contract: DESIGN.md 7b.
//
// Connected components (vertex connectivity; label = the smallest vertex index of the component):
//   k_mesh_init          parent[v] = v
//   k_mesh_hook          per non-degenerate triangle: m = min of its corners' parents; parent[r] = min(parent[r], m) for the others
//   k_mesh_jump          parent[v] = the ancestor reached by at most MESH_WALK links; a pass shortens every path 32-fold, so
//                        ceil(log2 V / 5) passes (the host launches exactly that many) leave the forest flat
//   k_mesh_label         triangle_label, component_triangles (one integer add per distinct label of a wave), the degenerate count
//   k_mesh_stats         components with a triangle, the largest triangle count
//   k_mesh_keep_flags    triangle kept / vertex used bytes (the fp64 comparison of the reference's numpy line)
//   scan.h's three (MeshKeepSrc) / k_mesh_keep_emit   stable compaction: the exclusive scan of the two flag arrays, then the copy
// Clean-up for export (ABI v14; twin: meshing.mesh_clean; contract: DESIGN.md 7e): a triangle with a repeated index goes, and of the
// triangles with the same three vertex indices (any rotation, either orientation) the one with the smallest triangle index stays:
//   k_mesh_clean_keys    the sorted corners (a < b < c) of a triangle as two keys: a (32 bits) and b 2^31 + c (62 bits) -- 93 bits in
//                        all, so no vertex index below 2^31 is folded; a degenerate triangle gets the largest keys
//   (the caller orders the triangles by (a, b, c, triangle index): two stable sorts)
//   k_mesh_clean_flags   in that order a triangle whose predecessor has the same corners is a duplicate; tflag / vflag bytes as above
//   scan.h's three (MeshKeepSrc) / k_mesh_keep_emit   the same compaction as the component filter's
// Nearest neighbour (exact; fp32 squared distance (dx dx + dy dy) + dz dz without contraction, ties to the smallest index):
//   k_nn_bbox / k_nn_header     box of the finite points -> the grid (at most one cell per four finite points, at least one per axis)
//   k_nn_count / scan.h's three (NnSrc) / k_nn_fill   counting sort of the points by cell (z fastest) into (x, y, z, index) records
//   k_nn_query           one thread per query: Chebyshev shells around the query's (clamped) cell until the stop rule proves the rest away
//
// Integer atomics, and why no result depends on their order: atomicMin on parent[] (a round's outcome may differ from call to call,
// the fixed point -- every vertex at the smallest index of its component -- cannot), atomicOr on the round's ``changed`` word,
// atomicAdd of counts (component_triangles, the totals, the cell histogram), atomicMax of the largest count, and atomicAdd on a
// cell's fill cursor (it orders the records inside a cell, which the query's (distance, index) minimum does not see).  No float
// atomics.  No workgroup waits for another one; the loop over rounds is on the host; every device loop is bounded by an argument
// or a constant, and every index read from a buffer is range-checked before it addresses memory, whatever the scratch holds.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"
#include "nn_grid.h"
#include "scan.h"

namespace es {

constexpr int MESH_WALK = 32;                                // links one thread of k_mesh_jump follows

static inline int mesh_jump_passes(long long V) {
    int bits = 0;
    while ((1ll << bits) < V) ++bits;                        // ceil(log2 V)
    return bits < 5 ? 1 : (bits + 4) / 5;
}

struct MeshScratch {
    int* parent;             // [V] the hook-and-jump forest; flat between rounds
    int* voff;               // [V] exclusive scan of vflag
    int* toff;               // [T] exclusive scan of tflag
    int* bsum;               // [nblk][2] used vertices / kept triangles of a chunk
    int* boff;               // [nblk][2] exclusive scan of bsum
    unsigned char* vflag;    // [V] vertex survives the filter
    unsigned char* tflag;    // [T] triangle survives the filter
    long long nblk, bytes;
};
static MeshScratch mesh_layout(const void* scratch, long long V, long long T) {          // a null scratch measures only
    Carver c(scratch);
    MeshScratch s;
    s.nblk = V > 0 || T > 0 ? scan_chunks(V > T ? V : T) : 1;
    s.parent = c.take<int>(V);
    s.voff = c.take<int>(V);
    s.toff = c.take<int>(T);
    s.bsum = c.take<int>(2 * s.nblk);
    s.boff = c.take<int>(2 * s.nblk);
    s.vflag = c.take<unsigned char>(V);
    s.tflag = c.take<unsigned char>(T);
    c.take<char>(16);          // (unused: es_mesh_scratch_bytes has always counted it)
    s.bytes = c.off;
    return s;
}

// a triangle takes part: three different corners, all of them vertices
__device__ __forceinline__ bool tri_load(const int* __restrict__ tris, long long t, int V, int& a, int& b, int& c) {
    a = tris[3 * t]; b = tris[3 * t + 1]; c = tris[3 * t + 2];
    return in_range(a, V) && in_range(b, V) && in_range(c, V) && a != b && b != c && a != c;
}
__device__ __forceinline__ int min3(int a, int b, int c) { return min(a, min(b, c)); }

__global__ __launch_bounds__(256) void k_mesh_init(int* __restrict__ parent, int V) {
    for (long long v = blockIdx.x * 256ll + threadIdx.x; v < V; v += gridDim.x * 256ll) parent[v] = (int)v;
}

__global__ __launch_bounds__(256) void k_mesh_hook(const int* __restrict__ tris, int V, long long T, int* parent, int* changed) {
    bool ch = false;
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < T; t += gridDim.x * 256ll) {
        int a, b, c;
        if (!tri_load(tris, t, V, a, b, c)) continue;
        const int ra = parent[a], rb = parent[b], rc = parent[c];
        if (!in_range(ra, V) || !in_range(rb, V) || !in_range(rc, V)) continue;          // (a forest es_mesh_cc_begin did not make)
        const int m = min3(ra, rb, rc);
        if (ra != m) { atomicMin(parent + ra, m); ch = true; }
        if (rb != m) { atomicMin(parent + rb, m); ch = true; }
        if (rc != m) { atomicMin(parent + rc, m); ch = true; }
    }
    if (__syncthreads_or(ch) && threadIdx.x == 0) atomicOr(changed, 1);
}

// parent[x] <= x always, so a path has fewer than V links.  A thread reads links other threads are shortening: whatever it reads is
// an ancestor at least as far as the link it replaces, so MESH_WALK reads climb MESH_WALK old links or reach the root, and after the
// pass every path is at most ceil(old length / MESH_WALK) long.
__global__ __launch_bounds__(256) void k_mesh_jump(int* parent, int V) {
    for (long long v = blockIdx.x * 256ll + threadIdx.x; v < V; v += gridDim.x * 256ll) {
        int p = parent[v];
        if (p == (int)v || !in_range(p, V)) continue;
        for (int i = 0; i < MESH_WALK; ++i) {
            const int pp = parent[p];
            if (pp == p || !in_range(pp, V)) break;
            p = pp;
        }
        parent[v] = p;
    }
}

__global__ __launch_bounds__(256) void k_mesh_label(const int* __restrict__ tris, int V, long long T, const int* __restrict__ parent,
                                                    int* __restrict__ triangle_label, int* component_triangles, unsigned long long* totals) {
    __shared__ int part[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int n_deg = 0;
    for (long long base = blockIdx.x * 256ll; base < T; base += gridDim.x * 256ll) {          // (wave-uniform trip count)
        const long long t = base + threadIdx.x;
        int lab = -1;
        if (t < T) {
            int a, b, c;
            if (tri_load(tris, t, V, a, b, c)) lab = parent[a];
            if (!in_range(lab, V)) lab = -1;
            triangle_label[t] = lab;
            n_deg += lab < 0 ? 1 : 0;
        }
        // one add per distinct label of the wave; every turn retires its leader, so there are at most 64 turns
        unsigned long long todo = __ballot(lab >= 0);
        for (int turn = 0; turn < 64 && todo; ++turn) {
            const int leader = __ffsll((long long)todo) - 1;
            const int l0 = __shfl(lab, leader, 64);
            const unsigned long long same = __ballot(lab == l0) & todo;
            if (lane == leader) atomicAdd(component_triangles + l0, (int)__popcll(same));
            todo &= ~same;
        }
    }
    n_deg = wscan_add(n_deg, lane);
    if (lane == 63) part[wv] = n_deg;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = part[0] + part[1] + part[2] + part[3];
        if (n) atomicAdd(totals + 2, (unsigned long long)n);
    }
}

__global__ __launch_bounds__(256) void k_mesh_stats(const int* __restrict__ component_triangles, int V, unsigned long long* totals) {
    __shared__ int part[4][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int n = 0, mx = 0;
    for (long long v = blockIdx.x * 256ll + threadIdx.x; v < V; v += gridDim.x * 256ll) {
        const int c = component_triangles[v];
        n += c > 0 ? 1 : 0;
        mx = max(mx, c);
    }
    n = wscan_add(n, lane);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if (lane == 63) { part[wv][0] = n; part[wv][1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int ns = part[0][0] + part[1][0] + part[2][0] + part[3][0];
        const int ms = max(max(part[0][1], part[1][1]), max(part[2][1], part[3][1]));
        if (ns) atomicAdd(totals, (unsigned long long)ns);
        if (ms) atomicMax(totals + 1, (unsigned long long)ms);
    }
}

// kept = not degenerate and not (count of its component < keep_ratio x the largest count), in fp64 like numpy's int64 < float64
__global__ __launch_bounds__(256) void k_mesh_keep_flags(const int* __restrict__ tris, int V, long long T, const int* __restrict__ triangle_label,
                                                         const int* __restrict__ component_triangles, double limit, int compact,
                                                         unsigned char* __restrict__ tflag, unsigned char* vflag) {
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < T; t += gridDim.x * 256ll) {
        int a, b, c;
        const bool ok = tri_load(tris, t, V, a, b, c);
        const int lab = triangle_label[t];
        const bool keep = ok && in_range(lab, V) && !((double)component_triangles[lab] < limit);
        tflag[t] = keep ? 1 : 0;
        if (keep && compact) { vflag[a] = 1; vflag[b] = 1; vflag[c] = 1; }          // (every writer stores the same byte)
    }
}

// 16 consecutive flags of a thread (0 beyond n)
__device__ __forceinline__ void flags_load(const unsigned char* __restrict__ f, long long n, long long i0, unsigned char (&c)[SCAN_PER_THREAD]) {
    if (i0 + SCAN_PER_THREAD <= n) {
        const uint4 w = *reinterpret_cast<const uint4*>(f + i0);          // 16-byte aligned: f is, i0 a multiple of 16
        __builtin_memcpy(c, &w, sizeof(c));
    } else {
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) c[i] = i0 + i < n ? f[i0 + i] : (unsigned char)0;
    }
}
// the scan's source: the two flag arrays, of different length -> voff[i], toff[i]
struct MeshKeepSrc {
    using sum_t = int;
    struct items_t { unsigned char v[SCAN_PER_THREAD], t[SCAN_PER_THREAD]; };
    const unsigned char *vflag, *tflag;
    long long V, T;
    int *voff, *toff;
    __device__ __forceinline__ void load(long long i0, items_t& c, int& nv, int& nt) const {
        flags_load(vflag, V, i0, c.v);
        flags_load(tflag, T, i0, c.t);
        nv = 0; nt = 0;
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) { nv += c.v[i] ? 1 : 0; nt += c.t[i] ? 1 : 0; }
    }
    __device__ __forceinline__ void store(long long i0, const items_t& c, int nv, int nt) const {
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD; ++i) {
            if (i0 + i < V) voff[i0 + i] = nv;
            if (i0 + i < T) toff[i0 + i] = nt;
            nv += c.v[i] ? 1 : 0; nt += c.t[i] ? 1 : 0;
        }
    }
};

// Every write is checked against the capacity of its output buffer, every index against V.
__global__ __launch_bounds__(256) void k_mesh_keep_emit(const float* __restrict__ verts, const int* __restrict__ tris, int V, long long T,
                                                        const int* __restrict__ voff, const int* __restrict__ toff,
                                                        const unsigned char* __restrict__ vflag, const unsigned char* __restrict__ tflag, int cap_v,
                                                        int cap_t, float* __restrict__ verts_out, int* __restrict__ tris_out,
                                                        long long* __restrict__ vertex_map) {
    const long long n = V > T ? V : T;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
        if (i < V && vflag[i]) {
            const int o = voff[i];
            if (in_range(o, cap_v)) {
                if (verts_out) {
                    verts_out[3 * (size_t)o] = verts[3 * i]; verts_out[3 * (size_t)o + 1] = verts[3 * i + 1]; verts_out[3 * (size_t)o + 2] = verts[3 * i + 2];
                }
                if (vertex_map) vertex_map[o] = i;
            }
        }
        if (i < T && tflag[i]) {
            const int o = toff[i];
            if (in_range(o, cap_t)) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int v = tris[3 * i + j];
                    tris_out[3 * (size_t)o + j] = in_range(v, V) ? voff[v] : -1;
                }
            }
        }
    }
}

// a < b < c of three different indices
__device__ __forceinline__ void sort3(int& a, int& b, int& c) {
    int t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
}

__global__ __launch_bounds__(256) void k_mesh_clean_keys(const int* __restrict__ tris, int V, long long T, int* __restrict__ key_hi,
                                                         long long* __restrict__ key_lo) {
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < T; t += gridDim.x * 256ll) {
        int a, b, c;
        if (tri_load(tris, t, V, a, b, c)) {
            sort3(a, b, c);
            key_hi[t] = a;
            key_lo[t] = ((long long)b << 31) | (long long)c;
        } else {
            key_hi[t] = 0x7fffffff;
            key_lo[t] = 0x7fffffffffffffffll;
        }
    }
}

// order[i] = the triangle at place i of the order by (corners, triangle index).  tflag is zeroed before the launch, so an ``order``
// that is no permutation drops triangles and cannot make a write go astray.
__global__ __launch_bounds__(256) void k_mesh_clean_flags(const int* __restrict__ tris, int V, long long T, const long long* __restrict__ order,
                                                          int compact, unsigned char* __restrict__ tflag, unsigned char* vflag,
                                                          unsigned long long* totals) {
    __shared__ int part[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int n_deg = 0;
    for (long long base = blockIdx.x * 256ll; base < T; base += gridDim.x * 256ll) {          // (wave-uniform trip count)
        const long long i = base + threadIdx.x;
        if (i >= T) continue;
        const long long t = order[i];
        if (t < 0 || t >= T) continue;
        int a, b, c;
        if (!tri_load(tris, t, V, a, b, c)) { ++n_deg; continue; }
        sort3(a, b, c);
        bool dup = false;
        if (i > 0) {
            const long long p = order[i - 1];
            int pa, pb, pc;
            if (p >= 0 && p < T && tri_load(tris, p, V, pa, pb, pc)) {
                sort3(pa, pb, pc);
                dup = pa == a && pb == b && pc == c;
            }
        }
        if (dup) continue;
        tflag[t] = 1;
        if (compact) { vflag[a] = 1; vflag[b] = 1; vflag[c] = 1; }          // (every writer stores the same byte)
    }
    n_deg = wscan_add(n_deg, lane);
    if (lane == 63) part[wv] = n_deg;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = part[0] + part[1] + part[2] + part[3];
        if (n) atomicAdd(totals + 2, (unsigned long long)n);
    }
}

// ---- nearest neighbour ----------------------------------------------------------------------------------------------------------------

// (the header, the scratch layout and the cell function: nn_grid.h, shared with csrc/surface.hip)

__global__ __launch_bounds__(256) void k_nn_bbox(const float* __restrict__ pts, long long P, float* __restrict__ part) {
    __shared__ float red[4][6];
    __shared__ int cnt[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int n = 0;
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < P; p += gridDim.x * 256ll) {
        const float x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
        if (!finite3(x, y, z)) continue;
        lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
        hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
        ++n;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64)); }
        n += __shfl_xor(n, o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[wv][a] = lo[a]; red[wv][3 + a] = hi[a]; }
        cnt[wv] = n;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        part[8 * (size_t)blockIdx.x + a] = fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]));
        part[8 * (size_t)blockIdx.x + 3 + a] = fmaxf(fmaxf(red[0][3 + a], red[1][3 + a]), fmaxf(red[2][3 + a], red[3][3 + a]));
    }
    if (threadIdx.x == 3) part[8 * (size_t)blockIdx.x + 6] = __int_as_float(cnt[0] + cnt[1] + cnt[2] + cnt[3]);
}

// One workgroup: the box of all parts, then thread 0 lays out the grid.  Cells are cubes of edge h = (volume of the axes that get
// more than one cell / target)^(1 / their number), n = floor(extent / h) per axis; an axis shorter than h gets one cell and leaves
// the product, which is then <= target = finite points / NN_PER_CELL: a query that looks at the whole grid reads fewer cell bounds
// than there are points.
__global__ __launch_bounds__(256) void k_nn_header(const float* __restrict__ part, int nparts, NnHeader* __restrict__ head) {
    __shared__ float red[4][6];
    __shared__ long long cnt[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    long long n = 0;
    for (int i = threadIdx.x; i < nparts; i += 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], part[8 * i + a]); hi[a] = fmaxf(hi[a], part[8 * i + 3 + a]); }
        n += __float_as_int(part[8 * i + 6]);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64)); }
        n += __shfl_xor(n, o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[wv][a] = lo[a]; red[wv][3 + a] = hi[a]; }
        cnt[wv] = n;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    NnHeader h;
    const long long nf = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    double ext[3];
    for (int a = 0; a < 3; ++a) {
        h.lo[a] = fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]));
        h.hi[a] = fmaxf(fmaxf(red[0][3 + a], red[1][3 + a]), fmaxf(red[2][3 + a], red[3][3 + a]));
        ext[a] = nf > 0 ? (double)h.hi[a] - (double)h.lo[a] : 0.0;
        h.n[a] = 1;
    }
    const double target = (double)(nf / NN_PER_CELL > 1 ? nf / NN_PER_CELL : 1);
    bool active[3] = {ext[0] > 0.0, ext[1] > 0.0, ext[2] > 0.0};
    for (int it = 0; it < 3; ++it) {          // an axis shorter than the cell edge leaves the set; at most three turns change it
        int k = 0;
        double vol = 1.0;
        for (int a = 0; a < 3; ++a) if (active[a]) { ++k; vol *= ext[a]; }
        if (k == 0) break;
        const double edge = k == 1 ? vol / target : (k == 2 ? sqrt(vol / target) : cbrt(vol / target));
        bool again = false;
        for (int a = 0; a < 3; ++a) {
            h.n[a] = 1;
            if (!active[a]) continue;
            const double c = floor(ext[a] / edge);
            if (!(c >= 2.0)) { active[a] = false; again = true; }
            else h.n[a] = (int)(c < 1048576.0 ? c : 1048576.0);
        }
        if (!again) break;
    }
    for (int a = 0; a < 3; ++a) if (!active[a]) h.n[a] = 1;
    if ((double)h.n[0] * h.n[1] * h.n[2] > target) h.n[0] = h.n[1] = h.n[2] = 1;          // (cannot happen; keeps the promise anyway)
    float hs = INFINITY;
    for (int a = 0; a < 3; ++a) {
        const float e = h.hi[a] - h.lo[a];
        h.inv_h[a] = h.n[a] > 1 ? (float)h.n[a] / e : 0.f;
        // the fp32 cell function below moves a cell boundary by at most a few 2^-23 of the extent: 2^-9 of a cell covers 2^11 cells an axis
        if (h.n[a] > 1) hs = fminf(hs, e / (float)h.n[a] * (1.f - 1.f / 512.f) - e * 4.8e-7f);
    }
    h.h_safe = (hs > 0.f && hs < INFINITY) ? hs : 0.f;
    h.n_finite = (int)nf;
    h.pad[0] = h.pad[1] = 0;
    *head = h;
}

__global__ __launch_bounds__(256) void k_nn_count(const float* __restrict__ pts, long long P, const NnHeader* __restrict__ head, int* __restrict__ cell,
                                                  int* count) {
    const NnHeader h = *head;
    const bool ok = nn_head_ok(h, P);
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < P; p += gridDim.x * 256ll) {
        const float x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
        int c = -1;
        if (ok && finite3(x, y, z))
            c = (nn_cell1(x, h.lo[0], h.inv_h[0], h.n[0]) * h.n[1] + nn_cell1(y, h.lo[1], h.inv_h[1], h.n[1])) * h.n[2] + nn_cell1(z, h.lo[2], h.inv_h[2], h.n[2]);
        cell[p] = c;
        if (c >= 0) atomicAdd(count + c, 1);
    }
}

// the scan's source: count[0 .. n) -> start[] (one sequence; the second stays 0)
struct NnSrc {
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

__global__ __launch_bounds__(256) void k_nn_fill(const float* __restrict__ pts, long long P, const int* __restrict__ cell, const int* __restrict__ start,
                                                 int* cursor, float4* __restrict__ rec) {
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < P; p += gridDim.x * 256ll) {
        const int c = cell[p];
        if (c < 0 || c >= P) continue;
        const long long o = (long long)start[c] + atomicAdd(cursor + c, 1);
        if (o < 0 || o >= P) continue;
        rec[o] = make_float4(pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], __int_as_float((int)p));
    }
}

// (the squared distance nn_dist2 and the correctly rounded square root nn_sqrt_rn: nn_grid.h, shared with csrc/cloud.hip)

// The records of cells [c0, c1] of one (x, y) column are contiguous (z fastest).  (d2, index) keeps the lexicographic minimum, so the
// order of the records inside a cell does not show.
__device__ __forceinline__ void nn_scan_run(const float4* __restrict__ rec, const int* __restrict__ start, long long P, int c0, int c1, float qx,
                                            float qy, float qz, float& best, int& arg) {
    long long s = start[c0], e = start[c1 + 1];
    s = s < 0 ? 0 : s;
    e = e > P ? P : e;
    for (long long i = s; i < e; ++i) {
        const float4 r = rec[i];
        const float d2 = nn_dist2(qx - r.x, qy - r.y, qz - r.z);
        const int id = __float_as_int(r.w);
        if (d2 < best || (d2 == best && id < arg)) { best = d2; arg = id; }
    }
}

// Stop rule.  Let c be the cell of q' = q clamped into the box [lo, hi] (q' = q inside it).  After shells 0 .. r every cell within
// Chebyshev distance r of c has been read, so a point p not yet seen has, along some axis a with more than one cell, a cell
// coordinate that differs from c_a by r + 1 or more.  The cell function is non-decreasing, so r whole cells lie between q'_a and
// p_a, and |p_a - q'_a| >= r h, h = h_safe a lower bound of every such cell's width.  All points lie in the box, the box is convex
// and q' is the point of it nearest to q, so (p - q').(q - q') <= 0 and |p - q|^2 >= |p - q'|^2 + |q' - q|^2 >= (r h)^2 + |q - q'|^2.
// The comparison is strict and the bound is shrunk by 2^-16, far more than the few 2^-24 by which the fp32 evaluation of either
// side can be off: a point not seen has a strictly larger fp32 squared distance than the best one, so it cannot win, not even a tie.
// r never exceeds the largest grid dimension - 1 (then every cell has been read), so the loop ends whatever the input is.
__global__ __launch_bounds__(256) void k_nn_query(const float* __restrict__ query, long long Q, long long P, const NnHeader* __restrict__ head,
                                                  const int* __restrict__ start, const float4* __restrict__ rec, float* __restrict__ dist,
                                                  int* __restrict__ index) {
    const NnHeader h = *head;
    const bool ok = nn_head_ok(h, P) && h.n_finite > 0;
    const int nx = h.n[0], ny = h.n[1], nz = h.n[2];
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < Q; i += gridDim.x * 256ll) {
        const float qx = query[3 * i], qy = query[3 * i + 1], qz = query[3 * i + 2];
        float best = INFINITY;
        int arg = -1;
        if (ok && finite3(qx, qy, qz)) {
            const float cx_ = fminf(fmaxf(qx, h.lo[0]), h.hi[0]), cy_ = fminf(fmaxf(qy, h.lo[1]), h.hi[1]), cz_ = fminf(fmaxf(qz, h.lo[2]), h.hi[2]);
            const float ox = qx - cx_, oy = qy - cy_, oz = qz - cz_;
            const float out2 = ox * ox + oy * oy + oz * oz;
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
                            nn_scan_run(rec, start, P, col + z0, col + z1, qx, qy, qz, best, arg);
                        } else {
                            if (cz - r >= 0) nn_scan_run(rec, start, P, col + cz - r, col + cz - r, qx, qy, qz, best, arg);
                            if (cz + r < nz && r > 0) nn_scan_run(rec, start, P, col + cz + r, col + cz + r, qx, qy, qz, best, arg);
                        }
                    }
                }
                const float reach = (float)r * h.h_safe;
                if (best < (reach * reach + out2) * (1.f - 1.f / 65536.f)) break;
            }
        }
        dist[i] = arg >= 0 ? nn_sqrt_rn(best) : INFINITY;
        index[i] = arg;
    }
}

static int mesh_check(long long V, long long T) {
    ES_REQUIRE(V >= 0 && T >= 0, "mesh: negative vertex or triangle count");
    ES_REQUIRE(V < MESH_MAX && T < MESH_MAX, "mesh: 2^31 vertices or triangles or more (indices are int32)");
    return ST_OK;
}
static int nn_check(long long P, long long Q) {
    ES_REQUIRE(P >= 0 && Q >= 0, "nearest: negative point or query count");
    ES_REQUIRE(P < MESH_MAX && Q < MESH_MAX, "nearest: 2^31 points or queries or more (indices are int32)");
    return ST_OK;
}

}  // namespace es

using namespace es;

extern "C" {

int64_t es_mesh_scratch_bytes(long long n_verts, long long n_tris) {
    if (mesh_check(n_verts, n_tris) != ST_OK) return -1;
    return mesh_layout(nullptr, n_verts, n_tris).bytes;
}

int es_mesh_cc_begin(const int* tris, long long V, long long T, void* scratch, void* stream) {
    if (const int s = mesh_check(V, T)) return s;
    ES_REQUIRE(tris || T == 0, "es_mesh_cc_begin needs tris");
    ES_SCRATCH_OK(scratch, "mesh scratch");
    if (V == 0) return ST_OK;
    const MeshScratch s = mesh_layout(scratch, V, T);
    hipLaunchKernelGGL(k_mesh_init, dim3(grid_for(V)), dim3(256), 0, static_cast<hipStream_t>(stream), s.parent, (int)V);
    return hip_last("es_mesh_cc_begin");
}

int es_mesh_cc_round(const int* tris, long long V, long long T, void* scratch, int* changed, void* stream) {
    if (const int s = mesh_check(V, T)) return s;
    ES_REQUIRE((tris || T == 0) && changed, "es_mesh_cc_round needs tris and changed");
    ES_SCRATCH_OK(scratch, "mesh scratch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ES_HIP(hipMemsetAsync(changed, 0, sizeof(int), st));
    if (V == 0 || T == 0) return ST_OK;
    const MeshScratch s = mesh_layout(scratch, V, T);
    hipLaunchKernelGGL(k_mesh_hook, dim3(grid_for(T)), dim3(256), 0, st, tris, (int)V, T, s.parent, changed);
    for (int pass = 0, n = mesh_jump_passes(V); pass < n; ++pass)
        hipLaunchKernelGGL(k_mesh_jump, dim3(grid_for(V)), dim3(256), 0, st, s.parent, (int)V);
    return hip_last("es_mesh_cc_round");
}

int es_mesh_cc_finish(const int* tris, long long V, long long T, const void* scratch, int* vertex_label, int* triangle_label, int* component_triangles,
                      long long* totals, void* stream) {
    if (const int s = mesh_check(V, T)) return s;
    ES_REQUIRE((tris || T == 0) && totals, "es_mesh_cc_finish needs tris and totals");
    ES_REQUIRE((V == 0 || (vertex_label && component_triangles)) && (T == 0 || triangle_label),
               "es_mesh_cc_finish needs vertex_label, triangle_label and component_triangles");
    ES_SCRATCH_OK(scratch, "mesh scratch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const MeshScratch s = mesh_layout(scratch, V, T);
    ES_HIP(hipMemsetAsync(totals, 0, 3 * sizeof(long long), st));
    if (V > 0) {
        ES_HIP(hipMemcpyAsync(vertex_label, s.parent, 4 * V, hipMemcpyDeviceToDevice, st));
        ES_HIP(hipMemsetAsync(component_triangles, 0, 4 * V, st));
    }
    unsigned long long* tot = reinterpret_cast<unsigned long long*>(totals);
    if (T > 0)
        hipLaunchKernelGGL(k_mesh_label, dim3(grid_for(T)), dim3(256), 0, st, tris, (int)V, T, s.parent, triangle_label, component_triangles, tot);
    if (V > 0) hipLaunchKernelGGL(k_mesh_stats, dim3(grid_for(V)), dim3(256), 0, st, component_triangles, (int)V, tot);
    return hip_last("es_mesh_cc_finish");
}

int es_mesh_keep_count(const int* tris, long long V, long long T, const int* triangle_label, const int* component_triangles, double keep_ratio,
                       long long max_triangles, int compact, void* scratch, long long* totals, void* stream) {
    if (const int s = mesh_check(V, T)) return s;
    ES_REQUIRE(keep_ratio >= 0.0 && keep_ratio <= 1.0, "es_mesh_keep_count: keep_ratio must be in [0, 1]");
    ES_REQUIRE(max_triangles >= 0 && max_triangles <= T, "es_mesh_keep_count: max_triangles outside 0..T");
    ES_REQUIRE(totals && (T == 0 || (tris && triangle_label && component_triangles)),
               "es_mesh_keep_count needs tris, triangle_label, component_triangles and totals");
    ES_SCRATCH_OK(scratch, "mesh scratch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const MeshScratch s = mesh_layout(scratch, V, T);
    if (V > 0) ES_HIP(hipMemsetAsync(s.vflag, compact ? 0 : 1, V, st));
    if (T > 0)
        hipLaunchKernelGGL(k_mesh_keep_flags, dim3(grid_for(T)), dim3(256), 0, st, tris, (int)V, T, triangle_label, component_triangles,
                           keep_ratio * (double)max_triangles, compact, s.tflag, s.vflag);
    scan_launch(MeshKeepSrc{s.vflag, s.tflag, V, T, s.voff, s.toff}, s.nblk, s.bsum, s.boff, totals, st);
    return hip_last("es_mesh_keep_count");
}

int es_mesh_keep_emit(const float* verts, const int* tris, long long V, long long T, const void* scratch, long long V2, long long T2, float* verts_out,
                      int* tris_out, long long* vertex_map, void* stream) {
    if (const int s = mesh_check(V, T)) return s;
    ES_REQUIRE(V2 >= 0 && V2 <= V && T2 >= 0 && T2 <= T, "es_mesh_keep_emit: kept counts outside 0..V / 0..T");
    ES_SCRATCH_OK(scratch, "mesh scratch");
    if (V2 == 0 && T2 == 0) return ST_OK;
    ES_REQUIRE((T2 == 0 || (tris && tris_out)) && (!verts_out || verts), "es_mesh_keep_emit needs tris, tris_out and verts for verts_out");
    const MeshScratch s = mesh_layout(scratch, V, T);
    hipLaunchKernelGGL(k_mesh_keep_emit, dim3(grid_for(V > T ? V : T)), dim3(256), 0, static_cast<hipStream_t>(stream), verts, tris, (int)V, T, s.voff,
                       s.toff, s.vflag, s.tflag, (int)V2, (int)T2, verts_out, tris_out, vertex_map);
    return hip_last("es_mesh_keep_emit");
}

int es_mesh_clean_keys(const int* tris, long long V, long long T, int* key_hi, long long* key_lo, void* stream) {
    if (const int s = mesh_check(V, T)) return s;
    if (T == 0) return ST_OK;
    ES_REQUIRE(tris && key_hi && key_lo, "es_mesh_clean_keys needs tris, key_hi and key_lo");
    hipLaunchKernelGGL(k_mesh_clean_keys, dim3(grid_for(T)), dim3(256), 0, static_cast<hipStream_t>(stream), tris, (int)V, T, key_hi, key_lo);
    return hip_last("es_mesh_clean_keys");
}

int es_mesh_clean_count(const int* tris, long long V, long long T, const long long* order, int compact, void* scratch, long long* totals,
                        void* stream) {
    if (const int s = mesh_check(V, T)) return s;
    ES_REQUIRE(totals && (T == 0 || (tris && order)), "es_mesh_clean_count needs tris, order and totals");
    ES_SCRATCH_OK(scratch, "mesh scratch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const MeshScratch s = mesh_layout(scratch, V, T);
    ES_HIP(hipMemsetAsync(totals, 0, 3 * sizeof(long long), st));
    if (V > 0) ES_HIP(hipMemsetAsync(s.vflag, compact ? 0 : 1, V, st));
    if (T > 0) {
        ES_HIP(hipMemsetAsync(s.tflag, 0, T, st));
        hipLaunchKernelGGL(k_mesh_clean_flags, dim3(grid_for(T)), dim3(256), 0, st, tris, (int)V, T, order, compact, s.tflag, s.vflag,
                           reinterpret_cast<unsigned long long*>(totals));
    }
    scan_launch(MeshKeepSrc{s.vflag, s.tflag, V, T, s.voff, s.toff}, s.nblk, s.bsum, s.boff, totals, st);
    return hip_last("es_mesh_clean_count");
}

int64_t es_nn_scratch_bytes(long long n_points) {
    if (nn_check(n_points, 0) != ST_OK) return -1;
    return nn_layout(nullptr, n_points).bytes;
}

int es_nn_build(const float* points, long long P, void* scratch, void* stream) {
    if (const int s = nn_check(P, 0)) return s;
    ES_REQUIRE(points || P == 0, "es_nn_build needs points");
    ES_SCRATCH_OK(scratch, "mesh scratch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const NnScratch s = nn_layout(scratch, P);
    const int nparts = (int)(grid_for(P) < (unsigned)NN_PARTS ? grid_for(P) : (unsigned)NN_PARTS);
    ES_HIP(hipMemsetAsync(s.count, 0, reinterpret_cast<char*>(s.start) - reinterpret_cast<char*>(s.count), st));          // count and cursor
    hipLaunchKernelGGL(k_nn_bbox, dim3(nparts), dim3(256), 0, st, points, P, s.part);
    hipLaunchKernelGGL(k_nn_header, dim3(1), dim3(256), 0, st, s.part, nparts, s.head);
    if (P == 0) return hip_last("es_nn_build");
    hipLaunchKernelGGL(k_nn_count, dim3(grid_for(P)), dim3(256), 0, st, points, P, s.head, s.cell, s.count);
    scan_launch(NnSrc{s.count, P + 1, s.start}, s.nblk, s.bsum, s.boff, nullptr, st);
    hipLaunchKernelGGL(k_nn_fill, dim3(grid_for(P)), dim3(256), 0, st, points, P, s.cell, s.start, s.cursor, s.rec);
    return hip_last("es_nn_build");
}

int es_nn_query(const float* query, long long Q, long long P, const void* scratch, float* dist, int* index, void* stream) {
    if (const int s = nn_check(P, Q)) return s;
    if (Q == 0) return ST_OK;
    ES_REQUIRE(query && dist && index, "es_nn_query needs query, dist and index");
    ES_SCRATCH_OK(scratch, "mesh scratch");
    const NnScratch s = nn_layout(scratch, P);
    hipLaunchKernelGGL(k_nn_query, dim3(grid_for(Q)), dim3(256), 0, static_cast<hipStream_t>(stream), query, Q, P, s.head, s.start, s.rec, dist, index);
    return hip_last("es_nn_query");
}

}  // extern "C"
