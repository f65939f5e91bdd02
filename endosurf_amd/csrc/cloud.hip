// Point-cloud clean-up queries on the device (additive to ABI v14): the two neighbour searches the reference's preprocess script runs
// through Open3D on the host (data/endonerf/preprocess.py:78-87, compute_nearest_neighbor_distance and remove_radius_outlier), over the
// uniform grid es_nn_build (csrc/mesh.hip, nn_grid.h) leaves in its scratch.  Numpy twins and specification: endosurf_amd/meshing.py
// self_nearest / radius_count / radius_outlier_mask.  Contract: DESIGN.md 7g.
//
//   k_cloud_self_nearest   one thread per point i: the lexicographic minimum of (d2, j) over the finite rows j != i, by the shell walk
//                          and the stop rule of k_nn_query (csrc/mesh.hip).  Point i lies inside the box of the finite points, so the
//                          clamped query q' of that rule is q itself and the bound of shell r is (r h_safe)^2.  A duplicate of the
//                          point is a neighbour at distance 0; the record whose index is i is the only one left out.
//   k_cloud_radius_count   one thread per query: the finite rows p with d2(q, p) <= r2, r2 one float on the device (so that "20 x the
//                          mean neighbour distance" needs no read-back).  With cap > 0 the thread stops reading at cap: the answer
//                          min(count, cap) does not depend on the order in which the records are read.
//
// d2 is the fp32 (dx dx + dy dy) + dz dz, every operation rounded on its own (nn_dist2_exact of nn_grid.h: the products pass through an
// empty asm statement, without which the back end fuses one of them into the sum); dist is its correctly rounded square root.  Both
// are numpy's bits, so the outputs equal the twins' bit for bit.
//
// Which cells a radius query reads.  Let p be a finite row with d2(q, p) <= r2.  Every term of d2 is non-negative and rounding is
// monotone, so already fl(dx dx) <= r2 with dx = fl(q_a - p_a) along each axis a.  A product rounds by at most 2^-24 of itself, or by
// 2^-150 where it underflows, and the difference by 2^-24 of itself (it is exact where it is tiny), so |q_a - p_a| <= R with
// R = sqrt(r2) (1 + 2^-16) + 2^-74, whatever way the few roundings of R's own evaluation fall.  Then q_a - R <= p_a <= q_a + R, and as
// p_a is a float and rounding is monotone, fl(q_a - R) <= p_a <= fl(q_a + R).  The cell function nn_cell1 is non-decreasing and is the
// same expression for points and queries, so p's cell coordinate lies in [nn_cell1(q_a - R), nn_cell1(q_a + R)]: no cell outside that
// range, along any axis, can hold a point that counts.  The records of a (x, y) column's z-range are contiguous (z fastest), so a
// column is one run of records.  Columns are read from the query's own column outwards -- the order cannot show in the answer, and a
// capped query meets its neighbours first.  A query that meets no early exit reads each cell of its range once: at most all of them,
// <= P / 4 cell bounds (NN_PER_CELL).  r2 = +inf gives R = +inf and the whole grid: the number of finite points (an overflowed d2 is
// +inf <= +inf).  r2 NaN or negative: every count is 0.  A non-finite query row: 0.
//
// The conventions of csrc/mesh.hip: 256 threads per workgroup; integer work only beside the distance; no atomics at all here; no
// workgroup waits for another; every device loop is bounded by the grid's dimensions (nn_head_ok: their product is <= P) or by P; the
// header is checked (nn_head_ok) and every record range read from the scratch is clamped into [0, P] before it addresses memory, so an
// uninitialised scratch yields inf / -1 / 0, not a fault.  Two calls give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"
#include "nn_grid.h"

namespace es {

// cells [c0, c1] of one column; the record of point ``self`` is left out
__device__ __forceinline__ void cloud_nearest_run(const float4* __restrict__ rec, const int* __restrict__ start, long long P, int c0, int c1, int self,
                                                  float qx, float qy, float qz, float& best, int& arg) {
    long long s = start[c0], e = start[c1 + 1];
    s = s < 0 ? 0 : s;
    e = e > P ? P : e;
    for (long long i = s; i < e; ++i) {
        const float4 r = rec[i];
        const int id = __float_as_int(r.w);
        if (id == self) continue;
        const float d2 = nn_dist2_exact(qx - r.x, qy - r.y, qz - r.z);
        if (d2 < best || (d2 == best && id < arg)) { best = d2; arg = id; }
    }
}

__global__ __launch_bounds__(256) void k_cloud_self_nearest(const float* __restrict__ pts, long long P, const NnHeader* __restrict__ head,
                                                            const int* __restrict__ start, const float4* __restrict__ rec, float* __restrict__ dist,
                                                            int* __restrict__ index) {
    const NnHeader h = *head;
    const bool ok = nn_head_ok(h, P) && h.n_finite > 0;
    const int nx = h.n[0], ny = h.n[1], nz = h.n[2];
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < P; i += gridDim.x * 256ll) {
        const float qx = pts[3 * i], qy = pts[3 * i + 1], qz = pts[3 * i + 2];
        float best = INFINITY;
        int arg = -1;
        if (ok && finite3(qx, qy, qz)) {
            const int cx = nn_cell1(qx, h.lo[0], h.inv_h[0], nx), cy = nn_cell1(qy, h.lo[1], h.inv_h[1], ny), cz = nn_cell1(qz, h.lo[2], h.inv_h[2], nz);
            const int rmax = max(max(max(cx, nx - 1 - cx), max(cy, ny - 1 - cy)), max(cz, nz - 1 - cz));
            for (int r = 0; r <= rmax; ++r) {
                const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
                const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
                for (int x = x0; x <= x1; ++x) {
                    const bool xface = x == cx - r || x == cx + r;
                    for (int y = y0; y <= y1; ++y) {
                        const int col = (x * ny + y) * nz;
                        if (xface || y == cy - r || y == cy + r) {
                            cloud_nearest_run(rec, start, P, col + z0, col + z1, (int)i, qx, qy, qz, best, arg);
                        } else {
                            if (cz - r >= 0) cloud_nearest_run(rec, start, P, col + cz - r, col + cz - r, (int)i, qx, qy, qz, best, arg);
                            if (cz + r < nz && r > 0) cloud_nearest_run(rec, start, P, col + cz + r, col + cz + r, (int)i, qx, qy, qz, best, arg);
                        }
                    }
                }
                const float reach = (float)r * h.h_safe;
                if (best < reach * reach * (1.f - 1.f / 65536.f)) break;          // (k_nn_query's stop rule with q' = q)
            }
        }
        dist[i] = arg >= 0 ? nn_sqrt_rn(best) : INFINITY;
        index[i] = arg;
    }
}

// cells [c0, c1] of one column; true once the cap is reached
__device__ __forceinline__ bool cloud_count_run(const float4* __restrict__ rec, const int* __restrict__ start, long long P, int c0, int c1, float qx,
                                                float qy, float qz, float r2, int cap, int& n) {
    long long s = start[c0], e = start[c1 + 1];
    s = s < 0 ? 0 : s;
    e = e > P ? P : e;
    for (long long i = s; i < e; ++i) {
        const float4 r = rec[i];
        if (nn_dist2_exact(qx - r.x, qy - r.y, qz - r.z) <= r2 && ++n == cap) return true;
    }
    return false;
}

__global__ __launch_bounds__(256) void k_cloud_radius_count(const float* __restrict__ query, long long Q, long long P, const NnHeader* __restrict__ head,
                                                            const int* __restrict__ start, const float4* __restrict__ rec,
                                                            const float* __restrict__ radius_sq, int cap, int* __restrict__ count) {
    const NnHeader h = *head;
    const float r2 = *radius_sq;
    const bool ok = nn_head_ok(h, P) && r2 >= 0.f;          // (a NaN compares false)
    const float R = nn_sqrt_rn(r2 >= 0.f ? r2 : 0.f) * (1.f + 1.f / 65536.f) + 0x1p-74f;
    const int nx = h.n[0], ny = h.n[1], nz = h.n[2];
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < Q; i += gridDim.x * 256ll) {
        const float qx = query[3 * i], qy = query[3 * i + 1], qz = query[3 * i + 2];
        int n = 0;
        if (ok && finite3(qx, qy, qz)) {
            const int x0 = nn_cell1(qx - R, h.lo[0], h.inv_h[0], nx), x1 = nn_cell1(qx + R, h.lo[0], h.inv_h[0], nx);
            const int y0 = nn_cell1(qy - R, h.lo[1], h.inv_h[1], ny), y1 = nn_cell1(qy + R, h.lo[1], h.inv_h[1], ny);
            const int z0 = nn_cell1(qz - R, h.lo[2], h.inv_h[2], nz), z1 = nn_cell1(qz + R, h.lo[2], h.inv_h[2], nz);
            const int cx = nn_cell1(qx, h.lo[0], h.inv_h[0], nx), cy = nn_cell1(qy, h.lo[1], h.inv_h[1], ny);          // in [x0, x1], [y0, y1]
            const int wx = max(cx - x0, x1 - cx), wy = max(cy - y0, y1 - cy);
            bool full = false;
            // x = cx, cx + 1, cx - 1, cx + 2, ...: every x of [x0, x1] once (side 1 of offset 0 is side 0 again and is skipped)
            for (int ox = 0; ox <= wx && !full; ++ox) {
                for (int sx = 0; sx < 2 && !full; ++sx) {
                    const int x = sx ? cx - ox : cx + ox;
                    if ((sx && ox == 0) || x < x0 || x > x1) continue;
                    for (int oy = 0; oy <= wy && !full; ++oy) {
                        for (int sy = 0; sy < 2 && !full; ++sy) {
                            const int y = sy ? cy - oy : cy + oy;
                            if ((sy && oy == 0) || y < y0 || y > y1) continue;
                            const int col = (x * ny + y) * nz;
                            full = cloud_count_run(rec, start, P, col + z0, col + z1, qx, qy, qz, r2, cap, n);
                        }
                    }
                }
            }
        }
        count[i] = n;
    }
}

static int cloud_check(long long P, long long Q) {
    ES_REQUIRE(P >= 0 && Q >= 0, "cloud: negative point or query count");
    ES_REQUIRE(P < MESH_MAX && Q < MESH_MAX, "cloud: 2^31 points or queries or more (indices are int32)");
    return ST_OK;
}

}  // namespace es

using namespace es;

extern "C" {

int es_cloud_self_nearest(const float* points, long long P, const void* scratch, float* dist, int* index, void* stream) {
    if (const int s = cloud_check(P, 0)) return s;
    if (P == 0) return ST_OK;
    ES_REQUIRE(points && dist && index, "es_cloud_self_nearest needs points, dist and index");
    ES_SCRATCH_OK(scratch, "nearest-neighbour scratch");
    const NnScratch s = nn_layout(scratch, P);
    hipLaunchKernelGGL(k_cloud_self_nearest, dim3(grid_for(P)), dim3(256), 0, static_cast<hipStream_t>(stream), points, P, s.head, s.start, s.rec, dist,
                       index);
    return hip_last("es_cloud_self_nearest");
}

int es_cloud_radius_count(const float* query, long long Q, long long P, const void* scratch, const float* radius_sq, int cap, int* count,
                          void* stream) {
    if (const int s = cloud_check(P, Q)) return s;
    ES_REQUIRE(cap >= 0, "es_cloud_radius_count: cap must be >= 0 (0 = no cap)");
    if (Q == 0) return ST_OK;
    ES_REQUIRE(query && radius_sq && count, "es_cloud_radius_count needs query, radius_sq and count");
    ES_SCRATCH_OK(scratch, "nearest-neighbour scratch");
    const NnScratch s = nn_layout(scratch, P);
    hipLaunchKernelGGL(k_cloud_radius_count, dim3(grid_for(Q)), dim3(256), 0, static_cast<hipStream_t>(stream), query, Q, P, s.head, s.start, s.rec,
                       radius_sq, cap, count);
    return hip_last("es_cloud_radius_count");
}

}  // extern "C"
