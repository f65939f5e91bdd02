// The uniform grid of the nearest-neighbour search (csrc/mesh.hip builds and queries it over points, csrc/surface.hip queries it over
// triangle centroids, csrc/cloud.hip queries it over the points themselves): the header a build leaves in the scratch, the scratch
// layout, the cell function, the checks a kernel makes before it trusts what the scratch holds, and the two pieces of arithmetic every
// query shares (the uncontracted squared distance, the correctly rounded square root).
#pragma once
#include <hip/hip_runtime.h>

#include "launch.h"
#include "scan.h"

namespace es {

constexpr long long MESH_MAX = 1ll << 31;                    // int32 indices
constexpr int NN_PARTS = 1024;                               // workgroups of the bounding-box reduction
constexpr int NN_PER_CELL = 4;                               // finite points per cell the grid aims for

struct NnHeader {            // 64 bytes at the start of the scratch, written by k_nn_header
    float lo[3];             // the box of the finite points (exact minima / maxima)
    float hi[3];
    float inv_h[3];          // cells per unit length along each axis (0 for an axis of one cell)
    float h_safe;            // a lower bound of the width of every cell of an axis that has more than one (the stop rule's h)
    int n[3];                // cells per axis, >= 1, n[0] n[1] n[2] <= max(1, finite points / NN_PER_CELL)
    int n_finite;
    int pad[2];
};
struct NnScratch {
    NnHeader* head;
    float* part;             // [NN_PARTS][8] lo, hi, finite count (as int bits) of a workgroup's points
    int* cell;               // [P] cell of each point, -1 for a non-finite one
    int* count;              // [P + 1] points per cell, then (k_nn_offsets) unused
    int* cursor;             // [P + 1] fill cursor of each cell (zeroed with count)
    int* start;              // [P + 1] first record of each cell; start[cells .. P] = finite points
    int* bsum;               // [nblk][2]
    int* boff;               // [nblk][2]
    float4* rec;             // [P] (x, y, z, index) sorted by cell
    long long nblk, bytes;
};
static_assert(sizeof(NnHeader) == 64, "the header's region");
static NnScratch nn_layout(const void* scratch, long long P) {          // a null scratch measures only
    Carver c(scratch);
    NnScratch s;
    s.nblk = scan_chunks(P + 1);
    s.head = c.take<NnHeader>(1);
    s.part = c.take<float>(8ll * NN_PARTS);
    s.cell = c.take<int>(P);
    s.count = c.take<int>(P + 1);
    s.cursor = c.take<int>(P + 1);          // (behind count: es_nn_build zeroes both with one memset)
    s.start = c.take<int>(P + 1);
    s.bsum = c.take<int>(2 * s.nblk);
    s.boff = c.take<int>(2 * s.nblk);
    s.rec = c.take<float4>(P);
    c.take<char>(16);          // (unused: es_nn_scratch_bytes has always counted it)
    s.bytes = c.off;
    return s;
}

__device__ __forceinline__ bool in_range(int i, int n) { return (unsigned)i < (unsigned)n; }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the cell coordinate of x along one axis: non-decreasing in x, the same expression for points and queries
__device__ __forceinline__ int nn_cell1(float x, float lo, float inv_h, int n) {
    const float f = (x - lo) * inv_h;
    if (!(f > 0.f)) return 0;                                     // (x <= lo, an axis of one cell, or inf x 0)
    return f >= (float)(n - 1) ? n - 1 : (int)f;
}
// the header as a kernel may use it: dimensions that the buffers can hold, whatever the scratch held
__device__ __forceinline__ bool nn_head_ok(const NnHeader& h, long long P) {
    return h.n[0] >= 1 && h.n[1] >= 1 && h.n[2] >= 1 && (long long)h.n[0] * h.n[1] <= P && (long long)h.n[0] * h.n[1] * h.n[2] <= P;
}

// (dx dx + dy dy) + dz dz with every product and sum rounded on its own: the library is built with -ffp-contract=fast, and a fused
// multiply-add here would give other last bits than the numpy twin (and than a caller's own fp32 check)
__device__ __forceinline__ float nn_dist2(float dx, float dy, float dz) {
#pragma clang fp contract(off)
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float s = xx + yy;
    return s + zz;
}

// nn_dist2 with every rounding where the source puts it.  The pragma above does not hold what it says: under -ffp-contract=fast the back
// end still fuses one product into the sum (a v_fma_f32 in the ISA; the open point of DESIGN 7b).  An empty asm statement makes each
// product a value the optimiser cannot look through, so it is rounded on its own and the sums are plain adds.  csrc/cloud.hip promises
// its twins' bits and uses this one; k_nn_query keeps nn_dist2 and the one-ulp slack DESIGN 7b states.
__device__ __forceinline__ float nn_dist2_exact(float dx, float dy, float dz) {
    float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    asm("" : "+v"(xx), "+v"(yy), "+v"(zz));
    return (xx + yy) + zz;
}

// The correctly rounded square root of x >= 0, whatever the accuracy of the device's sqrtf (measured: it is not numpy's): the
// neighbour s -+ 1 ulp replaces s when x lies beyond the midpoint between them, decided exactly -- a midpoint has 25 significant bits,
// so its square is exact in fp64.  Two turns cover a start that is 2 ulp off.
__device__ __forceinline__ float nn_sqrt_rn(float x) {
    float s = sqrtf(x);
    const double xd = (double)x;
    for (int turn = 0; turn < 2 && s > 0.f; ++turn) {
        const float lo = __int_as_float(__float_as_int(s) - 1), hi = __int_as_float(__float_as_int(s) + 1);
        const double m1 = 0.5 * ((double)lo + (double)s), m2 = 0.5 * ((double)s + (double)hi);
        if (xd < m1 * m1) s = lo;
        else if (xd > m2 * m2) s = hi;
        else break;
    }
    return s;
}

}  // namespace es
