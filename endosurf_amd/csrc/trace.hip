// Surface tracing, no grad: where a ray meets the level set  sdf(x + D(x, t)) = tau, by the per-row rule of endosurf_amd/tracing.py
// trace_surface (DESIGN.md 7j "Row rule") -- sphere tracing with a bracket phase -- the whole iteration of a tile's rays in ONE launch.
// One evaluation is k_query_sdf's (query.hip): the two bodies that kernel is made of, deform_eval and sdf_eval (field_eval.h), on the
// same 64-point tile (32 points for small batches), LDS carve, packed weights and bias prefetch.  Hence the value a
// row sees is, bit for bit, what es_query_sdf_tiles returns for that point on its 32- and 64-point tiles, whatever the row's place in
// the tile and whatever its neighbours hold.  fp32 only: decisions about signs and eps do not ride on the split kernels' budgets.
#include <cfloat>

#include "chain_common.h"
#include "encode.h"
#include "field_eval.h"
#include "host.h"
#include "launch.h"
#include "tabs.h"

namespace es {

struct TraceArgs {
    const float* rays;          // [N][9]
    int N, max_iters;
    float tau, eps, relax, min_step;
    float* depth;               // [N]
    int* status;                // [N]
    int* iters;                 // [N], nullable
    float* residual;            // [N], nullable
    float* points;              // [N][3], nullable
};

// tracing.py's status values; a live row is in phase MARCH (TRACE_LIVE) or REFINE
constexpr int TRACE_REFINE = -1, TRACE_LIVE = 0, TRACE_HIT = 1, TRACE_MISS = 2, TRACE_OCCUPIED = 3, TRACE_NOT_CONVERGED = 4;
constexpr int TRACE_LDS_BYTES = LEAN_LDS_BYTES + 192 * 4;          // + the canonical rows: 81 664 B, two workgroups per CU

// Product by product and sum by sum, as the twin takes them.  The library is built with -ffp-contract=fast, under which a product that
// feeds a sum is fused into it -- a plain one and __fmul_rn's alike; an empty asm statement makes the product a value the optimiser
// cannot look through, so it is rounded on its own (nn_grid.h nn_dist2_exact).
__device__ __forceinline__ float mul_rn(float a, float b) {
    float p = a * b;
    asm("" : "+v"(p));
    return p;
}
__device__ __forceinline__ float dot3_rn(const float (&a)[3], const float (&b)[3]) {
    return __fadd_rn(__fadd_rn(mul_rn(a[0], b[0]), mul_rn(a[1], b[1])), mul_rn(a[2], b[2]));
}
__device__ __forceinline__ float clamp0(float v) { return v < 0.f ? 0.f : v; }          // torch.clamp(min=0): a NaN stays a NaN

// The next depth inside the bracket (tracing.py _next): the regula-falsi point, else the midpoint; false when neither is strictly inside.
__device__ __forceinline__ bool trace_next(float z_lo, float f_lo, float z_hi, float f_hi, float& z) {
    const float rf = __fsub_rn(z_lo, __fdiv_rn(mul_rn(f_lo, __fsub_rn(z_hi, z_lo)), __fsub_rn(f_hi, f_lo)));
    if (rf > z_lo && rf < z_hi) { z = rf; return true; }          // (false for NaN)
    const float mid = mul_rn(0.5f, __fadd_rn(z_lo, z_hi));
    z = mid;
    return mid > z_lo && mid < z_hi;
}

// The row's thread (tid < PTS) keeps o, w, s, far, z, both bracket ends, status (which carries the phase), iters and what it will
// report in registers; px / pt hold the current point and time of every row, px rewritten for live rows only.  Frozen rows (and the rows at or past N,
// frozen from the start) still ride through the MFMAs, but none of their state changes.  Every workgroup runs at most max_iters
// evaluations -- an argument the ABI has validated -- and leaves the loop when none of its own rows is live: it waits for nothing
// outside itself.
template <bool DEFORM, bool HALF>
__global__ __launch_bounds__(NTHREADS, 2) void k_trace_surface(TraceArgs a, Tabs tb, const float4* __restrict__ packed,
                                                            const float* __restrict__ weff) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using Tile = LeanTile<HALF>;
    constexpr int RTC = Tile::RTC, PTS = Tile::PTS;
    float *mainT = lds + Tile::MAIN, *aux = lds + Tile::AUX, *red = lds + Tile::RED, *px = lds + Tile::PX, *pt = lds + Tile::PT;
    float* pxc = lds + Tile::END;          // [3][64]: the canonical point x + D of the point under evaluation (px)
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * PTS;
    const bool mine = tid < PTS && row0 + tid < a.N;          // this thread owns a ray of the batch
    const float inf = __builtin_inff();
    // What the row update and the final stores read of the arguments is kept in vector registers, of which this kernel has some to
    // spare: left in the scalar file through the two networks' loops, it is spilled there.
    float tau = a.tau, eps = a.eps, relax = a.relax, min_step = a.min_step;
    float *depth_out = a.depth, *residual_out = a.residual, *points_out = a.points;
    int *status_out = a.status, *iters_out = a.iters;
    int n_rays = a.N, b8d = tb.boff[NET_D * LAYERS + 8], b8s = tb.boff[NET_S * LAYERS + 8];          // (the last layers' bias offsets)
    asm volatile("" : "+v"(tau), "+v"(eps), "+v"(relax), "+v"(min_step), "+v"(depth_out), "+v"(residual_out), "+v"(points_out), "+v"(status_out),
                 "+v"(iters_out), "+v"(n_rays), "+v"(b8d), "+v"(b8s));
    float o[3] = {0.f, 0.f, 0.f}, w[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
    float s = 1.f, far = 0.f, z = 0.f, z_lo = 0.f, f_lo = 0.f, z_hi = 0.f, f_hi = 0.f, resid = 0.f, depth = inf;
    int status = TRACE_MISS, iters = 0;
    if (tid < 64) {
        float t = 0.f;
        if (mine) {
            const float* r = a.rays + 9 * (size_t)(row0 + tid);
            const float d[3] = {r[3], r[4], r[5]};
            o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
            t = r[8];
            const float dd = dot3_rn(d, d);
            const float d1 = __fdiv_rn(-dot3_rn(d, o), dd);
            const float q[3] = {__fadd_rn(o[0], mul_rn(d1, d[0])), __fadd_rn(o[1], mul_rn(d1, d[1])), __fadd_rn(o[2], mul_rn(d1, d[2]))};
            const float d2 = __fdiv_rn(__fsqrt_rn(clamp0(__fsub_rn(1.f, dot3_rn(q, q)))), __fsqrt_rn(dd));
            const float near = clamp0(__fsub_rn(d1, d2));
            far = __fadd_rn(d1, d2);
            const float inv = __fadd_rn(d[2], 1e-6f);
            w[0] = __fdiv_rn(d[0], inv); w[1] = __fdiv_rn(d[1], inv); w[2] = __fdiv_rn(d[2], inv);
            s = __fsqrt_rn(dot3_rn(w, w));
            if (far > near) {          // (false for NaN: such a ray misses)
                status = TRACE_LIVE;
                z = near;
#pragma unroll
                for (int i = 0; i < 3; ++i) p[i] = __fadd_rn(o[i], mul_rn(z, w[i]));
            }
        }
        const bool go = status == TRACE_LIVE;          // (rows that never start hold the origin of the unit ball at t = 0)
        px[tid] = go ? p[0] : 0.f; px[64 + tid] = go ? p[1] : 0.f; px[128 + tid] = go ? p[2] : 0.f; pt[tid] = go ? t : 0.f;
        if (!go) { p[0] = p[1] = p[2] = 0.f; }
    }
    __syncthreads();
    int tid_k = tid, wave_k = wave;          // (the loop's own copies, see below)
    const float4* packed_k = packed;
    const float* weff_k = weff;
    for (int k = 1; k <= a.max_iters; ++k) {
        // Each network's address arithmetic (quad offsets, fragment, bias and segment addresses) is derived afresh from a thread
        // index, a wave index and base pointers the compiler cannot see through: hoisted out of this loop as invariants, the two
        // networks' sets together exceed the register budget of two workgroups per CU and spill.
        if (DEFORM) {
            asm volatile("" : "+v"(tid_k), "+s"(wave_k), "+s"(packed_k), "+s"(weff_k));
            const int lane_k = tid_k & 63;
            const QuadOff<RTC> qo = quad_offsets<RTC>(0, 2 * wave_k, lane_k);
            deform_eval<RTC>(mainT, aux, red, px, pt, tb, packed_k, weff_k, qo, tid_k, lane_k, wave_k);
            if (tid_k < 192) {          // add_deform's statement, on the loop's own copies
                const int i = tid_k >> 6, row = tid_k & 63;
                pxc[i * 64 + row] = px[i * 64 + row] + (smalln_reduce<3>(red, i, row) + weff_k[b8d + i]);
            }
            __syncthreads();
        }
        {
            asm volatile("" : "+v"(tid_k), "+s"(wave_k), "+s"(packed_k), "+s"(weff_k));
            const int lane_k = tid_k & 63;
            const QuadOff<RTC> qo = quad_offsets<RTC>(0, 2 * wave_k, lane_k);
            sdf_eval<RTC>(mainT, aux, red, DEFORM ? pxc : px, tb, packed_k, weff_k, qo, tid_k, lane_k, wave_k);
        }
        if (status <= TRACE_LIVE) {          // (tid < PTS and the ray is in the batch)
            const float f = __fsub_rn(smalln_reduce<1>(red, 0, tid) + weff_k[b8s], tau);
            iters = k;
            resid = f;
#pragma unroll
            for (int i = 0; i < 3; ++i) p[i] = px[i * 64 + tid];          // the point just evaluated
            bool step = false;          // a new z inside the bracket is wanted
            if (!(fabsf(f) <= FLT_MAX)) {          // inf or NaN
                status = TRACE_NOT_CONVERGED;
            } else if (fabsf(f) <= eps) {
                status = TRACE_HIT; depth = z;
            } else if (status == TRACE_LIVE) {
                if (f > 0.f) {
                    z_lo = z; f_lo = f;
                    z = __fadd_rn(z, fmaxf(__fdiv_rn(mul_rn(relax, f), s), min_step));
                    if (z > far) status = TRACE_MISS;
                } else if (k == 1) {
                    status = TRACE_OCCUPIED; depth = 0.f;
                } else {
                    z_hi = z; f_hi = f; status = TRACE_REFINE; step = true;
                }
            } else {
                if (f > 0.f) { z_lo = z; f_lo = f; } else { z_hi = z; f_hi = f; }
                step = true;
            }
            if (step && !trace_next(z_lo, f_lo, z_hi, f_hi, z)) {          // the bracket has no interior in fp32: the row stops at its low end
                status = TRACE_HIT; depth = z_lo; resid = f_lo; z = z_lo;
#pragma unroll
                for (int i = 0; i < 3; ++i) p[i] = __fadd_rn(o[i], mul_rn(z_lo, w[i]));
            }
            if (status <= TRACE_LIVE) {
#pragma unroll
                for (int i = 0; i < 3; ++i) px[i * 64 + tid] = __fadd_rn(o[i], mul_rn(z, w[i]));
            }
        }
        // workgroup-uniform exit; also the barrier between this round's reads of ``red`` / writes of px and the next encoding
        if (!__syncthreads_or(status <= TRACE_LIVE)) break;
    }
    if (tid < PTS && row0 + tid < n_rays) {
        if (status <= TRACE_LIVE) status = TRACE_NOT_CONVERGED;          // the cap
        const int r = row0 + tid;
        depth_out[r] = depth;
        status_out[r] = status;
        if (iters_out) iters_out[r] = iters;
        if (residual_out) residual_out[r] = resid;
        if (points_out) { points_out[3 * (size_t)r] = p[0]; points_out[3 * (size_t)r + 1] = p[1]; points_out[3 * (size_t)r + 2] = p[2]; }
    }
}

// Rays per tile when the caller leaves the choice to the library (tile_points = 0): 32 at every batch size.  Measured (the
// tile-height table): 1 024 rays 14.9 against 26.2 ms on 64-ray tiles, 16 384 rays 22.9 against 34.6, one 640 x 512 frame 100.8 against
// 124.6.  A tile runs as many evaluations as its slowest row, and the mean over tiles of that maximum grows with the tile (39 of 128 on
// 32 rays where a ray needs 11 on average), which outweighs the better MFMA utilisation of 64 rows even when the chip is full.
constexpr int TRACE_DEFAULT_TILE = 32;

int trace_surface(const float* rays, int N, float tau, float eps, float relax, float min_step, int max_iters, int tile_points,
                  const float* packed, const float* weff, int use_deform, float* depth_out, int* status_out, int* iters_out,
                  float* residual_out, float* points_out, hipStream_t st) {
    if (N <= 0) return ST_OK;
    static constexpr decltype(&k_trace_surface<true, false>) KERNELS[] = {k_trace_surface<true, false>, k_trace_surface<true, true>,          // [(DEFORM ? 0 : 2) + HALF]
                                                                          k_trace_surface<false, false>, k_trace_surface<false, true>};
    static DeviceOnce attr_done;
    const bool half = (tile_points ? tile_points : TRACE_DEFAULT_TILE) == 32;
    const TraceArgs a{rays, N, max_iters, tau, eps, relax, min_step, depth_out, status_out, iters_out, residual_out, points_out};
    return launch_lean(KERNELS, attr_done, (use_deform ? 0 : 2) + half, TRACE_LDS_BYTES, N, half ? 32 : 64, st, "trace_surface", a,
                       make_tabs(), reinterpret_cast<const float4*>(packed), weff);
}

}  // namespace es
