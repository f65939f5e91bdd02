// The deformation network alone, no grad: D(x, t) of  x_c = x + D(x, t)  (reference DeformNetwork.forward, endosurf.py:724-738) and the
// inverse of  y -> y + D(y, t)  by the fixed-point iteration  y_k = c - D(y_{k-1}, t)  with the per-row stopping rule of
// endosurf_amd/tracking.py inverse_deform (DESIGN.md 7h "Row rule"), the whole iteration in ONE launch.  The evaluation is
// deform_eval (field_eval.h), the body k_query_sdf (query.hip) runs for its deformation half on the same tile: hence the same value of
// D per row, bit for bit, whatever the row's place in the tile and whatever its neighbours hold.  fp32 only.
#include <cfloat>

#include "chain_common.h"
#include "encode.h"
#include "field_eval.h"
#include "host.h"
#include "launch.h"
#include "tabs.h"

namespace es {

// x_c = x + D and / or D for explicit points (mode 0): k_query_sdf's prologue and deformation half followed by a store.  HALF: small
// batches run 32-point tiles (LeanTile, field_eval.h).
template <bool HALF>
__global__ __launch_bounds__(NTHREADS, 2) void k_deform_forward(PointSrc src, Tabs tb, const float4* __restrict__ packed,
                                                             const float* __restrict__ weff, float* __restrict__ xc_out,
                                                             float* __restrict__ d_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using Tile = LeanTile<HALF>;
    constexpr int RTC = Tile::RTC, PTS = Tile::PTS;
    float *mainT = lds + Tile::MAIN, *aux = lds + Tile::AUX, *red = lds + Tile::RED, *px = lds + Tile::PX, *pt = lds + Tile::PT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * PTS;
    const QuadOff<RTC> qo = quad_offsets<RTC>(0, 2 * wave, lane);
    if (tid < 64) {
        float x[3], t, d[3];
        load_point(src, tid < PTS ? row0 + tid : src.M, x, t, d);          // (rows past the tile's points or at or past M: zeros)
        px[tid] = x[0]; px[64 + tid] = x[1]; px[128 + tid] = x[2]; pt[tid] = t;
    }
    __syncthreads();
    deform_eval<RTC>(mainT, aux, red, px, pt, tb, packed, weff, qo, tid, lane, wave);
    if (tid < 192) {
        const int i = tid >> 6, row = tid & 63;
        if (row < PTS && row0 + row < src.M) {
            const float D = smalln_reduce<3>(red, i, row) + weff[tb.boff[NET_D * LAYERS + 8] + i];
            const size_t o = 3 * (size_t)(row0 + row) + i;
            if (d_out) d_out[o] = D;
            if (xc_out) xc_out[o] = px[i * 64 + row] + D;
        }
    }
}

// y with y + D(y, t) = c.  The row's thread (tid < 64) keeps c, step, iters and the live flag in registers; y and t are the tile's row
// scratch (px, pt), rewritten for live rows only.  Frozen rows (and the rows at or past M, frozen from the start) still ride through
// the MFMAs, but none of their state changes.  Every workgroup runs at most max_iters evaluations and leaves the loop when none of its
// own rows is live: it waits for nothing outside itself.
template <bool HALF>
__global__ __launch_bounds__(NTHREADS, 2) void k_deform_inverse(PointSrc src, Tabs tb, const float* __restrict__ init,
                                                             const float4* __restrict__ packed, const float* __restrict__ weff,
                                                             int max_iters, float tol, float* __restrict__ y_out,
                                                             float* __restrict__ step_out, int* __restrict__ iters_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using Tile = LeanTile<HALF>;
    constexpr int RTC = Tile::RTC, PTS = Tile::PTS;
    float *mainT = lds + Tile::MAIN, *aux = lds + Tile::AUX, *red = lds + Tile::RED, *px = lds + Tile::PX, *pt = lds + Tile::PT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * PTS;
    const QuadOff<RTC> qo = quad_offsets<RTC>(0, 2 * wave, lane);
    const bool mine = tid < PTS && row0 + tid < src.M;          // this thread owns a row of the batch
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, step = 0.f;
    int iters = 0, live = mine ? 1 : 0;
    if (tid < 64) {
        float x[3], t, d[3];
        load_point(src, tid < PTS ? row0 + tid : src.M, x, t, d);
        c0 = x[0]; c1 = x[1]; c2 = x[2];
        float y[3] = {c0, c1, c2};
        if (mine && init != nullptr) {
            const size_t o = 3 * (size_t)(row0 + tid);
            y[0] = init[o]; y[1] = init[o + 1]; y[2] = init[o + 2];
        }
        px[tid] = y[0]; px[64 + tid] = y[1]; px[128 + tid] = y[2]; pt[tid] = t;
    }
    __syncthreads();
    const int b8 = tb.boff[NET_D * LAYERS + 8];
    for (int k = 1; k <= max_iters; ++k) {
        deform_eval<RTC>(mainT, aux, red, px, pt, tb, packed, weff, qo, tid, lane, wave);
        if (live) {          // (tid < PTS and the row is in the batch)
            const float c[3] = {c0, c1, c2};
            float yn[3], e[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float D = smalln_reduce<3>(red, i, tid) + weff[b8 + i];
                yn[i] = c[i] - D;
                e[i] = yn[i] - px[i * 64 + tid];
            }
            // the twin's sum of squares, product by product (no contraction into fused multiply-adds)
            const float s = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(e[0], e[0]), __fmul_rn(e[1], e[1])), __fmul_rn(e[2], e[2])));
            const bool ok = s <= FLT_MAX;          // (false for inf and nan: the update is refused)
            if (ok) { px[tid] = yn[0]; px[64 + tid] = yn[1]; px[128 + tid] = yn[2]; }
            step = ok ? s : FLT_MAX;
            iters = k;
            live = ok && !(tol > 0.f && s <= tol);
        }
        // workgroup-uniform exit; also the barrier between this round's reads of ``red`` / writes of px and the next encoding
        if (!__syncthreads_or(live)) break;
    }
    if (mine) {
        const size_t o = 3 * (size_t)(row0 + tid);
        y_out[o] = px[tid]; y_out[o + 1] = px[64 + tid]; y_out[o + 2] = px[128 + tid];
        step_out[row0 + tid] = step;
        iters_out[row0 + tid] = iters;
    }
}

// 32-point tiles up to this many rows, 64-point tiles above.  Measured: the inverse at 2 630 rows 0.83 against 1.49 ms, at
// 8 192 1.09 against 1.87, at 16 384 1.39 against 1.54; at 32 768 the forward is 5 % faster on 64-point tiles and the inverse within 3 %.
constexpr int DEFORM_HALF_MAX_ROWS = 16384;

int deform_forward(const PointSrc& src, const float* packed, const float* weff, float* xc_out, float* d_out, hipStream_t st) {
    if (src.M <= 0) return ST_OK;
    static constexpr decltype(&k_deform_forward<false>) KERNELS[] = {k_deform_forward<false>, k_deform_forward<true>};          // [HALF]
    static DeviceOnce attr_done;
    const bool half = src.M <= DEFORM_HALF_MAX_ROWS;
    return launch_lean(KERNELS, attr_done, half, LEAN_LDS_BYTES, src.M, half ? 32 : 64, st, "deform_forward", src, make_tabs(),
                       reinterpret_cast<const float4*>(packed), weff, xc_out, d_out);
}

int deform_inverse(const PointSrc& src, const float* init, const float* packed, const float* weff, int max_iters, float tol, float* y_out,
                   float* step_out, int* iters_out, hipStream_t st) {
    if (src.M <= 0) return ST_OK;
    static constexpr decltype(&k_deform_inverse<false>) KERNELS[] = {k_deform_inverse<false>, k_deform_inverse<true>};          // [HALF]
    static DeviceOnce attr_done;
    const bool half = src.M <= DEFORM_HALF_MAX_ROWS;
    return launch_lean(KERNELS, attr_done, half, LEAN_LDS_BYTES, src.M, half ? 32 : 64, st, "deform_inverse", src, make_tabs(), init,
                       reinterpret_cast<const float4*>(packed), weff, max_iters, tol, y_out, step_out, iters_out);
}

}  // namespace es
