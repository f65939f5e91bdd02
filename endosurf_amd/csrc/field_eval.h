// One evaluation of the field  sdf(x + D(x, t))  on a lean tile's rows, written once.  Four kernels are built from these bodies: the SDF
// query (k_query_sdf, query.hip: one evaluation per launch), the deformation alone and its inverse (k_deform_forward, k_deform_inverse,
// deform.hip: deform_eval, looped for the inverse) and the surface tracer (k_trace_surface, trace.hip: both halves, looped).  They
// share the 64-point tile (32 points for small batches), the LDS carve, the packed weights, the barriers and the bias prefetch, so a
// row's D and a row's sdf have the same bits in all of them, whatever the row's place in the tile and whatever its neighbours hold:
// the tests that compare them bit for bit confirm a property this file gives by construction.  (k_deform_forward's load stage and the
// tracer's x + D stay written out in their kernels: through LeanTile::load_points / add_deform the compiler orders a few prologue
// instructions differently, and the ISA of those two units is held fixed.  The forward-mode kernels, k_deform_jet of deform_jet.hip and
// k_sdf_hessian of sdf_hess.hip, have bodies of their own -- several rows per point and an epilogue that gates or differentiates --
// and what they share is in jet.h.)
#pragma once
#include "chain_common.h"
#include "encode.h"
#include "tabs.h"

namespace es {

// The lean tile: where its parts lie in the workgroup's LDS (float offsets) and its first stage.  HALF: 32 points per workgroup -- the
// tile keeps its 64-row layout but only row-tile 0 carries points, so every layer issues half the MFMAs and twice as many workgroups
// share the batch; a row's arithmetic is the same in both.
template <bool HALF>
struct LeanTile {
    static constexpr int RTC = HALF ? 1 : 2;          // row tiles of 32 that carry points
    static constexpr int PTS = HALF ? 32 : 64;
    static constexpr int MAIN = 0;                    // the activations
    static constexpr int AUX = MAIN_FLOATS;           // the encoding rows
    static constexpr int RED = AUX;                   // [4][<=3][64]: aliases the encoding rows, dead by the time the tiny last layers run
    static constexpr int PX = AUX + AUX56_FLOATS;     // [3][64]: the rows' points
    static constexpr int PT = PX + 192;               // [64]: their times
    static constexpr int END = PT + 64;               // == LEAN_LDS_BYTES / 4: what a kernel adds of its own starts here
    // the tile's points and times into px / pt, behind a barrier (rows past the tile's points or at or past M: zeros)
    static __device__ __forceinline__ void load_points(float* px, float* pt, const PointSrc& src, int row0, int tid) {
        if (tid < 64) {
            float x[3], t, d[3];
            load_point(src, tid < PTS ? row0 + tid : src.M, x, t, d);
            px[tid] = x[0]; px[64 + tid] = x[1]; px[128 + tid] = x[2]; pt[tid] = t;
        }
        __syncthreads();
    }
};
static_assert(LeanTile<false>::END * 4 == LEAN_LDS_BYTES, "the lean tile fills LEAN_LDS_BYTES");

// One evaluation of the deformation MLP on the tile's rows (px [3][64], pt [64]): leaves the four k-partial sums of the 3 outputs in
// ``red`` (which aliases the encoding rows of ``aux``) behind a barrier; row r's D_i is  smalln_reduce<3>(red, i, r) + bias_i.
// The caller puts a barrier between its last read of ``red`` and the next call.
template <int RTC>
__device__ __forceinline__ void deform_eval(float* mainT, float* aux, float* red, const float* px, const float* pt, const Tabs& tb,
                                            const float4* __restrict__ packed, const float* __restrict__ weff, const QuadOff<RTC>& qo,
                                            int tid, int lane, int wave) {
    auto bias2 = [&](float(&b)[2], const float* __restrict__ bias) { b[0] = bias[64 * wave + (lane & 31)]; b[1] = bias[64 * wave + 32 + (lane & 31)]; };
    encode3<6>(aux, 0, px, tid);
    encode1<6>(aux, 39, pt, tid);
    zero_rows(aux, 52, 56, tid);
    __syncthreads();
    float bc[2], bn[2];   // this layer's and the NEXT layer's bias of this lane's two columns (requested a layer ahead)
    bias2(bn, weff + tb.boff[NET_D * LAYERS + 0]);
    {
        f32x16 acc[RTC][2];
        acc_zero(acc);
        bc[0] = bn[0]; bc[1] = bn[1];
        bias2(bn, weff + tb.boff[NET_D * LAYERS + 1]);
        gemm_seg<7, RTC, 2>(acc, aux, packed + tb.segoff[DF0], 0, 2 * wave, lane);
        for_quads_off(acc, qo, 0, 2 * wave, lane, [&](int row, int col, float(&v)[4], int off, int ni) {
            add_bias4(v, bc[ni]);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = relu1(v[i]);
            lds_store_quad_at(mainT, off, v);
        });
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 1; l <= 7; ++l) {
        f32x16 acc[RTC][2];
        acc_zero(acc);
        bc[0] = bn[0]; bc[1] = bn[1];
        if (l < 7) bias2(bn, weff + tb.boff[NET_D * LAYERS + l + 1]);
        gemm_seg<32, RTC, 2>(acc, mainT, packed + tb.segoff[DF0 + l], 0, 2 * wave, lane);
        __syncthreads();
        if (l == 3 && wave == 3) {      // (wave-uniform) IDR skip: next input = [h(204) | enc(52)] (1/sqrt2 folded into W4)
            for_quads_off(acc, qo, 0, 2 * wave, lane, [&](int row, int col, float(&v)[4], int off, int ni) {
                if (col >= 204) {
                    lds_load_quad(aux, col - 204, row, v);
                } else {
                    add_bias4(v, bc[ni]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = relu1(v[i]);
                }
                lds_store_quad_at(mainT, off, v);
            });
        } else {
            for_quads_off(acc, qo, 0, 2 * wave, lane, [&](int row, int col, float(&v)[4], int off, int ni) {
                add_bias4(v, bc[ni]);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = relu1(v[i]);
                lds_store_quad_at(mainT, off, v);
            });
        }
        __syncthreads();
    }
    smalln_partial<3>(mainT, weff + tb.woff[NET_D * LAYERS + 8], 256, red, tid);
    __syncthreads();
}

// x_c = x + D behind deform_eval: the tile's rows px plus D and its last-layer bias (at weff + b8) into xc -- px itself or another
// [3][64] -- behind a barrier, which is also the one deform_eval's contract asks for.
__device__ __forceinline__ void add_deform(float* xc, const float* px, const float* red, const float* weff, int b8, int tid) {
    if (tid < 192) {
        const int i = tid >> 6, row = tid & 63;
        xc[i * 64 + row] = px[i * 64 + row] + (smalln_reduce<3>(red, i, row) + weff[b8 + i]);
    }
    __syncthreads();
}

// The SDF network on the tile's canonical rows (pxc [3][64]), output column 0 only: leaves the four k-partial sums in ``red`` (which
// aliases the encoding rows of ``aux``) behind a barrier; row r's value is  smalln_reduce<1>(red, 0, r) + bias.  The caller puts a
// barrier between its last read of ``red`` and the next encoding.
template <int RTC>
__device__ __forceinline__ void sdf_eval(float* mainT, float* aux, float* red, const float* pxc, const Tabs& tb,
                                         const float4* __restrict__ packed, const float* __restrict__ weff, const QuadOff<RTC>& qo, int tid,
                                         int lane, int wave) {
    auto bias2 = [&](float(&b)[2], const float* __restrict__ bias) { b[0] = bias[64 * wave + (lane & 31)]; b[1] = bias[64 * wave + 32 + (lane & 31)]; };
    encode3<6>(aux, 0, pxc, tid);
    zero_rows(aux, 39, 40, tid);
    __syncthreads();
    float bc[2], bn[2];
    bias2(bn, weff + tb.boff[NET_S * LAYERS + 0]);
    {
        f32x16 acc[RTC][2];
        acc_zero(acc);
        bc[0] = bn[0]; bc[1] = bn[1];
        bias2(bn, weff + tb.boff[NET_S * LAYERS + 1]);
        gemm_seg<5, RTC, 2>(acc, aux, packed + tb.segoff[SF0], 0, 2 * wave, lane);
        for_quads_off(acc, qo, 0, 2 * wave, lane, [&](int row, int col, float(&v)[4], int off, int ni) {
            add_bias4(v, bc[ni]);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = softplus100(v[i]);
            lds_store_quad_at(mainT, off, v);
        });
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 1; l <= 7; ++l) {
        f32x16 acc[RTC][2];
        acc_zero(acc);
        bc[0] = bn[0]; bc[1] = bn[1];
        if (l < 7) bias2(bn, weff + tb.boff[NET_S * LAYERS + l + 1]);
        const int seg = l <= 4 ? SF0 + l : SF0 + l + 1;
        gemm_seg<32, RTC, 2>(acc, mainT, packed + tb.segoff[seg], 0, 2 * wave, lane);
        if (l == 4) gemm_seg<5, RTC, 2>(acc, aux, packed + tb.segoff[SF4A], 0, 2 * wave, lane);   // NeRF skip: + enc part
        __syncthreads();
        for_quads_off(acc, qo, 0, 2 * wave, lane, [&](int row, int col, float(&v)[4], int off, int ni) {
            add_bias4(v, bc[ni]);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = softplus100(v[i]);
            lds_store_quad_at(mainT, off, v);
        });
        __syncthreads();
    }
    smalln_partial<1>(mainT, weff + tb.woff[NET_S * LAYERS + 8], 256, red, tid);
    __syncthreads();
}

}  // namespace es
