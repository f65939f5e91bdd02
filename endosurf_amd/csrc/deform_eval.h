// One evaluation of the deformation network on a tile's rows, shared by the kernels that loop it inside one launch: the inverse of the
// deformation (deform.hip) and the surface tracer (trace.hip).  It is the deformation half of k_query_sdf (query.hip), statement by
// statement, so D of a row has that kernel's bits whatever the row's place in the tile and whatever its neighbours hold.
#pragma once
#include "chain_common.h"
#include "encode.h"
#include "tabs.h"

namespace es {

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

}  // namespace es
