// The forward-mode derivatives of the deformation map  x_c = x + D(x, t)  at a point, in ONE launch and nothing saved: no mask words,
// no u_l streams, no workspace.  One kernel, k_deform_jet<ROWS, HALF>, carries a point as ROWS MLP rows (a jet, jet.h):
//     slot 0 the value;  1..3 the tangents along e_x, e_y, e_z;  and for ROWS == 8:  4 the time tangent;  5..7 the second tangents xx, yy, zz.
// ROWS == 4 is the Jacobian J = I + dD/dx (reference get_deform_grad_from_observed_space, endosurf.py:621-658).
// ROWS == 8 adds the time derivative D_t = dD/dt and the pure second derivatives dd[i][k] = d2 D_i / d x_k^2: D is a
// ReLU MLP over an encoding that is separable by coordinate, so inside a linear region the mixed second derivatives (x_j x_k, j != k,
// and x_j t) vanish identically and these eight rows are the whole second-order picture.
// The scheme is deform_fwd_tile's (point_fwd_bodies.h): same LDS carve, packed weights, gemm_seg, bias prefetch and skip-layer
// instantiation, hence the same sums in the same order.  A row's J is, entry for entry, what three launches of the point forward along
// e_0, e_1, e_2 give, and jac_out and xc_out have the same bits at four and at eight rows.  Point q of lane half hi takes slots
// ROWS q .. ROWS q + ROWS - 1 (one quad, or two quads of one lane eight rows apart), so the value slot's ReLU mask gates its
// companions in registers.  Every row of the tile carries a point: 16 or 8 points on the 64-row tile, 8 or 4 on the 32-row tile.  A
// row's result does not depend on its place in the tile, on its neighbours or on the tile height.  fp32 only, explicit points only.
#include "chain_common.h"
#include "encode.h"
#include "field_eval.h"
#include "host.h"
#include "jet.h"
#include "launch.h"
#include "tabs.h"

namespace es {

// HALF: the 32-row tile (row tile 0 of the same LDS layout; every layer issues half the MFMAs and twice as many workgroups share the
// batch), as k_deform_forward's small tiles; a row's arithmetic is the same in both.
template <int ROWS, bool HALF>
__global__ __launch_bounds__(NTHREADS, 2) void k_deform_jet(PointSrc src, Tabs tb, const float4* __restrict__ packed,
                                                         const float* __restrict__ weff, float* __restrict__ jac_out,
                                                         float* __restrict__ dt_out, float* __restrict__ dd_out,
                                                         float* __restrict__ xc_out) {
    static_assert(ROWS == 4 || ROWS == 8, "value and three tangents, or those, the time tangent and three second tangents");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using Tile = LeanTile<HALF>;
    constexpr int RTC = Tile::RTC;
    constexpr int PPH = jet_pph(ROWS, RTC), PTS = jet_pts(ROWS, RTC);
    constexpr int PW = jet_pts(ROWS, 2);          // threads tid, tid + PW, ... share a point in the encoding
    float *mainT = lds + Tile::MAIN, *aux = lds + Tile::AUX, *red = lds + Tile::RED, *px = lds + Tile::PX, *pt = lds + Tile::PT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pt0 = blockIdx.x * PTS;

    if (tid < 16) {
        float x[3], t, d[3];
        load_point(src, tid < PTS ? pt0 + tid : src.M, x, t, d);          // (rows past the tile's points or at or past M: zeros)
        px[tid] = x[0]; px[64 + tid] = x[1]; px[128 + tid] = x[2]; pt[tid] = t;
    }
    zero_rows(aux, 0, 56, tid);
    __syncthreads();
    {   // encoding rows of tile point p = PPH hi + q, slots ROWS q ..: 18 items of space, 6 of time (entries from 39), one of identities
        const int p = tid % PW;
        for (int item = tid / PW; item < 25 && p < PTS; item += NTHREADS / PW) {
            const int hi = p / PPH, s0 = ROWS * (p % PPH);
            const int r0 = jet_row(s0, hi), rt = ROWS == 8 ? jet_row(s0 + 4, hi) : -1;
            auto tan = [&](int c) { return jet_row(s0 + 1 + c, hi); };
            auto sec = [&](int c) { return ROWS == 8 ? jet_row(s0 + 5 + c, hi) : -1; };
            if (item < 18) {
                jet_encode3<6>(aux, item, px, p, r0, tan, sec);
            } else if (item < 24) {
                jet_encode1<6>(aux, 39, item - 18, pt[p], r0, rt);
            } else {
                jet_encode3<6>(aux, 18, px, p, r0, tan, sec);
                jet_encode1<6>(aux, 39, 6, pt[p], r0, rt);
            }
        }
    }
    __syncthreads();

    // Epilogue as deform_fwd_tile's, minus everything it saves: the value slot's ReLU mask gates its ROWS - 1 companions in registers,
    // then the quads go to LDS.  No per-lane branch in the regular layers (the skip layer's copy, l == 3 and columns >= 204, wave 3
    // only, is its own instantiation behind a wave-uniform test); the bias is requested a layer ahead.
    const QuadOff<RTC> qo = quad_offsets<RTC>(0, 2 * wave, lane);
    auto bias2 = [&](float(&b)[2], int l) {
        const float* bias = weff + tb.boff[NET_D * LAYERS + l] + 64 * wave + (lane & 31);
        b[0] = bias[0]; b[1] = bias[32];
    };
    auto epi = [&](f32x16(&acc)[RTC][2], const float(&bc)[2], auto SKIP) {
        // point by point in for_quads_off's order (row tile, n-tile, quad), so that a point's store is issued under the next one's gating
#pragma unroll
        for (int ri = 0; ri < RTC; ++ri) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
                for (int s0 = 16 * ri; s0 < 16 * ri + 16; s0 += ROWS) {          // the point at slots s0 .. s0 + ROWS - 1
                    float z[ROWS / 4][4];          // its quads: four slots are four consecutive rows
#pragma unroll
                    for (int c = 0; c < ROWS; ++c) z[c >> 2][c & 3] = jet_get(acc, ni, s0 + c);
                    const int col = 32 * (2 * wave + ni) + (lane & 31);
                    if (decltype(SKIP)::value && col >= 204) {
#pragma unroll
                        for (int k = 0; k < ROWS / 4; ++k)          // IDR skip: next input = [h(204) | enc(52)] (1/sqrt2 folded into W4), every row of the jet
                            lds_load_quad(aux, col - 204, jet_row(s0 + 4 * k, lane >> 5), z[k]);
                    } else {
                        const float a0 = z[0][0] + bc[ni];
                        const bool m = a0 > 0.f;                         // the ReLU mask of the value row gates its companions
#pragma unroll
                        for (int c = 1; c < ROWS; ++c) z[c >> 2][c & 3] = m ? z[c >> 2][c & 3] : 0.f;
                        z[0][0] = m ? a0 : 0.f;
                    }
#pragma unroll
                    for (int k = 0; k < ROWS / 4; ++k) lds_store_quad_at(mainT, qo.o[(s0 >> 2) + k] + 2048 * ni, z[k]);          // (for_quads_off's offsets)
                }
            }
        }
    };
    float bc[2], bn[2];
    bias2(bn, 0);
    {
        f32x16 acc[RTC][2];
        acc_zero(acc);
        bc[0] = bn[0]; bc[1] = bn[1];
        bias2(bn, 1);
        gemm_seg<7, RTC, 2>(acc, aux, packed + tb.segoff[DF0], 0, 2 * wave, lane);
        epi(acc, bc, std::false_type{});
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 1; l <= 7; ++l) {
        f32x16 acc[RTC][2];
        acc_zero(acc);
        bc[0] = bn[0]; bc[1] = bn[1];
        if (l < 7) bias2(bn, l + 1);
        gemm_seg<32, RTC, 2>(acc, mainT, packed + tb.segoff[DF0 + l], 0, 2 * wave, lane);
        __syncthreads();
        if (l == 3 && wave == 3) epi(acc, bc, std::true_type{});
        else epi(acc, bc, std::false_type{});
        __syncthreads();
    }
    smalln_partial<3>(mainT, weff + tb.woff[NET_D * LAYERS + 8], 256, red, tid);
    __syncthreads();
    if (tid < 192) {
        const int i = tid >> 6, row = tid & 63, hi = (row >> 2) & 1, slot = jet_slot(row);
        const int q = slot / ROWS, c = slot - ROWS * q, p = PPH * hi + q;
        if (q < PPH && pt0 + p < src.M) {
            const float val = smalln_reduce<3>(red, i, row);
            const size_t gp = (size_t)(pt0 + p);
            if (c == 0) {
                if (xc_out) xc_out[gp * 3 + i] = px[i * 64 + p] + val + weff[tb.boff[NET_D * LAYERS + 8] + i];
            } else if (c < 4) {
                if (jac_out) jac_out[gp * 9 + i * 3 + (c - 1)] = val + (i == c - 1 ? 1.f : 0.f);          // J e_j = e_j + (dD/dx) e_j
            } else if (c == 4) {
                if (dt_out) dt_out[gp * 3 + i] = val;
            } else if (dd_out) {
                dd_out[gp * 9 + i * 3 + (c - 5)] = val;
            }
        }
    }
}

// The 32-row tile up to this many points, the 64-row tile above.
// Four rows per point: k_deform_forward's threshold in MLP rows (16 384 rows, deform.hip).  Measured, 8- against
// 16-point tiles: 0.084 against 0.137 ms at 2 048 points, 0.137 against 0.139 at 2 630, 0.141 against 0.141 at 4 096; 0.268 against
// 0.252 at 8 192 and 6 % slower from there on.
constexpr int JACOBIAN_HALF_MAX_POINTS = 4096;
// Eight rows per point: that rule would give 2 048 points; it is higher here because three short tiles per CU (3 072 points on 256 CUs)
// still finish before two tall ones.  Measured, 32- against 64-row tiles: 0.075 against 0.128 ms at 512 points, 0.080
// against 0.132 at 1 024, 0.140 against 0.139 at 2 048, 0.195 against 0.239 at 2 630, 0.200 against 0.239 at 3 072; 0.257 against 0.242
// at 4 096, 0.379 against 0.363 at 6 144, 0.504 against 0.477 at 8 192.
constexpr int KINEMATICS_HALF_MAX_POINTS = 3072;

template <int ROWS>
static int deform_jet(const PointSrc& src, int half_max_points, const char* name, const float* packed, const float* weff, float* jac_out,
                      float* dt_out, float* dd_out, float* xc_out, hipStream_t st) {
    if (src.M <= 0) return ST_OK;
    static constexpr decltype(&k_deform_jet<ROWS, false>) KERNELS[] = {k_deform_jet<ROWS, false>, k_deform_jet<ROWS, true>};          // [HALF]
    static DeviceOnce attr_done;
    const bool half = src.M <= half_max_points;
    return launch_lean(KERNELS, attr_done, half, LEAN_LDS_BYTES, src.M, jet_pts(ROWS, half ? 1 : 2), st, name, src, make_tabs(),
                       reinterpret_cast<const float4*>(packed), weff, jac_out, dt_out, dd_out, xc_out);
}

int deform_jacobian(const PointSrc& src, const float* packed, const float* weff, float* jac_out, float* xc_out, hipStream_t st) {
    return deform_jet<4>(src, JACOBIAN_HALF_MAX_POINTS, "deform_jacobian", packed, weff, jac_out, nullptr, nullptr, xc_out, st);
}

int deform_derivatives(const PointSrc& src, const float* packed, const float* weff, float* jac_out, float* dt_out, float* dd_out,
                       float* xc_out, hipStream_t st) {
    return deform_jet<8>(src, KINEMATICS_HALF_MAX_POINTS, "deform_derivatives", packed, weff, jac_out, dt_out, dd_out, xc_out, st);
}

}  // namespace es
