// Everything the kinematics of the deformation map need at a point, in ONE launch and nothing saved: the value
// x_c = x + D(x, t), the Jacobian J = I + dD/dx, the time derivative D_t = dD/dt and the pure second derivatives
// dd[i][k] = d2 D_i / d x_k^2.  D is a ReLU MLP over an encoding that is separable by coordinate, so inside a linear region the mixed
// second derivatives (x_j x_k, j != k, and x_j t) vanish identically and these eight MLP rows per point are the whole second-order
// picture:
//     slot 0 the value;  1..3 the tangents along e_x, e_y, e_z;  4 the time tangent;  5..7 the second tangents xx, yy, zz.
// The scheme is k_deform_jacobian's (deform_jac.hip) restated for eight rows: same LDS carve, packed weights, gemm_seg, bias prefetch
// and skip-layer instantiation, hence the same sums in the same order -- jac_out and xc_out are es_deform_jacobian's bit for bit.
// The row layout is k_sdf_hessian's (row_slots.h): point q of lane half hi takes slots 8 q .. 8 q + 7, two quads of one lane eight
// rows apart, so the value slot's ReLU mask gates its seven companions in registers.  Every row of the tile carries a point: 8 points
// on the 64-row tile, 4 on the 32-row tile.  A row's result does not depend on its place in the tile, on its neighbours or on the
// tile height.  fp32 only, explicit points only.
#include "chain_common.h"
#include "encode.h"
#include "host.h"
#include "launch.h"
#include "row_slots.h"
#include "tabs.h"

namespace es {

constexpr int KIN_ROWS = 8;          // MLP rows per point

template <bool HALF>
__global__ __launch_bounds__(NTHREADS, 2) void k_deform_kinematics(PointSrc src, Tabs tb, const float4* __restrict__ packed,
                                                                const float* __restrict__ weff, float* __restrict__ jac_out,
                                                                float* __restrict__ dt_out, float* __restrict__ dd_out,
                                                                float* __restrict__ xc_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* mainT = lds;
    float* aux = lds + MAIN_FLOATS;
    float* scr = aux + AUX56_FLOATS;
    float* px = scr;          // [3][16]
    float* pt = scr + 48;     // [16]
    float* red = aux;         // [4][3][64]: the encoding rows are dead after layer 3's epilogue
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int RTC = HALF ? 1 : 2;
    constexpr int PPH = 16 * RTC / KIN_ROWS;          // points per lane half: 4, or 2 on the HALF tile
    constexpr int PTS = 2 * PPH;
    const int pt0 = blockIdx.x * PTS;

    if (tid < 16) {
        float x[3], t, d[3];
        load_point(src, tid < PTS ? pt0 + tid : src.M, x, t, d);          // (rows past the tile's points or at or past M: zeros)
        px[tid] = x[0]; px[16 + tid] = x[1]; px[32 + tid] = x[2]; pt[tid] = t;
    }
    zero_rows(aux, 0, 56, tid);
    __syncthreads();
    {   // encoding rows of tile point p = PPH hi + q, slots 8 q ..: the value row; tangent row 1 + c = d enc / d x_c (non-zero in the
        // entries of coordinate c only); the time tangent row 4 = d enc / d t (1 in the time identity entry, index 39); second row
        // 5 + c = d2 enc / d x_c^2 (nothing in the identity part)
        const int p = tid & 7, item = tid >> 3;
        if (p < PTS && item < 25) {
            const int hi = p / PPH, s0 = KIN_ROWS * (p % PPH);
            const int r0 = hess_row(s0, hi);
            if (item < 18) {
                const int c = item % 3, i = item / 3;
                const int r1 = hess_row(s0 + 1 + c, hi), r2 = hess_row(s0 + 5 + c, hi);
                const float f = (float)(1 << i);
                float s, co;
                sincosf(px[c * 16 + p] * f, &s, &co);
                const int ks = enc_index(3, i, 0, c), kc = enc_index(3, i, 1, c);
                aux[swz(ks, r0)] = s;
                aux[swz(kc, r0)] = co;
                aux[swz(ks, r1)] = f * co;
                aux[swz(kc, r1)] = -f * s;
                aux[swz(ks, r2)] = -(f * f) * s;
                aux[swz(kc, r2)] = -(f * f) * co;
            } else if (item < 24) {
                const int i = item - 18;
                const int r4 = hess_row(s0 + 4, hi);
                const float f = (float)(1 << i);
                float s, co;
                sincosf(pt[p] * f, &s, &co);
                const int ks = 39 + enc_index(1, i, 0, 0), kc = 39 + enc_index(1, i, 1, 0);
                aux[swz(ks, r0)] = s;
                aux[swz(kc, r0)] = co;
                aux[swz(ks, r4)] = f * co;
                aux[swz(kc, r4)] = -f * s;
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) { aux[swz(c, r0)] = px[c * 16 + p]; aux[swz(c, hess_row(s0 + 1 + c, hi))] = 1.f; }
                aux[swz(39, r0)] = pt[p];
                aux[swz(39, hess_row(s0 + 4, hi))] = 1.f;
            }
        }
    }
    __syncthreads();

    // Epilogue as k_deform_jacobian's, for two quads per point: slot s of n-tile ni is acc[s >> 4][ni][s & 15], the value slot's mask
    // gates the other seven in registers, then the quads go to LDS (the skip layer's copy, l == 3 and columns >= 204, wave 3 only, is
    // its own instantiation behind a wave-uniform test).  The bias is requested a layer ahead.
    const QuadOff<RTC> qo = quad_offsets<RTC>(0, 2 * wave, lane);
    auto bias2 = [&](float(&b)[2], int l) {
        const float* bias = weff + tb.boff[NET_D * LAYERS + l] + 64 * wave + (lane & 31);
        b[0] = bias[0]; b[1] = bias[32];
    };
    auto epi = [&](f32x16(&acc)[RTC][2], const float(&bc)[2], auto SKIP) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
            for (int p = 0; p < PPH; ++p) {
                constexpr int H = KIN_ROWS;
                const float a0 = acc[(H * p) >> 4][ni][(H * p) & 15] + bc[ni];
                const bool m = a0 > 0.f;                         // the ReLU mask of the value row gates its companions
                acc[(H * p) >> 4][ni][(H * p) & 15] = m ? a0 : 0.f;
#pragma unroll
                for (int c = 1; c < H; ++c) {
                    const float z = acc[(H * p + c) >> 4][ni][(H * p + c) & 15];
                    acc[(H * p + c) >> 4][ni][(H * p + c) & 15] = m ? z : 0.f;
                }
            }
        }
        for_quads_off(acc, qo, 0, 2 * wave, lane, [&](int row, int col, float(&v)[4], int off, int ni) {
            if (decltype(SKIP)::value && col >= 204) lds_load_quad(aux, col - 204, row, v);   // IDR skip: next input = [h(204) | enc(52)], all eight rows
            lds_store_quad_at(mainT, off, v);
        });
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
        const int i = tid >> 6, row = tid & 63, hi = (row >> 2) & 1, slot = hess_slot(row);
        const int q = slot / KIN_ROWS, c = slot - KIN_ROWS * q, p = PPH * hi + q;
        if (q < PPH && pt0 + p < src.M) {
            const float val = smalln_reduce<3>(red, i, row);
            const size_t gp = (size_t)(pt0 + p);
            if (c == 0) {
                if (xc_out) xc_out[gp * 3 + i] = px[i * 16 + p] + val + weff[tb.boff[NET_D * LAYERS + 8] + i];
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

// The 4-point (32-row) tile up to this many points, the 8-point (64-row) tile above.  The family's rule of 16 384 MLP rows (deform.hip,
// deform_jac.hip) would be 2 048 points at eight rows per point; it is higher here because three short tiles per CU (3 072 points on
// 256 CUs) still finish before two tall ones.  Measured, 32- against 64-row tiles: 0.075 against 0.128 ms at 512 points,
// 0.080 against 0.132 at 1 024, 0.140 against 0.139 at 2 048, 0.195 against 0.239 at 2 630, 0.200 against 0.239 at 3 072; 0.257 against
// 0.242 at 4 096, 0.379 against 0.363 at 6 144, 0.504 against 0.477 at 8 192.
constexpr int KINEMATICS_HALF_MAX_POINTS = 3072;

int deform_derivatives(const PointSrc& src, const float* packed, const float* weff, float* jac_out, float* dt_out, float* dd_out,
                       float* xc_out, hipStream_t st) {
    if (src.M <= 0) return ST_OK;
    static constexpr decltype(&k_deform_kinematics<false>) KERNELS[] = {k_deform_kinematics<false>, k_deform_kinematics<true>};          // [HALF]
    static DeviceOnce attr_done;
    if (int e = allow_big_lds_once(attr_done, KERNELS, LEAN_LDS_BYTES)) return e;
    const bool half = src.M <= KINEMATICS_HALF_MAX_POINTS;
    const int pts = half ? 4 : 8;
    const dim3 grid((src.M + pts - 1) / pts), block(NTHREADS);
    const float4* pk = reinterpret_cast<const float4*>(packed);
    hipLaunchKernelGGL(KERNELS[half], grid, block, LEAN_LDS_BYTES, st, src, make_tabs(), pk, weff, jac_out, dt_out, dd_out, xc_out);
    return hip_last("deform_derivatives");
}

}  // namespace es
