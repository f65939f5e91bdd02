// Value, gradient and Hessian of the SDF network at canonical points, no grad: second-order forward mode in ONE launch and nothing
// saved -- no workspace, no mask words.  Ten MLP rows per point: row 0 the value, rows 1..3 the tangents along e_x,
// e_y, e_z, rows 4..9 the second tangents xx, xy, xz, yy, yz, zz.  The network is smooth (softplus, beta = 100), so the sweep is exact:
// with z the pre-activations of one column of one point, s = softplus(z_0), s' = 1 - exp(-100 s), s'' = 100 s' exp(-100 s),
//     h_0 = s,    h_j = s' z_j,    h_jk = s'' z_j z_k + s' z_jk,
// the bias added to the value row only.  The tile, LDS carve, packed weights, gemm_seg, bias prefetch and layer order are sdf_eval's
// (field_eval.h), so the value row's sums are taken in that order: a point's value is, bit for bit, es_query_sdf_tiles' without
// deformation on its 32- and 64-point tiles, whatever the row's place in the tile and whatever its neighbours hold.
//
// Row layout (jet.h): point q of a lane half takes slots 10 q .. 10 q + 9: three points per half, six per 64-row tile (60 of 64 rows),
// one per half and two per 32-row tile (20 of 32).  Every product of a point's rows is then between registers of one lane and the
// epilogue stays in registers.  Unused slots carry zeros.
// fp32 only, explicit points only; the time is not read.
#include "chain_common.h"
#include "encode.h"
#include "field_eval.h"
#include "host.h"
#include "jet.h"
#include "launch.h"
#include "tabs.h"

namespace es {

constexpr int HESS_ROWS = 10;          // MLP rows per point

template <bool HALF>
__global__ __launch_bounds__(NTHREADS, 2) void k_sdf_hessian(const float* __restrict__ x, int M, Tabs tb, const float4* __restrict__ packed,
                                                          const float* __restrict__ weff, float* __restrict__ sdf_out,
                                                          float* __restrict__ grad_out, float* __restrict__ hess_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using Tile = LeanTile<HALF>;
    constexpr int RTC = Tile::RTC;
    constexpr int PPH = jet_pph(HESS_ROWS, RTC), PTS = jet_pts(HESS_ROWS, RTC);          // points per lane half: 3, or 1 on the HALF tile
    float *mainT = lds + Tile::MAIN, *aux = lds + Tile::AUX, *red = lds + Tile::RED, *px = lds + Tile::PX;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pt0 = blockIdx.x * PTS;

    if (tid < 24) {          // px [3][64]: the tile's points (at or past M: zeros)
        const int c = tid >> 3, p = tid & 7;
        px[c * 64 + p] = (p < PTS && pt0 + p < M) ? x[3 * (size_t)(pt0 + p) + c] : 0.f;
    }
    zero_rows(aux, 0, 40, tid);
    __syncthreads();
    {   // encoding rows of tile point p = PPH hi + q, slots 10 q ..: the value row as encode3 writes it, tangent row j = d enc / d x_j
        // (non-zero in coordinate j's entries, 1 in its identity entry), second row jj = d2 enc / d x_j^2; the rows jk, j != k, stay zero
        const int p = tid & 7, item = tid >> 3;
        if (p < PTS && item < 19) {
            const int hi = p / PPH, s0 = HESS_ROWS * (p % PPH);
            jet_encode3<6>(aux, item, px, p, jet_row(s0, hi), [&](int c) { return jet_row(s0 + 1 + c, hi); },
                           [&](int c) { return jet_row(s0 + (c == 0 ? 4 : (c == 1 ? 7 : 9)), hi); });
        }
    }
    __syncthreads();

    const QuadOff<RTC> qo = quad_offsets<RTC>(0, 2 * wave, lane);
    auto bias2 = [&](float(&b)[2], const float* __restrict__ bias) { b[0] = bias[64 * wave + (lane & 31)]; b[1] = bias[64 * wave + 32 + (lane & 31)]; };
    // the second-order activation, in registers
    auto epi = [&](f32x16(&acc)[RTC][2], const float(&bc)[2]) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
            for (int p = 0; p < PPH; ++p) {
                float z[HESS_ROWS];
#pragma unroll
                for (int c = 0; c < HESS_ROWS; ++c) z[c] = jet_get(acc, ni, HESS_ROWS * p + c);
                const float s = softplus100(z[0] + bc[ni]);
                const float d1 = softplus100_grad_from_s(s);
                const float d2 = 100.f * d1 * __expf(-100.f * s);
                float h[HESS_ROWS];
                h[0] = s;
#pragma unroll
                for (int j = 0; j < 3; ++j) h[1 + j] = d1 * z[1 + j];
                int c = 4;
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int k = j; k < 3; ++k, ++c) h[c] = fmaf(d2 * z[1 + j], z[1 + k], d1 * z[c]);
#pragma unroll
                for (int cc = 0; cc < HESS_ROWS; ++cc) jet_set(acc, ni, HESS_ROWS * p + cc, h[cc]);
            }
        }
        for_quads_off(acc, qo, 0, 2 * wave, lane, [&](int row, int col, float(&v)[4], int off, int ni) { lds_store_quad_at(mainT, off, v); });
    };
    float bc[2], bn[2];          // this layer's and the NEXT layer's bias of this lane's two columns (requested a layer ahead)
    bias2(bn, weff + tb.boff[NET_S * LAYERS + 0]);
    {
        f32x16 acc[RTC][2];
        acc_zero(acc);
        bc[0] = bn[0]; bc[1] = bn[1];
        bias2(bn, weff + tb.boff[NET_S * LAYERS + 1]);
        gemm_seg<5, RTC, 2>(acc, aux, packed + tb.segoff[SF0], 0, 2 * wave, lane);
        epi(acc, bc);
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
        if (l == 4) gemm_seg<5, RTC, 2>(acc, aux, packed + tb.segoff[SF4A], 0, 2 * wave, lane);   // NeRF skip: + enc part, all ten rows
        __syncthreads();
        epi(acc, bc);
        __syncthreads();
    }
    smalln_partial<1>(mainT, weff + tb.woff[NET_S * LAYERS + 8], 256, red, tid);          // the last layer is linear: one row in, one row out
    __syncthreads();
    if (tid < 64) {
        const int row = tid, hi = (row >> 2) & 1, slot = jet_slot(row);
        const int q = slot / HESS_ROWS, c = slot - HESS_ROWS * q;
        if (q < PPH && pt0 + hi * PPH + q < M) {
            const size_t gp = (size_t)(pt0 + hi * PPH + q);
            const float val = smalln_reduce<1>(red, 0, row);
            if (c == 0) {
                if (sdf_out) sdf_out[gp] = val + weff[tb.boff[NET_S * LAYERS + 8]];
            } else if (c < 4) {
                if (grad_out) grad_out[gp * 3 + (c - 1)] = val;
            } else if (hess_out) {          // both mirror entries from the same register
                const int j = c < 7 ? 0 : (c < 9 ? 1 : 2), k = c < 7 ? c - 4 : (c < 9 ? c - 6 : 2);
                hess_out[gp * 9 + 3 * j + k] = val;
                hess_out[gp * 9 + 3 * k + j] = val;
            }
        }
    }
}

// The 32-row tile up to this many points, the 64-row tile above.  The family's threshold of 16 384 MLP rows (deform.hip, deform_jet.hip)
// would be 1 638 points at ten rows per point; it is lower here because the short tile carries points on 20 of its 32 rows where the
// tall one has 60 of 64.  Measured, 32- against 64-row tiles: 0.090 against 0.144 ms at 512 points (256 short tiles, one
// per CU), 0.141 against 0.142 at 1 024, 0.205 against 0.144 at 1 280, 0.207 against 0.145 at 1 536.
constexpr int HESSIAN_HALF_MAX_POINTS = 1024;

int sdf_hessian(const float* x, int M, const float* packed, const float* weff, int tile_rows, float* sdf_out, float* grad_out,
                float* hess_out, hipStream_t st) {
    if (M <= 0) return ST_OK;
    static constexpr decltype(&k_sdf_hessian<false>) KERNELS[] = {k_sdf_hessian<false>, k_sdf_hessian<true>};          // [HALF]
    static DeviceOnce attr_done;
    const bool half = tile_rows ? tile_rows == 32 : M <= HESSIAN_HALF_MAX_POINTS;
    return launch_lean(KERNELS, attr_done, half, LEAN_LDS_BYTES, M, jet_pts(HESS_ROWS, half ? 1 : 2), st, "sdf_hessian", x, M, make_tabs(),
                       reinterpret_cast<const float4*>(packed), weff, sdf_out, grad_out, hess_out);
}

}  // namespace es
