// The Jacobian of the deformation map, J(x, t) = I + dD/dx of  x_c = x + D(x, t)  (reference get_deform_grad_from_observed_space,
// endosurf.py:621-658), value and all three forward tangents in ONE launch and nothing saved: no mask words, no u_l streams, no
// workspace.  The scheme is deform_fwd_tile's (point_fwd_bodies.h), restated for four rows per point: row 4p is the value, rows
// 4p + 1 + j carry the tangent along e_j, so a quad of the MFMA result -- four consecutive rows of one column -- is one point, and
// the ReLU mask of its value row gates its three tangent rows in the epilogue.  Same LDS carve, packed weights, bias prefetch and
// skip-layer instantiation as there, hence the same sums in the same order: a row's J is, entry for entry, what three launches of
// the point forward along e_0, e_1, e_2 give, whatever the row's place in the tile and whatever its neighbours hold.
// fp32 only, explicit points only.
#include "chain_common.h"
#include "encode.h"
#include "host.h"
#include "launch.h"
#include "tabs.h"

namespace es {

// HALF: 8 points = 32 rows per workgroup (row tile 0 of the same LDS layout; every layer issues half the MFMAs and twice as many
// workgroups share the batch), as k_deform_forward's small tiles; a row's arithmetic is the same in both.
template <bool HALF>
__global__ __launch_bounds__(NTHREADS, 2) void k_deform_jacobian(PointSrc src, Tabs tb, const float4* __restrict__ packed,
                                                              const float* __restrict__ weff, float* __restrict__ jac_out,
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
    constexpr int PTS = HALF ? 8 : 16;
    const int pt0 = blockIdx.x * PTS;

    if (tid < 16) {
        float x[3], t, d[3];
        load_point(src, tid < PTS ? pt0 + tid : src.M, x, t, d);          // (rows past the tile's points or at or past M: zeros)
        px[tid] = x[0]; px[16 + tid] = x[1]; px[32 + tid] = x[2]; pt[tid] = t;
    }
    zero_rows(aux, 0, 56, tid);
    __syncthreads();
    {   // encoding rows: value row 4p, tangent row 4p + 1 + c = d enc / d x_c (non-zero in the entries of coordinate c only); the
        // time part has no tangent
        const int p = tid & 15;
        for (int item = tid >> 4; item < 25 && p < PTS; item += 16) {
            if (item < 18) {
                const int c = item % 3, i = item / 3;
                const float f = (float)(1 << i);
                float s, co;
                sincosf(px[c * 16 + p] * f, &s, &co);
                aux[swz(enc_index(3, i, 0, c), 4 * p)] = s;
                aux[swz(enc_index(3, i, 1, c), 4 * p)] = co;
                aux[swz(enc_index(3, i, 0, c), 4 * p + 1 + c)] = f * co;
                aux[swz(enc_index(3, i, 1, c), 4 * p + 1 + c)] = -f * s;
            } else if (item < 24) {
                const int i = item - 18;
                float s, co;
                sincosf(pt[p] * (float)(1 << i), &s, &co);
                aux[swz(39 + enc_index(1, i, 0, 0), 4 * p)] = s;
                aux[swz(39 + enc_index(1, i, 1, 0), 4 * p)] = co;
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) { aux[swz(c, 4 * p)] = px[c * 16 + p]; aux[swz(c, 4 * p + 1 + c)] = 1.f; }
                aux[swz(39, 4 * p)] = pt[p];
            }
        }
    }
    __syncthreads();

    // Epilogue as deform_fwd_tile's, minus everything it saves: no per-lane branch in the regular layers (the skip layer's copy,
    // l == 3 and columns >= 204, wave 3 only, is its own instantiation behind a wave-uniform test), the bias requested a layer ahead.
    const QuadOff<RTC> qo = quad_offsets<RTC>(0, 2 * wave, lane);
    auto bias2 = [&](float(&b)[2], int l) {
        const float* bias = weff + tb.boff[NET_D * LAYERS + l] + 64 * wave + (lane & 31);
        b[0] = bias[0]; b[1] = bias[32];
    };
    auto epi = [&](f32x16(&acc)[RTC][2], const float(&bc)[2], auto SKIP) {
        for_quads_off(acc, qo, 0, 2 * wave, lane, [&](int row, int col, float(&v)[4], int off, int ni) {      // rows: value, three tangents
            if (decltype(SKIP)::value && col >= 204) {
                lds_load_quad(aux, col - 204, row, v);          // IDR skip: next input = [h(204) | enc(52)] (1/sqrt2 folded into W4)
            } else {
                const float a0 = v[0] + bc[ni];
                const bool m = a0 > 0.f;                         // the ReLU mask of the value row gates its tangents
                v[0] = m ? a0 : 0.f; v[1] = m ? v[1] : 0.f; v[2] = m ? v[2] : 0.f; v[3] = m ? v[3] : 0.f;
            }
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
        const int i = tid >> 6, row = tid & 63, p = row >> 2, c = row & 3;
        if (p < PTS && pt0 + p < src.M) {
            const float val = smalln_reduce<3>(red, i, row);
            const size_t gp = (size_t)(pt0 + p);
            if (c == 0) {
                if (xc_out) xc_out[gp * 3 + i] = px[i * 16 + p] + val + weff[tb.boff[NET_D * LAYERS + 8] + i];
            } else if (jac_out) {
                jac_out[gp * 9 + i * 3 + (c - 1)] = val + (i == c - 1 ? 1.f : 0.f);          // J e_j = e_j + (dD/dx) e_j
            }
        }
    }
}

// 8-point tiles up to this many points, 16-point tiles above: k_deform_forward's threshold in MLP rows (16 384 rows, deform.hip).
// Measured, 8- against 16-point tiles: 0.084 against 0.137 ms at 2 048 points, 0.137 against 0.139 at 2 630, 0.141
// against 0.141 at 4 096; 0.268 against 0.252 at 8 192 and 6 % slower from there on.
constexpr int JACOBIAN_HALF_MAX_POINTS = 4096;

int deform_jacobian(const PointSrc& src, const float* packed, const float* weff, float* jac_out, float* xc_out, hipStream_t st) {
    if (src.M <= 0) return ST_OK;
    static constexpr decltype(&k_deform_jacobian<false>) KERNELS[] = {k_deform_jacobian<false>, k_deform_jacobian<true>};          // [HALF]
    static DeviceOnce attr_done;
    if (int e = allow_big_lds_once(attr_done, KERNELS, LEAN_LDS_BYTES)) return e;
    const bool half = src.M <= JACOBIAN_HALF_MAX_POINTS;
    const int pts = half ? 8 : 16;
    const dim3 grid((src.M + pts - 1) / pts), block(NTHREADS);
    const float4* pk = reinterpret_cast<const float4*>(packed);
    hipLaunchKernelGGL(KERNELS[half], grid, block, LEAN_LDS_BYTES, st, src, make_tabs(), pk, weff, jac_out, xc_out);
    return hip_last("deform_jacobian");
}

}  // namespace es
