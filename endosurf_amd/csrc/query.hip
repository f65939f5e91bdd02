// K2: fused no-grad SDF query  sdf(x + deform(x, t))  — the reference's
// EndoSurfNet.get_sdf_from_observed_space (endosurf.py:570-579: DeformNetwork.forward :724-738 then
// SDFNetwork.sdf :788-791), used by hierarchical up-sampling (:92, :281), ray marching (:375), the secant
// refinement (:435) and mesh extraction (:493).  One launch runs both 9-layer MLPs per 64-point tile with the
// activations resident in LDS; only 16 B/point are read and 4 B/point written.  The two MLPs are the bodies of field_eval.h, which the
// deformation kernels (deform.hip) and the surface tracer (trace.hip) run too: a row's value has this kernel's bits in all of them.
#include <cstdlib>

#include "chain_common.h"
#include "encode.h"
#include "field_eval.h"
#include "host.h"
#include "launch.h"
#include "tabs.h"
#include "timing.h"

namespace es {

// HALF: latency-bound small batches (secant iterations, 8-sample up-sampling queries) use 32-point tiles (LeanTile, field_eval.h).
template <bool DEFORM, bool HALF>
__global__ __launch_bounds__(NTHREADS, 2) void k_query_sdf(PointSrc src, Tabs tb, const float4* __restrict__ packed,
                                                        const float* __restrict__ weff, float* __restrict__ sdf_out, int ld_out,
                                                        const int* __restrict__ ray_done) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using Tile = LeanTile<HALF>;
    constexpr int RTC = Tile::RTC, PTS = Tile::PTS;
    float *mainT = lds + Tile::MAIN, *aux = lds + Tile::AUX, *red = lds + Tile::RED, *px = lds + Tile::PX, *pt = lds + Tile::PT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * PTS;
    if (ray_done != nullptr) {      // block-wise ray marching: a tile whose rays already have their first sign change is skipped
        const int r_first = row0 / src.n_per_ray, r_last = min(row0 + PTS - 1, src.M - 1) / src.n_per_ray;
        bool all_done = true;
        for (int r = r_first; r <= r_last; ++r) all_done = all_done && ray_done[r] != 0;
        if (all_done) return;       // workgroup-uniform
    }

    const QuadOff<RTC> qo = quad_offsets<RTC>(0, 2 * wave, lane);
    Tile::load_points(px, pt, src, row0, tid);
    if (DEFORM) {      // x_c = x + D(x, t), in place
        deform_eval<RTC>(mainT, aux, red, px, pt, tb, packed, weff, qo, tid, lane, wave);
        add_deform(px, px, red, weff, tb.boff[NET_D * LAYERS + 8], tid);
    }
    sdf_eval<RTC>(mainT, aux, red, px, tb, packed, weff, qo, tid, lane, wave);
    if (tid < PTS && row0 + tid < src.M) {
        const int i = row0 + tid;
        const size_t o = ld_out > 0 ? (size_t)(i / src.n_per_ray) * ld_out + (i % src.n_per_ray) : (size_t)i;   // [ray][ld_out] or flat
        sdf_out[o] = smalln_reduce<1>(red, 0, tid) + weff[tb.boff[NET_S * LAYERS + 8]];
    }
}

// tile_points: 0 = chosen by the batch size (<= 9 216 points: the 16-point tiles of query16.hip -- the up-sampling queries of 1 024 rays and
// the secant iterations are latency-bound on their own; <= 16 384: 32-point tiles, fewer than one 64-point tile per CU otherwise; above: 64),
// or 16 / 32 / 64 as the caller says.  A caller whose query SHARES the GPU with another chain of small launches asks for shorter tiles than
// the batch size alone suggests: the 32 768-point coarse query of a training step takes 0.48 ms on 512 64-point tiles when it runs alone,
// but next to the secant iterations those hold every workgroup slot for half a millisecond, while 1 024 32-point tiles turn the slots over
// twice as often (racing chains 1.42 -> 1.35 ms; 16-point tiles: 1.37 ms).
int query_sdf(const PointSrc& src, const float* packed, const float* weff, float* sdf_out, int use_deform, hipStream_t st,
              int ld_out, const int* ray_done, int tile_points) {
    int tp = tile_points ? tile_points : (src.M <= 9216 ? 16 : (src.M <= 16384 ? 32 : 64));
    if (tp == 16 && !(ld_out == 0 && ray_done == nullptr)) tp = 32;      // (the 16-point kernel writes flat outputs only)
    if (src.M > 0 && tp == 16)
        return query_sdf16(src, packed, weff, sdf_out, use_deform, st);   // latency-bound batches
    static constexpr decltype(&k_query_sdf<true, false>) KERNELS[] = {k_query_sdf<true, false>, k_query_sdf<true, true>,          // [(DEFORM ? 0 : 2) + HALF]
                                                                      k_query_sdf<false, false>, k_query_sdf<false, true>};
    static DeviceOnce attr_done;
    if (int e = allow_big_lds_once(attr_done, KERNELS, LEAN_LDS_BYTES)) return e;          // (here already: before the empty batch's return)
    if (src.M <= 0) return ST_OK;
    const Tabs tb = make_tabs();
    const bool half = tp == 32;
    ScopedTimer tm(ray_done ? KID_QUERY_EXIT : KID_QUERY, src.M, st);     // launches with early-exit tiles are not counted as work
    return launch_lean(KERNELS, attr_done, (use_deform ? 0 : 2) + half, LEAN_LDS_BYTES, src.M, half ? 32 : 64, st, "query_sdf", src, tb,
                       reinterpret_cast<const float4*>(packed), weff, sdf_out, ld_out, ray_done);
}

}  // namespace es
