// Segment visibility, no grad: is the straight segment from a to b free of the level set  sdf(x + D(x, t)) = tau, up to a margin before
// b -- the per-row rule of endosurf_amd/flow.py segment_visible (DESIGN.md 7o "Segment rule"), the whole walk of a tile's segments in ONE
// launch.  Built on field_eval.h exactly as k_trace_surface (trace.hip) is: the lean tile of 32 or 64 rows, the LDS carve of that
// kernel, deform_eval then sdf_eval per round, the row state in the row thread's registers, frozen rows riding through the MFMAs
// unchanged.  Hence the value a row sees is, bit for bit, what es_query_sdf_tiles returns for that point on its 32- and 64-point tiles,
// whatever the row's place in the tile and whatever its neighbours hold.  fp32 only.  No refinement, no bracket: a row stops at the
// first value <= 0, or when the end of its tested part has itself been evaluated.
#include <cfloat>

#include "chain_common.h"
#include "encode.h"
#include "field_eval.h"
#include "host.h"
#include "launch.h"
#include "tabs.h"

namespace es {

struct VisibleArgs {
    const float* origins;       // [M][3]
    const float* points;        // [M][3]
    const float* t;             // [M], or one value with t_scalar
    int M, t_scalar, max_iters;
    float margin, tau, relax, min_step;
    int* status;                // [M]
    int* iters;                 // [M], nullable
    float* blocker;             // [M], nullable
    float* clearance;           // [M], nullable
    float* free_to;             // [M], nullable
};

constexpr int VIS_LIVE = 0, VIS_FREE = ES_VISIBLE_FREE, VIS_OCCLUDED = ES_VISIBLE_OCCLUDED, VIS_UNKNOWN = ES_VISIBLE_UNKNOWN;
constexpr int VIS_LDS_BYTES = LEAN_LDS_BYTES + 192 * 4;          // trace.hip's TRACE_LDS_BYTES: + the canonical rows, two workgroups per CU

// Product by product and sum by sum, as the twin takes them (trace.hip mul_rn: under -ffp-contract=fast a product that feeds a sum is
// fused into it unless the optimiser cannot look through it).
__device__ __forceinline__ float vis_mul(float a, float b) {
    float p = a * b;
    asm("" : "+v"(p));
    return p;
}
__device__ __forceinline__ float vis_dot(const float (&a)[3], const float (&b)[3]) {
    return __fadd_rn(__fadd_rn(vis_mul(a[0], b[0]), vis_mul(a[1], b[1])), vis_mul(a[2], b[2]));
}
// The correctly rounded root, as the twin's: __fsqrt_rn is the hardware's approximate one unless the rounded OCML operations are configured in.
__device__ __forceinline__ float vis_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ float vis_clamp0(float v) { return v < 0.f ? 0.f : v; }          // torch.clamp(min=0): a NaN stays a NaN
__device__ __forceinline__ bool vis_finite(float v) { return fabsf(v) <= FLT_MAX; }

// The row's thread (tid < PTS) keeps a, u, s, s_end, last, status, iters, blocker, clearance and free_to in registers; px / pt hold the current
// point and time of every row, px rewritten for live rows only.  Every workgroup runs at most max_iters evaluations -- an argument the
// ABI has validated -- and leaves the loop when none of its own rows is live: it waits for nothing outside itself.
template <bool DEFORM, bool HALF>
__global__ __launch_bounds__(NTHREADS, 2) void k_segment_visible(VisibleArgs a, Tabs tb, const float4* __restrict__ packed,
                                                              const float* __restrict__ weff) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using Tile = LeanTile<HALF>;
    constexpr int RTC = Tile::RTC, PTS = Tile::PTS;
    float *mainT = lds + Tile::MAIN, *aux = lds + Tile::AUX, *red = lds + Tile::RED, *px = lds + Tile::PX, *pt = lds + Tile::PT;
    float* pxc = lds + Tile::END;          // [3][64]: the canonical point x + D of the point under evaluation (px)
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * PTS;
    const bool mine = tid < PTS && row0 + tid < a.M;          // this thread owns a segment of the batch
    const float inf = __builtin_inff();
    // (kept in vector registers through the two networks' loops, as in k_trace_surface)
    float tau = a.tau, relax = a.relax, min_step = a.min_step;
    float *blocker_out = a.blocker, *clearance_out = a.clearance, *free_to_out = a.free_to;
    int *status_out = a.status, *iters_out = a.iters;
    int n_rows = a.M, b8d = tb.boff[NET_D * LAYERS + 8], b8s = tb.boff[NET_S * LAYERS + 8];          // (the last layers' bias offsets)
    asm volatile("" : "+v"(tau), "+v"(relax), "+v"(min_step), "+v"(blocker_out), "+v"(clearance_out), "+v"(free_to_out), "+v"(status_out), "+v"(iters_out),
                 "+v"(n_rows), "+v"(b8d), "+v"(b8s));
    float o[3] = {0.f, 0.f, 0.f}, u[3] = {0.f, 0.f, 0.f};
    float s = 0.f, s_end = 0.f, blocker = inf, clearance = inf, free_to = -inf;
    int status = VIS_FREE, iters = 0;
    bool last = false;
    if (tid < 64) {
        float t = 0.f, p[3] = {0.f, 0.f, 0.f};
        if (mine) {
            const float* ra = a.origins + 3 * (size_t)(row0 + tid);
            const float* rb = a.points + 3 * (size_t)(row0 + tid);
            o[0] = ra[0]; o[1] = ra[1]; o[2] = ra[2];
            const float b[3] = {rb[0], rb[1], rb[2]};
            t = a.t[a.t_scalar ? 0 : row0 + tid];
            const float d[3] = {__fsub_rn(b[0], o[0]), __fsub_rn(b[1], o[1]), __fsub_rn(b[2], o[2])};
            const float L = vis_sqrt(vis_dot(d, d));
            const bool finite = vis_finite(o[0]) && vis_finite(o[1]) && vis_finite(o[2]) && vis_finite(b[0]) && vis_finite(b[1]) &&
                                vis_finite(b[2]) && vis_finite(t);
            if (!(finite && L > 0.f)) {
                status = VIS_UNKNOWN;
            } else {
                u[0] = __fdiv_rn(d[0], L); u[1] = __fdiv_rn(d[1], L); u[2] = __fdiv_rn(d[2], L);
                const float dd = vis_dot(u, u);
                const float d1 = __fdiv_rn(-vis_dot(u, o), dd);
                const float q[3] = {__fadd_rn(o[0], vis_mul(d1, u[0])), __fadd_rn(o[1], vis_mul(d1, u[1])), __fadd_rn(o[2], vis_mul(d1, u[2]))};
                const float d2 = __fdiv_rn(vis_sqrt(vis_clamp0(__fsub_rn(1.f, vis_dot(q, q)))), vis_sqrt(dd));
                const float s_in = vis_clamp0(__fsub_rn(d1, d2)), s_out = __fadd_rn(d1, d2);
                const float Lm = __fsub_rn(L, a.margin);
                s_end = Lm < s_out ? Lm : s_out;
                if (s_end > s_in) {          // (false for NaN: such a row is FREE without an evaluation)
                    status = VIS_LIVE;
                    s = s_in;
#pragma unroll
                    for (int i = 0; i < 3; ++i) p[i] = __fadd_rn(o[i], vis_mul(s, u[i]));
                }
            }
        }
        const bool go = status == VIS_LIVE;          // (rows that never start hold the origin of the unit ball at t = 0)
        px[tid] = go ? p[0] : 0.f; px[64 + tid] = go ? p[1] : 0.f; px[128 + tid] = go ? p[2] : 0.f; pt[tid] = go ? t : 0.f;
    }
    __syncthreads();
    int tid_k = tid, wave_k = wave;          // (the loop's own copies, see k_trace_surface)
    const float4* packed_k = packed;
    const float* weff_k = weff;
    for (int k = 1; k <= a.max_iters; ++k) {
        // Each network's address arithmetic is derived afresh from values the compiler cannot see through: hoisted out of this loop as
        // invariants, the two networks' sets together exceed the register budget of two workgroups per CU and spill (trace.hip).
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
        if (status == VIS_LIVE) {          // (tid < PTS and the segment is in the batch)
            const float f = __fsub_rn(smalln_reduce<1>(red, 0, tid) + weff_k[b8s], tau);
            iters = k;
            if (f < clearance) clearance = f;
            if (!vis_finite(f)) {          // inf or NaN
                status = VIS_UNKNOWN;
            } else if (f <= 0.f) {
                status = VIS_OCCLUDED; blocker = s;
            } else if (last) {
                status = VIS_FREE; free_to = s;
            } else {
                free_to = s;
                s = __fadd_rn(s, fmaxf(vis_mul(relax, f), min_step));
                if (s >= s_end) { s = s_end; last = true; }
#pragma unroll
                for (int i = 0; i < 3; ++i) px[i * 64 + tid] = __fadd_rn(o[i], vis_mul(s, u[i]));
            }
        }
        // workgroup-uniform exit; also the barrier between this round's reads of ``red`` / writes of px and the next encoding
        if (!__syncthreads_or(status == VIS_LIVE)) break;
    }
    if (tid < PTS && row0 + tid < n_rows) {
        if (status == VIS_LIVE) status = VIS_UNKNOWN;          // the cap
        const int r = row0 + tid;
        status_out[r] = status;
        if (iters_out) iters_out[r] = iters;
        if (blocker_out) blocker_out[r] = blocker;
        if (clearance_out) clearance_out[r] = clearance;
        if (free_to_out) free_to_out[r] = free_to;
    }
}

constexpr int VIS_DEFAULT_TILE = 32;          // as the tracer's: a tile runs as many evaluations as its slowest row

static int segment_visible(const VisibleArgs& a, int tile_points, const float* packed, const float* weff, int use_deform, hipStream_t st) {
    static constexpr decltype(&k_segment_visible<true, false>) KERNELS[] = {k_segment_visible<true, false>, k_segment_visible<true, true>,          // [(DEFORM ? 0 : 2) + HALF]
                                                                            k_segment_visible<false, false>, k_segment_visible<false, true>};
    static DeviceOnce attr_done;
    const bool half = (tile_points ? tile_points : VIS_DEFAULT_TILE) == 32;
    return launch_lean(KERNELS, attr_done, (use_deform ? 0 : 2) + half, VIS_LDS_BYTES, a.M, half ? 32 : 64, st, "es_segment_visible", a,
                       make_tabs(), reinterpret_cast<const float4*>(packed), weff);
}

}  // namespace es

using namespace es;

extern "C" int es_segment_visible(const float* origins, const float* points, const float* t, int t_scalar, int M, float margin, float tau,
                                  float relax, float min_step, int max_iters, int tile_points, const float* packed, const float* weff,
                                  int use_deform, int* status_out, int* iters_out, float* blocker_out, float* clearance_out, float* free_to_out, void* stream) {
    constexpr float FMAX = 3.402823466e+38f;          // (each comparison is false for NaN)
    ES_REQUIRE(M >= 0, "es_segment_visible: M must not be negative");
    ES_REQUIRE(margin >= 0.f && margin <= FMAX, "es_segment_visible: margin must be finite and not negative");
    ES_REQUIRE(tau >= -FMAX && tau <= FMAX, "es_segment_visible: tau must be finite");
    ES_REQUIRE(relax > 0.f && relax <= 1.f, "es_segment_visible: relax must be in (0, 1]");
    ES_REQUIRE(min_step > 0.f && min_step <= FMAX, "es_segment_visible: min_step must be finite and positive");
    ES_REQUIRE(max_iters >= 1 && max_iters <= ES_TRACE_MAX_ITERS, "es_segment_visible: max_iters must be in [1, 1024]");
    ES_REQUIRE(tile_points == 0 || tile_points == 32 || tile_points == 64, "es_segment_visible: tile_points: 0 (the library's choice), 32 or 64");
    if (M == 0) return ST_OK;
    ES_REQUIRE(origins && points && t && packed && weff && status_out,
               "es_segment_visible: null buffer (origins, points, t, packed, weff, status_out)");
    const VisibleArgs a{origins, points, t, M, t_scalar != 0, max_iters, margin, tau, relax, min_step, status_out, iters_out, blocker_out, clearance_out, free_to_out};
    return segment_visible(a, tile_points, packed, weff, use_deform, (hipStream_t)stream);
}
