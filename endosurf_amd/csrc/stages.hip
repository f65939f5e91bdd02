// Whole-stage calls of libendosurf_hip.so: the per-kernel launchers chained like the reference's render_rays / render_core / ray_marching
// (what a host without the Python drop-in binds).  No kernel lives here.  Each scratch layout is written once, as a Carver sequence
// that both es_*_scratch_floats (null base: measures) and the call (the caller's buffer: carves) run.
#include "chain_common.h"
#include "host.h"
#include "launch.h"
#include "workspace.h"

using namespace es;

static inline long long up64(size_t n) { return (long long)((n + 63) / 64 * 64); }      // every scratch region: a multiple of 64 floats (256 bytes)

// ---- es_sample_z: the sampling stage of render_rays --------------------------------------------------------------------------------
// z [N][S]: the ping-pong partner of z_out | sdf_a, sdf_b [N][S]: merged sdf, ping-pong | src [N][S]: merge permutation (int32) |
// sdf_c0 [N][n_samples]: sdf at the coarse depths | z_new, sdf_new [N][n_imp]: the new depths of one round and their sdf
struct SampleScratch { float *z, *sdf_a, *sdf_b; int* src; float *sdf_c0, *z_new, *sdf_new; long long floats; };
static SampleScratch sample_scratch(float* scratch, int N, int n_samples, int S, int n_imp) {
    Carver c(scratch);
    const long long NS = up64((size_t)N * S), NI = up64((size_t)N * n_imp);
    SampleScratch s{c.take<float>(NS), c.take<float>(NS), c.take<float>(NS), c.take<int>(NS), c.take<float>(up64((size_t)N * n_samples)),
                    c.take<float>(NI), c.take<float>(NI), 0};      // (a braced list is evaluated left to right)
    s.floats = c.off / (long long)sizeof(float);
    return s;
}
int64_t es_sample_scratch_floats(int N, int n_samples, int n_importance, int up_sample_steps) {
    if (N <= 0 || n_samples <= 0) return 0;
    const int n_imp_all = n_importance > 0 ? n_importance : 0;
    return sample_scratch(nullptr, N, n_samples, n_samples + n_imp_all, up_sample_steps > 0 ? n_imp_all / up_sample_steps : 0).floats;
}
int es_sample_z(const float* rays, const float* u_perturb, int N, int n_samples, int n_importance, int up_sample_steps, int upsample,
                const float* packed, const float* weff, int use_deform, float* z_out, float* scratch, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(rays && z_out && packed && weff && N >= 0 && n_samples >= 2, "es_sample_z arguments");
    hipStream_t st = (hipStream_t)stream;
    const bool do_up = upsample && n_importance > 0 && up_sample_steps > 0;
    const int S = n_samples + (do_up ? n_importance : 0);
    const float sample_dist = 2.0f / (float)n_samples;
    if (!do_up) return ray_setup(rays, u_perturb, N, n_samples, sample_dist, 0, z_out, S, nullptr, nullptr, st);
    ES_REQUIRE(scratch != nullptr && n_importance % up_sample_steps == 0, "es_sample_z needs scratch and n_importance divisible by up_sample_steps");
    const int n_imp = n_importance / up_sample_steps;
    const SampleScratch sc = sample_scratch(scratch, N, n_samples, S, n_imp);
    float* zbuf[2] = {z_out, sc.z};                           // ping-pong; the result must land in z_out
    int cur = up_sample_steps % 2;                            // so that after up_sample_steps swaps the current buffer is z_out
    if (int e = ray_setup(rays, u_perturb, N, n_samples, sample_dist, 0, zbuf[cur], S, nullptr, nullptr, st)) return e;
    PointSrc ps{};
    ps.rays = rays; ps.mode = 1; ps.t_scalar = 0;
    ps.z = zbuf[cur]; ps.n_per_ray = n_samples; ps.ldz = S; ps.M = N * n_samples;
    if (int e = query_sdf(ps, packed, weff, sc.sdf_c0, use_deform, st)) return e;
    const float* sdf_c = sc.sdf_c0;
    int ld_sdf = n_samples, n = n_samples;
    for (int i = 0; i < up_sample_steps; ++i) {
        if (int e = upsample_step(rays, zbuf[cur], S, sdf_c, ld_sdf, N, n, n_imp, 64.f * (float)(1 << i), sc.z_new, zbuf[cur ^ 1], S, sc.src, st)) return e;
        if (i + 1 != up_sample_steps) {
            ps.z = sc.z_new; ps.n_per_ray = n_imp; ps.ldz = n_imp; ps.M = N * n_imp;
            if (int e = query_sdf(ps, packed, weff, sc.sdf_new, use_deform, st)) return e;
            float* dst = sdf_c != sc.sdf_a ? sc.sdf_a : sc.sdf_b;
            if (int e = merge_sdf(sdf_c, ld_sdf, sc.sdf_new, n_imp, sc.src, S, N, n, dst, st)) return e;
            sdf_c = dst; ld_sdf = S;
        }
        cur ^= 1;
        n += n_imp;
    }
    return ST_OK;
}

// ---- es_render_forward / es_render_backward: render_core on given sample depths ---------------------------------------------------------
// mid [N*S]: section mid-points (forward) | d_sdf [N*S], d_go [N*S][3], d_rgb [N*S][3]: adjoints of the point outputs (backward)
struct RenderScratch { float *mid, *d_sdf, *d_go, *d_rgb; long long floats; };
static RenderScratch render_scratch(float* scratch, int N, int S) {
    Carver c(scratch);
    const long long P = up64((size_t)N * S), P3 = up64(3 * (size_t)N * S);
    RenderScratch r{c.take<float>(P), c.take<float>(P), c.take<float>(P3), c.take<float>(P3), 0};
    r.floats = c.off / (long long)sizeof(float);
    return r;
}
int64_t es_render_scratch_floats(int N, int S) {
    if (N <= 0 || S <= 0) return 0;
    return render_scratch(nullptr, N, S).floats;
}
static int render_points(const es_render_args* a, PointSrc& ps, int& flags) {
    ES_REQUIRE(a && a->c.rays && a->c.z && a->c.variance && a->ws && a->scratch && a->c.N >= 0 && a->c.S >= 1 && a->c.ldz >= a->c.S,
               "es_render arguments");
    ps = PointSrc{};
    ps.rays = a->c.rays; ps.z = render_scratch(a->scratch, a->c.N, a->c.S).mid; ps.mode = 1; ps.n_per_ray = a->c.S; ps.ldz = a->c.S; ps.M = a->c.N * a->c.S;
    flags = (a->flags & (ES_PF_DEFORM | ES_PF_SAVE | ES_PF_X3)) | ES_PF_COLOR;      // ES_PF_X3: opt-in split-precision weight gradients
    return ST_OK;
}
static CompositeArgs render_composite_args(const es_render_args* a, int flags) {
    CompositeArgs c = as_comp(&a->c);
    const WsLayout L = ws_layout(a->c.N * a->c.S, flags);
    c.sdf = a->ws + L.off[WS_SDF]; c.g_o = a->ws + L.off[WS_GO]; c.rgb = a->ws + L.off[WS_RGB];
    const RenderScratch r = render_scratch(a->scratch, a->c.N, a->c.S);
    c.d_sdf = r.d_sdf; c.d_go = r.d_go; c.d_rgb = r.d_rgb;
    c.n_aux = 0; c.g_aux_sdf = nullptr; c.g_aux_go = nullptr;      // (the whole-stage calls evaluate the ray samples only: scratch holds N*S rows)
    return c;
}
int es_render_forward(const es_render_args* a, const float* packed, const float* weff, void* stream) {
    if (a && a->c.N == 0) return ST_OK;      // an empty ray batch
    PointSrc ps; int flags;
    if (int e = render_points(a, ps, flags)) return e;
    ES_REQUIRE(packed && weff, "null weights");
    ES_REQUIRE(a->c.color && a->c.depth && a->c.weights && a->c.cdf && a->c.weight_max && a->c.eik_acc && a->c.wmax_idx, "es_render_forward outputs");
    hipStream_t st = (hipStream_t)stream;
    if (int e = mid_z(a->c.z, a->c.ldz, a->c.N, a->c.S, a->c.sample_dist, render_scratch(a->scratch, a->c.N, a->c.S).mid, st)) return e;
    if ((flags & ES_PF_X3) && (flags & ES_PF_SAVE) && a->packed_x3) flags = (flags & ~ES_PF_X3) | ES_PF_X3_CHAIN;      // training chain
    if (int e = point_forward(ps, packed, weff, a->ws, flags, 0, st, a->packed_x3)) return e;
    return composite(render_composite_args(a, flags), 0, st);
}
int es_render_backward(const es_render_args* a, const float* packed, const float* weff, float* dweff, void* stream) {
    if (a && a->c.N == 0) return ST_OK;      // an empty ray batch
    PointSrc ps; int flags;
    if (int e = render_points(a, ps, flags)) return e;
    ES_REQUIRE(packed && weff && dweff, "null weights / gradient buffer");
    ES_REQUIRE(flags & ES_PF_SAVE, "es_render_backward needs a forward run with ES_PF_SAVE");
    ES_REQUIRE(a->c.g_color && a->c.g_depth && a->c.g_eik && a->c.eik_den && a->c.d_invs_acc, "es_render_backward adjoints");
    hipStream_t st = (hipStream_t)stream;
    const CompositeArgs c = render_composite_args(a, flags);
    if (int e = composite(c, 1, st)) return e;
    if ((flags & ES_PF_X3) && a->packed_x3) flags |= ES_PF_X3_CHAIN;       // the forward of the same arguments ran the split-precision chain
    if (int e = point_backward_chains(ps, packed, weff, a->ws, flags, 0, c.d_sdf, c.d_go, c.d_rgb, st, a->packed_x3)) return e;
    return point_wgrad(ps.M, a->ws, flags, 0, c.d_sdf, dweff, a->wg_scratch, st);
}

// ---- es_ray_marching: ray_marching + secant ---------------------------------------------------------------------------------------------
// dprop, sdf [N][n_steps]: proposals and their sdf | state [N][4]: bracket | flags, done [N] (int32) | d_pred [N] |
// t, f_mid [N]: time and sdf of the secant points | x [N][3]: the secant points
struct MarchScratch { float *dprop, *sdf, *state; int *flags, *done; float *d_pred, *t, *f_mid, *x; long long floats; };
static MarchScratch march_scratch(float* scratch, int N, int n_steps) {
    Carver c(scratch);
    const long long NP = up64((size_t)N * n_steps), N1 = up64((size_t)N);
    MarchScratch m{c.take<float>(NP), c.take<float>(NP), c.take<float>(up64((size_t)N * 4)), c.take<int>(N1), c.take<int>(N1),
                   c.take<float>(N1), c.take<float>(N1), c.take<float>(N1), c.take<float>(up64((size_t)N * 3)), 0};
    m.floats = c.off / (long long)sizeof(float);
    return m;
}
int64_t es_march_scratch_floats(int N, int n_steps) {
    if (N <= 0 || n_steps <= 0) return 0;
    return march_scratch(nullptr, N, n_steps).floats;
}
int es_ray_marching(const float* rays, int N, int n_steps, int n_secant, float tau, int block, const float* packed, const float* weff,
                    int use_deform, float* d_out, float* scratch, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(rays && packed && weff && d_out && N >= 0 && n_steps >= 2 && n_secant >= 0, "es_ray_marching arguments");
    ES_REQUIRE(scratch != nullptr, "es_ray_marching needs scratch");
    hipStream_t st = (hipStream_t)stream;
    const MarchScratch m = march_scratch(scratch, N, n_steps);
    if (int e = ray_setup(rays, nullptr, N, n_steps, 0.f, 1, m.dprop, n_steps, nullptr, nullptr, st)) return e;
    PointSrc ps{};
    ps.rays = rays; ps.mode = 1;
    if (block > 0 && n_steps % block == 0 && n_steps > block) {
        if (hipMemsetAsync(m.sdf, 0, (size_t)N * n_steps * sizeof(float), st) != hipSuccess) return hip_last("es_ray_marching memset");
        for (int b = 0; b < n_steps / block; ++b) {          // skipped proposals read as 0: no sign change
            ps.z = m.dprop + (size_t)b * block; ps.n_per_ray = block; ps.ldz = n_steps; ps.M = N * block;
            if (int e = query_sdf(ps, packed, weff, m.sdf + (size_t)b * block, use_deform, st, n_steps, b ? m.done : nullptr)) return e;
            if (b + 1 < n_steps / block)
                if (int e = march_progress(m.sdf, N, n_steps, (b + 1) * block, tau, m.done, st)) return e;
        }
    } else {
        ps.z = m.dprop; ps.n_per_ray = n_steps; ps.ldz = n_steps; ps.M = N * n_steps;
        if (int e = query_sdf(ps, packed, weff, m.sdf, use_deform, st)) return e;
    }
    if (int e = march_find(m.sdf, m.dprop, N, n_steps, tau, m.state, m.flags, m.d_pred, st)) return e;
    PointSrc pm{};
    pm.x = m.x; pm.t = m.t; pm.mode = 0; pm.n_per_ray = 1; pm.ldz = 1; pm.M = N;
    for (int i = 0; i < n_secant; ++i) {
        if (int e = secant_points(rays, m.d_pred, N, m.x, m.t, st)) return e;
        if (int e = query_sdf(pm, packed, weff, m.f_mid, use_deform, st)) return e;
        if (int e = secant_update(m.f_mid, N, tau, m.state, m.d_pred, st)) return e;
    }
    return march_finish(m.d_pred, m.flags, N, d_out, st);
}
