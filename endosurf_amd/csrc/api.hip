// extern "C" surface of libendosurf_hip.so (declared in include/endosurf_hip.h): argument checks and forwarding to the launchers of
// host.h.  The whole-stage calls (es_sample_z, es_render_*, es_ray_marching) are in stages.hip.
#include "arch.h"
#include "chain_common.h"
#include "host.h"
#include "launch.h"
#include "workspace.h"

namespace es {
static inline PointSrc to_src(const es_points* p) { PointSrc s; static_cast<es_points&>(s) = *p; return s; }
static inline int check_src(const es_points* p) {
    ES_REQUIRE(p != nullptr, "es_points is null");
    ES_REQUIRE(p->M >= 0, "negative point count");
    if (p->M == 0) return ST_OK;
    if (p->mode == 0) {
        ES_REQUIRE(p->x && p->t, "mode 0 needs x and t");
    } else {
        ES_REQUIRE(p->mode == 1 || p->mode == 2, "unknown point-source mode");
        ES_REQUIRE(p->rays && p->z && p->n_per_ray > 0 && p->ldz >= p->n_per_ray, "modes 1/2 need rays, z, n_per_ray <= ldz");
        if (p->mode == 2) ES_REQUIRE(p->M_split >= 0 && p->M_split <= p->M && (p->M_split == p->M || (p->x && p->t)), "mode 2 needs M_split <= M and x, t");
    }
    return ST_OK;
}
// What a call on a point source checks first: the source, then its buffers -- the weights always, the per-point ones (``rows``) unless
// the batch is empty.
static inline int check_points(const es_points* p, bool weights, bool rows) {
    if (int e = check_src(p)) return e;
    ES_REQUIRE(weights && (rows || p->M == 0), "null buffer");
    return ST_OK;
}
// The deformation network alone (deform.hip): explicit points only, checked before anything is launched; an empty batch launches nothing.
static inline int check_deform_src(const es_points* p) {
    ES_REQUIRE(p != nullptr, "es_points is null");
    ES_REQUIRE(p->M >= 0, "negative point count");
    ES_REQUIRE(p->mode == 0, "the deformation calls take explicit points (mode 0)");
    return ST_OK;
}
static inline int check_mcolor(const es_points* pts, int flags, int m_color) {
    if (!(flags & ES_PF_COLOR) || m_color <= 0 || m_color == pts->M) return ST_OK;
    ES_REQUIRE(m_color < pts->M && m_color % 64 == 0, "m_color must be a multiple of 64 (tile aligned) or cover all points");
    ES_REQUIRE(pts->mode != 2 || m_color <= pts->M_split, "colour points must be ray samples");
    return ST_OK;
}
// The checks shared by the point-forward and point-backward entries, in the order all of them make them.  A backward needs a saved
// workspace and, with ES_PF_COLOR, the colour adjoint d_rgb; a forward needs view directions for the colour network.
static int check_point_call(const es_points* pts, bool weights, bool rows, int flags, int m_color, bool backward, const float* d_rgb = nullptr) {
    if (int e = check_src(pts)) return e;
    if (backward) ES_REQUIRE(flags & ES_PF_SAVE, "es_point_backward needs a workspace produced by the matching forward with ES_PF_SAVE");
    ES_REQUIRE(weights && (rows || pts->M == 0), "null buffer");
    if (backward) ES_REQUIRE(!(flags & ES_PF_COLOR) || d_rgb || pts->M == 0, "colour adjoint missing");
    else ES_REQUIRE(!(flags & ES_PF_COLOR) || pts->mode != 0 || pts->dirs, "colour evaluation needs view directions");
    return check_mcolor(pts, flags, m_color);
}
// The backward of a checked call: the chains, then the weight-gradient GEMMs.  stages: ES_BWD_* bits (15 = all of it); packed_x3: the
// split weights, for a workspace of the split-precision chain; wg_scratch: nullable (deterministic reduction).
static int run_backward(const es_points* pts, const float* packed, const void* packed_x3, const float* weff, float* ws, int flags, int m_color,
                        const float* d_sdf, const float* d_go, const float* d_rgb, float* dweff, float* wg_scratch, int stages, void* stream) {
    if (stages & ES_BWD_CHAINS)
        if (int e = point_backward_chains(to_src(pts), packed, weff, ws, flags, m_color, d_sdf, d_go, d_rgb, (hipStream_t)stream, packed_x3)) return e;
    if (stages >> 1) return point_wgrad(pts->M, ws, flags, m_color, d_sdf, dweff, wg_scratch, (hipStream_t)stream, stages >> 1);
    return ST_OK;
}
// The mesh arguments every es_geodesic_* entry takes: F frames of V vertices, T triangles, S sources.
static int check_geodesic_mesh(const float* vertices, const int* triangles, int F, long long V, long long T, int S) {
    ES_REQUIRE(F >= 0 && V >= 0 && T >= 0, "es_geodesic: negative count (F, V, T)");
    ES_REQUIRE(S >= 1, "es_geodesic: S must be at least 1");
    ES_REQUIRE(V < (1ll << 31) && T < (1ll << 31), "es_geodesic: V and T must be below 2^31");
    ES_REQUIRE(vertices || F == 0 || V == 0, "es_geodesic: null buffer (vertices)");
    ES_REQUIRE(triangles || T == 0, "es_geodesic: null buffer (triangles)");
    return ST_OK;
}
}  // namespace es

using namespace es;

extern "C" {

int es_abi_version(void) { return ES_ABI_VERSION; }
const char* es_last_error(void) { return last_error_buf(); }
int es_init(void) { return init_tables(); }

int64_t es_param_floats(void) { return PARAM_FLOATS; }
int64_t es_param_variance_off(void) { return PARAM_VARIANCE_OFF; }
int es_param_layout(int net, int layer, int64_t* bias_off, int64_t* g_off, int64_t* v_off, int* out_dim, int* in_dim) {
    ES_REQUIRE(net >= 0 && net < NETS && layer >= 0 && layer < LAYERS, "net/layer out of range");
    int64_t off = 0;
    for (int n = 0; n < NETS; ++n)
        for (int l = 0; l < LAYERS; ++l) {
            if (n == net && l == layer) {
                if (bias_off) *bias_off = off;
                if (g_off) *g_off = off + LAYER_N[n][l];
                if (v_off) *v_off = off + 2 * LAYER_N[n][l];
                if (out_dim) *out_dim = LAYER_N[n][l];
                if (in_dim) *in_dim = LAYER_K[n][l];
                return ST_OK;
            }
            off += (int64_t)LAYER_N[n][l] * (2 + LAYER_K[n][l]);
        }
    return ST_BAD_ARG;
}
int64_t es_weff_floats(void) { return WEFF_FLOATS; }
int es_weff_layout(int net, int layer, int64_t* w_off, int64_t* b_off) {
    ES_REQUIRE(net >= 0 && net < NETS && layer >= 0 && layer < LAYERS, "net/layer out of range");
    int64_t off = 0;
    for (int n = 0; n < NETS; ++n)
        for (int l = 0; l < LAYERS; ++l) {
            if (n == net && l == layer) {
                if (w_off) *w_off = off;
                if (b_off) *b_off = off + (int64_t)LAYER_N[n][l] * LAYER_K[n][l];
                return ST_OK;
            }
            off += (int64_t)LAYER_N[n][l] * (1 + LAYER_K[n][l]);
        }
    return ST_BAD_ARG;
}
int64_t es_packed_floats(void) { return (int64_t)PACKED_TOTAL_FLOATS; }

int es_weightnorm_pack(const float* params, float* weff, float* packed, int use_deform, void* stream) {
    ES_REQUIRE(params && weff && packed, "null buffer");
    return weightnorm_pack(params, weff, packed, use_deform, (hipStream_t)stream);
}
int es_weightnorm_backward(const float* params, const float* dweff, float* dparams, int use_deform, void* stream) {
    ES_REQUIRE(params && dweff && dparams, "null buffer");
    return weightnorm_backward(params, dweff, dparams, use_deform, (hipStream_t)stream);
}

int es_weightnorm_backward_layers(const float* params, const float* dweff, float* dparams, int first_layer, int n_layers, void* stream) {
    ES_REQUIRE(params && dweff && dparams, "null buffer");
    ES_REQUIRE(first_layer >= 0 && n_layers >= 0 && first_layer + n_layers <= NETS * LAYERS, "layers [first, first + n) of the 27 (network x 9 + layer)");
    return weightnorm_backward_layers(params, dweff, dparams, first_layer, n_layers, (hipStream_t)stream);
}

int es_query_sdf(const es_points* pts, const float* packed, const float* weff, float* sdf_out, int use_deform, void* stream) {
    if (int e = check_points(pts, packed && weff, sdf_out)) return e;
    return query_sdf(to_src(pts), packed, weff, sdf_out, use_deform, (hipStream_t)stream);
}
int es_query_sdf_tiles(const es_points* pts, const float* packed, const float* weff, float* sdf_out, int use_deform, int tile_points,
                       void* stream) {
    if (int e = check_points(pts, packed && weff, sdf_out)) return e;
    ES_REQUIRE(tile_points == 0 || tile_points == 16 || tile_points == 32 || tile_points == 64, "tile_points: 0 (by batch size), 16, 32 or 64");
    return query_sdf(to_src(pts), packed, weff, sdf_out, use_deform, (hipStream_t)stream, 0, nullptr, tile_points);
}
int es_query_sdf_rays(const es_points* pts, const float* packed, const float* weff, float* sdf_out, int ld_out, const int* ray_done,
                      int use_deform, void* stream) {
    if (int e = check_points(pts, packed && weff, sdf_out)) return e;
    ES_REQUIRE(pts->mode == 1 && pts->n_per_ray >= 1 && ld_out >= pts->n_per_ray, "es_query_sdf_rays takes ray samples (mode 1), ld_out >= n_per_ray");
    return query_sdf(to_src(pts), packed, weff, sdf_out, use_deform, (hipStream_t)stream, ld_out, ray_done);
}
int es_deform_forward(const es_points* pts, const float* packed, const float* weff, float* xc_out, float* d_out, void* stream) {
    if (int e = check_deform_src(pts)) return e;
    if (pts->M == 0) return ST_OK;
    ES_REQUIRE(pts->x && pts->t, "mode 0 needs x and t");
    ES_REQUIRE(packed && weff, "null buffer");
    ES_REQUIRE(xc_out || d_out, "es_deform_forward: both outputs are null");
    return deform_forward(to_src(pts), packed, weff, xc_out, d_out, (hipStream_t)stream);
}
int es_deform_inverse(const es_points* pts, const float* init, const float* packed, const float* weff, int max_iters, float tol, float* y_out,
                      float* step_out, int* iters_out, void* stream) {
    if (int e = check_deform_src(pts)) return e;
    ES_REQUIRE(max_iters >= 1, "es_deform_inverse: max_iters must be at least 1");
    ES_REQUIRE(tol >= 0.f && tol <= 3.402823466e+38f, "es_deform_inverse: tol must be finite and not negative");          // (false for NaN)
    if (pts->M == 0) return ST_OK;
    ES_REQUIRE(pts->x && pts->t, "mode 0 needs x and t");
    ES_REQUIRE(packed && weff && y_out && step_out && iters_out, "null buffer");
    return deform_inverse(to_src(pts), init, packed, weff, max_iters, tol, y_out, step_out, iters_out, (hipStream_t)stream);
}
int es_deform_jacobian(const es_points* pts, const float* packed, const float* weff, float* jac_out, float* xc_out, void* stream) {
    if (int e = check_deform_src(pts)) return e;
    if (pts->M == 0) return ST_OK;
    ES_REQUIRE(pts->x && pts->t, "mode 0 needs x and t");
    ES_REQUIRE(packed && weff, "null buffer");
    ES_REQUIRE(jac_out || xc_out, "es_deform_jacobian: both outputs are null");
    return deform_jacobian(to_src(pts), packed, weff, jac_out, xc_out, (hipStream_t)stream);
}
int es_strain_rows(const float* jac_from, const float* jac_to, const float* normals, int M, float* F_out, float* det_out, float* stretch_out,
                   float* area_out, float* surface_out, unsigned char* valid_out, void* stream) {
    ES_REQUIRE(M >= 0, "negative row count");
    if (M == 0) return ST_OK;
    ES_REQUIRE(jac_to, "null buffer");
    ES_REQUIRE(F_out || det_out || stretch_out || area_out || surface_out || valid_out, "es_strain_rows: every output is null");
    ES_REQUIRE(normals || !(area_out || surface_out), "es_strain_rows: the surface outputs need normals");
    return strain_rows(jac_from, jac_to, normals, M, F_out, det_out, stretch_out, area_out, surface_out, valid_out, (hipStream_t)stream);
}
int es_trace_surface(const float* rays, int N, float tau, float eps, float relax, float min_step, int max_iters, int tile_points,
                     const float* packed, const float* weff, int use_deform, float* depth_out, int* status_out, int* iters_out,
                     float* residual_out, float* points_out, void* stream) {
    constexpr float FMAX = 3.402823466e+38f;          // (each comparison is false for NaN)
    ES_REQUIRE(N >= 0, "es_trace_surface: N must not be negative");
    ES_REQUIRE(tau >= -FMAX && tau <= FMAX, "es_trace_surface: tau must be finite");
    ES_REQUIRE(eps >= 0.f && eps <= FMAX, "es_trace_surface: eps must be finite and not negative");
    ES_REQUIRE(relax > 0.f && relax <= 1.f, "es_trace_surface: relax must be in (0, 1]");
    ES_REQUIRE(min_step > 0.f && min_step <= FMAX, "es_trace_surface: min_step must be finite and positive");
    ES_REQUIRE(max_iters >= 1 && max_iters <= ES_TRACE_MAX_ITERS, "es_trace_surface: max_iters must be in [1, 1024]");
    ES_REQUIRE(tile_points == 0 || tile_points == 32 || tile_points == 64, "es_trace_surface: tile_points: 0 (the library's choice), 32 or 64");
    if (N == 0) return ST_OK;
    ES_REQUIRE(rays && packed && weff && depth_out && status_out, "es_trace_surface: null buffer (rays, packed, weff, depth_out, status_out)");
    return trace_surface(rays, N, tau, eps, relax, min_step, max_iters, tile_points, packed, weff, use_deform, depth_out, status_out, iters_out,
                         residual_out, points_out, (hipStream_t)stream);
}
int es_sdf_hessian(const es_points* pts, const float* packed, const float* weff, int tile_rows, float* sdf_out, float* grad_out,
                   float* hess_out, void* stream) {
    ES_REQUIRE(pts != nullptr, "es_points is null");
    ES_REQUIRE(pts->M >= 0, "negative point count");
    ES_REQUIRE(pts->mode == 0, "es_sdf_hessian takes explicit points (mode 0)");
    ES_REQUIRE(tile_rows == 0 || tile_rows == 32 || tile_rows == 64, "es_sdf_hessian: tile_rows: 0 (by batch size), 32 or 64");
    if (pts->M == 0) return ST_OK;
    ES_REQUIRE(pts->x && packed && weff, "es_sdf_hessian: null buffer (x, packed, weff)");
    ES_REQUIRE(sdf_out || grad_out || hess_out, "es_sdf_hessian: every output is null");
    return sdf_hessian(pts->x, pts->M, packed, weff, tile_rows, sdf_out, grad_out, hess_out, (hipStream_t)stream);
}
int es_curvature_rows(const float* grad_c, const float* hess_c, const float* jac, const float* dd, int M, float* grad_o, float* hess_o,
                      float* mean_out, float* gauss_out, float* principal_out, unsigned char* valid_out, void* stream) {
    ES_REQUIRE(M >= 0, "negative row count");
    if (M == 0) return ST_OK;
    ES_REQUIRE(grad_c && hess_c, "es_curvature_rows: null buffer (grad_c, hess_c)");
    ES_REQUIRE(grad_o || hess_o || mean_out || gauss_out || principal_out || valid_out, "es_curvature_rows: every output is null");
    return curvature_rows(grad_c, hess_c, jac, dd, M, grad_o, hess_o, mean_out, gauss_out, principal_out, valid_out, (hipStream_t)stream);
}
int es_deform_derivatives(const es_points* pts, const float* packed, const float* weff, float* jac_out, float* dt_out, float* dd_out,
                          float* xc_out, void* stream) {
    if (int e = check_deform_src(pts)) return e;
    if (pts->M == 0) return ST_OK;
    ES_REQUIRE(pts->x && pts->t, "mode 0 needs x and t");
    ES_REQUIRE(packed && weff, "null buffer");
    ES_REQUIRE(jac_out || dt_out || dd_out || xc_out, "es_deform_derivatives: every output is null");
    return deform_derivatives(to_src(pts), packed, weff, jac_out, dt_out, dd_out, xc_out, (hipStream_t)stream);
}
int es_kinematics_rows(const float* jac, const float* d_t, const float* dd, const float* normals, int M, float* velocity, float* speed,
                       float* L, float* rate, float* principal, float* divergence, float* vorticity, float* area_rate,
                       float* surface_rates, unsigned char* valid, void* stream) {
    ES_REQUIRE(M >= 0, "negative row count");
    if (M == 0) return ST_OK;
    ES_REQUIRE(jac && d_t && dd, "es_kinematics_rows: null buffer (jac, d_t, dd)");
    ES_REQUIRE(velocity || speed || L || rate || principal || divergence || vorticity || area_rate || surface_rates || valid,
               "es_kinematics_rows: every output is null");
    ES_REQUIRE(normals || !(area_rate || surface_rates), "es_kinematics_rows: the surface outputs need normals");
    return kinematics_rows(jac, d_t, dd, normals, M, velocity, speed, L, rate, principal, divergence, vorticity, area_rate, surface_rates,
                           valid, (hipStream_t)stream);
}
int es_geodesic_seed(const float* vertices, const int* triangles, int F, long long V, long long T, int S, const int* seed_field,
                     const int* seed_vertex, const double* seed_value, long long n_seeds, unsigned long long* cur,
                     unsigned long long* next, void* stream) {
    if (int e = check_geodesic_mesh(vertices, triangles, F, V, T, S)) return e;
    ES_REQUIRE(n_seeds >= 0, "es_geodesic_seed: negative count (n_seeds)");
    if (F == 0 || V == 0) return ST_OK;
    ES_REQUIRE(cur && next, "es_geodesic_seed: null buffer (cur, next)");
    ES_REQUIRE(cur != next, "es_geodesic_seed: cur and next must be two buffers");
    ES_REQUIRE(n_seeds == 0 || (seed_field && seed_vertex && seed_value), "es_geodesic_seed: null buffer (seed_field, seed_vertex, seed_value)");
    return geodesic_seed(vertices, triangles, F, V, T, S, seed_field, seed_vertex, seed_value, n_seeds, cur, next, (hipStream_t)stream);
}
int es_geodesic_sweep(const float* vertices, const int* triangles, int F, long long V, long long T, int S,
                      const unsigned long long* cur, unsigned long long* next, int* changed, void* stream) {
    if (int e = check_geodesic_mesh(vertices, triangles, F, V, T, S)) return e;
    ES_REQUIRE((cur && next) || F == 0 || V == 0, "es_geodesic_sweep: null buffer (cur, next)");
    ES_REQUIRE(cur != next || !cur, "es_geodesic_sweep: cur and next must be two buffers");
    return geodesic_sweep(vertices, triangles, F, V, T, S, cur, next, changed, (hipStream_t)stream);
}
int es_geodesic_read(const unsigned long long* field, const float* vertices, const int* triangles, int F, long long V, long long T, int S,
                     const int* target_triangle, const double* target_point, long long Q, const int* source_triangle,
                     const double* source_point, float* out, void* stream) {
    if (int e = check_geodesic_mesh(vertices, triangles, F, V, T, S)) return e;
    ES_REQUIRE(Q >= 0, "es_geodesic_read: negative count (Q)");
    if (F == 0 || Q == 0) return ST_OK;
    ES_REQUIRE(out && target_triangle && target_point, "es_geodesic_read: null buffer (target_triangle, target_point, out)");
    ES_REQUIRE(field || V == 0, "es_geodesic_read: null buffer (field)");
    ES_REQUIRE(!source_triangle == !source_point, "es_geodesic_read: source_triangle and source_point go together");
    return geodesic_read(field, vertices, triangles, F, V, T, S, target_triangle, target_point, Q, source_triangle, source_point, out,
                         (hipStream_t)stream);
}
int es_geodesic_finish(const unsigned long long* field, long long n, float* out, void* stream) {
    ES_REQUIRE(n >= 0, "es_geodesic_finish: negative count (n)");
    if (n == 0) return ST_OK;
    ES_REQUIRE(field && out, "es_geodesic_finish: null buffer (field, out)");
    return geodesic_finish(field, n, out, (hipStream_t)stream);
}
int64_t es_packed_x3_bytes(void) { return (int64_t)packed_x3_bytes(); }
int es_pack_x3(const float* weff, void* packed_x3, int use_deform, void* stream) {
    ES_REQUIRE(weff && packed_x3, "null buffer");
    return pack_x3(weff, packed_x3, use_deform, (hipStream_t)stream);
}
int es_query_sdf_x3(const es_points* pts, const void* packed_x3, const float* weff, float* sdf_out, int ld_out, const int* ray_done,
                    int use_deform, void* stream) {
    if (int e = check_points(pts, packed_x3 && weff, sdf_out)) return e;
    ES_REQUIRE(ld_out == 0 || (pts->mode == 1 && ld_out >= pts->n_per_ray), "ld_out > 0 needs ray samples (mode 1), ld_out >= n_per_ray");
    ES_REQUIRE(ray_done == nullptr || pts->mode == 1, "ray_done needs ray samples (mode 1)");
    return query_sdf_x3(to_src(pts), packed_x3, weff, sdf_out, use_deform, (hipStream_t)stream, ld_out, ray_done);
}
int es_variance_terms(const float* variance, const float* d_invs_acc, float* s_val, float* d_var, void* stream) {
    ES_REQUIRE(variance && (s_val || d_var) && (!d_var || d_invs_acc), "es_variance_terms arguments");
    return variance_terms(variance, d_invs_acc, s_val, d_var, (hipStream_t)stream);
}
// The per-ray calls below return at once for an empty ray batch (N == 0): nothing to do, whatever the (possibly null) buffers.
int es_march_progress(const float* sdf, int N, int n, int n_valid, float tau, int* done, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(sdf && done && n >= 2 && n_valid >= 1 && n_valid <= n, "es_march_progress arguments");
    return march_progress(sdf, N, n, n_valid, tau, done, (hipStream_t)stream);
}

int es_ray_setup(const float* rays, const float* u, int N, int n, float sample_dist, int lin_mode, float* z, int ldz,
                 float* near_out, float* far_out, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(rays && z && N >= 0 && n >= 1 && ldz >= n, "es_ray_setup arguments");
    return ray_setup(rays, u, N, n, sample_dist, lin_mode, z, ldz, near_out, far_out, (hipStream_t)stream);
}
int es_upsample_step(const float* rays, const float* z_in, int ld_in, const float* sdf_in, int ld_sdf, int N, int n, int n_imp,
                     float inv_s, float* z_new, float* z_out, int ld_out, int32_t* src_idx, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(rays && z_in && sdf_in && z_new && z_out && src_idx && ld_in >= n && ld_sdf >= n, "es_upsample_step arguments");
    return upsample_step(rays, z_in, ld_in, sdf_in, ld_sdf, N, n, n_imp, inv_s, z_new, z_out, ld_out, src_idx, (hipStream_t)stream);
}
int es_merge_sdf(const float* sdf_in, int ld_in, const float* sdf_new, int n_imp, const int32_t* src_idx, int ld_out, int N, int n,
                 float* sdf_out, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(sdf_in && sdf_new && src_idx && sdf_out && sdf_out != sdf_in, "es_merge_sdf arguments (out must not alias in)");
    return merge_sdf(sdf_in, ld_in, sdf_new, n_imp, src_idx, ld_out, N, n, sdf_out, (hipStream_t)stream);
}
int es_mid_z(const float* z, int ldz, int N, int S, float sample_dist, float* mid, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(z && mid && ldz >= S && S >= 1, "es_mid_z arguments");
    return mid_z(z, ldz, N, S, sample_dist, mid, (hipStream_t)stream);
}
int es_composite_forward(const es_composite_args* a, void* stream) {
    if (a && a->N == 0) return ST_OK;      // an empty ray batch
    ES_REQUIRE(a && a->rays && a->z && a->sdf && a->g_o && a->rgb && a->variance, "es_composite_forward inputs");
    ES_REQUIRE(a->color && a->depth && a->weights && a->cdf && a->weight_max && a->eik_acc && a->wmax_idx, "es_composite_forward outputs");
    return composite(as_comp(a), 0, (hipStream_t)stream);
}
int es_composite_backward(const es_composite_args* a, void* stream) {
    if (a && a->N == 0) return ST_OK;      // an empty ray batch
    ES_REQUIRE(a && a->rays && a->z && a->sdf && a->g_o && a->rgb && a->variance, "es_composite_backward inputs");
    ES_REQUIRE(a->n_aux >= 0, "es_composite_backward: negative n_aux");
    ES_REQUIRE(a->g_color && a->g_depth && a->g_eik && a->eik_den && a->d_sdf && a->d_go && a->d_rgb && a->d_invs_acc,
               "es_composite_backward adjoints");
    return composite(as_comp(a), 1, (hipStream_t)stream);
}
int es_march_find(const float* sdf, const float* dprop, int N, int n, float tau, float* state, int32_t* flags, float* d_pred, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(sdf && dprop && state && flags && d_pred && n >= 2, "es_march_find arguments");
    return march_find(sdf, dprop, N, n, tau, state, flags, d_pred, (hipStream_t)stream);
}
int es_secant_points(const float* rays, const float* d_pred, int N, float* x, float* t, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(rays && d_pred && x && t, "es_secant_points arguments");
    return secant_points(rays, d_pred, N, x, t, (hipStream_t)stream);
}
int es_secant_update(const float* sdf_mid, int N, float tau, float* state, float* d_pred, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(sdf_mid && state && d_pred, "es_secant_update arguments");
    return secant_update(sdf_mid, N, tau, state, d_pred, (hipStream_t)stream);
}
int es_march_finish(const float* d_pred, const int32_t* flags, int N, float* d_out, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(d_pred && flags && d_out, "es_march_finish arguments");
    return march_finish(d_pred, flags, N, d_out, (hipStream_t)stream);
}

int64_t es_point_workspace_floats(int M, int flags) { return M <= 0 ? 0 : (int64_t)ws_layout(M, flags).off[WS_COUNT]; }
int64_t es_point_workspace_offset(int M, int flags, int buffer_id) {
    if (M <= 0 || buffer_id < 0 || buffer_id >= WS_COUNT) return -1;
    return (int64_t)ws_layout(M, flags).off[buffer_id];
}
int es_point_forward(const es_points* pts, const float* packed, const float* weff, float* ws, int flags, int m_color, void* stream) {
    if (int e = check_point_call(pts, packed && weff, ws, flags, m_color, false)) return e;
    return point_forward(to_src(pts), packed, weff, ws, flags, m_color, (hipStream_t)stream);
}
int es_point_forward_rows(const es_points* pts, const float* packed, const float* weff, float* ws, int flags, int m_color, int row0, int nrows,
                          void* stream) {
    if (int e = check_points(pts, packed && weff, ws)) return e;
    ES_REQUIRE(!(flags & (ES_PF_X3 | ES_PF_X3_CHAIN)), "es_point_forward_rows: fp32 family only");
    ES_REQUIRE(!(flags & ES_PF_COLOR) || pts->mode != 0 || pts->dirs, "colour evaluation needs view directions");
    ES_REQUIRE(row0 >= 0 && nrows >= 0, "es_point_forward_rows: negative row range");
    if (int e = check_mcolor(pts, flags, m_color)) return e;
    return point_forward_rows(to_src(pts), packed, weff, ws, flags, m_color, row0, nrows, (hipStream_t)stream);
}
int es_eod_points(const float* rays, const float* depth_gt, const float* mask, int N, float* x, float* t, float* inside, void* stream) {
    ES_REQUIRE(N >= 0 && (N == 0 || (rays && depth_gt && x && t)), "es_eod_points buffers");
    ES_REQUIRE(inside == nullptr || mask != nullptr || N == 0, "es_eod_points: the inside mask needs the ray mask");
    return eod_points(rays, depth_gt, mask, N, x, t, inside, (hipStream_t)stream);
}
int es_sn_points(const float* rays, const float* mask, const float* d_i, const float* u, float rad, int N, float* x, float* t,
                 unsigned char* valid, void* stream) {
    ES_REQUIRE(N >= 0 && (N == 0 || (rays && mask && d_i && u && x && t && valid)), "es_sn_points buffers");
    return sn_points(rays, mask, d_i, u, rad, N, x, t, valid, (hipStream_t)stream);
}
int es_eod_loss(const float* rays, const float* pts, const float* mask, const float* sdf, const float* g_o, int N, float* out, float* inside,
                void* stream) {
    ES_REQUIRE(N >= 0 && out && (N == 0 || (rays && pts && mask && sdf && g_o && inside)), "es_eod_loss buffers");
    return eod_loss(rays, pts, mask, sdf, g_o, N, out, inside, (hipStream_t)stream);
}
int es_eod_loss_backward(const float* rays, const float* inside, const float* sdf, const float* g_o, const float* out, const float* g_sdf_err,
                         const float* g_ang_err, int N, float* d_sdf, float* d_go, void* stream) {
    ES_REQUIRE(N >= 0 && (N == 0 || (rays && inside && sdf && g_o && out && d_sdf && d_go)), "es_eod_loss_backward buffers");
    return eod_loss_bwd(rays, inside, sdf, g_o, out, g_sdf_err, g_ang_err, N, d_sdf, d_go, (hipStream_t)stream);
}
int es_sn_loss(const float* g, const unsigned char* valid, int N, float* out, void* stream) {
    ES_REQUIRE(N >= 0 && out && (N == 0 || (g && valid)), "es_sn_loss buffers");
    return sn_loss(g, valid, N, out, (hipStream_t)stream);
}
int es_sn_loss_backward(const float* g, const unsigned char* valid, const float* out, const float* g_loss, int N, float* d_g, void* stream) {
    ES_REQUIRE(N >= 0 && (N == 0 || (g && valid && out && g_loss && d_g)), "es_sn_loss_backward buffers");
    return sn_loss_bwd(g, valid, out, g_loss, N, d_g, (hipStream_t)stream);
}
int es_copy2(float* da, const float* sa, long long na, float* db, const float* sb, long long nb, void* stream) {
    ES_REQUIRE(na >= 0 && nb >= 0 && (na == 0 || (da && sa)) && (nb == 0 || (db && sb)), "es_copy2 buffers");
    return copy2(da, sa, na, db, sb, nb, (hipStream_t)stream);
}
int es_point_vjp(const es_points* pts, const float* packed, const float* weff, float* ws, int flags, void* stream) {
    if (int e = check_points(pts, packed && weff, ws)) return e;
    ES_REQUIRE(flags & ES_PF_DEFORM, "es_point_vjp is the reverse sweep of the deformation network (ES_PF_DEFORM)");
    ES_REQUIRE(!(flags & ES_PF_X3_CHAIN), "the workspace must come from es_point_forward (fp32 family: its ReLU mask words)");
    return point_vjp(to_src(pts), packed, weff, ws, flags, (hipStream_t)stream);
}
int es_color_forward(const es_points* pts, const float* packed, const float* weff, float* ws, void* stream) {
    if (int e = check_points(pts, packed && weff, ws)) return e;
    ES_REQUIRE(pts->mode == 0 && pts->dirs, "es_color_forward takes explicit points with their view directions");
    return color_forward(to_src(pts), packed, weff, ws, (hipStream_t)stream);
}
int es_point_forward_x3(const es_points* pts, const float* packed, const void* packed_x3, const float* weff, float* ws, int flags, int m_color,
                        void* stream) {
    if (int e = check_point_call(pts, packed && packed_x3 && weff, ws, flags, m_color, false)) return e;
    // no-grad evaluation: ES_PF_X3; with ES_PF_SAVE: the split-precision TRAINING chain (ES_PF_X3_CHAIN; backward: es_point_backward_x3)
    const int mode = (flags & ES_PF_SAVE) ? ES_PF_X3_CHAIN : ES_PF_X3;
    return point_forward(to_src(pts), packed, weff, ws, (flags & ~(ES_PF_X3 | ES_PF_X3_CHAIN)) | mode, m_color, (hipStream_t)stream, packed_x3);
}
int es_point_backward_x3(const es_points* pts, const float* packed, const void* packed_x3, const float* weff, float* ws, int flags, int m_color,
                         const float* d_sdf, const float* d_go, const float* d_rgb, float* dweff, float* wg_scratch, void* stream) {
    if (int e = check_point_call(pts, packed && packed_x3 && weff && dweff, ws && d_sdf && d_go, flags, m_color, true, d_rgb)) return e;
    flags |= ES_PF_X3_CHAIN | ES_PF_X3;          // chain kernels of the split-precision family, weight-gradient GEMMs in split precision
    return run_backward(pts, packed, packed_x3, weff, ws, flags, m_color, d_sdf, d_go, d_rgb, dweff, wg_scratch, 15, stream);
}
int es_point_backward_det(const es_points* pts, const float* packed, const float* weff, float* ws, int flags, int m_color,
                          const float* d_sdf, const float* d_go, const float* d_rgb, float* dweff, float* wg_scratch, void* stream) {
    if (int e = check_point_call(pts, packed && weff && dweff, ws && d_sdf && d_go, flags, m_color, true, d_rgb)) return e;
    return run_backward(pts, packed, nullptr, weff, ws, flags, m_color, d_sdf, d_go, d_rgb, dweff, wg_scratch, 15, stream);
}
int es_point_backward(const es_points* pts, const float* packed, const float* weff, float* ws, int flags, int m_color,
                      const float* d_sdf, const float* d_go, const float* d_rgb, float* dweff, void* stream) {
    return es_point_backward_det(pts, packed, weff, ws, flags, m_color, d_sdf, d_go, d_rgb, dweff, nullptr, stream);
}
int es_point_backward_stages(const es_points* pts, const float* packed, const float* weff, float* ws, int flags, int m_color,
                             const float* d_sdf, const float* d_go, const float* d_rgb, float* dweff, float* wg_scratch, int stages, void* stream) {
    if (int e = check_point_call(pts, packed && weff && dweff, ws && d_sdf && d_go, flags, m_color, true, d_rgb)) return e;
    ES_REQUIRE(!(flags & ES_PF_X3_CHAIN), "the staged backward is the fp32 family's (a workspace of es_point_forward)");
    ES_REQUIRE(stages > 0 && stages < 16, "stages: ES_BWD_CHAINS | ES_BWD_WGRAD_DEFORM | ES_BWD_WGRAD_SDF | ES_BWD_WGRAD_COLOR");
    return run_backward(pts, packed, nullptr, weff, ws, flags, m_color, d_sdf, d_go, d_rgb, dweff, wg_scratch, stages, stream);
}
int64_t es_wgrad_scratch_floats(void) { return (int64_t)wgrad_det_floats(); }
int es_gemm_atb(const float* X, const float* dA, int M, float* out, int split_precision, float* wg_scratch, void* stream) {
    ES_REQUIRE(X && dA && out && M > 0 && M % 64 == 0, "es_gemm_atb: X [M][256], dA [M][256], out [256][256], M a multiple of 64");
    return gemm_atb(X, dA, M, out, split_precision, wg_scratch, (hipStream_t)stream);
}

int es_train_loss(const es_loss_args* a, void* stream) {
    // an empty batch (N == 0) still launches -- the terms, the total and the normalisers are defined -- and its per-ray buffers may be null
    ES_REQUIRE(a && a->eik, "es_train_loss inputs");
    ES_REQUIRE(a->N == 0 || (a->color_map && a->depth_map && a->aux_sdf && a->aux_go && a->rays && a->eod_pts && a->color_gt && a->depth_gt &&
                             a->mask && a->cmask && a->valid_sn), "es_train_loss inputs");
    ES_REQUIRE(a->den_out || (a->terms && a->g_eik && (a->N == 0 || (a->g_color && a->g_depth && a->g_aux_sdf && a->g_aux_go))),
               "es_train_loss outputs");
    ES_REQUIRE(!a->den_global || a->world >= 1.f, "es_train_loss: den_global needs the world size");
    return train_loss(*reinterpret_cast<const LossArgs*>(a), (hipStream_t)stream);
}

int es_zero(void* p, long long nbytes, void* stream) {
    ES_REQUIRE((p || nbytes == 0) && nbytes >= 0, "es_zero arguments");
    return zero(p, nbytes, (hipStream_t)stream);
}
int es_uniform(float* out, long long n, unsigned long long seed, unsigned long long subsequence, const double* subsequence_dev, void* stream) {
    ES_REQUIRE((out || n == 0) && n >= 0, "es_uniform arguments");
    return uniform(out, n, seed, subsequence, subsequence_dev, (hipStream_t)stream);
}
int es_scale(float* out, const float* in, long long n, const float* s, void* stream) {
    ES_REQUIRE(((out && in) || n == 0) && n >= 0 && s, "es_scale arguments");
    return scale(out, in, n, s, (hipStream_t)stream);
}
int es_render_finish(const float* eik_acc, const float* aux_sdf_ws, const float* aux_go_ws, int n_aux, float* eik, float* eik_den, float* aux_sdf,
                     float* aux_go, void* stream) {
    ES_REQUIRE(eik_acc && eik && eik_den && n_aux >= 0 && (n_aux == 0 || (aux_sdf_ws && aux_go_ws && aux_sdf && aux_go)), "es_render_finish arguments");
    return render_finish(eik_acc, aux_sdf_ws, aux_go_ws, n_aux, eik, eik_den, aux_sdf, aux_go, (hipStream_t)stream);
}

int es_train_aux_points(const float* rays, const float* depth_gt, const float* mask, const float* d_i, const float* u, float rad, int N,
                        float* x, float* t, unsigned char* valid, void* stream) {
    if (N == 0) return ST_OK;
    ES_REQUIRE(rays && depth_gt && mask && d_i && u && x && t && valid && N >= 0, "es_train_aux_points buffers");
    return train_aux_points(rays, depth_gt, mask, d_i, u, rad, N, x, t, valid, (hipStream_t)stream);
}

int es_adam_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float beta1, float beta2, float eps,
                 float step_size, float bc2_sqrt, float grad_scale, const float* g_extra, long long extra_index, void* stream) {
    ES_REQUIRE(params && grad && exp_avg && exp_avg_sq && n >= 0, "es_adam_step buffers");
    ES_REQUIRE(g_extra == nullptr || (extra_index >= 0 && extra_index < n), "es_adam_step extra gradient index");
    return adam_step(params, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, step_size, bc2_sqrt, grad_scale, g_extra, extra_index,
                     (hipStream_t)stream);
}
int es_train_schedule(double* state, double lr_init, double n_iter, double warm_up_end, double lr_alpha, double beta1, double beta2,
                      float grad_scale, double anneal_end, float* scal, void* stream) {
    ES_REQUIRE(state && scal && n_iter > warm_up_end && warm_up_end >= 0, "es_train_schedule arguments");
    return train_schedule(state, lr_init, n_iter, warm_up_end, lr_alpha, beta1, beta2, grad_scale, anneal_end, scal, (hipStream_t)stream);
}
int es_adam_step_dev(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float beta1, float beta2, float eps,
                     const float* scal, const float* g_extra, long long extra_index, void* stream) {
    ES_REQUIRE(params && grad && exp_avg && exp_avg_sq && scal && n >= 0, "es_adam_step_dev buffers");
    ES_REQUIRE(g_extra == nullptr || (extra_index >= 0 && extra_index < n), "es_adam_step_dev extra gradient index");
    return adam_step_dev(params, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, scal, g_extra, extra_index, (hipStream_t)stream);
}

}  // extern "C"
