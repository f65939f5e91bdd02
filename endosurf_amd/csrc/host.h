// Host-side boundary between the translation units of libendosurf_hip.so: every function that one .hip unit defines and another
// calls is declared here, once, with its default arguments here and nowhere else.  The defining unit and every calling unit include
// this header, so a signature or a default that changes in one place is a compile error in the other.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include "../../include/endosurf_hip.h"

namespace es {

struct PointSrc; struct WsLayout; struct FwdArgs; struct BwdArgs;      // chain_common.h, workspace.h, point_fwd_bodies.h, point_bwd_bodies.h

// Argument blocks of the compositing kernels and of the fused training-loss kernel: the public structs themselves (their fields are
// documented in include/endosurf_hip.h), under the names the kernels take them by.
struct CompositeArgs : ::es_composite_args {};
struct LossArgs : ::es_loss_args {};
static_assert(sizeof(CompositeArgs) == sizeof(es_composite_args) && std::is_standard_layout<CompositeArgs>::value, "es::CompositeArgs is es_composite_args");
static_assert(sizeof(LossArgs) == sizeof(es_loss_args) && std::is_standard_layout<LossArgs>::value, "es::LossArgs is es_loss_args");
inline const CompositeArgs& as_comp(const es_composite_args* a) { return *reinterpret_cast<const CompositeArgs*>(a); }

// pack.hip
int init_tables();
int weightnorm_pack(const float* params, float* weff, float* packed, int use_deform, hipStream_t st);
int weightnorm_backward(const float* params, const float* dweff, float* dparams, int use_deform, hipStream_t st);
int weightnorm_backward_layers(const float* params, const float* dweff, float* dparams, int first_layer, int n_layers, hipStream_t st);

// query.hip, query16.hip, query_x3.hip
int query_sdf(const PointSrc& src, const float* packed, const float* weff, float* sdf_out, int use_deform, hipStream_t st,
              int ld_out = 0, const int* ray_done = nullptr, int tile_points = 0);
int query_sdf16(const PointSrc& src, const float* packed, const float* weff, float* sdf_out, int use_deform, hipStream_t st);
size_t packed_x3_bytes();
int pack_x3(const float* weff, void* packed_x3, int use_deform, hipStream_t st);
int query_sdf_x3(const PointSrc& src, const void* packed_x3, const float* weff, float* sdf_out, int use_deform, hipStream_t st, int ld_out, const int* ray_done);

// deform.hip
int deform_forward(const PointSrc& src, const float* packed, const float* weff, float* xc_out, float* d_out, hipStream_t st);
int deform_inverse(const PointSrc& src, const float* init, const float* packed, const float* weff, int max_iters, float tol, float* y_out,
                   float* step_out, int* iters_out, hipStream_t st);

// trace.hip
int trace_surface(const float* rays, int N, float tau, float eps, float relax, float min_step, int max_iters, int tile_points,
                  const float* packed, const float* weff, int use_deform, float* depth_out, int* status_out, int* iters_out,
                  float* residual_out, float* points_out, hipStream_t st);

// deform_jet.hip, strain.hip
int deform_jacobian(const PointSrc& src, const float* packed, const float* weff, float* jac_out, float* xc_out, hipStream_t st);
int strain_rows(const float* jac_from, const float* jac_to, const float* normals, int M, float* F_out, float* det_out, float* stretch_out,
                float* area_out, float* surface_out, unsigned char* valid_out, hipStream_t st);

// sdf_hess.hip, curvature.hip
int sdf_hessian(const float* x, int M, const float* packed, const float* weff, int tile_rows, float* sdf_out, float* grad_out,
                float* hess_out, hipStream_t st);
int curvature_rows(const float* grad_c, const float* hess_c, const float* jac, const float* dd, int M, float* grad_o, float* hess_o,
                   float* mean_out, float* gauss_out, float* principal_out, unsigned char* valid_out, hipStream_t st);

// deform_jet.hip, kinematics.hip
int deform_derivatives(const PointSrc& src, const float* packed, const float* weff, float* jac_out, float* dt_out, float* dd_out,
                       float* xc_out, hipStream_t st);
int kinematics_rows(const float* jac, const float* d_t, const float* dd, const float* normals, int M, float* vel_out, float* speed_out,
                    float* L_out, float* rate_out, float* principal_out, float* div_out, float* vort_out, float* area_out,
                    float* surface_out, unsigned char* valid_out, hipStream_t st);

// geodesic.hip
int geodesic_seed(const float* vertices, const int* tris, int F, long long V, long long T, int S, const int* seed_field,
                  const int* seed_vertex, const double* seed_value, long long n_seeds, unsigned long long* cur, unsigned long long* next,
                  hipStream_t st);
int geodesic_sweep(const float* vertices, const int* tris, int F, long long V, long long T, int S, const unsigned long long* cur,
                   unsigned long long* next, int* changed, hipStream_t st);
int geodesic_read(const unsigned long long* field, const float* vertices, const int* tris, int F, long long V, long long T, int S,
                  const int* target_tri, const double* target_pt, long long Q, const int* source_tri, const double* source_pt, float* out,
                  hipStream_t st);
int geodesic_finish(const unsigned long long* field, long long n, float* out, hipStream_t st);

// point_fwd.hip, point_bwd.hip
int point_forward(const PointSrc& src, const float* packed, const float* weff, float* ws, int flags, int m_color, hipStream_t st,
                  const void* packed_x3 = nullptr);
int point_forward_rows(const PointSrc& src, const float* packed, const float* weff, float* ws, int flags, int m_color, int row0, int nrows, hipStream_t st);
int point_vjp(const PointSrc& src, const float* packed, const float* weff, float* ws, int flags, hipStream_t st);
int color_forward(const PointSrc& src, const float* packed, const float* weff, float* ws, hipStream_t st);
int point_backward_chains(const PointSrc& src, const float* packed, const float* weff, float* ws, int flags, int m_color,
                          const float* d_sdf, const float* d_go, const float* d_rgb, hipStream_t st, const void* packed_x3 = nullptr);

// infer_x3r.hip (called by point_fwd.hip)
int deform_jvp_x3r(const PointSrc& src, const void* packed_r, const float* weff, float* ws, const WsLayout& L, bool save, hipStream_t st);
int deform_vjp_x3r(const PointSrc& src, const void* packed_r, const float* weff, float* ws, const WsLayout& L, bool save, hipStream_t st, int m_rows = 0);
int deform_jvp_x3r_with_tail(const FwdArgs& fa, const void* packed_r, int m_main, hipStream_t st);
int sdf_fwd_x3r(const PointSrc& src, const void* packed_r, const float* weff, float* ws, const WsLayout& L, bool deform, bool color, hipStream_t st);
int color_fwd_x3r(const PointSrc& src, const void* packed_r, const float* weff, float* ws, const WsLayout& L, bool deform, int Mcp, bool save, hipStream_t st);

// train_x3r.hip (called by point_bwd.hip)
int deform_tan_x3r(const PointSrc& src, const void* packed_r, const float* weff, float* ws, const WsLayout& L, const float* d_go, hipStream_t st, int m_rows = 0);
int deform_bwd_x3r_with_tail(const BwdArgs& ba, const void* packed_r, int m_main, hipStream_t st);
int color_bwd_x3r(const PointSrc& src, const void* packed_r, const float* weff, float* ws, const WsLayout& L, bool deform, int m_color, const float* d_rgb, hipStream_t st);
int deform_bwd_x3r(const void* packed_r, const float* weff, float* ws, const WsLayout& L, int M, int m_color, hipStream_t st);

// wgrad.hip
int point_wgrad(int M, float* ws, int flags, int m_color, const float* d_sdf, float* dweff, float* det, hipStream_t st, int net_mask = 7);
size_t wgrad_det_floats();
int gemm_atb(const float* X, const float* dA, int M, float* out, int x3, float* det, hipStream_t st);

// rays.hip
int ray_setup(const float* rays, const float* u, int N, int n, float sample_dist, int lin_mode, float* z, int ldz, float* near_out, float* far_out, hipStream_t st);
int upsample_step(const float* rays, const float* z_in, int ld_in, const float* sdf_in, int ld_sdf, int N, int n, int n_imp,
                  float inv_s, float* z_new, float* z_out, int ld_out, int* src_idx, hipStream_t st);
int merge_sdf(const float* sdf_in, int ld_in, const float* sdf_new, int n_imp, const int* src_idx, int ld_out, int N, int n, float* sdf_out, hipStream_t st);
int mid_z(const float* z, int ldz, int N, int S, float sample_dist, float* mid, hipStream_t st);
int composite(const CompositeArgs& a, int backward, hipStream_t st);
int variance_terms(const float* variance, const float* d_invs_acc, float* s_val, float* d_var, hipStream_t st);
int march_progress(const float* sdf, int N, int n, int n_valid, float tau, int* done, hipStream_t st);
int march_find(const float* sdf, const float* dprop, int N, int n, float tau, float* state, int* flags, float* d_pred, hipStream_t st);
int secant_points(const float* rays, const float* d_pred, int N, float* x, float* t, hipStream_t st);
int secant_update(const float* sdf_mid, int N, float tau, float* state, float* d_pred, hipStream_t st);
int march_finish(const float* d_pred, const int* flags, int N, float* d_out, hipStream_t st);
int train_aux_points(const float* rays, const float* depth_gt, const float* mask, const float* d_i, const float* u, float rad, int N, float* x, float* t, unsigned char* valid, hipStream_t st);

// aux.hip
int eod_points(const float* rays, const float* depth_gt, const float* mask, int N, float* x, float* t, float* inside, hipStream_t st);
int sn_points(const float* rays, const float* mask, const float* d_i, const float* u, float rad, int N, float* x, float* t, unsigned char* valid, hipStream_t st);
int eod_loss(const float* rays, const float* pts, const float* mask, const float* sdf, const float* go, int N, float* out, float* inside, hipStream_t st);
int eod_loss_bwd(const float* rays, const float* inside, const float* sdf, const float* go, const float* out, const float* g_sdf_err,
                 const float* g_ang_err, int N, float* d_sdf, float* d_go, hipStream_t st);
int sn_loss(const float* g, const unsigned char* valid, int N, float* out, hipStream_t st);
int sn_loss_bwd(const float* g, const unsigned char* valid, const float* out, const float* g_loss, int N, float* d_g, hipStream_t st);
int copy2(float* da, const float* sa, long long na, float* db, const float* sb, long long nb, hipStream_t st);

// loss.hip, optim.hip, step.hip
int train_loss(const LossArgs& a, hipStream_t st);
int train_schedule(double* state, double lr_init, double n_iter, double warm_up_end, double lr_alpha, double beta1, double beta2, float grad_scale, double anneal_end, float* scal, hipStream_t st);
int adam_step_dev(float* p, const float* g, float* m, float* v, long long n, float beta1, float beta2, float eps, const float* scal, const float* g_extra, long long extra_index, hipStream_t st);
int adam_step(float* p, const float* g, float* m, float* v, long long n, float beta1, float beta2, float eps, float step_size,
              float bc2_sqrt, float grad_scale, const float* g_extra, long long extra_index, hipStream_t st);
int uniform(float* out, long long n, unsigned long long seed, unsigned long long subseq, const double* subseq_dev, hipStream_t st);
int scale(float* out, const float* in, long long n, const float* s, hipStream_t st);
int zero(void* p, long long nbytes, hipStream_t st);
int render_finish(const float* eik_acc, const float* aux_sdf_ws, const float* aux_go_ws, int n_aux, float* eik, float* eik_den, float* aux_sdf, float* aux_go, hipStream_t st);

}  // namespace es
