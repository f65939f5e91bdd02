// The image side of the pixel tracks (endosurf_amd/flow.py is the specification and the fp64 twin): elementwise kernels,
// one thread per row, fp64 inside, fp32 (or bytes) out.
//   k_pixel_rays        float pixel (x, y) -> ray [9]: d = R normalize(K^-1 [x, y, 1]), o = the pose's translation, columns 6:8 zero, t
//   k_flow_project      tracked rows [F P][3] through their frame's pinhole camera (the 17 numbers of meshing.camera_params, read per
//                       frame from a [F][17] fp64 buffer; k_rast_project's operation order) -> float pixel, camera z, front, in_image
//                       and the segment origin (the camera centre) of each row, in one pass
//   k_flow_resolve      flags -> visible, valid; pixels, flow = pixels - source pixels, scene_flow = points - source points, zero on
//                       rows that are not valid
//   k_sample_bilinear   images [n][H][W][C] at float positions, row r in image r / rows_per_image: two row blends, then the column blend, each a + f (b - a)
//   k_flow_panel        flow (u, v) -> RGB bytes through the six-sector HSV map written out in flow.flow_to_rgb
// No atomics and no scratch: the same bits from call to call.  Every loop is bounded by an argument (the grid stride by the row count,
// the channel loop by C) and every index is checked before it addresses memory: the frame of a row against F, the texel against the image.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"

namespace es {

constexpr long long FLOW_MAX_ROWS = (1ll << 31) - 1;          // rows x 3 coordinates are indexed with size_t, rows with int
constexpr int FLOW_MAX_SIZE = 1 << 15;                        // largest image side
constexpr int FLOW_MAX_CHANNELS = 64;

struct RayCamera {
    double kinv[9], R[9], o[3];
};

__global__ __launch_bounds__(256) void k_pixel_rays(const float* __restrict__ pixels, int P, RayCamera c, float t, float* __restrict__ rays) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < P; r += gridDim.x * 256) {
        const double x = pixels[2 * (size_t)r], y = pixels[2 * (size_t)r + 1];
        double v[3], d[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = (c.kinv[3 * i] * x + c.kinv[3 * i + 1] * y) + c.kinv[3 * i + 2];
        const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = v[i] / n;
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = (c.R[3 * i] * v[0] + c.R[3 * i + 1] * v[1]) + c.R[3 * i + 2] * v[2];
        float* out = rays + 9 * (size_t)r;
        out[0] = (float)c.o[0]; out[1] = (float)c.o[1]; out[2] = (float)c.o[2];
        out[3] = (float)d[0]; out[4] = (float)d[1]; out[5] = (float)d[2];
        out[6] = 0.f; out[7] = 0.f; out[8] = t;
    }
}

__global__ __launch_bounds__(256) void k_flow_project(const float* __restrict__ points, int F, int P, const double* __restrict__ cameras,
                                                      int per_frame, int height, int width, float* __restrict__ pixel, float* __restrict__ zc,
                                                      unsigned char* __restrict__ front, unsigned char* __restrict__ inside,
                                                      float* __restrict__ origin) {
    const long long n = (long long)F * P;
    for (long long r = blockIdx.x * 256ll + threadIdx.x; r < n; r += gridDim.x * 256ll) {
        const int f = (int)(r / P);
        if (f < 0 || f >= F) continue;          // (cannot happen for r < F P; the frame index addresses the camera table)
        const double* c = cameras + (per_frame ? 17 * (size_t)f : 0);
        const float fx = points[3 * (size_t)r], fy = points[3 * (size_t)r + 1], fz = points[3 * (size_t)r + 2];
        const double dx = (double)fx - c[9], dy = (double)fy - c[10], dz = (double)fz - c[11];
        const double x = (c[0] * dx + c[3] * dy) + c[6] * dz;
        const double y = (c[1] * dx + c[4] * dy) + c[7] * dz;
        const double z = (c[2] * dx + c[5] * dy) + c[8] * dz;
        const double pu = (c[12] * x + c[13] * y) / z + c[14], pv = c[15] * y / z + c[16];
        const bool finite = isfinite(fx) && isfinite(fy) && isfinite(fz) && isfinite(z);
        const bool fr = finite && isfinite(pu) && isfinite(pv) && z > 0.0;
        const float u32 = fr ? (float)pu : 0.f, v32 = fr ? (float)pv : 0.f;          // the flags below read the pixel as it is stored
        if (pixel) { pixel[2 * (size_t)r] = u32; pixel[2 * (size_t)r + 1] = v32; }
        if (zc) zc[r] = finite ? (float)z : __builtin_nanf("");
        if (front) front[r] = fr;
        if (inside) inside[r] = fr && u32 >= 0.f && u32 <= (float)(width - 1) && v32 >= 0.f && v32 <= (float)(height - 1);
        if (origin) { origin[3 * (size_t)r] = (float)c[9]; origin[3 * (size_t)r + 1] = (float)c[10]; origin[3 * (size_t)r + 2] = (float)c[11]; }
    }
}

__global__ __launch_bounds__(256) void k_flow_resolve(const float* __restrict__ pixel, const float* __restrict__ points,
                                                      const float* __restrict__ src_pixels, const float* __restrict__ src_points,
                                                      const unsigned char* __restrict__ src_valid, const unsigned char* __restrict__ converged,
                                                      const unsigned char* __restrict__ inside, const int* __restrict__ status, int F, int P,
                                                      unsigned char* __restrict__ visible, unsigned char* __restrict__ valid,
                                                      float* __restrict__ pixels_out, float* __restrict__ flow, float* __restrict__ scene) {
    const long long n = (long long)F * P;
    for (long long r = blockIdx.x * 256ll + threadIdx.x; r < n; r += gridDim.x * 256ll) {
        const int p = (int)(r % P);
        const bool vis = status[r] == ES_VISIBLE_FREE;
        const bool ok = src_valid[p] && converged[r] && inside[r] && vis;
        visible[r] = vis;
        valid[r] = ok;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float v = pixel[2 * (size_t)r + i];
            pixels_out[2 * (size_t)r + i] = ok ? v : 0.f;
            flow[2 * (size_t)r + i] = ok ? (float)((double)v - (double)src_pixels[2 * (size_t)p + i]) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
            scene[3 * (size_t)r + i] = ok ? (float)((double)points[3 * (size_t)r + i] - (double)src_points[3 * (size_t)p + i]) : 0.f;
    }
}

__global__ __launch_bounds__(256) void k_sample_bilinear(const float* __restrict__ images, int n_images, int H, int W, int C,
                                                         const float* __restrict__ pixels, const unsigned char* __restrict__ valid, long long M,
                                                         long long rows_per_image, const float* __restrict__ background, float* __restrict__ out) {
    for (long long r = blockIdx.x * 256ll + threadIdx.x; r < M; r += gridDim.x * 256ll) {
        const float x = pixels[2 * (size_t)r], y = pixels[2 * (size_t)r + 1];
        const long long f = r / rows_per_image;          // the image this row samples: checked before it addresses memory
        const bool ok = f >= 0 && f < n_images && (!valid || valid[r]) && x >= 0.f && x <= (float)(W - 1) && y >= 0.f &&
                        y <= (float)(H - 1);          // (false for NaN)
        float* o = out + (size_t)r * C;
        if (!ok) {
            for (int ch = 0; ch < C; ++ch) o[ch] = background[ch];
            continue;
        }
        const float* image = images + (size_t)f * H * W * C;
        int j0 = (int)floorf(x), i0 = (int)floorf(y);
        j0 = j0 > W - 2 ? W - 2 : j0; j0 = j0 < 0 ? 0 : j0;
        i0 = i0 > H - 2 ? H - 2 : i0; i0 = i0 < 0 ? 0 : i0;
        const int j1 = j0 + 1 > W - 1 ? W - 1 : j0 + 1, i1 = i0 + 1 > H - 1 ? H - 1 : i0 + 1;          // all four in [0, W) x [0, H)
        const double fx = (double)x - (double)j0, fy = (double)y - (double)i0;
        const float *p00 = image + ((size_t)i0 * W + j0) * C, *p01 = image + ((size_t)i0 * W + j1) * C;
        const float *p10 = image + ((size_t)i1 * W + j0) * C, *p11 = image + ((size_t)i1 * W + j1) * C;
        for (int ch = 0; ch < C; ++ch) {
            const double a = p00[ch], b = p01[ch], c = p10[ch], d = p11[ch];
            const double top = a + fx * (b - a), bottom = c + fx * (d - c);
            o[ch] = (float)(top + fy * (bottom - top));
        }
    }
}

__global__ __launch_bounds__(256) void k_flow_panel(const float* __restrict__ flow, long long n, double max_flow, unsigned char* __restrict__ rgb) {
    for (long long r = blockIdx.x * 256ll + threadIdx.x; r < n; r += gridDim.x * 256ll) {
        const float fu = flow[2 * (size_t)r], fv = flow[2 * (size_t)r + 1];
        double c[3] = {0.0, 0.0, 0.0};
        if (isfinite(fu) && isfinite(fv)) {
            const double u = fu, v = fv;
            double h = atan2(v, u) / (2.0 * 3.14159265358979323846);
            h = h - floor(h);
            if (!(h < 1.0)) h = 0.0;          // (-tiny mod 1)
            double s = sqrt(u * u + v * v) / max_flow;
            s = s > 1.0 ? 1.0 : s;
            const double h6 = 6.0 * h, fl = floor(h6), f = h6 - fl;
            int i = (int)fl % 6;
            i = i < 0 ? i + 6 : i;
            const double p = 1.0 - s, q = 1.0 - s * f, t = 1.0 - s * (1.0 - f);
            switch (i) {
                case 0: c[0] = 1.0; c[1] = t; c[2] = p; break;
                case 1: c[0] = q; c[1] = 1.0; c[2] = p; break;
                case 2: c[0] = p; c[1] = 1.0; c[2] = t; break;
                case 3: c[0] = p; c[1] = q; c[2] = 1.0; break;
                case 4: c[0] = t; c[1] = p; c[2] = 1.0; break;
                default: c[0] = 1.0; c[1] = p; c[2] = q; break;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[3 * (size_t)r + k] = (unsigned char)floor(255.0 * c[k] + 0.5);
    }
}

}  // namespace es

using namespace es;

extern "C" {

int es_pixel_rays(const float* pixels, long long P, const double* camera, float t, float* rays, void* stream) {
    ES_REQUIRE(P >= 0, "es_pixel_rays: P must not be negative");
    ES_REQUIRE(P <= FLOW_MAX_ROWS / 9, "es_pixel_rays: P: 9 P must stay below 2^31");
    ES_REQUIRE(camera, "es_pixel_rays needs camera (21 doubles on the host)");
    RayCamera c;
    for (int k = 0; k < 21; ++k) ES_REQUIRE(std::isfinite(camera[k]), "es_pixel_rays: camera parameters must be finite");
    for (int k = 0; k < 9; ++k) { c.kinv[k] = camera[k]; c.R[k] = camera[9 + k]; }
    for (int k = 0; k < 3; ++k) c.o[k] = camera[18 + k];
    if (P == 0) return ST_OK;
    ES_REQUIRE(pixels && rays, "es_pixel_rays: null buffer (pixels, rays)");
    hipLaunchKernelGGL(k_pixel_rays, dim3(grid_for(P)), dim3(256), 0, static_cast<hipStream_t>(stream), pixels, (int)P, c, t, rays);
    return hip_last("es_pixel_rays");
}

int es_flow_project(const float* points, int F, long long P, const double* cameras, int per_frame, int height, int width, float* pixel,
                    float* z, unsigned char* front, unsigned char* in_image, float* origin, void* stream) {
    ES_REQUIRE(F >= 0 && P >= 0, "es_flow_project: F and P must not be negative");
    ES_REQUIRE(P <= FLOW_MAX_ROWS && (F == 0 || P <= FLOW_MAX_ROWS / 3 / F), "es_flow_project: F, P: 3 F P must stay below 2^31");
    ES_REQUIRE(!in_image || (height >= 1 && height <= FLOW_MAX_SIZE && width >= 1 && width <= FLOW_MAX_SIZE),
               "es_flow_project: height and width must be in [1, 32768] when in_image is asked for");
    if (F == 0 || P == 0) return ST_OK;
    ES_REQUIRE(points && cameras, "es_flow_project: null buffer (points, cameras)");
    ES_REQUIRE(reinterpret_cast<uintptr_t>(cameras) % 8 == 0, "es_flow_project: cameras must be 8-byte aligned");
    ES_REQUIRE(pixel || z || front || in_image || origin, "es_flow_project: every output is null");
    hipLaunchKernelGGL(k_flow_project, dim3(grid_for((long long)F * P)), dim3(256), 0, static_cast<hipStream_t>(stream), points, F, (int)P,
                       cameras, per_frame != 0, height, width, pixel, z, front, in_image, origin);
    return hip_last("es_flow_project");
}

int es_flow_resolve(const float* pixel, const float* points, const float* source_pixels, const float* source_points,
                    const unsigned char* source_valid, const unsigned char* converged, const unsigned char* in_image, const int* status, int F,
                    long long P, unsigned char* visible, unsigned char* valid, float* pixels_out, float* flow, float* scene_flow, void* stream) {
    ES_REQUIRE(F >= 0 && P >= 0, "es_flow_resolve: F and P must not be negative");
    ES_REQUIRE(P <= FLOW_MAX_ROWS && (F == 0 || P <= FLOW_MAX_ROWS / 3 / F), "es_flow_resolve: F, P: 3 F P must stay below 2^31");
    if (F == 0 || P == 0) return ST_OK;
    ES_REQUIRE(pixel && points && source_pixels && source_points && source_valid && converged && in_image && status,
               "es_flow_resolve: null buffer (an input)");
    ES_REQUIRE(visible && valid && pixels_out && flow && scene_flow, "es_flow_resolve: null buffer (an output)");
    hipLaunchKernelGGL(k_flow_resolve, dim3(grid_for((long long)F * P)), dim3(256), 0, static_cast<hipStream_t>(stream), pixel, points,
                       source_pixels, source_points, source_valid, converged, in_image, status, F, (int)P, visible, valid, pixels_out, flow,
                       scene_flow);
    return hip_last("es_flow_resolve");
}

int es_sample_bilinear(const float* images, int n_images, int height, int width, int channels, const float* pixels, const unsigned char* valid,
                       long long M, long long rows_per_image, const float* background, float* out, void* stream) {
    ES_REQUIRE(M >= 0, "es_sample_bilinear: M must not be negative");
    ES_REQUIRE(n_images >= 1, "es_sample_bilinear: n_images must be at least 1");
    ES_REQUIRE(rows_per_image >= 1, "es_sample_bilinear: rows_per_image must be at least 1");
    ES_REQUIRE(height >= 1 && height <= FLOW_MAX_SIZE && width >= 1 && width <= FLOW_MAX_SIZE, "es_sample_bilinear: height and width must be in [1, 32768]");
    ES_REQUIRE(channels >= 1 && channels <= FLOW_MAX_CHANNELS, "es_sample_bilinear: channels must be in [1, 64]");
    ES_REQUIRE(M <= FLOW_MAX_ROWS / channels && (long long)height * width <= FLOW_MAX_ROWS / channels / n_images,
               "es_sample_bilinear: M channels and n_images height width channels must stay below 2^31");
    ES_REQUIRE(M <= rows_per_image * n_images, "es_sample_bilinear: M rows need M <= rows_per_image n_images");
    if (M == 0) return ST_OK;
    ES_REQUIRE(images && pixels && background && out, "es_sample_bilinear: null buffer (images, pixels, background, out)");
    hipLaunchKernelGGL(k_sample_bilinear, dim3(grid_for(M)), dim3(256), 0, static_cast<hipStream_t>(stream), images, n_images, height, width,
                       channels, pixels, valid, M, rows_per_image, background, out);
    return hip_last("es_sample_bilinear");
}

int es_flow_panel(const float* flow, long long n, double max_flow, unsigned char* rgb, void* stream) {
    ES_REQUIRE(n >= 0, "es_flow_panel: n must not be negative");
    ES_REQUIRE(n <= FLOW_MAX_ROWS / 3, "es_flow_panel: n: 3 n must stay below 2^31");
    ES_REQUIRE(max_flow > 0.0 && max_flow <= 1.7976931348623157e308, "es_flow_panel: max_flow must be finite and positive");
    if (n == 0) return ST_OK;
    ES_REQUIRE(flow && rgb, "es_flow_panel: null buffer (flow, rgb)");
    hipLaunchKernelGGL(k_flow_panel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), flow, n, max_flow, rgb);
    return hip_last("es_flow_panel");
}

}  // extern "C"
