// Depth fusion (endosurf_amd/fusion.py is the specification and the fp64 twin): a truncated signed distance volume from
// depth frames, one thread per voxel.
//   k_tsdf_integrate   voxel n walks the frames f = 0 .. F-1 in index order INSIDE the thread: q = R^T (p - t), nearest pixel of the
//                      projection (meshing.project_vertices' expressions, fp64), s = depth - z, and where the pixel counts and s >= -trunc
//                      three plain fp32 additions: tsdf_sum += fp32(min(1, s / trunc)), color_sum += the pixel's colour, weight += 1.
//                      State is read once and written once per call; the camera row of a frame is one wave-uniform load.
//   k_tsdf_finalize    tsdf = tsdf_sum / weight where weight > 0, else +1; colour likewise, else 0
//   k_volume_sample    a volume [R][R][R][C] at world points, trilinear in fp64: z blends, then y, then x, each a + f (b - a)
// No atomics and no scratch, and the order of a voxel's additions is the frame order: the same bits from call to call and however the
// frames are split into calls or the voxels into chunks.  The state holds sums, so there is no multiply-add next to an accumulation; the
// fp64 expressions are compiled with contraction off, so that they are the twin's operation for operation.  Every loop is bounded by an
// argument (the grid stride by N or M, the frame loop by F, the channel loop by C) and every index is checked before it addresses
// memory: the pixel against the image, the cell against the volume.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"

namespace es {

constexpr long long FUSE_MAX_INDEX = (1ll << 31) - 1;          // row, pixel and cell counts stay below 2^31; addresses are size_t
constexpr int FUSE_MAX_SIZE = 8192;                            // largest image side
constexpr int FUSE_MAX_CHANNELS = 8;

struct SampleBounds {
    double lo[3], hi[3];
};

__global__ __launch_bounds__(256) void k_tsdf_integrate(const float* __restrict__ positions, long long frame_stride,
                                                        const unsigned char* __restrict__ valid, int N, int F,
                                                        const float* __restrict__ depth, const float* __restrict__ color,
                                                        const unsigned char* __restrict__ mask, const double* __restrict__ cameras, int H,
                                                        int W, double trunc, double depth_trunc, float* __restrict__ tsdf_sum,
                                                        float* __restrict__ weight, float* __restrict__ color_sum) {
#pragma clang fp contract(off)
    const double jmax = (double)(W - 1), imax = (double)(H - 1);
    for (long long n = blockIdx.x * 256ll + threadIdx.x; n < N; n += gridDim.x * 256ll) {
        float ts = tsdf_sum[n], wt = weight[n];
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if (color_sum) { c0 = color_sum[3 * (size_t)n]; c1 = color_sum[3 * (size_t)n + 1]; c2 = color_sum[3 * (size_t)n + 2]; }
        const float* p = positions + 3 * (size_t)n;
        float px = p[0], py = p[1], pz = p[2];
        for (int f = 0; f < F; ++f) {
            if (frame_stride) {
                const float* pf = p + 3 * (size_t)frame_stride * f;
                px = pf[0]; py = pf[1]; pz = pf[2];
            }
            if (valid && !valid[(size_t)f * N + n]) continue;
            const double* c = cameras + 17 * (size_t)f;          // (wave-uniform: the frame index is the same on every lane)
            const double dx = (double)px - c[9], dy = (double)py - c[10], dz = (double)pz - c[11];
            const double x = (c[0] * dx + c[3] * dy) + c[6] * dz;
            const double y = (c[1] * dx + c[4] * dy) + c[7] * dz;
            const double z = (c[2] * dx + c[5] * dy) + c[8] * dz;
            if (!(z > 0.0)) continue;          // (false for NaN)
            const double u = (c[12] * x + c[13] * y) / z + c[14], v = c[15] * y / z + c[16];
            const double fj = floor(u + 0.5), fi = floor(v + 0.5);
            if (!(fj >= 0.0 && fj <= jmax && fi >= 0.0 && fi <= imax)) continue;          // (false for NaN): the pixel is in the image
            const size_t pix = ((size_t)f * H + (size_t)(int)fi) * W + (size_t)(int)fj;
            const float d = depth[pix];
            if (!(isfinite(d) && d > 0.f && (double)d <= depth_trunc)) continue;
            if (mask && !mask[pix]) continue;
            const double s = (double)d - z;
            if (s < -trunc) continue;
            const double r = s / trunc;
            ts += (float)(r < 1.0 ? r : 1.0);
            wt += 1.f;
            if (color) { c0 += color[3 * pix]; c1 += color[3 * pix + 1]; c2 += color[3 * pix + 2]; }
        }
        tsdf_sum[n] = ts;
        weight[n] = wt;
        if (color_sum) { color_sum[3 * (size_t)n] = c0; color_sum[3 * (size_t)n + 1] = c1; color_sum[3 * (size_t)n + 2] = c2; }
    }
}

__global__ __launch_bounds__(256) void k_tsdf_finalize(const float* __restrict__ tsdf_sum, const float* __restrict__ weight,
                                                       const float* __restrict__ color_sum, long long N, float* __restrict__ tsdf,
                                                       float* __restrict__ color) {
    for (long long n = blockIdx.x * 256ll + threadIdx.x; n < N; n += gridDim.x * 256ll) {
        const float w = weight[n];
        const bool seen = w > 0.f;
        // (the fp64 quotient of two fp32 numbers, rounded to fp32, is the correctly rounded fp32 quotient)
        tsdf[n] = seen ? (float)((double)tsdf_sum[n] / (double)w) : 1.f;
        if (color)
#pragma unroll
            for (int k = 0; k < 3; ++k) color[3 * (size_t)n + k] = seen ? (float)((double)color_sum[3 * (size_t)n + k] / (double)w) : 0.f;
    }
}

__global__ __launch_bounds__(256) void k_volume_sample(const float* __restrict__ volume, int R, int C, const float* __restrict__ points,
                                                       long long M, SampleBounds b, float* __restrict__ values,
                                                       unsigned char* __restrict__ inside) {
#pragma clang fp contract(off)
    const double top = (double)(R - 1);
    for (long long r = blockIdx.x * 256ll + threadIdx.x; r < M; r += gridDim.x * 256ll) {
        double g[3];
        bool in = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            g[k] = ((double)points[3 * (size_t)r + k] - b.lo[k]) / (b.hi[k] - b.lo[k]) * top;
            in = in && g[k] >= 0.0 && g[k] <= top;          // (false for NaN)
        }
        inside[r] = in;
        float* o = values + (size_t)r * C;
        if (!in) {
            for (int ch = 0; ch < C; ++ch) o[ch] = 0.f;
            continue;
        }
        int i0[3];
        double fr[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int i = (int)floor(g[k]);
            i = i > R - 2 ? R - 2 : i; i = i < 0 ? 0 : i;          // the cell [i, i + 1] lies in [0, R - 1]
            i0[k] = i;
            fr[k] = g[k] - (double)i;
        }
        const size_t sx = (size_t)R * R * C, sy = (size_t)R * C, sz = (size_t)C;
        const float* base = volume + i0[0] * sx + i0[1] * sy + i0[2] * sz;
        for (int ch = 0; ch < C; ++ch) {
            double yb[2];
#pragma unroll
            for (int ix = 0; ix < 2; ++ix) {
                double zb[2];
#pragma unroll
                for (int iy = 0; iy < 2; ++iy) {
                    const double a = base[ix * sx + iy * sy + ch], e = base[ix * sx + iy * sy + sz + ch];
                    zb[iy] = a + fr[2] * (e - a);
                }
                yb[ix] = zb[0] + fr[1] * (zb[1] - zb[0]);
            }
            o[ch] = (float)(yb[0] + fr[0] * (yb[1] - yb[0]));
        }
    }
}

static bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace es

using namespace es;

extern "C" {

int es_tsdf_integrate(const float* positions, long long frame_stride, const unsigned char* valid, long long N, int F, const float* depth,
                      const float* color, const unsigned char* mask, const double* cameras, int height, int width, double trunc,
                      double depth_trunc, float* tsdf_sum, float* weight, float* color_sum, void* stream) {
    ES_REQUIRE(N >= 0 && F >= 0, "es_tsdf_integrate: N and F must not be negative");
    ES_REQUIRE(height >= 1 && height <= FUSE_MAX_SIZE && width >= 1 && width <= FUSE_MAX_SIZE,
               "es_tsdf_integrate: height and width must be in [1, 8192]");
    ES_REQUIRE(N <= FUSE_MAX_INDEX / 3, "es_tsdf_integrate: N: 3 N must stay below 2^31");
    ES_REQUIRE(F == 0 || N <= FUSE_MAX_INDEX / F, "es_tsdf_integrate: F, N: F N must stay below 2^31");
    ES_REQUIRE(F == 0 || (long long)height * width <= FUSE_MAX_INDEX / F, "es_tsdf_integrate: F, height, width: F H W must stay below 2^31");
    ES_REQUIRE(trunc > 0.0 && trunc <= 1.7976931348623157e308, "es_tsdf_integrate: trunc must be finite and positive");
    ES_REQUIRE(depth_trunc > 0.0, "es_tsdf_integrate: depth_trunc must be positive (it may be infinite)");
    ES_REQUIRE(frame_stride == 0 || frame_stride == N, "es_tsdf_integrate: frame_stride must be 0 (one lattice for all frames) or N");
    if (N == 0 || F == 0) return ST_OK;          // (an empty buffer may be a null pointer: nothing below is asked of an empty call)
    ES_REQUIRE((color != nullptr) == (color_sum != nullptr), "es_tsdf_integrate: color and color_sum go together");
    ES_REQUIRE(positions && depth && cameras && tsdf_sum && weight, "es_tsdf_integrate: null buffer (positions, depth, cameras, tsdf_sum, weight)");
    ES_REQUIRE(aligned(positions, 4) && aligned(depth, 4) && aligned(tsdf_sum, 4) && aligned(weight, 4) && aligned(color, 4) &&
                   aligned(color_sum, 4), "es_tsdf_integrate: fp32 buffers must be 4-byte aligned");
    ES_REQUIRE(aligned(cameras, 8), "es_tsdf_integrate: cameras must be 8-byte aligned");
    hipLaunchKernelGGL(k_tsdf_integrate, dim3(grid_for(N)), dim3(256), 0, static_cast<hipStream_t>(stream), positions, frame_stride, valid,
                       (int)N, F, depth, color, mask, cameras, height, width, trunc, depth_trunc, tsdf_sum, weight, color_sum);
    return hip_last("es_tsdf_integrate");
}

int es_tsdf_finalize(const float* tsdf_sum, const float* weight, const float* color_sum, long long N, float* tsdf, float* color,
                     void* stream) {
    ES_REQUIRE(N >= 0, "es_tsdf_finalize: N must not be negative");
    ES_REQUIRE(N <= FUSE_MAX_INDEX / 3, "es_tsdf_finalize: N: 3 N must stay below 2^31");
    ES_REQUIRE((color != nullptr) == (color_sum != nullptr), "es_tsdf_finalize: color and color_sum go together");
    if (N == 0) return ST_OK;
    ES_REQUIRE(tsdf_sum && weight && tsdf, "es_tsdf_finalize: null buffer (tsdf_sum, weight, tsdf)");
    hipLaunchKernelGGL(k_tsdf_finalize, dim3(grid_for(N)), dim3(256), 0, static_cast<hipStream_t>(stream), tsdf_sum, weight, color_sum, N,
                       tsdf, color);
    return hip_last("es_tsdf_finalize");
}

int es_volume_sample(const float* volume, int resolution, int channels, const float* points, long long M, const double* bounds,
                     float* values, unsigned char* inside, void* stream) {
    ES_REQUIRE(M >= 0, "es_volume_sample: M must not be negative");
    ES_REQUIRE(resolution >= 2 && resolution <= 2048, "es_volume_sample: resolution must be in [2, 2048]");
    ES_REQUIRE(channels >= 1 && channels <= FUSE_MAX_CHANNELS, "es_volume_sample: channels must be in [1, 8]");
    ES_REQUIRE((long long)resolution * resolution * resolution <= FUSE_MAX_INDEX / channels,
               "es_volume_sample: resolution^3 channels must stay below 2^31");
    ES_REQUIRE(M <= FUSE_MAX_INDEX / 8, "es_volume_sample: M: 8 M must stay below 2^31");
    ES_REQUIRE(bounds, "es_volume_sample needs bounds (6 doubles on the host: bound_min, bound_max)");
    SampleBounds b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = bounds[k]; b.hi[k] = bounds[3 + k];
        ES_REQUIRE(std::isfinite(b.lo[k]) && std::isfinite(b.hi[k]) && b.hi[k] > b.lo[k], "es_volume_sample: bounds must be finite with bound_max > bound_min");
    }
    if (M == 0) return ST_OK;
    ES_REQUIRE(volume && points && values && inside, "es_volume_sample: null buffer (volume, points, values, inside)");
    hipLaunchKernelGGL(k_volume_sample, dim3(grid_for(M)), dim3(256), 0, static_cast<hipStream_t>(stream), volume, resolution, channels,
                       points, M, b, values, inside);
    return hip_last("es_volume_sample");
}

}  // extern "C"
