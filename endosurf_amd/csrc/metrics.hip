// Frame evaluation (ABI v13): what the reference's eval() does with whole rendered frames once they exist -- SSIM, the masked squared
// sums behind PSNR and RMSE, and the rgb / depth / normal panels of its eval picture (src/trainer/utils.py cal_ssim, cal_psnr, cal_rmse,
// gen_rgb, gen_depth, gen_normal) -- without moving an image to the host.  Numpy twins: endosurf_amd/imaging.py, which are the
// specification.  Contract: DESIGN.md 7d.  Images are channel-last fp32 [n][H][W][C]; a mask is per pixel, [n][H][W], nullable = ones.
//
//   k_ssim              one workgroup per (frame, 32 x 32 tile of the "valid" map [H-10][W-10]): stages the 42 x 42 x C inputs of both
//                       images, already multiplied by the mask (in fp32, as the reference multiplies), and the 121-entry window in LDS
//                       (at most 56 KB + 1 KB); every thread then owns four map positions (rows ty, ty + 8, ty + 16, ty + 24 of column
//                       tx) and runs the 121 taps once per channel with the five fp64 moments a, b, aa, bb, ab of each in registers.
//                       Optional map store; one fp64 partial sum per workgroup
//   k_masked_sq_sums    one workgroup per (frame, 2048 pixels): S = sum (a - b)^2 m over pixels and channels, M = sum m over pixels,
//                       fp64; two partials per workgroup
//   k_frame_reduce      one workgroup per frame: the frame's partials added in index order (thread t owns a contiguous run, the runs are
//                       combined by the fixed tree of block_scan2) -> out[f] (/ the map size for SSIM), out[n + f]
//   k_frame_total       one workgroup: the same over the frames -> out[K n ...] (the mean of the per-frame SSIMs; sum S, sum M)
//   k_panel_rgb / _depth / _normal
//                       one thread per pixel, three byte stores at out[(f H + y) pitch + 3 (col + x)]: the caller points several panels
//                       at the columns of one sheet, so nothing is concatenated afterwards
//
// No atomics at all: a partial is written by exactly one workgroup and read by a later launch, so two calls give the same bits whatever
// the scratch held before.  No workgroup waits for another.  Every device loop is bounded by an argument or a constant.  Every address
// is built from indices checked against n, H, W, C; the host side refuses sizes whose products leave int32.  The window is data (121
// floats from the caller): after its rounding to fp32 it is not an outer product, and a separable evaluation would move map entries by
// 2e-6.  The library is compiled with contraction, so a w * x + acc here is one fma where the twin rounds twice: the device is held to
// the twin within a tolerance (1e-10 per map entry), bit-exact only from call to call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"
#include "scan.h"

namespace es {

constexpr int SSIM_K = 11;                                   // window side
constexpr int SSIM_TAPS = SSIM_K * SSIM_K;
constexpr int SSIM_TILE = 32;                                // map positions per workgroup and axis
constexpr int SSIM_IN = SSIM_TILE + SSIM_K - 1;              // 42 input rows / columns of a tile
constexpr int SSIM_PLANE = SSIM_IN * SSIM_IN;                // floats of one channel of one image in LDS
constexpr int SSIM_MAX_C = 4;                                // 2 x 4 x 1764 floats = 56 448 bytes of LDS
constexpr int SSIM_ROWS = SSIM_TILE / 8;                     // map positions of one thread (256 threads = 8 rows of 32)
constexpr int EVAL_MAX_SIZE = 8192;                          // largest image side
constexpr int EVAL_MAX_C = 16;                               // channels of es_masked_sq_sums
constexpr long long EVAL_MAX_COUNT = 1ll << 31;              // every element count stays inside int32
constexpr int SQ_PER_THREAD = 8;
constexpr int SQ_CHUNK = 256 * SQ_PER_THREAD;                // pixels per workgroup of k_masked_sq_sums

static inline int ssim_tiles_x(int W) { return (W - SSIM_K + 1 + SSIM_TILE - 1) / SSIM_TILE; }
static inline int ssim_tiles_y(int H) { return (H - SSIM_K + 1 + SSIM_TILE - 1) / SSIM_TILE; }
static inline int sq_blocks(int H, int W) { return (int)(((long long)H * W + SQ_CHUNK - 1) / SQ_CHUNK); }

__global__ __launch_bounds__(256) void k_ssim(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mask,
                                              const float* __restrict__ win, int H, int W, int C, int tiles_x, int tiles_per_frame, double c1,
                                              double c2, double* __restrict__ part, double* __restrict__ map) {
    extern __shared__ float ssim_lds[];          // a: [C][42][42], then b the same
    __shared__ double sw[SSIM_TAPS];
    __shared__ double red[4][2];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / tiles_per_frame, tile = blockIdx.x % tiles_per_frame;
    const int oy0 = (tile / tiles_x) * SSIM_TILE, ox0 = (tile % tiles_x) * SSIM_TILE;
    float* sa = ssim_lds;
    float* sb = ssim_lds + C * SSIM_PLANE;
    if (tid < SSIM_TAPS) sw[tid] = (double)win[tid];
    const int row_len = SSIM_IN * C;
    const size_t frame = (size_t)f * H * W;
    for (int e = tid; e < SSIM_IN * row_len; e += 256) {          // (global order: row, column, channel)
        const int r = e / row_len, rem = e % row_len, col = rem / C, c = rem % C;
        const int y = oy0 + r, x = ox0 + col;
        float va = 0.f, vb = 0.f;
        if (y < H && x < W) {
            const size_t p = frame + (size_t)y * W + x;
            const float m = mask ? mask[p] : 1.f;
            va = a[p * C + c] * m;
            vb = b[p * C + c] * m;
        }
        sa[c * SSIM_PLANE + r * SSIM_IN + col] = va;
        sb[c * SSIM_PLANE + r * SSIM_IN + col] = vb;
    }
    __syncthreads();

    const int tx = tid & 31, ty = tid >> 5;
    const int Ho = H - SSIM_K + 1, Wo = W - SSIM_K + 1;
    double sum = 0.0;
    for (int c = 0; c < C; ++c) {
        double acc[SSIM_ROWS][5];
#pragma unroll
        for (int k = 0; k < SSIM_ROWS; ++k) {
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[k][q] = 0.0;
        }
        const float* pa = sa + c * SSIM_PLANE + ty * SSIM_IN + tx;
        const float* pb = sb + c * SSIM_PLANE + ty * SSIM_IN + tx;
#pragma unroll 1
        for (int i = 0; i < SSIM_K; ++i) {
#pragma unroll
            for (int j = 0; j < SSIM_K; ++j) {
                const double w = sw[i * SSIM_K + j];
#pragma unroll
                for (int k = 0; k < SSIM_ROWS; ++k) {
                    const double x = (double)pa[(8 * k + i) * SSIM_IN + j], y = (double)pb[(8 * k + i) * SSIM_IN + j];
                    acc[k][0] += w * x;
                    acc[k][1] += w * y;
                    acc[k][2] += w * (x * x);
                    acc[k][3] += w * (y * y);
                    acc[k][4] += w * (x * y);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < SSIM_ROWS; ++k) {
            const int oy = oy0 + ty + 8 * k, ox = ox0 + tx;
            if (oy < Ho && ox < Wo) {
                const double mu1 = acc[k][0], mu2 = acc[k][1];
                const double mu12 = mu1 * mu2, mu11 = mu1 * mu1, mu22 = mu2 * mu2;
                const double s1 = acc[k][2] - mu11, s2 = acc[k][3] - mu22, s12 = acc[k][4] - mu12;
                const double v = ((2.0 * mu12 + c1) * (2.0 * s12 + c2)) / ((mu11 + mu22 + c1) * (s1 + s2 + c2));
                sum += v;
                if (map) map[(((size_t)f * Ho + oy) * Wo + ox) * C + c] = v;
            }
        }
    }
    double none = 0.0, total[2];
    block_scan2(sum, none, red, total);
    if (tid == 0) part[blockIdx.x] = total[0];
}

__global__ __launch_bounds__(256) void k_masked_sq_sums(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mask,
                                                        int P, int C, int nblk, double* __restrict__ part) {
    __shared__ double red[4][2];
    const int f = blockIdx.x / nblk, blk = blockIdx.x % nblk;
    double S = 0.0, M = 0.0;
#pragma unroll 1
    for (int k = 0; k < SQ_PER_THREAD; ++k) {
        const long long p = (long long)blk * SQ_CHUNK + k * 256 + threadIdx.x;
        if (p < P) {
            const size_t g = (size_t)f * P + (size_t)p;
            const double m = mask ? (double)mask[g] : 1.0;
            for (int c = 0; c < C; ++c) {
                const double d = (double)a[g * C + c] - (double)b[g * C + c];
                S += (d * d) * m;
            }
            M += m;
        }
    }
    double total[2];
    block_scan2(S, M, red, total);
    if (threadIdx.x == 0) { part[2 * (size_t)blockIdx.x] = total[0]; part[2 * (size_t)blockIdx.x + 1] = total[1]; }
}

// out[f] = (sum of the frame's first partials) / div0, and with K == 2: out[n + f] = the sum of its second ones.
__global__ __launch_bounds__(256) void k_frame_reduce(const double* __restrict__ part, int nblk, int K, double div0, int n, double* __restrict__ out) {
    __shared__ double red[4][2];
    const int f = blockIdx.x;
    const int per = (nblk + 255) / 256, c0 = threadIdx.x * per, c1 = c0 + per < nblk ? c0 + per : nblk;
    double v0 = 0.0, v1 = 0.0, total[2];
    for (int c = c0; c < c1; ++c) {
        const size_t at = ((size_t)f * nblk + c) * K;
        v0 += part[at];
        if (K == 2) v1 += part[at + 1];
    }
    block_scan2(v0, v1, red, total);
    if (threadIdx.x == 0) {
        out[f] = total[0] / div0;
        if (K == 2) out[n + f] = total[1];
    }
}

// out[K n] = (out[0] + ... + out[n - 1]) / div0, and with K == 2: out[2 n + 1] = out[n] + ... + out[2 n - 1].
__global__ __launch_bounds__(256) void k_frame_total(int K, double div0, int n, double* __restrict__ out) {
    __shared__ double red[4][2];
    const int per = (n + 255) / 256, c0 = threadIdx.x * per, c1 = c0 + per < n ? c0 + per : n;
    double v0 = 0.0, v1 = 0.0, total[2];
    for (int c = c0; c < c1; ++c) {
        v0 += out[c];
        if (K == 2) v1 += out[n + c];
    }
    block_scan2(v0, v1, red, total);
    if (threadIdx.x == 0) {
        out[(size_t)K * n] = total[0] / div0;
        if (K == 2) out[(size_t)K * n + 1] = total[1];
    }
}

struct PanelOut {
    unsigned char* out;              // the first byte of frame 0, row 0 of the picture the panel goes into
    long long pitch;                 // bytes from one row of that picture to the next (its frames follow each other: H rows each)
    int col;                         // the panel's first column there, in pixels
};
__device__ __forceinline__ unsigned char* panel_at(const PanelOut& o, long long p, int H, int W) {
    const long long row = p / W;          // = f H + y
    const int x = (int)(p % W);
    return o.out + row * o.pitch + 3ll * (o.col + x);
}
__device__ __forceinline__ unsigned char panel_byte(double v) { return (unsigned char)(int)fmin(fmax(v, 0.0), 255.0); }          // (NaN -> 0)

__global__ __launch_bounds__(256) void k_panel_rgb(const float* __restrict__ x, long long pixels, int H, int W, int C, PanelOut o) {
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < pixels; p += gridDim.x * 256ll) {
        unsigned char* q = panel_at(o, p, H, W);
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = panel_byte(256.0 * (double)x[p * C + (C == 3 ? c : 0)]);
    }
}

__global__ __launch_bounds__(256) void k_panel_depth(const float* __restrict__ d, long long pixels, int H, int W, double depth_max, PanelOut o) {
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < pixels; p += gridDim.x * 256ll) {
        unsigned char* q = panel_at(o, p, H, W);
        const double r = fmin(fmax((double)d[p] / depth_max, 0.0), 1.0);
        const unsigned char v = panel_byte(255.0 - r * 255.0);
        q[0] = v; q[1] = v; q[2] = v;
    }
}

__global__ __launch_bounds__(256) void k_panel_normal(const float* __restrict__ nrm, const float* __restrict__ rot, long long pixels, int H, int W,
                                                      int revert, float* __restrict__ out_f, PanelOut o) {
    const long long per_frame = (long long)H * W;
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < pixels; p += gridDim.x * 256ll) {
        const float* r = rot + 9 * (p / per_frame);
        const double x = (double)nrm[3 * p], y = (double)nrm[3 * p + 1], z = (double)nrm[3 * p + 2];
        const double len = sqrt((x * x + y * y) + z * z) + 1e-10;
        const double ux = x / len, uy = y / len, uz = z / len;
        unsigned char* q = panel_at(o, p, H, W);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double v = ((double)r[3 * i] * ux + (double)r[3 * i + 1] * uy) + (double)r[3 * i + 2] * uz;
            if (revert) v = -v;
            if (out_f) out_f[3 * p + i] = (float)v;
            q[i] = panel_byte(128.0 * v + 128.0);
        }
    }
}

static int eval_sizes(int n, int H, int W, int C, int min_side, int max_c) {
    ES_REQUIRE(n >= 0, "negative frame count");
    ES_REQUIRE(H >= min_side && H <= EVAL_MAX_SIZE && W >= min_side && W <= EVAL_MAX_SIZE,
               min_side > 1 ? "image height and width must be 11..8192 (the window is 11 x 11)" : "image height and width must be 1..8192");
    ES_REQUIRE(C >= 1 && C <= max_c, "channel count out of range");
    ES_REQUIRE((long long)n * H * W * (C > 3 ? C : 3) < EVAL_MAX_COUNT, "2^31 image elements or more in one call");
    return ST_OK;
}
static int ssim_sizes(int n, int H, int W, int C) {
    if (const int s = eval_sizes(n, H, W, C, SSIM_K, SSIM_MAX_C)) return s;
    ES_REQUIRE((long long)n * (H - SSIM_K + 1) * (W - SSIM_K + 1) * C < EVAL_MAX_COUNT, "2^31 SSIM map entries or more in one call");
    ES_REQUIRE((long long)n * ssim_tiles_x(W) * ssim_tiles_y(H) < EVAL_MAX_COUNT, "2^31 SSIM tiles or more in one call");
    return ST_OK;
}
static int panel_out(int n, int H, int W, unsigned char* out, long long pitch, int col, PanelOut& o) {
    if (const int s = eval_sizes(n, H, W, 3, 1, 3)) return s;
    ES_REQUIRE(col >= 0 && pitch >= 3ll * ((long long)col + W), "panel does not fit its picture: pitch < 3 (col + W) or col < 0");
    ES_REQUIRE((long long)n * H * pitch < (1ll << 40), "picture too large");
    ES_REQUIRE(n == 0 || out, "panel needs an output picture");
    o.out = out; o.pitch = pitch; o.col = col;
    return ST_OK;
}

}  // namespace es

using namespace es;

#define EVAL_ALIGNED8(p, what) ES_REQUIRE(p && reinterpret_cast<uintptr_t>(p) % 8 == 0, what " must be an 8-byte aligned device buffer")

extern "C" {

int64_t es_ssim_scratch_bytes(int n, int height, int width) {
    if (ssim_sizes(n, height, width, 1) != ST_OK) return -1;
    return 8ll * (n > 0 ? n : 1) * ssim_tiles_x(width) * ssim_tiles_y(height);
}

int es_ssim(const float* a, const float* b, const float* mask, const float* window, int n, int height, int width, int channels, double data_range,
            void* scratch, double* out, double* map, void* stream) {
    if (const int s = ssim_sizes(n, height, width, channels)) return s;
    ES_REQUIRE(std::isfinite(data_range) && data_range > 0.0, "data_range must be finite and positive");
    if (n == 0) return ST_OK;
    ES_REQUIRE(a && b && window, "es_ssim needs a, b and the 121-entry window");
    EVAL_ALIGNED8(scratch, "ssim scratch");
    EVAL_ALIGNED8(out, "ssim out");
    ES_REQUIRE(reinterpret_cast<uintptr_t>(map) % 8 == 0, "ssim map must be 8-byte aligned");
    const int tx = ssim_tiles_x(width), tiles = tx * ssim_tiles_y(height);
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    const size_t lds = 2ull * channels * SSIM_PLANE * sizeof(float);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(scratch);
    hipLaunchKernelGGL(k_ssim, dim3((unsigned)(n * tiles)), dim3(256), lds, st, a, b, mask, window, height, width, channels, tx, tiles, c1, c2, part, map);
    const double entries = (double)(height - SSIM_K + 1) * (double)(width - SSIM_K + 1) * (double)channels;
    hipLaunchKernelGGL(k_frame_reduce, dim3((unsigned)n), dim3(256), 0, st, part, tiles, 1, entries, n, out);
    hipLaunchKernelGGL(k_frame_total, dim3(1), dim3(256), 0, st, 1, (double)n, n, out);
    return hip_last("es_ssim");
}

int64_t es_sq_sums_scratch_bytes(int n, int height, int width) {
    if (eval_sizes(n, height, width, 1, 1, EVAL_MAX_C) != ST_OK) return -1;
    return 16ll * (n > 0 ? n : 1) * sq_blocks(height, width);
}

int es_masked_sq_sums(const float* a, const float* b, const float* mask, int n, int height, int width, int channels, void* scratch, double* out,
                      void* stream) {
    if (const int s = eval_sizes(n, height, width, channels, 1, EVAL_MAX_C)) return s;
    const int nblk = sq_blocks(height, width);
    ES_REQUIRE((long long)n * nblk < EVAL_MAX_COUNT, "2^31 workgroups or more in one call");
    if (n == 0) return ST_OK;
    ES_REQUIRE(a && b, "es_masked_sq_sums needs a and b");
    EVAL_ALIGNED8(scratch, "sq-sums scratch");
    EVAL_ALIGNED8(out, "sq-sums out");
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(scratch);
    hipLaunchKernelGGL(k_masked_sq_sums, dim3((unsigned)(n * nblk)), dim3(256), 0, st, a, b, mask, height * width, channels, nblk, part);
    hipLaunchKernelGGL(k_frame_reduce, dim3((unsigned)n), dim3(256), 0, st, part, nblk, 2, 1.0, n, out);
    hipLaunchKernelGGL(k_frame_total, dim3(1), dim3(256), 0, st, 2, 1.0, n, out);
    return hip_last("es_masked_sq_sums");
}

int es_eval_panel_rgb(const float* x, int n, int height, int width, int channels, unsigned char* out, long long pitch, int col, void* stream) {
    PanelOut o;
    if (const int s = panel_out(n, height, width, out, pitch, col, o)) return s;
    ES_REQUIRE(channels == 1 || channels == 3, "an rgb panel takes 1 or 3 channels");
    if (n == 0) return ST_OK;
    ES_REQUIRE(x, "es_eval_panel_rgb needs its image");
    const long long pixels = (long long)n * height * width;
    hipLaunchKernelGGL(k_panel_rgb, dim3(grid_for(pixels)), dim3(256), 0, static_cast<hipStream_t>(stream), x, pixels, height, width, channels, o);
    return hip_last("es_eval_panel_rgb");
}

int es_eval_panel_depth(const float* depth, int n, int height, int width, double depth_max, unsigned char* out, long long pitch, int col, void* stream) {
    PanelOut o;
    if (const int s = panel_out(n, height, width, out, pitch, col, o)) return s;
    ES_REQUIRE(std::isfinite(depth_max) && depth_max > 0.0, "depth_max must be finite and positive");
    if (n == 0) return ST_OK;
    ES_REQUIRE(depth, "es_eval_panel_depth needs its image");
    const long long pixels = (long long)n * height * width;
    hipLaunchKernelGGL(k_panel_depth, dim3(grid_for(pixels)), dim3(256), 0, static_cast<hipStream_t>(stream), depth, pixels, height, width, depth_max, o);
    return hip_last("es_eval_panel_depth");
}

int es_eval_panel_normal(const float* normals, const float* rot, int n, int height, int width, int revert, float* out_f, unsigned char* out,
                         long long pitch, int col, void* stream) {
    PanelOut o;
    if (const int s = panel_out(n, height, width, out, pitch, col, o)) return s;
    if (n == 0) return ST_OK;
    ES_REQUIRE(normals && rot, "es_eval_panel_normal needs normals and one 3 x 3 rotation per frame");
    const long long pixels = (long long)n * height * width;
    hipLaunchKernelGGL(k_panel_normal, dim3(grid_for(pixels)), dim3(256), 0, static_cast<hipStream_t>(stream), normals, rot, pixels, height, width,
                       revert != 0, out_f, o);
    return hip_last("es_eval_panel_normal");
}

}  // extern "C"
