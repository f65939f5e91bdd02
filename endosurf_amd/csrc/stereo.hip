// Stereo disparity by semi-global matching over a census cost (endosurf_amd/stereo.py is the specification and the twin).
// Every kernel takes a batch of n image pairs; all arithmetic up to the sub-pixel step is integer, so the results are the twin's bits.
//   k_stereo_census   one thread per pixel: the 62-bit signature of the 9 x 7 window, border replicated
//   k_sgm_cost        one thread per (pixel, d): popcount(cl ^ cr) as a byte, 63 where the right column is left of the image
//   k_sgm_aggregate   ONE WAVEFRONT PER PATH LINE of one direction, lanes over d in blocks of KD = ceil(D / 64) consecutive disparities
//                     (lane l owns d = KD l .. KD l + KD - 1).  Along the line the step is sequential: min_k by an xor butterfly of
//                     __shfl, d -+ 1 across the lane boundary by one __shfl_up and one __shfl_down, the rest in the lane's registers;
//                     the costs of the next step are loaded before the current step reduces.  S += L_r by a plain read-modify-write:
//                     within a launch (one direction) every pixel lies on exactly one line, so each element has one owner; the first
//                     direction stores instead of adding, so S needs no clearing.  The sum of integers is the same in any order.
//   k_sgm_right       one wavefront per right-view pixel, lanes over d: dR = argmin_d S[y, x + d + dmin, d] over the columns that
//                     exist, -1 for none; the argmin is the minimum of the unsigned keys (sum << 16 | d), so ties go to the smallest d
//   k_sgm_select      one wavefront per pixel, lanes over d (the row of D sums is one coalesced read): argmin by the same keys, the
//                     second minimum for the uniqueness test, then lane 0: left-right check against dR, parabola sub-pixel (one
//                     fp64 division, one fp64 addition), d0 / disparity / flags / valid
//   k_speckle_init / k_speckle_sweep / k_speckle_count / k_speckle_apply
//                     segments of valid pixels by minimum-label propagation, in place: pixel p alone writes label[p], which only ever
//                     decreases and never leaves p's segment (a neighbour's label, or the label of its own label), so the fixed point --
//                     every pixel holds the smallest pixel index of its segment -- does not depend on the order of reads; sizes by
//                     integer atomics on 32-bit words; a pixel of a segment below the size limit is cleared.
// No float atomics, no inline assembly, no LDS.  Every index is checked against the image or the disparity range before it addresses
// memory, every loop is bounded by an argument, and the aggregation's invalid lanes (d >= D) neither load nor store.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/endosurf_hip.h"
#include "launch.h"

namespace es {

constexpr int STEREO_MAX_SIZE = 8192;
constexpr int STEREO_MAX_D = 256;
constexpr int STEREO_MAX_PENALTY = 1024;
constexpr long long STEREO_MAX_INDEX = (1ll << 31) - 1;
constexpr int STEREO_OUTSIDE = 63;
constexpr int STEREO_FAR = 1 << 20;          // a path cost no minimum picks: (63 + 1024) 8 stays far below it, and sums of two stay in int32

__global__ __launch_bounds__(256) void k_stereo_census(const unsigned char* __restrict__ grey, long long n_pix, int H, int W,
                                                       long long* __restrict__ out) {
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < n_pix; p += gridDim.x * 256ll) {
        const int x = (int)(p % W), y = (int)((p / W) % H);
        const unsigned char* img = grey + (p - (long long)y * W - x);
        const int c = img[(size_t)y * W + x];
        unsigned long long bits = 0;
        for (int j = -3; j <= 3; ++j) {
            const int yy = min(max(y + j, 0), H - 1);
#pragma unroll
            for (int i = -4; i <= 4; ++i) {
                if (i == 0 && j == 0) continue;
                const int xx = min(max(x + i, 0), W - 1);
                bits = (bits << 1) | (unsigned long long)(img[(size_t)yy * W + xx] < c);
            }
        }
        out[p] = (long long)bits;
    }
}

__global__ __launch_bounds__(256) void k_sgm_cost(const long long* __restrict__ cl, const long long* __restrict__ cr, long long total,
                                                  int W, int D, int dmin, unsigned char* __restrict__ C) {
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += gridDim.x * 256ll) {
        const long long p = e / D;
        const int d = (int)(e - p * D), x = (int)(p % W);
        const int xr = x - dmin - d;          // (dmin <= 8192: no wrap)
        C[e] = xr < 0 ? (unsigned char)STEREO_OUTSIDE : (unsigned char)__popcll((unsigned long long)(cl[p] ^ cr[p - dmin - d]));
    }
}

// The minimum of a value over the wavefront, on every lane: an xor butterfly of six __shfl.
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// The start pixel and the length of path line ``line`` (0 <= line < lines of the direction) of direction ``dir`` in an H x W image.
__device__ __forceinline__ void path_line(int dir, int line, int H, int W, int& y0, int& x0, int& dy, int& dx, int& len) {
    switch (dir >> 1) {
        case 0: y0 = line; x0 = 0; dy = 0; dx = 1; len = W; break;                                            // rows
        case 1: y0 = 0; x0 = line; dy = 1; dx = 0; len = H; break;                                            // columns
        case 2:                                                                                               // down-right diagonals
            y0 = line < W ? 0 : line - W + 1; x0 = line < W ? line : 0; dy = 1; dx = 1;
            len = min(H - y0, W - x0);
            break;
        default:                                                                                              // down-left diagonals
            y0 = line < W ? 0 : line - W + 1; x0 = line < W ? line : W - 1; dy = 1; dx = -1;
            len = min(H - y0, x0 + 1);
            break;
    }
    if (dir & 1) {          // the opposite direction walks the same line from its other end
        y0 += (len - 1) * dy; x0 += (len - 1) * dx;
        dy = -dy; dx = -dx;
    }
}

template <int KD>
__global__ __launch_bounds__(256) void k_sgm_aggregate(const unsigned char* __restrict__ C, unsigned short* __restrict__ S, int n, int H,
                                                       int W, int D, int dir, int lines, int P1, int P2, int first) {
    const int lane = threadIdx.x & 63;
    const long long wave = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (wave >= (long long)n * lines) return;          // (wave-uniform: whole wavefronts leave)
    const int img = (int)(wave / lines), line = (int)(wave - (long long)img * lines);
    int y, x, dy, dx, len;
    path_line(dir, line, H, W, y, x, dy, dx, len);
    const int d_lo = lane * KD;
    bool live[KD];
#pragma unroll
    for (int k = 0; k < KD; ++k) live[k] = d_lo + k < D;
    const size_t image = (size_t)img * H * W;
    const long long stride = ((long long)dy * W + dx) * D;          // elements from one pixel's row of D to the next one's
    long long at = (long long)((image + (size_t)y * W + x) * D) + d_lo;
    int cost[KD], next[KD], L[KD];
#pragma unroll
    for (int k = 0; k < KD; ++k) { cost[k] = live[k] ? C[at + k] : 0; next[k] = 0; L[k] = STEREO_FAR; }
    for (int step = 0; step < len; ++step) {
        if (step + 1 < len) {          // the next pixel's costs are on their way while this step reduces
#pragma unroll
            for (int k = 0; k < KD; ++k) next[k] = live[k] ? C[at + stride + k] : 0;
        }
        if (step == 0) {
#pragma unroll
            for (int k = 0; k < KD; ++k) L[k] = live[k] ? cost[k] : STEREO_FAR;
        } else {
            int m = L[0];
#pragma unroll
            for (int k = 1; k < KD; ++k) m = min(m, L[k]);
            m = wave_min(m);
            int below = __shfl_up(L[KD - 1], 1, 64), above = __shfl_down(L[0], 1, 64);
            if (lane == 0) below = STEREO_FAR;
            if (lane == 63) above = STEREO_FAR;
            int prev[KD];
#pragma unroll
            for (int k = 0; k < KD; ++k) prev[k] = L[k];
#pragma unroll
            for (int k = 0; k < KD; ++k) {
                const int lo = k > 0 ? prev[k - 1] : below, hi = k + 1 < KD ? prev[k + 1] : above;
                const int best = min(min(prev[k], m + P2), min(lo, hi) + P1);
                L[k] = live[k] ? cost[k] + best - m : STEREO_FAR;
            }
        }
#pragma unroll
        for (int k = 0; k < KD; ++k)
            if (live[k]) S[at + k] = (unsigned short)(first ? L[k] : S[at + k] + L[k]);
#pragma unroll
        for (int k = 0; k < KD; ++k) cost[k] = next[k];
        at += stride;
    }
}

// The argmin of up to 256 sums spread over a wavefront, smallest d on ties: the minimum of the UNSIGNED keys (sum << 16 | d), which order
// every uint16 sum; no key reaches STEREO_NO_KEY because d <= 255.  STEREO_NO_SUM is above every sum.
constexpr unsigned STEREO_NO_KEY = 0xffffffffu;
constexpr int STEREO_NO_SUM = 0x7fffffff;

__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void k_sgm_right(const unsigned short* __restrict__ S, long long n_pix, int W, int D, int dmin,
                                                   int* __restrict__ dR) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = gridDim.x * 4ll;
    for (long long p = blockIdx.x * 4ll + (threadIdx.x >> 6); p < n_pix; p += n_waves) {          // one wavefront per right-view pixel
        const int x = (int)(p % W);
        unsigned key = STEREO_NO_KEY;
#pragma unroll
        for (int k = 0; k < STEREO_MAX_D / 64; ++k) {
            const int d = lane + 64 * k;          // (dmin <= 8192: x + dmin + d stays far inside int32)
            if (d < D && x + dmin + d < W) key = min(key, ((unsigned)S[(size_t)(p + dmin + d) * D + d] << 16) | (unsigned)d);
        }
        key = wave_min(key);
        if (lane == 0) dR[p] = key == STEREO_NO_KEY ? -1 : (int)(key & 0xffffu);
    }
}

__global__ __launch_bounds__(256) void k_sgm_select(const unsigned short* __restrict__ S, const int* __restrict__ dR, long long n_pix,
                                                    int W, int D, int dmin, int uniqueness, int lr_max, int subpixel,
                                                    int* __restrict__ d0_out, float* __restrict__ disparity,
                                                    unsigned char* __restrict__ flags, unsigned char* __restrict__ valid) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = gridDim.x * 4ll;
    for (long long p = blockIdx.x * 4ll + (threadIdx.x >> 6); p < n_pix; p += n_waves) {          // one wavefront per pixel, lanes over d
        const unsigned short* s = S + (size_t)p * D;
        int v[STEREO_MAX_D / 64];
        unsigned key = STEREO_NO_KEY;
#pragma unroll
        for (int k = 0; k < STEREO_MAX_D / 64; ++k) {
            const int d = lane + 64 * k;
            v[k] = d < D ? (int)s[d] : -1;
            if (d < D) key = min(key, ((unsigned)v[k] << 16) | (unsigned)d);
        }
        key = wave_min(key);          // (D >= 1: some lane holds a key)
        const int d0 = (int)(key & 0xffffu), s0 = (int)(key >> 16);
        int s2 = STEREO_NO_SUM;          // the smallest sum at least two disparities away from d0, STEREO_NO_SUM while there is none
#pragma unroll
        for (int k = 0; k < STEREO_MAX_D / 64; ++k) {
            const int d = lane + 64 * k;
            if (d < D && (d < d0 - 1 || d > d0 + 1)) s2 = min(s2, v[k]);
        }
        s2 = wave_min(s2);
        if (lane != 0) continue;
        int f = 0;
        if (s2 != STEREO_NO_SUM && s2 * (100 - uniqueness) < s0 * 100) f |= 1;          // (both products stay below 2^23)
        const int x = (int)(p % W), xr = x - dmin - d0;
        bool ok = xr >= 0;
        if (ok) {
            const int dr = dR[p - dmin - d0];
            ok = dr >= 0 && abs(d0 - dr) <= lr_max;
        }
        if (!ok) f |= 2;
        double delta = 0.0;
        if (subpixel && d0 > 0 && d0 < D - 1) {
            const int a = s[d0 - 1], b = s[d0 + 1], den = a + b - 2 * s0;
            if (den > 0) delta = (double)(a - b) / (double)(2 * den);
        }
        const bool good = f == 0;
        d0_out[p] = good ? d0 : -1;
        disparity[p] = good ? (float)((double)(dmin + d0) + delta) : 0.f;
        flags[p] = (unsigned char)f;
        valid[p] = good;
    }
}

__global__ __launch_bounds__(256) void k_speckle_init(const unsigned char* __restrict__ valid, long long n_pix, int* __restrict__ label) {
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < n_pix; p += gridDim.x * 256ll) label[p] = valid[p] ? (int)p : -1;
}

__global__ __launch_bounds__(256) void k_speckle_sweep(const int* __restrict__ d0, long long n_pix, int H, int W, int range,
                                                       int* label, int* changed) {
    bool any = false;
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < n_pix; p += gridDim.x * 256ll) {
        const int mine = __atomic_load_n(label + p, __ATOMIC_RELAXED);
        if (mine < 0) continue;
        const int x = (int)(p % W), y = (int)((p / W) % H), d = d0[p];
        int best = mine;
        const long long nb[4] = {p - 1, p + 1, p - W, p + W};
        const bool in[4] = {x > 0, x + 1 < W, y > 0, y + 1 < H};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!in[k]) continue;
            const int other = __atomic_load_n(label + nb[k], __ATOMIC_RELAXED);
            const long long diff = (long long)d0[nb[k]] - d;          // (64 bits: d0 is any int32)
            if (other >= 0 && (diff < 0 ? -diff : diff) <= range) best = min(best, other);
        }
        // the pixel that ``best`` names is in this segment, so its label is too; a label is a pixel index of the same image, in range
        const int jump = __atomic_load_n(label + best, __ATOMIC_RELAXED);
        if (jump >= 0) best = min(best, jump);
        if (best < mine) {
            __atomic_store_n(label + p, best, __ATOMIC_RELAXED);
            any = true;
        }
    }
    if (changed && any) __atomic_store_n(changed, 1, __ATOMIC_RELAXED);
}

__global__ __launch_bounds__(256) void k_speckle_count(const int* __restrict__ label, long long n_pix, int* __restrict__ sizes) {
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < n_pix; p += gridDim.x * 256ll) {
        const int l = label[p];
        if (l >= 0) atomicAdd(sizes + l, 1);
    }
}

__global__ __launch_bounds__(256) void k_speckle_apply(const int* __restrict__ label, const int* __restrict__ sizes, long long n_pix,
                                                       int size, unsigned char* __restrict__ valid, int* __restrict__ d0,
                                                       float* __restrict__ disparity, unsigned char* __restrict__ flags) {
    for (long long p = blockIdx.x * 256ll + threadIdx.x; p < n_pix; p += gridDim.x * 256ll) {
        const int l = label[p];
        if (l < 0 || sizes[l] >= size) continue;
        valid[p] = 0;
        if (d0) d0[p] = -1;
        if (disparity) disparity[p] = 0.f;
        if (flags) flags[p] |= 4;
    }
}

static bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// the checks every entry shares: 0 to go on, 1 with the message set
static int stereo_shape(const char* who, int n, int H, int W, int D) {
    static thread_local char msg[160];
    snprintf(msg, sizeof msg, "%s: ", who);
    const size_t at = strlen(msg);
    auto bad = [&](const char* what) {
        snprintf(msg + at, sizeof msg - at, "%s", what);
        return fail(ST_BAD_ARG, msg, nullptr);
    };
    if (n < 0) return bad("n must not be negative");
    if (H < 1 || H > STEREO_MAX_SIZE || W < 1 || W > STEREO_MAX_SIZE) return bad("height and width must be in [1, 8192]");
    if (D < 1 || D > STEREO_MAX_D) return bad("max_disparity must be in [1, 256]");
    if (n > 0 && (long long)H * W * D > STEREO_MAX_INDEX / n) return bad("n, height, width, max_disparity: n H W D must stay below 2^31");
    return ST_OK;
}

struct SpeckleScratch {
    int *right, *label, *sizes;
    long long bytes;
    SpeckleScratch(const void* scratch, long long n_pix) : bytes(0) {
        Carver c(scratch);
        right = c.take<int>(n_pix);
        label = c.take<int>(n_pix);
        sizes = c.take<int>(n_pix);
        bytes = c.off;
    }
};

}  // namespace es

using namespace es;

extern "C" {

int64_t es_stereo_scratch_bytes(int n, int height, int width) {
    if (n <= 0 || height <= 0 || width <= 0) return 0;
    return SpeckleScratch(nullptr, (long long)n * height * width).bytes;
}

int es_stereo_census(const unsigned char* grey, int n, int height, int width, long long* census, void* stream) {
    if (int e = stereo_shape("es_stereo_census", n, height, width, 1)) return e;
    if (n == 0) return ST_OK;
    ES_REQUIRE(grey && census, "es_stereo_census: null buffer (grey, census)");
    ES_REQUIRE(aligned(census, 8), "es_stereo_census: census must be 8-byte aligned");
    const long long n_pix = (long long)n * height * width;
    hipLaunchKernelGGL(k_stereo_census, dim3(grid_for(n_pix)), dim3(256), 0, static_cast<hipStream_t>(stream), grey, n_pix, height, width,
                       census);
    return hip_last("es_stereo_census");
}

int es_sgm_cost(const long long* census_left, const long long* census_right, int n, int height, int width, int max_disparity,
                int min_disparity, unsigned char* cost, void* stream) {
    if (int e = stereo_shape("es_sgm_cost", n, height, width, max_disparity)) return e;
    ES_REQUIRE(min_disparity >= 0 && min_disparity <= STEREO_MAX_SIZE, "es_sgm_cost: min_disparity must be in [0, 8192]");
    if (n == 0) return ST_OK;
    ES_REQUIRE(census_left && census_right && cost, "es_sgm_cost: null buffer (census_left, census_right, cost)");
    ES_REQUIRE(aligned(census_left, 8) && aligned(census_right, 8), "es_sgm_cost: census_left and census_right must be 8-byte aligned");
    const long long total = (long long)n * height * width * max_disparity;
    hipLaunchKernelGGL(k_sgm_cost, dim3(grid_for(total)), dim3(256), 0, static_cast<hipStream_t>(stream), census_left, census_right, total,
                       width, max_disparity, min_disparity, cost);
    return hip_last("es_sgm_cost");
}

int es_sgm_aggregate(const unsigned char* cost, int n, int height, int width, int max_disparity, int p1, int p2, int paths,
                     unsigned short* sums, void* stream) {
    if (int e = stereo_shape("es_sgm_aggregate", n, height, width, max_disparity)) return e;
    ES_REQUIRE(0 <= p1 && p1 <= p2 && p2 <= STEREO_MAX_PENALTY, "es_sgm_aggregate: p1, p2 must satisfy 0 <= p1 <= p2 <= 1024");
    ES_REQUIRE(paths == 4 || paths == 8, "es_sgm_aggregate: paths must be 4 or 8");
    if (n == 0) return ST_OK;
    ES_REQUIRE(cost && sums, "es_sgm_aggregate: null buffer (cost, sums)");
    ES_REQUIRE(aligned(sums, 2), "es_sgm_aggregate: sums must be 2-byte aligned");
    const int kd = (max_disparity + 63) / 64;
    for (int dir = 0; dir < paths; ++dir) {
        const int lines = dir < 2 ? height : dir < 4 ? width : height + width - 1;
        const dim3 grid((unsigned)(((long long)n * lines + 3) / 4)), block(256);          // n lines <= n H W < 2^31
        const hipStream_t st = static_cast<hipStream_t>(stream);
        const int first = dir == 0;
        switch (kd) {
            case 1: hipLaunchKernelGGL(k_sgm_aggregate<1>, grid, block, 0, st, cost, sums, n, height, width, max_disparity, dir, lines, p1, p2, first); break;
            case 2: hipLaunchKernelGGL(k_sgm_aggregate<2>, grid, block, 0, st, cost, sums, n, height, width, max_disparity, dir, lines, p1, p2, first); break;
            case 3: hipLaunchKernelGGL(k_sgm_aggregate<3>, grid, block, 0, st, cost, sums, n, height, width, max_disparity, dir, lines, p1, p2, first); break;
            default: hipLaunchKernelGGL(k_sgm_aggregate<4>, grid, block, 0, st, cost, sums, n, height, width, max_disparity, dir, lines, p1, p2, first); break;
        }
        if (int e = hip_last("es_sgm_aggregate")) return e;
    }
    return ST_OK;
}

int es_sgm_select(const unsigned short* sums, int n, int height, int width, int max_disparity, int min_disparity, int uniqueness,
                  int lr_max, int subpixel, int* d0, float* disparity, unsigned char* flags, unsigned char* valid, void* scratch,
                  void* stream) {
    if (int e = stereo_shape("es_sgm_select", n, height, width, max_disparity)) return e;
    ES_REQUIRE(min_disparity >= 0 && min_disparity <= STEREO_MAX_SIZE, "es_sgm_select: min_disparity must be in [0, 8192]");
    ES_REQUIRE(uniqueness >= 0 && uniqueness <= 100, "es_sgm_select: uniqueness must be in [0, 100]");
    ES_REQUIRE(lr_max >= 0, "es_sgm_select: lr_max must not be negative");
    if (n == 0) return ST_OK;
    ES_REQUIRE(sums && d0 && disparity && flags && valid, "es_sgm_select: null buffer (sums, d0, disparity, flags, valid)");
    ES_REQUIRE(aligned(sums, 2) && aligned(d0, 4) && aligned(disparity, 4), "es_sgm_select: sums must be 2-byte, d0 and disparity 4-byte aligned");
    ES_SCRATCH_OK(scratch, "es_sgm_select: scratch");
    const long long n_pix = (long long)n * height * width;
    const SpeckleScratch sc(scratch, n_pix);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 waves(grid_for(n_pix, 4));          // one wavefront per pixel, four to a workgroup
    hipLaunchKernelGGL(k_sgm_right, waves, dim3(256), 0, st, sums, n_pix, width, max_disparity, min_disparity, sc.right);
    hipLaunchKernelGGL(k_sgm_select, waves, dim3(256), 0, st, sums, sc.right, n_pix, width, max_disparity, min_disparity,
                       uniqueness, lr_max, subpixel != 0, d0, disparity, flags, valid);
    return hip_last("es_sgm_select");
}

int es_speckle_label(const int* d0, const unsigned char* valid, int n, int height, int width, int speckle_range, int begin, void* scratch,
                     int* changed, void* stream) {
    if (int e = stereo_shape("es_speckle_label", n, height, width, 1)) return e;
    ES_REQUIRE(speckle_range >= 0, "es_speckle_label: speckle_range must not be negative");
    if (n == 0) return ST_OK;
    ES_REQUIRE(d0 && valid, "es_speckle_label: null buffer (d0, valid)");
    ES_REQUIRE(aligned(d0, 4) && aligned(changed, 4), "es_speckle_label: d0 and changed must be 4-byte aligned");
    ES_SCRATCH_OK(scratch, "es_speckle_label: scratch");
    const long long n_pix = (long long)n * height * width;
    const SpeckleScratch sc(scratch, n_pix);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (begin) hipLaunchKernelGGL(k_speckle_init, dim3(grid_for(n_pix)), dim3(256), 0, st, valid, n_pix, sc.label);
    if (changed) ES_HIP(hipMemsetAsync(changed, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_speckle_sweep, dim3(grid_for(n_pix)), dim3(256), 0, st, d0, n_pix, height, width, speckle_range, sc.label, changed);
    return hip_last("es_speckle_label");
}

int es_speckle_apply(int n, int height, int width, int speckle_size, void* scratch, unsigned char* valid, int* d0, float* disparity,
                     unsigned char* flags, void* stream) {
    if (int e = stereo_shape("es_speckle_apply", n, height, width, 1)) return e;
    ES_REQUIRE(speckle_size >= 0, "es_speckle_apply: speckle_size must not be negative");
    if (n == 0) return ST_OK;
    ES_REQUIRE(valid, "es_speckle_apply: null buffer (valid)");
    ES_REQUIRE(aligned(d0, 4) && aligned(disparity, 4), "es_speckle_apply: d0 and disparity must be 4-byte aligned");
    ES_SCRATCH_OK(scratch, "es_speckle_apply: scratch");
    const long long n_pix = (long long)n * height * width;
    const SpeckleScratch sc(scratch, n_pix);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    ES_HIP(hipMemsetAsync(sc.sizes, 0, sizeof(int) * (size_t)n_pix, st));
    hipLaunchKernelGGL(k_speckle_count, dim3(grid_for(n_pix)), dim3(256), 0, st, sc.label, n_pix, sc.sizes);
    hipLaunchKernelGGL(k_speckle_apply, dim3(grid_for(n_pix)), dim3(256), 0, st, sc.label, sc.sizes, n_pix, speckle_size, valid, d0,
                       disparity, flags);
    return hip_last("es_speckle_apply");
}

}  // extern "C"
