// Integer scans shared by iso.hip, band.hip, mesh.hip and raster.hip (256 threads = 4 wavefronts of 64): the in-workgroup pieces, and
// the exclusive scan of two sequences over any number of items in three launches,
//   k_scan_blocksum   per chunk of SCAN_CHUNK items: the sums of both sequences
//   k_scan_blocks     exclusive scan of the chunk sums (one workgroup), totals
//   k_scan_offsets    per chunk: exclusive scan + chunk offset -> each thread's sums in front of its items, for the client's store
// as templates over a client's *source*, a small struct passed to the kernels by value:
//   using sum_t (int: a chunk's sums fit 32 bits, or long long), items_t (a thread's SCAN_PER_THREAD consecutive items, in registers)
//   __device__ void load(long long i0, items_t& c, sum_t& a, sum_t& b) const        items i0 .. i0 + 15 (neutral beyond the end) and the
//                                                                                   sums of their terms of the two sequences
//   __device__ void store(long long i0, const items_t& c, sum_t a, sum_t b) const   a, b: the sums in front of item i0; walks the items,
//                                                                                   writes what the client keeps, range-checks every write
// No atomics, no hand-off between workgroups inside a launch, no loop without a bound: the results are bit-identical from call to call.
#pragma once
#include <hip/hip_runtime.h>

namespace es {

constexpr int SCAN_PER_THREAD = 16;                          // consecutive items of one thread
constexpr int SCAN_CHUNK = 256 * SCAN_PER_THREAD;            // items per workgroup
inline long long scan_chunks(long long n) { return (n + SCAN_CHUNK - 1) / SCAN_CHUNK; }

// inclusive scan across the 64 lanes (rays.hip wscan_add, for integers)
template <class T>
__device__ __forceinline__ T wscan_add(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
    return v;
}
// exclusive scan of (a, b) over the 256 threads of a workgroup; ``total`` receives the workgroup's sums
template <class T>
__device__ __forceinline__ void block_scan2(T& a, T& b, T (&part)[4][2], T (&total)[2]) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const T ia = wscan_add(a, lane), ib = wscan_add(b, lane);
    if (lane == 63) { part[wv][0] = ia; part[wv][1] = ib; }
    __syncthreads();
    T oa = 0, ob = 0, ta = 0, tb = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wv) { oa += part[w][0]; ob += part[w][1]; }
        ta += part[w][0]; tb += part[w][1];
    }
    a = oa + ia - a; b = ob + ib - b;
    total[0] = ta; total[1] = tb;
    __syncthreads();
}

// this thread's items of its workgroup's chunk -> c, and the exclusive scan of their sums over the workgroup -> (a, b)
template <class Src>
__device__ __forceinline__ long long scan_chunk(const Src& src, typename Src::items_t& c, typename Src::sum_t& a, typename Src::sum_t& b,
                                                typename Src::sum_t (&total)[2]) {
    using T = typename Src::sum_t;
    __shared__ T part[4][2];
    const long long i0 = (long long)blockIdx.x * SCAN_CHUNK + threadIdx.x * SCAN_PER_THREAD;
    src.load(i0, c, a, b);
    block_scan2(a, b, part, total);
    return i0;
}

template <class Src>
__global__ __launch_bounds__(256) void k_scan_blocksum(Src src, typename Src::sum_t* __restrict__ bsum) {
    typename Src::items_t c;
    typename Src::sum_t a, b, total[2];
    scan_chunk(src, c, a, b, total);
    if (threadIdx.x == 0) { bsum[2 * (size_t)blockIdx.x] = total[0]; bsum[2 * (size_t)blockIdx.x + 1] = total[1]; }
}

// One workgroup: thread i owns a contiguous run of chunks.  Offsets are kept in 64 bits (the totals may exceed the range of T: the
// caller must look at them before it emits) and stored truncated.  ``totals`` may be null.
template <class T>
__global__ __launch_bounds__(256) void k_scan_blocks(const T* __restrict__ bsum, long long nchunk, T* __restrict__ boff, long long* __restrict__ totals) {
    __shared__ long long part[4][2];
    const long long per = (nchunk + 255) / 256, c0 = threadIdx.x * per, c1 = c0 + per < nchunk ? c0 + per : nchunk;
    long long sa = 0, sb = 0;
    for (long long c = c0; c < c1; ++c) { sa += bsum[2 * c]; sb += bsum[2 * c + 1]; }
    long long total[2];
    block_scan2(sa, sb, part, total);
    for (long long c = c0; c < c1; ++c) {
        boff[2 * c] = (T)sa; boff[2 * c + 1] = (T)sb;
        sa += bsum[2 * c]; sb += bsum[2 * c + 1];
    }
    if (threadIdx.x == 0 && totals) { totals[0] = total[0]; totals[1] = total[1]; }
}

template <class Src>
__global__ __launch_bounds__(256) void k_scan_offsets(Src src, const typename Src::sum_t* __restrict__ boff) {
    using T = typename Src::sum_t;
    typename Src::items_t c;
    T a, b, total[2];
    const long long i0 = scan_chunk(src, c, a, b, total);
    src.store(i0, c, a + boff[2 * (size_t)blockIdx.x], b + boff[2 * (size_t)blockIdx.x + 1]);
}

// the three launches over ``nchunk`` chunks; bsum and boff are [nchunk][2]
template <class Src>
inline void scan_launch(const Src& src, long long nchunk, typename Src::sum_t* bsum, typename Src::sum_t* boff, long long* totals, hipStream_t st) {
    hipLaunchKernelGGL(k_scan_blocksum<Src>, dim3((unsigned)nchunk), dim3(256), 0, st, src, bsum);
    hipLaunchKernelGGL(k_scan_blocks<typename Src::sum_t>, dim3(1), dim3(256), 0, st, bsum, nchunk, boff, totals);
    hipLaunchKernelGGL(k_scan_offsets<Src>, dim3((unsigned)nchunk), dim3(256), 0, st, src, boff);
}

}  // namespace es
