// Workgroup scans shared by the compaction kernels of iso.hip and band.hip (256 threads = 4 wavefronts of 64).
#pragma once
#include <hip/hip_runtime.h>

namespace es {

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

}  // namespace es
