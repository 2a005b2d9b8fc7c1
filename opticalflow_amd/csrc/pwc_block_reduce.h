// Workgroup sums of the loss and metric operators, and the record their tile partials are kept in.  Two summation orders exist and
// each kernel keeps its own, because the order of the fp64 additions is what makes a result bit-reproducible:
//   tree_sum       every lane's value through LDS, halving tree over the lane index (proxy loss, supervised losses, fb metrics,
//                  KITTI score)
//   wave_block_sum xor tree inside each wave, then the waves in ascending order (epipolar refit, threshold and loss)
// Integer sums are order-free; they ride along in whichever form the kernel uses.
// wave_block_max is the maximum of one float per lane (flow statistics); a maximum has no order to keep.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace pwc {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// LDS of tree_sum for a workgroup of NT lanes with ND doubles and NI 64-bit counts per lane; the caller declares it __shared__
template <int NT, int ND, int NI = 0> struct TreeLds { double d[ND][NT]; long long n[NI][NT]; };
template <int NT, int ND> struct TreeLds<NT, ND, 0> { double d[ND][NT]; };
template <int NT, int NI> struct TreeLds<NT, 0, NI> { long long n[NI][NT]; };

// fixed-order workgroup sum of d[0..ND) and n[0..NI) (pass nullptr for the absent kind): x[tid] += x[tid + s] for s = NT/2 .. 1.
// The result is in every lane, and the closing barrier leaves lds free for the next call.
template <int NT, int ND, int NI>
__device__ __forceinline__ void tree_sum(TreeLds<NT, ND, NI> &lds, double *d, long long *n) {
    const int tid = threadIdx.x;
    if constexpr (ND > 0) {
#pragma unroll
        for (int k = 0; k < ND; ++k) lds.d[k][tid] = d[k];
    }
    if constexpr (NI > 0) {
#pragma unroll
        for (int k = 0; k < NI; ++k) lds.n[k][tid] = n[k];
    }
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            if constexpr (ND > 0) {
#pragma unroll
                for (int k = 0; k < ND; ++k) lds.d[k][tid] += lds.d[k][tid + s];
            }
            if constexpr (NI > 0) {
#pragma unroll
                for (int k = 0; k < NI; ++k) lds.n[k][tid] += lds.n[k][tid + s];
            }
        }
        __syncthreads();
    }
    if constexpr (ND > 0) {
#pragma unroll
        for (int k = 0; k < ND; ++k) d[k] = lds.d[k][0];
    }
    if constexpr (NI > 0) {
#pragma unroll
        for (int k = 0; k < NI; ++k) n[k] = lds.n[k][0];
    }
    __syncthreads();
}

// LDS of wave_block_sum for a workgroup of NT lanes: up to KMAX values of T (double or a 64-bit count) per wave
template <typename T, int NT, int KMAX = 1> struct WaveLds { T v[(NT / 64) * KMAX]; };

// per wave xor tree, then the waves in ascending order, of K values per lane; the result is in every lane.  The opening barrier
// lets lds be used again right after an earlier call.
template <typename T, int NT, int KMAX, int K>
__device__ __forceinline__ void wave_block_sum(WaveLds<T, NT, KMAX> &lds, T (&v)[K]) {
    static_assert(K <= KMAX, "WaveLds too small");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) lds.v[wv * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        T s = lds.v[k];
        for (int o = 1; o < NT / 64; ++o) s += lds.v[o * K + k];
        v[k] = s;
    }
}

// workgroup maximum of one float per lane (flow statistics): xor tree inside each wave, then the waves through lds.  A maximum of
// ordinary numbers does not depend on the order, so no order is promised; the result is in every lane.  Barriers as wave_block_sum.
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

template <int NT>
__device__ __forceinline__ float wave_block_max(WaveLds<float, NT, 1> &lds, float v) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) lds.v[wv] = v;
    __syncthreads();
    float m = lds.v[0];
    for (int o = 1; o < NT / 64; ++o) m = fmaxf(m, lds.v[o]);
    return m;
}

// what a tile workgroup leaves in the workspace, and what the finish kernel puts in the workspace head
template <int N> struct TilePartial {
    double sum;
    long long count[N];
};
static_assert(sizeof(TilePartial<1>) == 16 && offsetof(TilePartial<1>, count) == 8, "fb metrics workspace layout");
static_assert(sizeof(TilePartial<2>) == 24 && offsetof(TilePartial<2>, count) == 8, "KITTI score workspace layout");

}  // namespace pwc
