// Largest |v| of a float tensor as float bits, the prepass of the deterministic (fixed-point) backward scatters (pwc_warp.hip,
// pwc_warp_corr_bwd.hip).  The bit pattern of |v| orders like the value for finite numbers and puts +inf (0x7f800000) and every
// NaN above them, so a result >= kAbsmaxNonFinite says the tensor has no fixed-point form.
#pragma once
#include "pwc_common.h"

namespace pwc {
namespace {

constexpr unsigned kAbsmaxNonFinite = 0x7f800000u;

// B images of n elements, batch stride bs; grid.x = B * per_img workgroups (the batch folded into x: any B).  Each workgroup reduces
// its share through LDS and adds ONE atomicMax to *out (zeroed before): adds to one address serialise at the memory side, so the
// launcher keeps the grid near 128 workgroups.
__global__ void __launch_bounds__(256)
absmax_bits_kernel(const float *__restrict__ v, int64_t n, int64_t bs, int per_img, unsigned *out) {
    __shared__ unsigned wmax[4];
    const int img = blockIdx.x / per_img, part = blockIdx.x - img * per_img;
    const float *vb = v + (int64_t)img * bs;
    unsigned m = 0;
    const int64_t n4 = (reinterpret_cast<uintptr_t>(vb) & 15u) ? 0 : n / 4;     // float4 body when 16-byte aligned
    for (int64_t i = (int64_t)part * 256 + threadIdx.x; i < n4; i += (int64_t)per_img * 256) {
        const float4 q = reinterpret_cast<const float4 *>(vb)[i];
        m = max(max(m, max(__float_as_uint(fabsf(q.x)), __float_as_uint(fabsf(q.y)))),
                max(__float_as_uint(fabsf(q.z)), __float_as_uint(fabsf(q.w))));
    }
    for (int64_t i = n4 * 4 + (int64_t)part * 256 + threadIdx.x; i < n; i += (int64_t)per_img * 256)
        m = max(m, __float_as_uint(fabsf(vb[i])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        if (m) atomicMax(out, m);
    }
}

// max |v| over B images of n elements (batch stride bs, elements) into *out, which must be zero before (async, on st)
void launch_absmax_bits(const float *v, int64_t n, int64_t bs, int B, unsigned *out, hipStream_t st) {
    const int64_t need = (n / 4 + 255) / 256 + 1;
    const int64_t share = (128 + (int64_t)B - 1) / B;
    const int64_t per_img = need < share ? need : share;
    hipLaunchKernelGGL(absmax_bits_kernel, dim3((unsigned)(per_img * B)), dim3(256), 0, st, v, n, bs, (int)per_img, out);
}

}  // namespace
}  // namespace pwc
