// Helpers shared by the two KITTI augmentation kernels (pwc_augment.hip, pwc_augment_full.hip): border folding, OpenCV's
// saturating double -> int rounding, the per-tap ground-truth decode and the row store.  Definitions: include/pwc_hip.h.
#pragma once
#include "pwc_common.h"

namespace pwc_aug {

constexpr int kTH = 8, kTW = 128, kPix = 4, kThreads = 256;
constexpr int kLanesX = kTW / kPix;            // 32 lanes across a tile row
static_assert(kLanesX * kTH == kThreads, "augment tile");

// BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba) for any p: period 2(len-1), len == 1 -> 0
__device__ __forceinline__ int reflect101(int p, int len) {
    if (len == 1) return 0;
    const int period = 2 * (len - 1);
    int m = p % period;
    if (m < 0) m += period;
    return m < len ? m : period - m;
}

// BORDER_REFLECT (fedcba|abcdefgh|hgfedcb) for any p: period 2 len
__device__ __forceinline__ int reflect_edge(int p, int len) {
    const int period = 2 * len;
    int m = p % period;
    if (m < 0) m += period;
    return m < len ? m : period - 1 - m;
}

// saturate_cast<int>(double): round half to even; out-of-range values saturate and NaN becomes INT_MIN (never undefined)
__device__ __forceinline__ int round_i32(double v) {
    return (int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0);
}

__device__ __forceinline__ int wrap_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }

// ground truth of one sample: (u, v, valid) at element `o` of the sample's slot
struct Gt {
    const float *fu, *fv;
    const uint8_t *valid;
    const uint16_t *png;
    __device__ __forceinline__ void tap(int o, float &u, float &v, float &m) const {
        if (png) {
            const uint16_t *p = png + 3 * (int64_t)o;
            u = ((float)p[0] - 32768.0f) / 64.0f;
            v = ((float)p[1] - 32768.0f) / 64.0f;
            m = p[2] != 0 ? 1.0f : 0.0f;
        } else {
            u = fu[o];
            v = fv[o];
            m = (!valid || valid[o] != 0) ? 1.0f : 0.0f;
        }
    }
};

template <bool VEC>
__device__ __forceinline__ void store_row(float *__restrict__ row, int x0, int crop_w, const float (&v)[kPix]) {
    if (VEC) {
        *reinterpret_cast<float4 *>(row + x0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k)
            if (x0 + k < crop_w) row[x0 + k] = v[k];
    }
}

}  // namespace pwc_aug
