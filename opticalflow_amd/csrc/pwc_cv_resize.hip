// cv2.resize-exact (INTER_LINEAR) resize on the device (opticalflow_amd/cv_resize.py): the image-space steps of script_pwc.py:43-83 and
// topview.py:79-119 (compute_flow) -- both frames resized to multiples of 64, channel order flipped, / 255, HWC -> CHW, stacked; and the
// network's quarter-resolution flow times a gain, resized to the image, u and v rescaled.  The arithmetic is the statement of OpenCV's
// published algorithm in opticalflow_amd/harness.py (pinned by tests/test_harness.py; cv2 parity unpinned):
//   geometry, per axis, made on the HOST (cv_resize.axis_table): first tap s0 (int32) and fractional weight f (float32) per output index;
//            the second tap is min(s0 + 1, I - 1).  The kernels clamp s0 into [0, I), so no table content makes a tap leave the image.
//   frames : a0 = rint((1.f - fx) * 2048), a1 = rint(fx * 2048) (half to even, each on its own), D = S[s0] * a0 + S[s1] * a1 in int32,
//            byte = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2, out = lut[c_out][byte].  Equal sizes need no branch:
//            weight 2048 is exact on bytes.
//   flow   : t = src * gain; row = t[s0] * (1.f - fx) + t[s1] * fx; val = row[y0] * (1.f - fy) + row[y1] * fy; dst = val * (fu | fv), every
//            product and sum rounded to float32 (-ffp-contract=off).  Equal sizes: cv2 copies, dst = (src * gain) * f, so -0.0, inf and NaN
//            stay where they are (the weights 1 and 0 would make +0.0 of -0.0 and NaN of an inf's neighbour).
// Work decomposition: a direct four-tap gather.  One thread owns four consecutive outputs of one row (all three channels of a frame,
// both channels of a flow) and ends with 16-byte stores, one per plane.  Neither resize has reuse worth staging: the frames are
// stretched by at most 64 / 63 per axis at the sizes the scripts use, so a source byte feeds one or two outputs, and the flow's source
// is a sixteenth of its output and stays in cache.  The byte table lives in LDS (768 floats per workgroup).
#include <stdint.h>

#include "pwc_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxDim = 1 << 20;

struct Tap {
    int s0, s1;
    float f;
};

// one row of an axis table as the kernels use it: whatever the table holds, both taps are inside [0, in)
__device__ __forceinline__ Tap load_tap(const int32_t *__restrict__ s0, const float *__restrict__ f, int i, int in) {
    Tap t;
    t.s0 = min(max(s0[i], 0), in - 1);
    t.s1 = min(t.s0 + 1, in - 1);
    t.f = f[i];
    return t;
}

// cvRound(w * 2048): round half to even (v_rndne_f32); the product by a power of two is exact
__device__ __forceinline__ int coef11(float w) { return (int)rintf(w * 2048.f); }

__global__ void __launch_bounds__(256)
cv_frames_kernel(const uint8_t *__restrict__ src, float *__restrict__ out, int H, int W, int h, int w, const int32_t *__restrict__ xs0,
                 const float *__restrict__ xfx, const int32_t *__restrict__ ys0, const float *__restrict__ yfy,
                 const float *__restrict__ lut, int flip, int64_t bso, int group, int vec, int qpr) {
    __shared__ float s_lut[768];
    for (int i = threadIdx.x; i < 768; i += 256) s_lut[i] = lut[i];
    __syncthreads();

    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;      // quad of this frame: (row, four columns)
    if (q >= (int64_t)h * qpr) return;
    const int y = (int)(q / qpr), x = 4 * (int)(q - (int64_t)y * qpr);
    const int f = blockIdx.y;

    const Tap ty = load_tap(ys0, yfy, y, H);
    const int b0 = coef11(1.f - ty.f), b1 = coef11(ty.f);
    const uint8_t *img = src + (int64_t)f * H * W * 3;
    const uint8_t *r0 = img + (int64_t)ty.s0 * W * 3, *r1 = img + (int64_t)ty.s1 * W * 3;

    float v[3][4];
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        const Tap tx = load_tap(xs0, xfx, min(x + px, w - 1), W);
        const int a0 = coef11(1.f - tx.f), a1 = coef11(tx.f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int d0 = (int)r0[3 * tx.s0 + c] * a0 + (int)r0[3 * tx.s1 + c] * a1;
            const int d1 = (int)r1[3 * tx.s0 + c] * a0 + (int)r1[3 * tx.s1 + c] * a1;
            const int byte = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
            const int co = flip ? 2 - c : c;
            v[co][px] = s_lut[co * 256 + min(max(byte, 0), 255)];
        }
    }

    const int64_t plane = (int64_t)h * w;
    float *o = out + (int64_t)(f % group) * bso + (int64_t)(f / group) * 3 * plane + (int64_t)y * w + x;
    if (vec) {                                   // w % 4 == 0 and every plane row 16-byte aligned: the quad is whole
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4 *>(o + c * plane) = (f32x4){v[c][0], v[c][1], v[c][2], v[c][3]};
    } else {
#pragma unroll
        for (int px = 0; px < 4; ++px)
            if (x + px < w) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c * plane + px] = v[c][px];
            }
    }
}

// kCopy: both sizes are equal, cv2 copies.  Compile-time, so the resampling instantiation carries no branch for it.
template <bool kCopy>
__global__ void __launch_bounds__(256)
cv_flow_kernel(const float *__restrict__ src, float *__restrict__ dst, int ih, int iw, int oh, int ow, const int32_t *__restrict__ xs0,
               const float *__restrict__ xfx, const int32_t *__restrict__ ys0, const float *__restrict__ yfy, float gain, float fu,
               float fv, int hwc, int64_t bss, int vec, int qpr) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)oh * qpr) return;
    const int y = (int)(q / qpr), x = 4 * (int)(q - (int64_t)y * qpr);
    const int n = blockIdx.y;
    const float *img = src + (int64_t)n * bss;
    const int64_t iplane = (int64_t)ih * iw, oplane = (int64_t)oh * ow;

    float v[2][4];
    if (kCopy) {
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const int64_t at = (int64_t)y * iw + min(x + px, ow - 1);
            v[0][px] = (img[at] * gain) * fu;
            v[1][px] = (img[iplane + at] * gain) * fv;
        }
    } else {
        const Tap ty = load_tap(ys0, yfy, y, ih);
        const float wy0 = 1.f - ty.f, wy1 = ty.f;
        const float *r0 = img + (int64_t)ty.s0 * iw, *r1 = img + (int64_t)ty.s1 * iw;
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const Tap tx = load_tap(xs0, xfx, min(x + px, ow - 1), iw);
            const float wx0 = 1.f - tx.f, wx1 = tx.f;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float *p0 = r0 + c * iplane, *p1 = r1 + c * iplane;
                const float top = (p0[tx.s0] * gain) * wx0 + (p0[tx.s1] * gain) * wx1;
                const float bot = (p1[tx.s0] * gain) * wx0 + (p1[tx.s1] * gain) * wx1;
                v[c][px] = (top * wy0 + bot * wy1) * (c ? fv : fu);
            }
        }
    }

    if (hwc) {
        float *o = dst + ((int64_t)n * oplane + (int64_t)y * ow + x) * 2;
        if (vec) {                               // ow % 4 == 0 and dst 16-byte aligned: eight whole floats, 32-byte aligned
            *reinterpret_cast<f32x4 *>(o) = (f32x4){v[0][0], v[1][0], v[0][1], v[1][1]};
            *reinterpret_cast<f32x4 *>(o + 4) = (f32x4){v[0][2], v[1][2], v[0][3], v[1][3]};
        } else {
#pragma unroll
            for (int px = 0; px < 4; ++px)
                if (x + px < ow) {
                    o[2 * px] = v[0][px];
                    o[2 * px + 1] = v[1][px];
                }
        }
    } else {
        float *o = dst + (int64_t)n * 2 * oplane + (int64_t)y * ow + x;
        if (vec) {
            *reinterpret_cast<f32x4 *>(o) = (f32x4){v[0][0], v[0][1], v[0][2], v[0][3]};
            *reinterpret_cast<f32x4 *>(o + oplane) = (f32x4){v[1][0], v[1][1], v[1][2], v[1][3]};
        } else {
#pragma unroll
            for (int px = 0; px < 4; ++px)
                if (x + px < ow) {
                    o[px] = v[0][px];
                    o[oplane + px] = v[1][px];
                }
        }
    }
}

bool bad_dim(int v) { return v <= 0 || v > kMaxDim; }

}  // namespace

extern "C" int pwc_cv_resize_frames_u8(const void *frames_u8, void *out_f32, int n, int H, int W, int h, int w, const int32_t *xs0,
                                       const float *xfx, const int32_t *ys0, const float *yfy, const float *lut768, int flip_channels,
                                       int64_t out_bstride, int out_group, void *stream) {
    if (!frames_u8 || !out_f32 || !xs0 || !xfx || !ys0 || !yfy || !lut768) PWC_FAIL(PWC_EINVAL, "pwc_cv_resize_frames_u8: null pointer");
    if (n <= 0 || bad_dim(H) || bad_dim(W) || bad_dim(h) || bad_dim(w) || out_group <= 0)
        PWC_FAIL(PWC_EINVAL, "pwc_cv_resize_frames_u8: bad shape (sizes must be in 1..2^20, n and out_group positive)");
    const int halves = (n + out_group - 1) / out_group;
    if (out_bstride < (int64_t)3 * halves * h * w) PWC_FAIL(PWC_EINVAL, "pwc_cv_resize_frames_u8: batch stride smaller than the tensor");
    if (n > 65535) PWC_FAIL(PWC_EINVAL, "pwc_cv_resize_frames_u8: grid too large (n > 65535)");
    if (pwc::misaligned({out_f32, xs0, xfx, ys0, yfy, lut768}))
        PWC_FAIL(PWC_EALIGN, "pwc_cv_resize_frames_u8: out / tables must be 4-byte aligned");
    const int qpr = (w + 3) / 4;
    const int64_t blocks = ((int64_t)h * qpr + 255) / 256;
    if (blocks > 0x7fffffff) PWC_FAIL(PWC_EINVAL, "pwc_cv_resize_frames_u8: grid too large");
    const int vec = (w % 4 == 0) && pwc::aligned16(out_f32) && (out_bstride % 4 == 0);
    hipLaunchKernelGGL(cv_frames_kernel, dim3((unsigned)blocks, n), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t *>(frames_u8), static_cast<float *>(out_f32), H, W, h, w, xs0, xfx, ys0, yfy, lut768,
                       flip_channels ? 1 : 0, out_bstride, out_group, vec, qpr);
    return pwc::check_launch("cv_frames_kernel");
}

extern "C" int pwc_cv_resize_flow_f32(const void *src, void *dst, int n, int in_h, int in_w, int out_h, int out_w, const int32_t *xs0,
                                      const float *xfx, const int32_t *ys0, const float *yfy, float gain, float fu, float fv, int hwc,
                                      int64_t src_bstride, void *stream) {
    if (!src || !dst || !xs0 || !xfx || !ys0 || !yfy) PWC_FAIL(PWC_EINVAL, "pwc_cv_resize_flow_f32: null pointer");
    if (n <= 0 || bad_dim(in_h) || bad_dim(in_w) || bad_dim(out_h) || bad_dim(out_w))
        PWC_FAIL(PWC_EINVAL, "pwc_cv_resize_flow_f32: bad shape (sizes must be in 1..2^20, n positive)");
    if (src_bstride < (int64_t)2 * in_h * in_w) PWC_FAIL(PWC_EINVAL, "pwc_cv_resize_flow_f32: batch stride smaller than the tensor");
    if (n > 65535) PWC_FAIL(PWC_EINVAL, "pwc_cv_resize_flow_f32: grid too large (n > 65535)");
    if (pwc::misaligned({src, dst, xs0, xfx, ys0, yfy}))
        PWC_FAIL(PWC_EALIGN, "pwc_cv_resize_flow_f32: src / dst / tables must be 4-byte aligned");
    const int qpr = (out_w + 3) / 4;
    const int64_t blocks = ((int64_t)out_h * qpr + 255) / 256;
    if (blocks > 0x7fffffff) PWC_FAIL(PWC_EINVAL, "pwc_cv_resize_flow_f32: grid too large");
    const int vec = (out_w % 4 == 0) && pwc::aligned16(dst);
    const bool copy = in_h == out_h && in_w == out_w;
    hipLaunchKernelGGL(copy ? cv_flow_kernel<true> : cv_flow_kernel<false>, dim3((unsigned)blocks, n), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<const float *>(src), static_cast<float *>(dst), in_h, in_w, out_h,
                       out_w, xs0, xfx, ys0, yfy, gain, fu, fv, hwc ? 1 : 0, src_bstride, vec, qpr);
    return pwc::check_launch("cv_flow_kernel");
}
