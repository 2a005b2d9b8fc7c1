// What the two KITTI augmentation kernels (pwc_augment.hip, pwc_augment_full.hip) share: the kernel arguments and the host entry
// that checks and fills them, the record's geometry check, the per-sample sources, border folding, OpenCV's saturating
// double -> int rounding, the per-tap ground-truth decode and the nine-plane store.  Definitions: include/pwc_hip.h.
#pragma once
#include "pwc_common.h"

namespace pwc_aug {

constexpr int kTH = 8, kTW = 128, kPix = 4, kThreads = 256;
constexpr int kLanesX = kTW / kPix;            // 32 lanes across a tile row
static_assert(kLanesX * kTH == kThreads, "augment tile");

// kernel arguments, by value; P = the parameter record of the entry
template <typename P>
struct Args {
    const uint8_t *frames;
    const void *gt;
    const uint8_t *valid;
    const P *params;
    float *x, *flow, *vout;
    int *status;
    int Hs, Ws, crop_h, crop_w, gt_kind;
};

// the checks both records share: the sample fits its slot, the crop fits the sample, the origin keeps the window inside it
template <typename P>
__device__ __forceinline__ bool bad_geometry(const P &p, int Hs, int Ws, int ch, int cw) {
    const int H = p.h, W = p.w;
    return H < 1 || H > Hs || W < 1 || W > Ws || ch > H || cw > W || p.y0 < 0 || p.y0 > H - ch || p.x0 < 0 || p.x0 > W - cw;
}

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

// what a sample is read from: its two frames and its ground truth, each at the start of the sample's slot
struct Src {
    const uint8_t *f1, *f2;
    Gt g;
};

template <typename P>
__device__ __forceinline__ void set_sources(Src &S, const Args<P> &a, int b) {
    const int64_t slot = (int64_t)a.Hs * a.Ws;
    S.f1 = a.frames + (int64_t)b * 2 * slot * 3;
    S.f2 = S.f1 + slot * 3;
    S.g.png = a.gt_kind == 1 ? static_cast<const uint16_t *>(a.gt) + (int64_t)b * slot * 3 : nullptr;
    S.g.fu = static_cast<const float *>(a.gt) + (int64_t)b * 2 * slot;
    S.g.fv = S.g.fu + slot;
    S.g.valid = a.valid ? a.valid + (int64_t)b * slot : nullptr;
}

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

// the lane's kPix pixels of row y of sample b: six image planes, two flow planes, the mask
template <bool VEC>
__device__ __forceinline__ void store_planes(float *x, float *flow, float *vout, int crop_h, int crop_w, int b, int y, int x0,
                                             const float (&out)[9][kPix]) {
    const int64_t plane = (int64_t)crop_h * crop_w, row = (int64_t)y * crop_w;
#pragma unroll
    for (int c = 0; c < 6; ++c) store_row<VEC>(x + ((int64_t)b * 6 + c) * plane + row, x0, crop_w, out[c]);
    store_row<VEC>(flow + ((int64_t)b * 2) * plane + row, x0, crop_w, out[6]);
    store_row<VEC>(flow + ((int64_t)b * 2 + 1) * plane + row, x0, crop_w, out[7]);
    store_row<VEC>(vout + (int64_t)b * plane + row, x0, crop_w, out[8]);
}

// The body of both extern "C" entries (one signature, include/pwc_hip.h): every argument check, then one launch of `vec` (16-byte
// stores) or `scalar` (guarded 4-byte stores).  `entry` names the entry in the messages, `kernel` the launch in check_launch.
template <typename P>
int launch(const char *entry, const char *kernel, void (*vec)(Args<P>), void (*scalar)(Args<P>), const void *frames, const void *gt,
           int gt_kind, const void *valid, int n, int Hs, int Ws, int crop_h, int crop_w, const void *params, void *x, void *flow,
           void *vout, void *status, void *stream) {
    if (!frames || !gt || !params || !x || !flow || !vout || !status) PWC_FAIL(PWC_EINVAL, "%s: null pointer", entry);
    if (n <= 0 || Hs <= 0 || Ws <= 0 || crop_h <= 0 || crop_w <= 0)
        PWC_FAIL(PWC_EINVAL, "%s: bad shape n=%d slot=%dx%d crop=%dx%d", entry, n, Hs, Ws, crop_h, crop_w);
    if (n > 65535 || Hs > 32767 || Ws > 32767) PWC_FAIL(PWC_EINVAL, "%s: needs n <= 65535 and a slot of at most 32767 x 32767", entry);
    if (crop_h > Hs || crop_w > Ws) PWC_FAIL(PWC_EINVAL, "%s: crop %dx%d larger than the slot %dx%d", entry, crop_h, crop_w, Hs, Ws);
    if (gt_kind != 0 && gt_kind != 1) PWC_FAIL(PWC_EINVAL, "%s: unknown gt_kind %d (0 = float planes, 1 = uint16 PNG samples)", entry, gt_kind);
    if (gt_kind == 1 && valid) PWC_FAIL(PWC_EINVAL, "%s: gt_kind 1 carries its own validity, valid must be NULL", entry);
    if (pwc::misaligned({x, flow, vout, status}) || pwc::misaligned({gt}, gt_kind == 1 ? 2 : 4))
        PWC_FAIL(PWC_EALIGN, "%s: float / int32 pointers must be 4-byte aligned, a uint16 gt 2-byte aligned", entry);
    if (pwc::misaligned({params}, 8)) PWC_FAIL(PWC_EALIGN, "%s: the parameter buffer must be 8-byte aligned", entry);
    Args<P> a;
    a.frames = static_cast<const uint8_t *>(frames);
    a.gt = gt;
    a.valid = static_cast<const uint8_t *>(valid);
    a.params = static_cast<const P *>(params);
    a.x = static_cast<float *>(x);
    a.flow = static_cast<float *>(flow);
    a.vout = static_cast<float *>(vout);
    a.status = static_cast<int *>(status);
    a.Hs = Hs; a.Ws = Ws; a.crop_h = crop_h; a.crop_w = crop_w; a.gt_kind = gt_kind;
    const dim3 grid((crop_w + kTW - 1) / kTW, (crop_h + kTH - 1) / kTH, n);
    const bool wide = crop_w % kPix == 0 && !pwc::misaligned({x, flow, vout}, 16);
    hipLaunchKernelGGL(wide ? vec : scalar, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return pwc::check_launch(kernel);
}

}  // namespace pwc_aug
