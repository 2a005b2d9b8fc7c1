// KITTI training batches on the device: the reduced augmentation (cv2.warpAffine of both frames, the flow planes and the valid mask,
// then the linear part applied to the flow vectors), the random crop and the horizontal flip of KittiFlowDataset
// (data_processing_or.py:228-294) in one launch, from the raw uint8 frames and the ground truth.  Only the crop window is computed; the
// arithmetic is spelled out in include/pwc_hip.h and restated in tests/augment_oracle.py, and the two agree bit for bit.
//
// One workgroup = one 8 x 128 tile of one sample's window, 256 lanes; a lane produces kPix = 4 consecutive x' of one row, so that each
// of the nine output planes gets one 16-byte store per lane (a wave writes two 512-byte row pieces) when the window's width is a
// multiple of 4 and the outputs are 16-byte aligned, and guarded 4-byte stores otherwise (the ragged right edge included).  A flipped
// sample reverses the READ side (xs = crop_w - 1 - x').  The taps are plain byte / half-word / float gathers that neighbouring lanes
// share through the caches (a wave touches two source rows of ~130 pixels per output row); nothing is staged in LDS.  The coordinates
// (four fp64 products, four rint) are computed once per pixel and serve both frames and the ground truth.
//
// Bounds: a per-sample record is checked by the kernel before anything is read (the sample's outputs become zeros and status 1 when
// it fails); with a record that passes, the warp == 0 read position lies in [0, h) x [0, w) by the crop-origin check and every
// warped tap index is folded into [0, len) by reflect101 whatever the matrix holds, so no record can become an out-of-bounds gather.
#include "pwc_augment_taps.h"

namespace {

using namespace pwc_aug;
static_assert(sizeof(pwc_augment_params) == 88, "augment parameter record");

struct Args {
    const uint8_t *frames;
    const void *gt;
    const uint8_t *valid;
    const pwc_augment_params *params;
    float *x, *flow, *vout;
    int *status;
    int Hs, Ws, crop_h, crop_w, gt_kind;
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void kitti_augment_kernel(Args a) {
    const int tid = threadIdx.x, b = blockIdx.z;
    const int y = blockIdx.y * kTH + tid / kLanesX;
    const int x0 = blockIdx.x * kTW + (tid % kLanesX) * kPix;
    const pwc_augment_params P = a.params[b];
    const int H = P.h, W = P.w;
    const bool bad = H < 1 || H > a.Hs || W < 1 || W > a.Ws || a.crop_h > H || a.crop_w > W || P.y0 < 0 || P.y0 > H - a.crop_h ||
                     P.x0 < 0 || P.x0 > W - a.crop_w;
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) a.status[b] = bad ? 1 : 0;
    if (y >= a.crop_h || x0 >= a.crop_w) return;

    float out[9][kPix];
#pragma unroll
    for (int c = 0; c < 9; ++c)
#pragma unroll
        for (int k = 0; k < kPix; ++k) out[c][k] = 0.0f;

    if (!bad) {
        const int64_t slot = (int64_t)a.Hs * a.Ws;
        const uint8_t *f1 = a.frames + (int64_t)b * 2 * slot * 3, *f2 = f1 + slot * 3;
        Gt g;
        g.png = a.gt_kind == 1 ? static_cast<const uint16_t *>(a.gt) + (int64_t)b * slot * 3 : nullptr;
        g.fu = static_cast<const float *>(a.gt) + (int64_t)b * 2 * slot;
        g.fv = g.fu + slot;
        g.valid = a.valid ? a.valid + (int64_t)b * slot : nullptr;
        const int Y = P.y0 + y;
        const bool warp = P.warp != 0, flip = P.flip != 0;
        // the row terms of the fixed-point coordinates are the same for the lane's pixels
        const int X0 = warp ? wrap_add(round_i32((P.m[1] * (double)Y + P.m[2]) * 1024.0), 16) : 0;
        const int Y0 = warp ? wrap_add(round_i32((P.m[4] * (double)Y + P.m[5]) * 1024.0), 16) : 0;
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const int xo = x0 + k;
            if (xo >= a.crop_w) continue;
            const int X = P.x0 + (flip ? a.crop_w - 1 - xo : xo);
            float u, v, m;
            if (!warp) {
                const int o = Y * W + X;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    out[c][k] = (float)f1[3 * (int64_t)o + c] / 255.0f;
                    out[3 + c][k] = (float)f2[3 * (int64_t)o + c] / 255.0f;
                }
                g.tap(o, u, v, m);
            } else {
                const int ad = round_i32(P.m[0] * (double)X * 1024.0), bd = round_i32(P.m[3] * (double)X * 1024.0);
                const int Xq = wrap_add(X0, ad) >> 5, Yq = wrap_add(Y0, bd) >> 5;
                const int sx = Xq >> 5, sy = Yq >> 5, fx = Xq & 31, fy = Yq & 31;
                const int xa = reflect101(sx, W), xb = reflect101(sx + 1, W);
                const int ya = reflect101(sy, H) * W, yb = reflect101(sy + 1, H) * W;
                const int o00 = ya + xa, o01 = ya + xb, o10 = yb + xa, o11 = yb + xb;
                const int i00 = (32 - fy) * (32 - fx), i01 = (32 - fy) * fx, i10 = fy * (32 - fx), i11 = fy * fx;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int p1 = f1[3 * (int64_t)o00 + c] * i00 + f1[3 * (int64_t)o01 + c] * i01 + f1[3 * (int64_t)o10 + c] * i10 +
                                   f1[3 * (int64_t)o11 + c] * i11;
                    const int p2 = f2[3 * (int64_t)o00 + c] * i00 + f2[3 * (int64_t)o01 + c] * i01 + f2[3 * (int64_t)o10 + c] * i10 +
                                   f2[3 * (int64_t)o11 + c] * i11;
                    out[c][k] = (float)((p1 + 512) >> 10) / 255.0f;
                    out[3 + c][k] = (float)((p2 + 512) >> 10) / 255.0f;
                }
                const float gx = (float)fx / 32.0f, gy = (float)fy / 32.0f;
                const float w00 = (1.0f - gy) * (1.0f - gx), w01 = (1.0f - gy) * gx, w10 = gy * (1.0f - gx), w11 = gy * gx;
                float u00, v00, m00, u01, v01, m01, u10, v10, m10, u11, v11, m11;
                g.tap(o00, u00, v00, m00);
                g.tap(o01, u01, v01, m01);
                g.tap(o10, u10, v10, m10);
                g.tap(o11, u11, v11, m11);
                const float fu = ((u00 * w00 + u01 * w01) + u10 * w10) + u11 * w11;
                const float fv = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11;
                const float fm = ((m00 * w00 + m01 * w01) + m10 * w10) + m11 * w11;
                u = P.a[0] * fu + P.a[1] * fv;
                v = P.a[2] * fu + P.a[3] * fv;
                m = fm > 0.5f ? 1.0f : 0.0f;
            }
            out[6][k] = flip ? u * -1.0f : u;
            out[7][k] = v;
            out[8][k] = m;
        }
    }

    const int64_t plane = (int64_t)a.crop_h * a.crop_w, row = (int64_t)y * a.crop_w;
#pragma unroll
    for (int c = 0; c < 6; ++c) store_row<VEC>(a.x + ((int64_t)b * 6 + c) * plane + row, x0, a.crop_w, out[c]);
    store_row<VEC>(a.flow + ((int64_t)b * 2) * plane + row, x0, a.crop_w, out[6]);
    store_row<VEC>(a.flow + ((int64_t)b * 2 + 1) * plane + row, x0, a.crop_w, out[7]);
    store_row<VEC>(a.vout + (int64_t)b * plane + row, x0, a.crop_w, out[8]);
}

}  // namespace

extern "C" int pwc_kitti_augment(const void *frames, const void *gt, int gt_kind, const void *valid, int n, int Hs, int Ws, int crop_h,
                                 int crop_w, const void *params, void *x, void *flow, void *valid_out, void *status, void *stream) {
    if (!frames || !gt || !params || !x || !flow || !valid_out || !status) PWC_FAIL(PWC_EINVAL, "pwc_kitti_augment: null pointer");
    if (n <= 0 || Hs <= 0 || Ws <= 0 || crop_h <= 0 || crop_w <= 0)
        PWC_FAIL(PWC_EINVAL, "pwc_kitti_augment: bad shape n=%d slot=%dx%d crop=%dx%d", n, Hs, Ws, crop_h, crop_w);
    if (n > 65535 || Hs > 32767 || Ws > 32767) PWC_FAIL(PWC_EINVAL, "pwc_kitti_augment: needs n <= 65535 and a slot of at most 32767 x 32767");
    if (crop_h > Hs || crop_w > Ws) PWC_FAIL(PWC_EINVAL, "pwc_kitti_augment: crop %dx%d larger than the slot %dx%d", crop_h, crop_w, Hs, Ws);
    if (gt_kind != 0 && gt_kind != 1) PWC_FAIL(PWC_EINVAL, "pwc_kitti_augment: unknown gt_kind %d (0 = float planes, 1 = uint16 PNG samples)", gt_kind);
    if (gt_kind == 1 && valid) PWC_FAIL(PWC_EINVAL, "pwc_kitti_augment: gt_kind 1 carries its own validity, valid must be NULL");
    if (pwc::misaligned({x, flow, valid_out, status}) || pwc::misaligned({gt}, gt_kind == 1 ? 2 : 4))
        PWC_FAIL(PWC_EALIGN, "pwc_kitti_augment: float / int32 pointers must be 4-byte aligned, a uint16 gt 2-byte aligned");
    if (pwc::misaligned({params}, 8)) PWC_FAIL(PWC_EALIGN, "pwc_kitti_augment: the parameter buffer must be 8-byte aligned");
    Args a;
    a.frames = static_cast<const uint8_t *>(frames);
    a.gt = gt;
    a.valid = static_cast<const uint8_t *>(valid);
    a.params = static_cast<const pwc_augment_params *>(params);
    a.x = static_cast<float *>(x);
    a.flow = static_cast<float *>(flow);
    a.vout = static_cast<float *>(valid_out);
    a.status = static_cast<int *>(status);
    a.Hs = Hs; a.Ws = Ws; a.crop_h = crop_h; a.crop_w = crop_w; a.gt_kind = gt_kind;
    const dim3 grid((crop_w + kTW - 1) / kTW, (crop_h + kTH - 1) / kTH, n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (crop_w % kPix == 0 && !pwc::misaligned({x, flow, valid_out}, 16))
        hipLaunchKernelGGL(kitti_augment_kernel<true>, grid, dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL(kitti_augment_kernel<false>, grid, dim3(kThreads), 0, st, a);
    return pwc::check_launch("kitti_augment_kernel");
}
