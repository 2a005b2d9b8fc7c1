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
#include "pwc_augment_common.h"

namespace {

using namespace pwc_aug;
static_assert(sizeof(pwc_augment_params) == 88, "augment parameter record");

template <bool VEC>
__global__ __launch_bounds__(kThreads) void kitti_augment_kernel(Args<pwc_augment_params> a) {
    const int tid = threadIdx.x, b = blockIdx.z;
    const int y = blockIdx.y * kTH + tid / kLanesX;
    const int x0 = blockIdx.x * kTW + (tid % kLanesX) * kPix;
    const pwc_augment_params P = a.params[b];
    const int H = P.h, W = P.w;
    const bool bad = bad_geometry(P, a.Hs, a.Ws, a.crop_h, a.crop_w);
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) a.status[b] = bad ? 1 : 0;
    if (y >= a.crop_h || x0 >= a.crop_w) return;

    float out[9][kPix];
#pragma unroll
    for (int c = 0; c < 9; ++c)
#pragma unroll
        for (int k = 0; k < kPix; ++k) out[c][k] = 0.0f;

    if (!bad) {
        Src S;
        set_sources(S, a, b);
        const uint8_t *f1 = S.f1, *f2 = S.f2;
        const Gt &g = S.g;
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

    store_planes<VEC>(a.x, a.flow, a.vout, a.crop_h, a.crop_w, b, y, x0, out);
}

}  // namespace

extern "C" int pwc_kitti_augment(const void *frames, const void *gt, int gt_kind, const void *valid, int n, int Hs, int Ws, int crop_h,
                                 int crop_w, const void *params, void *x, void *flow, void *valid_out, void *status, void *stream) {
    return launch<pwc_augment_params>("pwc_kitti_augment", "kitti_augment_kernel", kitti_augment_kernel<true>, kitti_augment_kernel<false>, frames,
                                      gt, gt_kind, valid, n, Hs, Ws, crop_h, crop_w, params, x, flow, valid_out, status, stream);
}
