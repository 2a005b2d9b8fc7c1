// cv2.warpPerspective-exact warp of 8-bit BGR frames on the device (opticalflow_amd/cv_warp.py): the step of topview.py:218,232 that
// turns a camera frame into the top view, with the script's defaults INTER_LINEAR, BORDER_CONSTANT, border value 0.  The arithmetic is
// this project's statement of OpenCV's published algorithm (imgproc's warpPerspective + the 8-bit bilinear remap), written out in
// include/pwc_hip.h and as NumPy in tests/cv_warp_oracle.py; cv2 is not available here, so cv2 parity is unpinned, and with it the one
// point the published source does not settle: how the int16 weight table stores 32768 at ax = ay = 0 (taken as 32768 here, so that an
// identity warp returns the image).
//   coordinates, float64, every product and sum rounded (-ffp-contract=off), formed from OpenCV's block origin xb = (x / bw0) * bw0:
//            X0 = (Mi[0]*xb + Mi[1]*y) + Mi[2] (Y0, W0 alike);  Wd = W0 + Mi[6]*x1;  Wd = Wd != 0 ? 32.0 / Wd : 0.0 (IEEE division);
//            fX = max(INT_MIN, min(INT_MAX, (X0 + Mi[0]*x1) * Wd)) in std::max / std::min's comparison form (a NaN becomes INT_MAX);
//            X = cvRound(fX) (half to even);  sx = clamp(X >> 5, -32768, 32767);  ax = X & 31;  Y, sy, ay alike.
//   pixel  , integer: D = (sum over the four taps of wx * wy * S + 512) >> 10 with wx in {32 - ax, ax}, wy in {32 - ay, ay}; a tap
//            outside the source contributes 0.  This is OpenCV's 15-bit table form with w15 = 32 * wx * wy, exact at 1 / 32 steps.
// Work decomposition: a gather with no reuse worth staging (a source byte feeds about one output).  One thread owns four consecutive
// destination pixels of one row, 12 bytes: three whole dwords where every destination row starts on a dword and w % 4 == 0, single
// bytes otherwise.  The nine doubles of a frame's matrix are the same for the whole workgroup (blockIdx.y is the frame) and are read
// through the scalar cache.  A pixel whose four taps lie inside the source (nearly all of them under the script's matrix) reads them
// straight; any other reads bytes at clamped addresses with the weight zeroed when outside: no address leaves the frame.
#include <stdint.h>

#include "pwc_common.h"

namespace {

constexpr int kMaxDim = 32767;                 // the statement's int16 coordinate range

// cvRound of the clamped product: std::min(INT_MAX, v) and std::max(INT_MIN, .) as OpenCV writes them, then round half to even
__device__ __forceinline__ int fixed_coord(double v) {
    double f = v < 2147483647.0 ? v : 2147483647.0;
    f = -2147483648.0 < f ? f : -2147483648.0;
    return (int)rint(f);
}

// one destination pixel from its four taps (three bytes each), packed B | G << 8 | R << 16
__device__ __forceinline__ uint32_t blend(const uint8_t *t00, const uint8_t *t01, const uint8_t *t10, const uint8_t *t11, int w00,
                                          int w01, int w10, int w11) {
    uint32_t p = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        p |= (uint32_t)((w00 * (int)t00[c] + w01 * (int)t01[c] + w10 * (int)t10[c] + w11 * (int)t11[c] + 512) >> 10) << (8 * c);
    return p;
}

__global__ void __launch_bounds__(256)
cv_warp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int H, int W, int h, int w, const double *__restrict__ mat,
               int mat_stride, int64_t sbs, int64_t dbs, int bw0, int vec, int qpr) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;      // quad of this frame: (row, four columns)
    if (q >= (int64_t)h * qpr) return;
    const int y = (int)(q / qpr), x = 4 * (int)(q - (int64_t)y * qpr);
    const int f = blockIdx.y;
    const double *m = mat + (int64_t)f * mat_stride;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6], m7 = m[7], m8 = m[8];
    const uint8_t *img = src + (int64_t)f * sbs;
    const uint32_t W3 = 3u * (uint32_t)W;

    int xb = (x / bw0) * bw0;                                       // OpenCV's block origin of the first pixel
    const double yd = (double)y;
    uint32_t px_bgr[4];
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        const int xx = min(x + px, w - 1);                          // past the row's end: recomputed, never stored
        if (xx - xb >= bw0) xb += bw0;
        const double xbd = (double)xb, x1 = (double)(xx - xb);
        const double X0 = (m0 * xbd + m1 * yd) + m2;
        const double Y0 = (m3 * xbd + m4 * yd) + m5;
        const double W0 = (m6 * xbd + m7 * yd) + m8;
        double Wd = W0 + m6 * x1;
        Wd = (Wd != 0.0) ? 32.0 / Wd : 0.0;
        const int X = fixed_coord((X0 + m0 * x1) * Wd), Y = fixed_coord((Y0 + m3 * x1) * Wd);
        const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);
        const int ax = X & 31, ay = Y & 31;

        uint32_t p;
        if ((uint32_t)sx < (uint32_t)(W - 1) && (uint32_t)sy < (uint32_t)(H - 1)) {   // all four taps inside: nearly every pixel
            const uint8_t *t = img + ((uint32_t)sy * W3 + 3u * (uint32_t)sx);       // below 2^32: sizes are at most 32767
            p = blend(t, t + 3, t + W3, t + W3 + 3, (32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay);
        } else {                                                                    // clamped addresses, zeroed weights
            const int wx0 = (uint32_t)sx < (uint32_t)W ? 32 - ax : 0, wx1 = (uint32_t)(sx + 1) < (uint32_t)W ? ax : 0;
            const int wy0 = (uint32_t)sy < (uint32_t)H ? 32 - ay : 0, wy1 = (uint32_t)(sy + 1) < (uint32_t)H ? ay : 0;
            const uint32_t cx0 = 3u * min(max(sx, 0), W - 1), cx1 = 3u * min(max(sx + 1, 0), W - 1);
            const uint8_t *r0 = img + (uint32_t)min(max(sy, 0), H - 1) * W3, *r1 = img + (uint32_t)min(max(sy + 1, 0), H - 1) * W3;
            const int w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;
            p = (w00 | w01 | w10 | w11) ? blend(r0 + cx0, r0 + cx1, r1 + cx0, r1 + cx1, w00, w01, w10, w11) : 0u;   // wholly outside: no read
        }
        px_bgr[px] = p;
    }

    uint8_t *o = dst + (int64_t)f * dbs + ((int64_t)y * w + x) * 3;
    if (vec) {                                   // w % 4 == 0, dst and its batch stride dword-aligned: twelve whole bytes
        uint32_t *o32 = reinterpret_cast<uint32_t *>(o);
        o32[0] = px_bgr[0] | (px_bgr[1] << 24);
        o32[1] = (px_bgr[1] >> 8) | (px_bgr[2] << 16);
        o32[2] = (px_bgr[2] >> 16) | (px_bgr[3] << 8);
    } else {
#pragma unroll
        for (int px = 0; px < 4; ++px)
            if (x + px < w) {
                o[3 * px] = (uint8_t)px_bgr[px];
                o[3 * px + 1] = (uint8_t)(px_bgr[px] >> 8);
                o[3 * px + 2] = (uint8_t)(px_bgr[px] >> 16);
            }
    }
}

bool bad_dim(int v) { return v <= 0 || v > kMaxDim; }

}  // namespace

extern "C" int pwc_cv_warp_perspective_u8(const void *src_u8, void *dst_u8, int n, int H, int W, int h, int w, const double *mat9,
                                          int mat_stride, int64_t src_bstride, int64_t dst_bstride, void *stream) {
    if (!src_u8 || !dst_u8 || !mat9) PWC_FAIL(PWC_EINVAL, "pwc_cv_warp_perspective_u8: null pointer");
    if (bad_dim(H) || bad_dim(W) || bad_dim(h) || bad_dim(w))
        PWC_FAIL(PWC_EINVAL, "pwc_cv_warp_perspective_u8: bad shape (sizes must be in 1..32767)");
    if (n <= 0 || n > 65535) PWC_FAIL(PWC_EINVAL, "pwc_cv_warp_perspective_u8: n must be in 1..65535");
    if (mat_stride != 0 && mat_stride != 9) PWC_FAIL(PWC_EINVAL, "pwc_cv_warp_perspective_u8: mat_stride must be 0 or 9");
    if (src_bstride < (int64_t)3 * H * W || dst_bstride < (int64_t)3 * h * w)
        PWC_FAIL(PWC_EINVAL, "pwc_cv_warp_perspective_u8: batch stride smaller than the frame");
    if (pwc::misaligned({mat9}, 8)) PWC_FAIL(PWC_EALIGN, "pwc_cv_warp_perspective_u8: mat9 must be 8-byte aligned");
    const int bh0 = h < 16 ? h : 16;
    const int bw0 = (1024 / bh0) < w ? (1024 / bh0) : w;
    const int qpr = (w + 3) / 4;
    const int64_t blocks = ((int64_t)h * qpr + 255) / 256;          // at most 32767 * 8192 / 256
    const int vec = (w % 4 == 0) && !pwc::misaligned({dst_u8}) && (dst_bstride % 4 == 0);
    hipLaunchKernelGGL(cv_warp_kernel, dim3((unsigned)blocks, n), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t *>(src_u8), static_cast<uint8_t *>(dst_u8), H, W, h, w, mat9, mat_stride, src_bstride,
                       dst_bstride, bw0, vec, qpr);
    return pwc::check_launch("cv_warp_kernel");
}
