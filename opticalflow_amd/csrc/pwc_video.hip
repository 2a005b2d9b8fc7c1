// Front of the video pipeline as one kernel (reference pwc_extract_flow_video.py:27-42; host mirror opticalflow_amd/video.py
// frame_to_tensor + kitti.pad_to_64): raw frames uint8 [n][H][W][3] (HWC, as cv2 decodes them) -> float [n][3][Hp][Wp] planes, Hp / Wp =
// H / W rounded up to multiples of 64.
//   channel : output channel c reads source channel 2 - c when `bgr` (cv2.cvtColor(BGR2RGB)), else c;
//   value   : (float)byte / 255.0f, the IEEE division of `astype(np.float32) / 255.0` -- NOT a multiplication by 1 / 255, which differs
//             from the quotient for 126 of the 256 byte values;
//   padding : replicate at the bottom / right = a clamped source coordinate.
// The source may be one slot of a larger buffer (batch stride in bytes) and its rows are 3 * W bytes, so nothing is assumed about its
// alignment: a thread whose twelve bytes happen to start on a dword boundary reads three dwords, every other thread reads bytes.
#include <stdint.h>

#include "pwc_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// thread = four consecutive output columns of one (frame, row): 12 source bytes (fewer at the right edge) -> three 16-byte stores
__global__ void __launch_bounds__(256)
video_ingest_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, int H, int W, int Hp, int Wp, int64_t sbs, int64_t bsd,
                    int bgr, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int wq = Wp >> 2;
    const int xq = (int)(idx % wq);
    int64_t t = idx / wq;
    const int y = (int)(t % Hp);
    const int64_t b = t / Hp;
    const uint8_t *row = src + b * sbs + (int64_t)min(y, H - 1) * W * 3;
    const int x0 = 4 * xq;
    uint8_t px[12];                                                            // px[3 * q + channel] of column x0 + q
    const uint8_t *p = row + (int64_t)x0 * 3;
    if (x0 + 3 < W && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
        const uint32_t *p4 = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t v = p4[k];
            px[4 * k + 0] = (uint8_t)(v & 255u);
            px[4 * k + 1] = (uint8_t)((v >> 8) & 255u);
            px[4 * k + 2] = (uint8_t)((v >> 16) & 255u);
            px[4 * k + 3] = (uint8_t)(v >> 24);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint8_t *s = row + (int64_t)min(x0 + q, W - 1) * 3;          // replicate padding = clamped source coordinate
#pragma unroll
            for (int c = 0; c < 3; ++c) px[3 * q + c] = s[c];
        }
    }
    float *o = dst + b * bsd + (int64_t)y * Wp + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint8_t lo = px[3 * q + c], hi = px[3 * q + 2 - c];
            v[q] = __fdiv_rn((float)(bgr ? hi : lo), 255.0f);
        }
        *reinterpret_cast<f32x4 *>(o + (int64_t)c * Hp * Wp) = v;
    }
}

}  // namespace

extern "C" int pwc_video_ingest_u8(const void *frames_u8, void *x, int n, int H, int W, int bgr, int64_t src_bstride, int64_t x_bstride,
                                   void *stream) {
    if (!frames_u8 || !x) PWC_FAIL(PWC_EINVAL, "pwc_video_ingest_u8: null pointer");
    if (n <= 0 || H <= 0 || W <= 0 || H > (1 << 20) || W > (1 << 20)) PWC_FAIL(PWC_EINVAL, "pwc_video_ingest_u8: bad shape (sizes must be in 1..2^20)");
    const int Hp = (H + 63) / 64 * 64, Wp = (W + 63) / 64 * 64;
    if (src_bstride < (int64_t)3 * H * W) PWC_FAIL(PWC_EINVAL, "pwc_video_ingest_u8: source batch stride smaller than the frame (3*H*W bytes)");
    if (x_bstride < (int64_t)3 * Hp * Wp) PWC_FAIL(PWC_EINVAL, "pwc_video_ingest_u8: x batch stride smaller than 3*Hp*Wp");
    if (!pwc::aligned16(x) || (x_bstride & 3)) PWC_FAIL(PWC_EALIGN, "pwc_video_ingest_u8: x must be 16-byte aligned with a batch stride that is a multiple of 4");
    const int64_t total = (int64_t)n * Hp * (Wp >> 2);
    if ((total + 255) / 256 > 0x7fffffffLL) PWC_FAIL(PWC_EINVAL, "pwc_video_ingest_u8: grid too large");
    hipLaunchKernelGGL(video_ingest_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t *>(frames_u8), static_cast<float *>(x), H, W, Hp, Wp, src_bstride, x_bstride, bgr ? 1 : 0, total);
    return pwc::check_launch("video_ingest_kernel");
}
