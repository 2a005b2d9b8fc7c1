// train2.py's training batches on the device: KittiAugmentationPipeline (data_processing.py:136-279) -- crop, flip, rotation, integer
// translation, brightness / contrast, Gaussian blur, /255 -- in one launch, from the raw uint8 frames and the ground truth.  The
// reference crops first, so every stage lives inside the crop window and every border reflection is about the window's edges; the
// stages are applied read-side, last stage first.  The arithmetic is spelled out in include/pwc_hip.h and restated in the reference's
// forward order in tests/augment_full_oracle.py, and the two agree bit for bit.
//
// One workgroup = one 8 x 128 tile of one sample's window, 256 lanes, a lane owns kPix = 4 consecutive x of one row (the layout and
// the stores of pwc_augment.hip).  The sample's flags are workgroup-uniform, so no stage branch diverges.
//   no blur: nothing is staged; one coordinate chain per pixel serves both frames and the ground truth.
//   blur:    the uint8-truncated image after the brightness stage is staged for the tile plus a 3-pixel halo (14 x 134 positions, six
//            channel planes of 14 x 136 bytes = 11424 B of LDS; 1.83 chains per output pixel), each halo position mapped by
//            BORDER_REFLECT_101 in WINDOW coordinates before the chain, so it may lie anywhere in the window.  The horizontal pass
//            writes uint16 (6 x 14 x 128 x 2 = 21504 B), the vertical pass reads it.  A kernel of 3 or 5 taps is centred in the 7-tap
//            frame with zero weights.  Flow and mask need no halo: they come out of the chain that stages the lane's own pixels.
//
// Bounds: a record is checked by the kernel before anything is read (zeros and status 1 when it fails).  With a record that passes,
// every window position -- shifted, rotated or a halo -- is folded into [0, crop_h) x [0, crop_w) by reflect_edge / reflect101 whatever
// the matrix or the shift holds, and the window lies inside the sample by the crop-origin check, so no record becomes an
// out-of-bounds gather.  The blur weights are read only below ksize <= 7 and must add up to 256, so the uint16 pass cannot overflow.
#include "pwc_augment_common.h"

namespace {

using namespace pwc_aug;
static_assert(sizeof(pwc_augment_full_params) == 128, "full augmentation parameter record");

constexpr int kHalo = 3, kTaps = 2 * kHalo + 1;
constexpr int kSH = kTH + 2 * kHalo, kSW = kTW + 2 * kHalo;     // 14 x 134 staged positions
constexpr int kSWp = (kSW + 3) / 4 * 4;                           // rows padded to whole 32-bit words
constexpr int kRing = kSH * kSW - kTH * kTW;                      // 852 halo positions around the 1024 owned ones
static_assert(kRing == 2 * kHalo * kSW + 2 * kHalo * kTH, "halo ring");
static_assert(kSWp / 4 >= kLanesX + 2, "the horizontal pass reads three words per lane");

__device__ __forceinline__ float blend(float p00, float p01, float p10, float p11, float w00, float w01, float w10, float w11) {
    return ((p00 * w00 + p01 * w01) + p10 * w10) + p11 * w11;
}

// Stages 6..2 of the header for window position (y, x), any integers already folded into the window: the image values in [0, 255]
// after the brightness stage (IMG) and / or the flow vector and the fractional mask (GT).
template <bool IMG, bool GT>
__device__ __forceinline__ void chain(const Src &S, const pwc_augment_full_params &P, int ch, int cw, int y, int x, float (&img)[6],
                                      float &u, float &v, float &m) {
    if (P.trans != 0) {
        y = reflect_edge(y - P.ty, ch);
        x = reflect_edge(x - P.tx, cw);
    }
    const bool flip = P.flip != 0;
    if (P.rot == 0) {
        const int o = (P.y0 + y) * P.w + P.x0 + (flip ? cw - 1 - x : x);
        if (IMG) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                img[c] = (float)S.f1[3 * (int64_t)o + c];
                img[3 + c] = (float)S.f2[3 * (int64_t)o + c];
            }
        }
        if (GT) {
            S.g.tap(o, u, v, m);
            if (flip) u = -u;
        }
    } else {
        const double Xd = (double)x, Yd = (double)y;
        const int ad = round_i32(P.m[0] * Xd * 1024.0), bd = round_i32(P.m[3] * Xd * 1024.0);
        const int X0 = wrap_add(round_i32((P.m[1] * Yd + P.m[2]) * 1024.0), 16);
        const int Y0 = wrap_add(round_i32((P.m[4] * Yd + P.m[5]) * 1024.0), 16);
        const int Xq = wrap_add(X0, ad) >> 5, Yq = wrap_add(Y0, bd) >> 5;
        const int sx = Xq >> 5, sy = Yq >> 5, fx = Xq & 31, fy = Yq & 31;
        int xa = reflect_edge(sx, cw), xb = reflect_edge(sx + 1, cw);
        if (flip) {
            xa = cw - 1 - xa;
            xb = cw - 1 - xb;
        }
        const int ya = (P.y0 + reflect_edge(sy, ch)) * P.w + P.x0, yb = (P.y0 + reflect_edge(sy + 1, ch)) * P.w + P.x0;
        const int o00 = ya + xa, o01 = ya + xb, o10 = yb + xa, o11 = yb + xb;
        const float gx = (float)fx / 32.0f, gy = (float)fy / 32.0f;
        const float w00 = (1.0f - gy) * (1.0f - gx), w01 = (1.0f - gy) * gx, w10 = gy * (1.0f - gx), w11 = gy * gx;
        if (IMG) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                img[c] = blend((float)S.f1[3 * (int64_t)o00 + c], (float)S.f1[3 * (int64_t)o01 + c], (float)S.f1[3 * (int64_t)o10 + c],
                               (float)S.f1[3 * (int64_t)o11 + c], w00, w01, w10, w11);
                img[3 + c] = blend((float)S.f2[3 * (int64_t)o00 + c], (float)S.f2[3 * (int64_t)o01 + c], (float)S.f2[3 * (int64_t)o10 + c],
                                   (float)S.f2[3 * (int64_t)o11 + c], w00, w01, w10, w11);
            }
        }
        if (GT) {
            float u00, v00, m00, u01, v01, m01, u10, v10, m10, u11, v11, m11;
            S.g.tap(o00, u00, v00, m00);
            S.g.tap(o01, u01, v01, m01);
            S.g.tap(o10, u10, v10, m10);
            S.g.tap(o11, u11, v11, m11);
            if (flip) {
                u00 = -u00;
                u01 = -u01;
                u10 = -u10;
                u11 = -u11;
            }
            const float fu = blend(u00, u01, u10, u11, w00, w01, w10, w11);
            const float fv = blend(v00, v01, v10, v11, w00, w01, w10, w11);
            m = blend(m00, m01, m10, m11, w00, w01, w10, w11);
            // the reference's second line reads the u it has just overwritten (u is a view), in float64
            u = (float)((double)fu * P.cs[0] - (double)fv * P.cs[1]);
            v = (float)((double)u * P.cs[1] + (double)fv * P.cs[0]);
        }
    }
    if (IMG && P.bright != 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float t = P.gain * (img[c] - 127.5f) + 127.5f;
            img[c] = fminf(fmaxf(t, 0.0f), 255.0f);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void kitti_augment_full_kernel(Args<pwc_augment_full_params> a) {
    __shared__ __align__(16) uint8_t tile8[6][kSH][kSWp];
    __shared__ __align__(16) uint16_t hrow[6][kSH][kTW];

    const int tid = threadIdx.x, b = blockIdx.z, ly = tid / kLanesX, lx = tid % kLanesX;
    const int ty0 = blockIdx.y * kTH, tx0 = blockIdx.x * kTW;
    const int y = ty0 + ly, x0 = tx0 + lx * kPix;
    const int ch = a.crop_h, cw = a.crop_w;
    const pwc_augment_full_params P = a.params[b];
    const uint16_t *wk = a.params[b].wk;           // indexed at run time: read from memory, not from the register copy
    bool bad = bad_geometry(P, a.Hs, a.Ws, ch, cw);
    if (P.trans != 0)
        bad = bad || P.tx < -PWC_AUGMENT_FULL_MAX_SHIFT || P.tx > PWC_AUGMENT_FULL_MAX_SHIFT || P.ty < -PWC_AUGMENT_FULL_MAX_SHIFT ||
              P.ty > PWC_AUGMENT_FULL_MAX_SHIFT;
    int w7[kTaps];
#pragma unroll
    for (int i = 0; i < kTaps; ++i) w7[i] = 0;
    if (P.blur != 0) {
        const int ks = P.ksize;
        if (ks != 3 && ks != 5 && ks != 7) {
            bad = true;
        } else {
            const int off = kHalo - (ks - 1) / 2;
            int sum = 0;
#pragma unroll
            for (int i = 0; i < kTaps; ++i) {
                const int j = i - off;
                w7[i] = (j >= 0 && j < ks) ? (int)wk[j] : 0;
                sum += w7[i];
            }
            bad = bad || sum != 256;
        }
    }
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) a.status[b] = bad ? 1 : 0;
    const bool live = y < ch && x0 < cw;

    float out[9][kPix];
#pragma unroll
    for (int c = 0; c < 9; ++c)
#pragma unroll
        for (int k = 0; k < kPix; ++k) out[c][k] = 0.0f;

    if (!bad) {                                    // bad and every flag are the same for the whole workgroup
        Src S;
        set_sources(S, a, b);
        float img[6], u = 0.0f, v = 0.0f, m = 0.0f;

        if (P.blur == 0) {
            if (live) {
#pragma unroll
                for (int k = 0; k < kPix; ++k) {
                    if (x0 + k >= cw) continue;
                    chain<true, true>(S, P, ch, cw, y, x0 + k, img, u, v, m);
#pragma unroll
                    for (int c = 0; c < 6; ++c) out[c][k] = img[c] / 255.0f;
                    out[6][k] = u;
                    out[7][k] = v;
                    out[8][k] = m;
                }
            }
        } else {
            // the lane's own four positions first: one chain gives the staged image bytes and the flow and mask it will store (a
            // position past the window's edge is folded like a halo: a neighbour's blur may read it)
            {
                const int wy = reflect101(y, ch);
#pragma unroll
                for (int k = 0; k < kPix; ++k) {
                    chain<true, true>(S, P, ch, cw, wy, reflect101(x0 + k, cw), img, u, v, m);
#pragma unroll
                    for (int c = 0; c < 6; ++c) tile8[c][ly + kHalo][lx * kPix + k + kHalo] = (uint8_t)(int)img[c];
                    out[6][k] = u;
                    out[7][k] = v;
                    out[8][k] = m;
                }
            }
            // then the ring: kHalo rows above and below, kHalo columns left and right
            for (int p = tid; p < kRing; p += kThreads) {
                int r, c;
                if (p < 2 * kHalo * kSW) {
                    r = p / kSW;
                    c = p - r * kSW;
                    if (r >= kHalo) r += kTH;
                } else {
                    const int q = p - 2 * kHalo * kSW;
                    r = kHalo + q / (2 * kHalo);
                    c = q % (2 * kHalo);
                    if (c >= kHalo) c += kTW;
                }
                chain<true, false>(S, P, ch, cw, reflect101(ty0 + r - kHalo, ch), reflect101(tx0 + c - kHalo, cw), img, u, v, m);
#pragma unroll
                for (int k = 0; k < 6; ++k) tile8[k][r][c] = (uint8_t)(int)img[k];
            }
            __syncthreads();
            // horizontal pass: the four outputs of a lane group need staged columns 4 gx .. 4 gx + 9 = three aligned words
            for (int q = tid; q < 6 * kSH * kLanesX; q += kThreads) {
                const int gx = q % kLanesX, r = (q / kLanesX) % kSH, c = q / (kLanesX * kSH);
                const uint32_t *rp = reinterpret_cast<const uint32_t *>(&tile8[c][r][0]) + gx;
                const uint32_t wd[3] = {rp[0], rp[1], rp[2]};
                uint32_t s[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) s[i] = (wd[i / 4] >> (8 * (i % 4))) & 255u;
                uint32_t h[kPix];
#pragma unroll
                for (int k = 0; k < kPix; ++k) {
                    uint32_t acc = 0;
#pragma unroll
                    for (int i = 0; i < kTaps; ++i) acc += (uint32_t)w7[i] * s[k + i];
                    h[k] = acc;                    // <= 256 * 255, fits uint16
                }
                *reinterpret_cast<uint2 *>(&hrow[c][r][gx * kPix]) = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    uint32_t acc[kPix] = {0, 0, 0, 0};
#pragma unroll
                    for (int j = 0; j < kTaps; ++j) {
                        const uint2 hv = *reinterpret_cast<const uint2 *>(&hrow[c][ly + j][lx * kPix]);
                        acc[0] += (uint32_t)w7[j] * (hv.x & 0xffffu);
                        acc[1] += (uint32_t)w7[j] * (hv.x >> 16);
                        acc[2] += (uint32_t)w7[j] * (hv.y & 0xffffu);
                        acc[3] += (uint32_t)w7[j] * (hv.y >> 16);
                    }
#pragma unroll
                    for (int k = 0; k < kPix; ++k) out[c][k] = (float)((acc[k] + 32768u) >> 16) / 255.0f;
                }
            }
        }
    }
    if (!live) return;

    store_planes<VEC>(a.x, a.flow, a.vout, a.crop_h, a.crop_w, b, y, x0, out);
}

}  // namespace

extern "C" int pwc_kitti_augment_full(const void *frames, const void *gt, int gt_kind, const void *valid, int n, int Hs, int Ws, int crop_h,
                                      int crop_w, const void *params, void *x, void *flow, void *mask_out, void *status, void *stream) {
    return launch<pwc_augment_full_params>("pwc_kitti_augment_full", "kitti_augment_full_kernel", kitti_augment_full_kernel<true>,
                                           kitti_augment_full_kernel<false>, frames, gt, gt_kind, valid, n, Hs, Ws, crop_h, crop_w, params, x,
                                           flow, mask_out, status, stream);
}
