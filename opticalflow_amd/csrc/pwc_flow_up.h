// Upsampled flow of the self-supervised scripts (upsample_flow_to, align_corners=True, vectors scaled by W/w and H/h), shared by
// pwc_proxy_loss.hip and pwc_fb_metrics.hip so that both evaluate it with the same fp32 operations in the same order
// (include/pwc_hip.h spells them out; -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pwc {

// geometry of the upsampling: flow [2][h][w] to the image grid H x W; same = ((h,w) == (H,W)), the flow is used as it is
struct UpGeo {
    int H, W, h, w, same;
    float rh, rw, sy, sx;
};

inline UpGeo up_geo_make(int H, int W, int h, int w) {
    UpGeo g;
    g.H = H; g.W = W; g.h = h; g.w = w;
    g.same = (h == H && w == W) ? 1 : 0;
    g.rh = (float)(h - 1) / (float)(H - 1);
    g.rw = (float)(w - 1) / (float)(W - 1);
    g.sy = (float)((double)H / (double)h);
    g.sx = (float)((double)W / (double)w);
    return g;
}

// (u, v) at full-resolution pixel (Y, X); f = flow of this image ([2][h][w])
__device__ __forceinline__ float2 up_flow(const float *f, const UpGeo &g, int Y, int X) {
    if (g.same) return make_float2(f[(int64_t)Y * g.W + X], f[(int64_t)g.H * g.W + (int64_t)Y * g.W + X]);
    const float fy = g.rh * (float)Y, fx = g.rw * (float)X;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < g.h - 1 ? 1 : 0), x1 = x0 + (x0 < g.w - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
    const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
    const float *fu = f, *fv = f + (int64_t)g.h * g.w;
    const int a = y0 * g.w, b = y1 * g.w;
    const float u = ly0 * (lx0 * fu[a + x0] + lx1 * fu[a + x1]) + ly1 * (lx0 * fu[b + x0] + lx1 * fu[b + x1]);
    const float v = ly0 * (lx0 * fv[a + x0] + lx1 * fv[a + x1]) + ly1 * (lx0 * fv[b + x0] + lx1 * fv[b + x1]);
    return make_float2(u * g.sx, v * g.sy);
}

// Cropped upsample of the KITTI evaluation loop (`unpad` + `flow_resize` of inference_kitti.py:66-91), shared by flow_upsample_kernel
// (pwc_kitti.hip) and the score kernel (pwc_kitti_score.hip) so that both evaluate it with the same fp32 operations in the same order:
// the top-left hc x wc of a [2][Hq][Wq] field, bilinear with align_corners = True (F.interpolate's arithmetic: source = dst * (in - 1) /
// (out - 1), weights 1 - l and l), u * (w / wc), v * (h / hc).
struct CropUp {
    int Hq, Wq, hc, wc;
    float rh, rw, su, sv;
};

inline CropUp crop_up_make(int Hq, int Wq, int crop_h, int crop_w, int out_h, int out_w) {
    CropUp g;
    g.Hq = Hq; g.Wq = Wq; g.hc = crop_h; g.wc = crop_w;
    // F.interpolate(align_corners = True): scale = (in - 1) / (out - 1) in float (0 for a one-pixel output)
    g.rh = out_h > 1 ? (float)(crop_h - 1) / (float)(out_h - 1) : 0.f;
    g.rw = out_w > 1 ? (float)(crop_w - 1) / (float)(out_w - 1) : 0.f;
    g.su = (float)((double)out_w / (double)crop_w);
    g.sv = (float)((double)out_h / (double)crop_h);
    return g;
}

// (u, v) at output pixel (y, x); p = quarter-resolution flow of this item ([2][Hq][Wq])
__device__ __forceinline__ float2 crop_up_flow(const float *__restrict__ p, const CropUp &g, int y, int x) {
    const float fy = g.rh * (float)y, fx = g.rw * (float)x;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < g.hc - 1 ? 1 : 0), x1 = x0 + (x0 < g.wc - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0, my = 1.0f - ly, mx = 1.0f - lx;
    const int64_t plane = (int64_t)g.Hq * g.Wq;
    float r[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *pc = p + c * plane;
        const float v = my * (mx * pc[(int64_t)y0 * g.Wq + x0] + lx * pc[(int64_t)y0 * g.Wq + x1]) +
                        ly * (mx * pc[(int64_t)y1 * g.Wq + x0] + lx * pc[(int64_t)y1 * g.Wq + x1]);
        r[c] = v * (c == 0 ? g.su : g.sv);
    }
    return make_float2(r[0], r[1]);
}

}  // namespace pwc
