// Upsampled flow of the self-supervised scripts (upsample_flow_to, align_corners=True, vectors scaled by W/w and H/h), shared by
// pwc_proxy_loss.hip and pwc_fb_metrics.hip so that both evaluate it with the same fp32 operations in the same order
// (include/pwc_hip.h spells them out; -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pwc {

// (u, v) at full-resolution pixel (Y, X); f = flow of this image ([2][h][w]).  G provides H, W, h, w, same = ((h,w) == (H,W)),
// rh = (float)(h-1) / (float)(H-1), rw alike, sy = (float)((double)H / h), sx alike.
template <typename G>
__device__ __forceinline__ float2 up_flow(const float *f, const G &g, int Y, int X) {
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

}  // namespace pwc
