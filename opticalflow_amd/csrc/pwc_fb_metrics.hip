// No-ground-truth validation metrics of the reference's two self-supervised scripts, fused into one pass over the image grid:
// forward-backward cycle consistency (train_pseudo.py:178-193 _forward_backward_consistency, train_fundamental.py:397-409
// forward_backward_cycle) and the out-of-bounds ratio (train_pseudo.py:210-236 _oob_ratio, train_fundamental.py:412-428 oob_ratio).
//   a       = up(flow12)(Y, X)                     bilinear align_corners=True of the [h,w] field, x * W/w, y * H/h (identity when
//                                                  (h,w) == (H,W)): upsample_flow_to of both scripts
//   (px,py) = (X + a.x, Y + a.y);  oob = px < 0 || px > W-1 || py < 0 || py > H-1
//   wv      = bilinear(up(flow21), clamp(px, 0, W-1), clamp(py, 0, H-1))     grid_sample(bilinear, border, align_corners=True);
//                                                  each of the four taps is up(flow21) at an integer pixel, evaluated from [h,w]
//   cycle  += |a.x + wv.x| + |a.y + wv.y|
// out = {cycle / (B*2*H*W), oob_count / (B*H*W)}.  The fp32 arithmetic of up() and of the sample point is that of
// pwc_proxy_loss.hip, operation by operation (include/pwc_hip.h; -ffp-contract=off).
//
// Work split as in pwc_proxy_loss.hip: one workgroup = one 16 x 64 tile of one image, 256 lanes, each owning the column tid % 64
// of the rows tid / 64 + 4 k.  Neither field is staged in LDS.  flow12 is read as the proxy loss reads its flow -- the tile's
// pixels interpolate from a 5 x 17 window of the quarter-resolution field, 8 loads per pixel that hit L1 after the first row.  The
// flow21 taps are gathers at data-dependent positions (32 loads per pixel) from a field of B*2*h*w floats that stays in L2;
// no window of it is known before a.  Nothing image-sized is written: each workgroup leaves {fp64 cycle sum,
// int64 oob count} (fixed tree order) in the workspace and one final workgroup adds them in workgroup order.  No atomics: the
// result is bit-reproducible.
#include "pwc_block_reduce.h"
#include "pwc_common.h"
#include "pwc_flow_up.h"

namespace {

constexpr int kTH = 16, kTW = 64, kThreads = 256;
constexpr int kRowStep = kThreads / kTW;      // 4
constexpr int kPix = kTH / kRowStep;          // 4 pixels per lane
using Rec = pwc::TilePartial<1>;               // {double cycle_sum, int64 oob_count}: workspace = the total, then one per tile

struct Geo : pwc::UpGeo {
    int B, tiles_x, tiles_y;
    int64_t bs12, bs21;
};

using pwc::up_flow;   // pwc_flow_up.h: upsampled flow (u, v) at full-resolution pixel (Y, X)

__global__ __launch_bounds__(kThreads) void fb_tile_kernel(const float *flow12, const float *flow21, Rec *part, Geo g) {
    __shared__ pwc::TreeLds<kThreads, 1, 1> red;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int col = tid % kTW, row0 = tid / kTW;
    const float *f12 = flow12 + (int64_t)b * g.bs12;
    const float *f21 = flow21 ? flow21 + (int64_t)b * g.bs21 : nullptr;
    const float lx = (float)(g.W - 1), ly = (float)(g.H - 1);
    double cyc = 0.0;
    long long oob = 0;
    const int X = blockIdx.x * kTW + col;
#pragma unroll 1
    for (int k = 0; k < kPix; ++k) {
        const int Y = blockIdx.y * kTH + row0 + k * kRowStep;
        if (Y >= g.H || X >= g.W) continue;
        const float2 a = up_flow(f12, g, Y, X);
        const float px = (float)X + a.x, py = (float)Y + a.y;
        if (px < 0.0f || px > lx || py < 0.0f || py > ly) ++oob;
        if (!f21) continue;
        const float ix = fminf(fmaxf(px, 0.0f), lx), iy = fminf(fmaxf(py, 0.0f), ly);
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const int x1 = x0 + 1 < g.W ? x0 + 1 : x0, y1 = y0 + 1 < g.H ? y0 + 1 : y0;   // past the edge: weight 0
        const float tx = ix - fx, ty = iy - fy;
        const float2 v00 = up_flow(f21, g, y0, x0), v01 = up_flow(f21, g, y0, x1);
        const float2 v10 = up_flow(f21, g, y1, x0), v11 = up_flow(f21, g, y1, x1);
        const float wx = (1.0f - ty) * ((1.0f - tx) * v00.x + tx * v01.x) + ty * ((1.0f - tx) * v10.x + tx * v11.x);
        const float wy = (1.0f - ty) * ((1.0f - tx) * v00.y + tx * v01.y) + ty * ((1.0f - tx) * v10.y + tx * v11.y);
        cyc += (double)(fabsf(a.x + wx) + fabsf(a.y + wy));
    }
    pwc::tree_sum(red, &cyc, &oob);
    if (tid == 0) {
        const int64_t lin = blockIdx.x + (int64_t)g.tiles_x * (blockIdx.y + (int64_t)g.tiles_y * blockIdx.z);
        part[lin] = Rec{cyc, {oob}};
    }
}

__global__ __launch_bounds__(kThreads) void fb_finish_kernel(Rec *ws, int64_t nblk, int with_cycle, double ncycle, double npix,
                                                             float *out) {
    __shared__ pwc::TreeLds<kThreads, 1, 1> red;
    const int tid = threadIdx.x;
    const Rec *part = ws + 1;
    double c = 0.0;
    long long n = 0;
    for (int64_t i = tid; i < nblk; i += kThreads) {
        c += part[i].sum;
        n += part[i].count[0];
    }
    pwc::tree_sum(red, &c, &n);
    if (tid == 0) {
        ws[0] = Rec{c, {n}};
        out[0] = with_cycle ? (float)(c / ncycle) : 0.0f;
        out[1] = (float)((double)n / npix);
    }
}

}  // namespace

extern "C" int64_t pwc_fb_metrics_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    return (int64_t)sizeof(Rec) * (1 + (int64_t)B * ((H + kTH - 1) / kTH) * ((W + kTW - 1) / kTW));
}

extern "C" int pwc_fb_metrics(const void *flow12, const void *flow21, int B, int h, int w, int H, int W,
                              int64_t flow12_bstride, int64_t flow21_bstride,
                              void *workspace, int64_t workspace_bytes, void *out2, void *stream) {
    if (!flow12 || !workspace || !out2) PWC_FAIL(PWC_EINVAL, "pwc_fb_metrics: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0)
        PWC_FAIL(PWC_EINVAL, "pwc_fb_metrics: bad shape B=%d H=%d W=%d h=%d w=%d", B, H, W, h, w);
    if (H < 2 || W < 2 || h < 2 || w < 2 || H < h || W < w)
        PWC_FAIL(PWC_EINVAL, "pwc_fb_metrics: declined geometry H=%d W=%d h=%d w=%d (needs 2 <= h <= H, 2 <= w <= W)", H, W, h, w);
    if ((int64_t)B * 2 * H * W >= 0x80000000LL || B > 65535 || (H + kTH - 1) / kTH > 65535)
        PWC_FAIL(PWC_EINVAL, "pwc_fb_metrics: needs B*2*H*W < 2^31, B <= 65535 and H <= 16 * 65535");
    if (flow12_bstride < 2LL * h * w || (flow21 && flow21_bstride < 2LL * h * w))
        PWC_FAIL(PWC_EINVAL, "pwc_fb_metrics: batch stride smaller than the tensor");
    if (pwc::misaligned({flow12, flow21, out2}))
        PWC_FAIL(PWC_EINVAL, "pwc_fb_metrics: needs 4-byte aligned operands");
    const int64_t need = pwc_fb_metrics_workspace_bytes(B, H, W);
    if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u))
        PWC_FAIL(PWC_EINVAL, "pwc_fb_metrics: workspace needs %lld bytes, 8-byte aligned", (long long)need);
    Geo g;
    static_cast<pwc::UpGeo &>(g) = pwc::up_geo_make(H, W, h, w);
    g.B = B;
    g.tiles_x = (W + kTW - 1) / kTW;
    g.tiles_y = (H + kTH - 1) / kTH;
    g.bs12 = flow12_bstride;
    g.bs21 = flow21_bstride;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Rec *ws = static_cast<Rec *>(workspace);
    const int64_t nblk = (int64_t)g.tiles_x * g.tiles_y * B;
    hipLaunchKernelGGL(fb_tile_kernel, dim3(g.tiles_x, g.tiles_y, B), dim3(kThreads), 0, st, static_cast<const float *>(flow12),
                       static_cast<const float *>(flow21), ws + 1, g);
    hipLaunchKernelGGL(fb_finish_kernel, dim3(1), dim3(kThreads), 0, st, ws, nblk, flow21 ? 1 : 0, (double)B * 2 * H * W,
                       (double)B * H * W, static_cast<float *>(out2));
    return pwc::check_launch("fb_tile_kernel");
}
