// KITTI scoring on the device (reference inference_kitti.py:94-128 epe_metric / fl_all_metric, inference.py:105-159 compute_epe /
// compute_fl): the network's quarter-resolution flow goes straight to per-sample {sum of EPE, #valid, #outliers}; no full-resolution
// flow is written unless the caller asks for it.  Per output pixel (b, y, x), fp32 with no contraction (include/pwc_hip.h):
//   pred  = crop_up_flow(flow_q[b], y, x)          pwc_flow_up.h: exactly what pwc_flow_upsample_f32 writes at that pixel
//   gt    = float planes + uint8 validity, or the KITTI PNG samples (uint16 R, G, B): u = (R - 32768) / 64, v alike, valid = B != 0
//   epe   = sqrt(du^2 + dv^2);  mag = sqrt(gu^2 + gv^2);  outlier = epe > max(3, 0.05 * mag)
//
// Work split as in pwc_fb_metrics.hip: one workgroup = one 16 x 64 tile of one sample, 256 lanes, each owning the column tid % 64 of
// the rows tid / 64 + 4 k.  The quarter-resolution taps of a tile are a 5 x 17 window that hits L1 after the first row.  A row of the
// uint16 ground truth is 6 W bytes and so only 2-byte aligned in general: each lane reads its pixel's three samples as 2-byte loads (a
// wave's 64 pixels are 384 contiguous bytes; the three loads share the same cache lines).  Each workgroup leaves {fp64 sum, int64
// valid, int64 outliers} (fixed tree order) in the workspace; one final workgroup per sample adds that sample's tiles in tile order.
// No atomics: the result is bit-reproducible.
#include "pwc_block_reduce.h"
#include "pwc_common.h"
#include "pwc_flow_up.h"

namespace {

constexpr int kTH = 16, kTW = 64, kThreads = 256;
constexpr int kRowStep = kThreads / kTW;      // 4
constexpr int kPix = kTH / kRowStep;          // 4 pixels per lane
using Rec = pwc::TilePartial<2>;               // {double sum_epe, int64 {valid, outliers}}: workspace = one per sample, then one per tile

struct Geo {
    pwc::CropUp up;
    int H, W, tiles_x, tiles_y;
    int64_t bsq;
};

template <int KIND, bool WRITE>
__global__ __launch_bounds__(kThreads) void score_tile_kernel(const float *__restrict__ flow_q, const void *__restrict__ gt,
                                                              const uint8_t *__restrict__ valid, float *__restrict__ flow_out,
                                                              Rec *__restrict__ part, Geo g) {
    __shared__ pwc::TreeLds<kThreads, 1, 2> red;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int col = tid % kTW, row0 = tid / kTW;
    const float *q = flow_q + (int64_t)b * g.bsq;
    const int64_t npix = (int64_t)g.H * g.W;
    double sum = 0.0;
    long long cnt[2] = {0, 0};                 // valid, outliers
    const int x = blockIdx.x * kTW + col;
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        const int y = blockIdx.y * kTH + row0 + k * kRowStep;
        if (y >= g.H || x >= g.W) continue;
        const float2 pred = pwc::crop_up_flow(q, g.up, y, x);
        const int64_t pix = (int64_t)y * g.W + x;
        if (WRITE) {
            flow_out[(int64_t)b * 2 * npix + pix] = pred.x;
            flow_out[((int64_t)b * 2 + 1) * npix + pix] = pred.y;
        }
        float gu, gv;
        bool ok;
        if (KIND == 1) {
            const uint16_t *s = static_cast<const uint16_t *>(gt) + ((int64_t)b * npix + pix) * 3;
            gu = ((float)s[0] - 32768.0f) / 64.0f;
            gv = ((float)s[1] - 32768.0f) / 64.0f;
            ok = s[2] != 0;
        } else {
            const float *f = static_cast<const float *>(gt) + (int64_t)b * 2 * npix + pix;
            gu = f[0];
            gv = f[npix];
            ok = valid ? valid[(int64_t)b * npix + pix] != 0 : true;
        }
        if (!ok) continue;
        const float du = pred.x - gu, dv = pred.y - gv;
        const float epe = sqrtf(du * du + dv * dv);
        const float mag = sqrtf(gu * gu + gv * gv);
        sum += (double)epe;
        ++cnt[0];
        if (epe > fmaxf(3.0f, 0.05f * mag)) ++cnt[1];
    }
    pwc::tree_sum(red, &sum, cnt);
    if (tid == 0) {
        const int64_t lin = blockIdx.x + (int64_t)g.tiles_x * (blockIdx.y + (int64_t)g.tiles_y * blockIdx.z);
        part[lin] = Rec{sum, {cnt[0], cnt[1]}};
    }
}

// workgroup b adds the tiles of sample b in tile order
__global__ __launch_bounds__(kThreads) void score_finish_kernel(Rec *__restrict__ ws, int n, int64_t tiles, float *__restrict__ out) {
    __shared__ pwc::TreeLds<kThreads, 1, 2> red;
    const int tid = threadIdx.x, b = blockIdx.x;
    const Rec *part = ws + n + (int64_t)b * tiles;
    double s = 0.0;
    long long cnt[2] = {0, 0};
    for (int64_t i = tid; i < tiles; i += kThreads) {
        s += part[i].sum;
        cnt[0] += part[i].count[0];
        cnt[1] += part[i].count[1];
    }
    pwc::tree_sum(red, &s, cnt);
    if (tid == 0) {
        ws[b] = Rec{s, {cnt[0], cnt[1]}};
        const long long nv = cnt[0], no = cnt[1];
        const float nan = __builtin_nanf("");
        out[2 * b] = nv ? (float)(s / (double)nv) : nan;
        out[2 * b + 1] = nv ? (float)(100.0 * (double)no / (double)nv) : nan;
    }
}

}  // namespace

extern "C" int64_t pwc_kitti_score_workspace_bytes(int n, int out_h, int out_w) {
    if (n <= 0 || out_h <= 0 || out_w <= 0) return -1;
    return (int64_t)sizeof(Rec) * n * (1 + (int64_t)((out_h + kTH - 1) / kTH) * ((out_w + kTW - 1) / kTW));
}

extern "C" int pwc_kitti_score(const void *flow_q, int n, int Hq, int Wq, int crop_h, int crop_w, int out_h, int out_w, int64_t q_bstride,
                               const void *gt, int gt_kind, const void *valid, void *flow_out, void *workspace, int64_t workspace_bytes,
                               void *out, void *stream) {
    if (!flow_q || !gt || !workspace || !out) PWC_FAIL(PWC_EINVAL, "pwc_kitti_score: null pointer");
    if (n <= 0 || Hq <= 0 || Wq <= 0 || crop_h <= 0 || crop_w <= 0 || out_h <= 0 || out_w <= 0)
        PWC_FAIL(PWC_EINVAL, "pwc_kitti_score: bad shape n=%d Hq=%d Wq=%d crop=%dx%d out=%dx%d", n, Hq, Wq, crop_h, crop_w, out_h, out_w);
    if (crop_h > Hq || crop_w > Wq)
        PWC_FAIL(PWC_EINVAL, "pwc_kitti_score: crop %dx%d larger than the map %dx%d", crop_h, crop_w, Hq, Wq);
    if (q_bstride < (int64_t)2 * Hq * Wq) PWC_FAIL(PWC_EINVAL, "pwc_kitti_score: batch stride smaller than the tensor");
    if (gt_kind != 0 && gt_kind != 1) PWC_FAIL(PWC_EINVAL, "pwc_kitti_score: unknown gt_kind %d (0 = float planes, 1 = uint16 RGB)", gt_kind);
    if (gt_kind == 1 && valid) PWC_FAIL(PWC_EINVAL, "pwc_kitti_score: valid must be NULL with gt_kind 1 (the blue sample is the validity)");
    if ((int64_t)n * 2 * out_h * out_w >= 0x80000000LL || n > 65535 || (out_h + kTH - 1) / kTH > 65535)
        PWC_FAIL(PWC_EINVAL, "pwc_kitti_score: needs n*2*out_h*out_w < 2^31, n <= 65535 and out_h <= 16 * 65535");
    const int64_t need = pwc_kitti_score_workspace_bytes(n, out_h, out_w);
    if (workspace_bytes < need) PWC_FAIL(PWC_EINVAL, "pwc_kitti_score: workspace needs %lld bytes, got %lld", (long long)need, (long long)workspace_bytes);
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) PWC_FAIL(PWC_EALIGN, "pwc_kitti_score: workspace must be 8-byte aligned");
    if (pwc::misaligned({flow_q, flow_out, out}) || pwc::misaligned({gt}, gt_kind == 1 ? 2 : 4))
        PWC_FAIL(PWC_EALIGN, "pwc_kitti_score: needs 4-byte aligned float operands and a 2-byte aligned uint16 ground truth");
    Geo g;
    g.up = pwc::crop_up_make(Hq, Wq, crop_h, crop_w, out_h, out_w);
    g.H = out_h; g.W = out_w;
    g.tiles_x = (out_w + kTW - 1) / kTW;
    g.tiles_y = (out_h + kTH - 1) / kTH;
    g.bsq = q_bstride;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Rec *ws = static_cast<Rec *>(workspace);
    const dim3 grid(g.tiles_x, g.tiles_y, n), block(kThreads);
    const float *fq = static_cast<const float *>(flow_q);
    const uint8_t *vd = static_cast<const uint8_t *>(valid);
    float *fo = static_cast<float *>(flow_out);
    Rec *part = ws + n;
    if (gt_kind == 1) {
        if (fo) hipLaunchKernelGGL((score_tile_kernel<1, true>), grid, block, 0, st, fq, gt, vd, fo, part, g);
        else hipLaunchKernelGGL((score_tile_kernel<1, false>), grid, block, 0, st, fq, gt, vd, fo, part, g);
    } else {
        if (fo) hipLaunchKernelGGL((score_tile_kernel<0, true>), grid, block, 0, st, fq, gt, vd, fo, part, g);
        else hipLaunchKernelGGL((score_tile_kernel<0, false>), grid, block, 0, st, fq, gt, vd, fo, part, g);
    }
    hipLaunchKernelGGL(score_finish_kernel, dim3(n), block, 0, st, ws, n, (int64_t)g.tiles_x * g.tiles_y, static_cast<float *>(out));
    return pwc::check_launch("score_tile_kernel");
}
