// Supervised flow losses of the reference's fine-tuning scripts train.py / train2.py, forward and backward w.r.t. the predicted
// flows.
//
// Full-resolution Charbonnier / EPE of an upsampled flow (train.py:31-48 + :69-72, train2.py:100-122 + :202-213):
//   up    = interpolate(pred, (H,W), bilinear, align_corners=False) * (W/w, H/h)          (pred itself when (h,w) == (H,W))
//   epe   = sqrt(|up - gt|^2 + eps^2)
//   rule 0 (MaskedCharbonnier): loss = sum(epe * [m > 0.5]) / max(sum [m > 0.5], 1)
//   rule 1 (compute_epe, eps 0): loss = sum(epe * m) / (sum m + 1e-8)                     (no mask: the mean, either rule)
// The forward samples pred on the fly (the upsampled flow is never written).  The backward gathers into each low-resolution
// pixel the full-resolution pixels whose align_corners=False taps use it, separably: a row pass sums along X into
// rows[B][2][H][w] (fp64, workspace), computing the full-resolution gradient on the fly; a column pass sums along Y.
//
// Multiscale loss (train2.py:124-167), all levels in one launch, tiles flattened across levels.  Level l (pred [B,2,h,w]):
//   gt_s   = interpolate(gt, (h,w), bilinear, align_corners=False) / (W/w, H/h)   -- 4 taps of the full-resolution GT per pixel
//   mask_s = interpolate(mask, (h,w), nearest)                                     -- raw values
//   charb  = sum(sqrt(|pred - gt_s|^2 + eps^2) * [mask_s > 0.5]) / max(sum [mask_s > 0.5], 1)
//   photo  = sum_c |im1_s - grid_sample(im2_s, x + pred, zeros, align_corners=True)| * mask_s / (sum mask_s + 1e-8)
//   smooth = mean(|dx pred| * exp(-mean_c |dx im1_s|)) + mean(|dy pred| * exp(-mean_c |dy im1_s|))
//   total  = sum_l w_l (charb + lambda_photo * photo + lambda_smooth * smooth)
// im1_s / im2_s (bilinear, align_corners=False) are written to the workspace by a resize launch only when a lambda is > 0.
// The backward is elementwise per prediction pixel: w_l g / den_l times the Charbonnier slope, the bilinear slope of the
// zero-padded im2_s at the sample point, and the 3-tap stencil of the smoothness term.
//
// torch's index arithmetic, in fp32 (the library is built with -ffp-contract=off):
//   bilinear, align_corners=False: scale = (float)in / (float)out;  s = max(scale * ((float)dst + 0.5) - 0.5, 0);  i0 = (int)s;
//     i1 = i0 + (i0 < in-1);  l1 = s - i0;  l0 = 1 - l1;  v = l0 (l0x a00 + l1x a01) + l1 (l0x a10 + l1x a11)
//   nearest: min((int)floorf((float)dst * ((float)in / (float)out)), in-1)
//
// Reductions: per-workgroup fp64 partials in a fixed tree order, then one workgroup adds them in workgroup order.  No float
// atomics: every result is bit-reproducible.
#include "pwc_block_reduce.h"
#include "pwc_common.h"

namespace {

constexpr int kThreads = 256, kPer = 4, kChunk = kThreads * kPer;   // 1024 pixels per workgroup (lane t: t + 256 k)
constexpr int kMaxLevels = 8;
constexpr int kImgC = 3;                                             // images [B,6,H,W] = (im1, im2), train2.py:139

struct Lin {
    int i0, i1;
    float l0, l1;
};

// torch's area_pixel_compute_source_index (align_corners=False) and the taps of upsample_bilinear2d
__device__ __forceinline__ Lin src_linear(float scale, int dst, int n_in) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    Lin r;
    r.i0 = (int)s;
    r.i1 = r.i0 + (r.i0 < n_in - 1 ? 1 : 0);
    r.l1 = s - (float)r.i0;
    r.l0 = 1.0f - r.l1;
    return r;
}

__device__ __forceinline__ int src_nearest(float scale, int dst, int n_in) {
    const int s = (int)floorf((float)dst * scale);
    return s < n_in - 1 ? s : n_in - 1;
}

__device__ __forceinline__ float interp(const float *p, int ld, const Lin &ly, const Lin &lx) {
    const float *r0 = p + (int64_t)ly.i0 * ld, *r1 = p + (int64_t)ly.i1 * ld;
    return ly.l0 * (lx.l0 * r0[lx.i0] + lx.l1 * r0[lx.i1]) + ly.l1 * (lx.l0 * r1[lx.i0] + lx.l1 * r1[lx.i1]);
}

using pwc::misaligned;
using pwc::mask_val;

__device__ __forceinline__ float sgn(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

// ------------------------------------------------------------------------------------------------ full-resolution loss
struct FlowArgs {
    const float *pred, *gt;
    const void *mask;
    int mask_u8, rule;
    float eps2;
    int B, H, W, h, w;
    float rh, rw;            // (float)h / H, (float)w / W: upsampling source scales
    float vx, vy;            // (float)(W / w), (float)(H / h): vector scales
    int64_t bs_p, bs_g, bs_m;
    double *part;            // [nblk][2]
    const float *fwd_out;    // {loss, den} (backward)
    const float *gout;       // {g_loss, g_den} (backward; g_den is ignored)
    double *rows;            // [B][2][H][w] (backward)
    float *gpred;            // [B][2][h][w] dense (backward)
};

struct Up {
    float du, dv, epe, m;
};

// upsampled prediction minus GT at full-resolution pixel (Y, X) of image b, its Charbonnier and its mask weight (rule applied)
__device__ __forceinline__ Up flow_pixel(const FlowArgs &a, int b, int Y, int X) {
    const Lin ly = src_linear(a.rh, Y, a.h), lx = src_linear(a.rw, X, a.w);
    const float *p = a.pred + (int64_t)b * a.bs_p;
    const int64_t lp = (int64_t)a.h * a.w, plane = (int64_t)a.H * a.W, q = (int64_t)Y * a.W + X;
    const float u = interp(p, a.w, ly, lx) * a.vx;
    const float v = interp(p + lp, a.w, ly, lx) * a.vy;
    const float *g = a.gt + (int64_t)b * a.bs_g + q;
    Up r;
    r.du = u - g[0];
    r.dv = v - g[plane];
    r.epe = sqrtf(r.du * r.du + r.dv * r.dv + a.eps2);
    const float mv = mask_val(a.mask, a.mask_u8, (int64_t)b * a.bs_m + q);
    r.m = a.rule == 0 ? (mv > 0.5f ? 1.0f : 0.0f) : mv;
    return r;
}

__global__ __launch_bounds__(kThreads) void flow_fwd_kernel(FlowArgs a) {
    __shared__ pwc::TreeLds<kThreads, 2> red;
    const int64_t plane = (int64_t)a.H * a.W, tot = (int64_t)a.B * plane;
    double v[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int64_t e = (int64_t)blockIdx.x * kChunk + k * kThreads + threadIdx.x;
        if (e < tot) {
            const int b = (int)(e / plane);
            const int64_t q = e - (int64_t)b * plane;
            const int Y = (int)(q / a.W), X = (int)(q - (int64_t)Y * a.W);
            const Up r = flow_pixel(a, b, Y, X);
            v[0] += (double)(r.epe * r.m);
            v[1] += (double)r.m;
        }
    }
    pwc::tree_sum(red, v, nullptr);
    if (threadIdx.x == 0) {
        a.part[blockIdx.x * 2] = v[0];
        a.part[blockIdx.x * 2 + 1] = v[1];
    }
}

__global__ __launch_bounds__(kThreads) void flow_finish_kernel(const double *part, int64_t nblk, int masked, int rule, float *out) {
    __shared__ pwc::TreeLds<kThreads, 2> red;
    double v[2] = {0.0, 0.0};
    for (int64_t i = threadIdx.x; i < nblk; i += kThreads) {
        v[0] += part[i * 2];
        v[1] += part[i * 2 + 1];
    }
    pwc::tree_sum(red, v, nullptr);
    if (threadIdx.x == 0) {
        // the mask sum is a float32 sum in the reference; +1e-8 in fp32 as well (rule 1), max(., 1) (rule 0)
        const float s = (float)v[1];
        const float den = !masked ? s : (rule == 0 ? (s > 1.0f ? s : 1.0f) : s + 1e-8f);
        out[0] = (float)(v[0] / (double)den);
        out[1] = den;
    }
}

// full-resolution indices Y whose align_corners=False taps use low-resolution index i: i0(Y) in {i-1, i}; i0 is non-decreasing
__device__ __forceinline__ int first_user(int i, float scale, int n_out, int n_in) {
    int Y = (int)floorf(((float)i - 0.5f) / scale - 0.5f) - 2;   // within a few ulps of the answer; walked to the exact one
    Y = Y < 0 ? 0 : (Y > n_out ? n_out : Y);
    while (Y > 0 && src_linear(scale, Y - 1, n_in).i0 >= i - 1) --Y;
    while (Y < n_out && src_linear(scale, Y, n_in).i0 < i - 1) ++Y;
    return Y;
}
__device__ __forceinline__ float user_weight(const Lin &l, int i) {
    return (l.i0 == i ? l.l0 : 0.0f) + (l.i1 == i ? l.l1 : 0.0f);
}

// row pass: rows[b][c][Y][j] = sum_X wx(X, j) * m * d_c / epe over the X that use column j (fixed order, fp64)
__global__ __launch_bounds__(kThreads) void flow_rows_kernel(FlowArgs a) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t per_b = (int64_t)a.H * a.w;
    if (e >= (int64_t)a.B * per_b) return;
    const int b = (int)(e / per_b);
    const int64_t r = e - (int64_t)b * per_b;
    const int Y = (int)(r / a.w), j = (int)(r - (int64_t)Y * a.w);
    double s0 = 0.0, s1 = 0.0;
    for (int X = first_user(j, a.rw, a.W, a.w); X < a.W; ++X) {
        const Lin lx = src_linear(a.rw, X, a.w);
        if (lx.i0 > j) break;
        const float wx = user_weight(lx, j);
        const Up u = flow_pixel(a, b, Y, X);
        if (u.m != 0.0f) {
            const float gm = u.m / u.epe;
            s0 += (double)wx * (double)(gm * u.du);
            s1 += (double)wx * (double)(gm * u.dv);
        }
    }
    double *o = a.rows + (int64_t)b * 2 * per_b + r;
    o[0] = s0;
    o[per_b] = s1;
}

// column pass: grad_pred[b][c][i][j] = g / den * scale_c * sum_Y wy(Y, i) rows[b][c][Y][j]
__global__ __launch_bounds__(kThreads) void flow_cols_kernel(FlowArgs a) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t lp = (int64_t)a.h * a.w;
    if (e >= (int64_t)a.B * lp) return;
    const int b = (int)(e / lp);
    const int64_t q = e - (int64_t)b * lp;
    const int i = (int)(q / a.w), j = (int)(q - (int64_t)i * a.w);
    const int64_t per_b = (int64_t)a.H * a.w;
    const double *rw = a.rows + (int64_t)b * 2 * per_b + j;
    double s0 = 0.0, s1 = 0.0;
    for (int Y = first_user(i, a.rh, a.H, a.h); Y < a.H; ++Y) {
        const Lin ly = src_linear(a.rh, Y, a.h);
        if (ly.i0 > i) break;
        const double wy = user_weight(ly, i);
        s0 += wy * rw[(int64_t)Y * a.w];
        s1 += wy * rw[per_b + (int64_t)Y * a.w];
    }
    const float gs = a.gout[0] / a.fwd_out[1];
    float *o = a.gpred + (int64_t)b * 2 * lp + q;
    o[0] = gs * ((float)s0 * a.vx);
    o[lp] = gs * ((float)s1 * a.vy);
}

// ------------------------------------------------------------------------------------------------ multiscale loss
struct Level {
    const float *pred;
    float *grad;             // backward: [B][2][h][w] dense
    int64_t bs_p;
    int h, w;
    float sh, sw;            // (float)H / h, (float)W / w: bilinear and nearest source scales
    float ivx, ivy;          // 1 / (float)(W / w), 1 / (float)(H / h): torch divides by a CPU scalar as a * (1 / b)
    float weight;
    int64_t blk0, nblk;      // workgroups of the level in the flattened grid
    int64_t ims;             // float offset of im_s [B][6][h][w] in the image area of the workspace
};

struct MsArgs {
    Level lv[kMaxLevels];
    int L;
    const float *gt, *img;
    const void *mask;
    int mask_u8;
    int B, H, W;
    int64_t bs_g, bs_m, bs_i;
    float eps2, lp, ls;
    float *ims;              // resized images (lambda_photo > 0 or lambda_smooth > 0)
    double *part;            // [nblk][6]
    const float *fwd_out;    // backward: {total, lvl[L], den_c[L], den_p[L]}
    const float *gout;       // backward: g_total (the other entries get no gradient)
};

__device__ __forceinline__ int level_of(const MsArgs &a, int64_t blk) {
    int l = 0;
    while (l + 1 < a.L && blk >= a.lv[l + 1].blk0) ++l;
    return l;
}

// im_s of every level: interpolate(images, (h,w), bilinear, align_corners=False); blockIdx.y = level
__global__ __launch_bounds__(kThreads) void ms_resize_kernel(MsArgs a) {
    const Level &v = a.lv[blockIdx.y];
    const int64_t lp = (int64_t)v.h * v.w, n = (int64_t)a.B * 2 * kImgC * lp;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const int64_t bc = e / lp, q = e - bc * lp;
    const int b = (int)(bc / (2 * kImgC)), c = (int)(bc - (int64_t)b * 2 * kImgC);
    const int y = (int)(q / v.w), x = (int)(q - (int64_t)y * v.w);
    const Lin ly = src_linear(v.sh, y, a.H), lx = src_linear(v.sw, x, a.W);
    a.ims[v.ims + e] = interp(a.img + (int64_t)b * a.bs_i + (int64_t)c * a.H * a.W, a.W, ly, lx);
}

// grid_sample(bilinear, zeros, align_corners=True) of plane p [h][w] at (ix, iy); slope = d/d(ix), d/d(iy)
__device__ __forceinline__ float sample_zeros(const float *p, int h, int w, float ix, float iy, float2 *slope) {
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const float tx = ix - fx, ty = iy - fy;
    const bool bx0 = x0 >= 0 && x0 < w, bx1 = x1 >= 0 && x1 < w, by0 = y0 >= 0 && y0 < h, by1 = y1 >= 0 && y1 < h;
    const float v00 = (by0 && bx0) ? p[y0 * w + x0] : 0.0f;
    const float v01 = (by0 && bx1) ? p[y0 * w + x1] : 0.0f;
    const float v10 = (by1 && bx0) ? p[y1 * w + x0] : 0.0f;
    const float v11 = (by1 && bx1) ? p[y1 * w + x1] : 0.0f;
    if (slope) {
        slope->x = (1.0f - ty) * (v01 - v00) + ty * (v11 - v10);
        slope->y = (1.0f - tx) * (v10 - v00) + tx * (v11 - v01);
    }
    return (1.0f - ty) * ((1.0f - tx) * v00 + tx * v01) + ty * ((1.0f - tx) * v10 + tx * v11);
}

// exp(-mean_c |im1_s(c, y, x) - im1_s(c, y + dy, x + dx)|) (train2.py:89-94; imgs[:, :3] of im1_s is all of it)
__device__ __forceinline__ float edge_weight(const float *im1, int64_t lp, int64_t q, int64_t d) {
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < kImgC; ++c) s += fabsf(im1[c * lp + q] - im1[c * lp + q + d]);
    return expf(-(s / (float)kImgC));
}

struct MsPix {
    int b, y, x;
    int64_t q;               // y * w + x
};

__device__ __forceinline__ bool ms_pixel(const MsArgs &a, const Level &v, int64_t e, MsPix &p) {
    const int64_t lp = (int64_t)v.h * v.w;
    if (e >= (int64_t)a.B * lp) return false;
    p.b = (int)(e / lp);
    p.q = e - (int64_t)p.b * lp;
    p.y = (int)(p.q / v.w);
    p.x = (int)(p.q - (int64_t)p.y * v.w);
    return true;
}

// GT at the level (bilinear downsample, vectors rescaled) and the raw nearest mask
__device__ __forceinline__ void level_gt(const MsArgs &a, const Level &v, const MsPix &p, float &gu, float &gv, float &m) {
    const Lin ly = src_linear(v.sh, p.y, a.H), lx = src_linear(v.sw, p.x, a.W);
    const float *g = a.gt + (int64_t)p.b * a.bs_g;
    gu = interp(g, a.W, ly, lx) * v.ivx;
    gv = interp(g + (int64_t)a.H * a.W, a.W, ly, lx) * v.ivy;
    const int my = src_nearest(v.sh, p.y, a.H), mx = src_nearest(v.sw, p.x, a.W);
    m = mask_val(a.mask, a.mask_u8, (int64_t)p.b * a.bs_m + (int64_t)my * a.W + mx);
}

__global__ __launch_bounds__(kThreads) void ms_fwd_kernel(MsArgs a) {
    __shared__ pwc::TreeLds<kThreads, 6> red;
    const int l = level_of(a, blockIdx.x);
    const Level &v = a.lv[l];
    const int64_t lp = (int64_t)v.h * v.w;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int k = 0; k < kPer; ++k) {
        MsPix p;
        if (!ms_pixel(a, v, ((int64_t)blockIdx.x - v.blk0) * kChunk + k * kThreads + threadIdx.x, p)) continue;
        const float *f = v.pred + (int64_t)p.b * v.bs_p;
        const float fu = f[p.q], fv = f[lp + p.q];
        float gu, gv, m;
        level_gt(a, v, p, gu, gv, m);
        const float du = fu - gu, dv = fv - gv;
        const float epe = sqrtf(du * du + dv * dv + a.eps2);
        const float valid = m > 0.5f ? 1.0f : 0.0f;
        s[0] += (double)(epe * valid);
        s[1] += (double)valid;
        if (a.lp > 0.0f || a.ls > 0.0f) {
            const float *im1 = a.ims + v.ims + (int64_t)p.b * 2 * kImgC * lp, *im2 = im1 + kImgC * lp;
            if (a.lp > 0.0f) {
                const float ix = (float)p.x + fu, iy = (float)p.y + fv;
                float ph = 0.0f;
#pragma unroll
                for (int c = 0; c < kImgC; ++c)
                    ph += fabsf(im1[c * lp + p.q] - sample_zeros(im2 + c * lp, v.h, v.w, ix, iy, nullptr)) * m;
                s[2] += (double)ph;
                s[3] += (double)m;
            }
            if (a.ls > 0.0f) {
                if (p.x < v.w - 1)
                    s[4] += (double)((fabsf(fu - f[p.q + 1]) + fabsf(fv - f[lp + p.q + 1])) * edge_weight(im1, lp, p.q, 1));
                if (p.y < v.h - 1)
                    s[5] += (double)((fabsf(fu - f[p.q + v.w]) + fabsf(fv - f[lp + p.q + v.w])) * edge_weight(im1, lp, p.q, v.w));
            }
        }
    }
    pwc::tree_sum(red, s, nullptr);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a.part[blockIdx.x * 6 + k] = s[k];
    }
}

__global__ __launch_bounds__(kThreads) void ms_finish_kernel(MsArgs a, float *out) {
    __shared__ pwc::TreeLds<kThreads, 6> red;
    double total = 0.0;
    for (int l = 0; l < a.L; ++l) {
        const Level &v = a.lv[l];
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t i = threadIdx.x; i < v.nblk; i += kThreads)
#pragma unroll
            for (int k = 0; k < 6; ++k) s[k] += a.part[(v.blk0 + i) * 6 + k];
        pwc::tree_sum(red, s, nullptr);
        if (threadIdx.x == 0) {
            const float sc = (float)s[1], sp = (float)s[3];
            const float den_c = sc > 1.0f ? sc : 1.0f;    // valid.sum().clamp(min=1.0)
            const float den_p = sp + 1e-8f;                // mask.sum() + 1e-8
            double lvl = s[0] / (double)den_c;
            if (a.lp > 0.0f) lvl += (double)a.lp * (s[2] / (double)den_p);
            if (a.ls > 0.0f) {
                const double nx = (double)a.B * 2 * v.h * (v.w - 1), ny = (double)a.B * 2 * (v.h - 1) * v.w;
                lvl += (double)a.ls * (s[4] / nx + s[5] / ny);
            }
            total += (double)v.weight * lvl;
            out[1 + l] = (float)lvl;
            out[1 + a.L + l] = den_c;
            out[1 + 2 * a.L + l] = den_p;
        }
    }
    if (threadIdx.x == 0) out[0] = (float)total;
}

__global__ __launch_bounds__(kThreads) void ms_bwd_kernel(MsArgs a) {
    const int l = level_of(a, blockIdx.x);
    const Level &v = a.lv[l];
    const int64_t lp = (int64_t)v.h * v.w;
    const float g = a.gout[0] * v.weight;
    const float gc = g / a.fwd_out[1 + a.L + l];
    const float gp = g * a.lp / a.fwd_out[1 + 2 * a.L + l];
    const float gsx = g * a.ls / (float)((double)a.B * 2 * v.h * (v.w - 1));
    const float gsy = g * a.ls / (float)((double)a.B * 2 * (v.h - 1) * v.w);
#pragma unroll 1
    for (int k = 0; k < kPer; ++k) {
        MsPix p;
        if (!ms_pixel(a, v, ((int64_t)blockIdx.x - v.blk0) * kChunk + k * kThreads + threadIdx.x, p)) continue;
        const float *f = v.pred + (int64_t)p.b * v.bs_p;
        const float fu = f[p.q], fv = f[lp + p.q];
        float gu, gv, m;
        level_gt(a, v, p, gu, gv, m);
        const float du = fu - gu, dv = fv - gv;
        const float epe = sqrtf(du * du + dv * dv + a.eps2);
        float ou = 0.0f, ov = 0.0f;
        if (m > 0.5f) {
            ou = gc * (du / epe);
            ov = gc * (dv / epe);
        }
        if (a.lp > 0.0f || a.ls > 0.0f) {
            const float *im1 = a.ims + v.ims + (int64_t)p.b * 2 * kImgC * lp, *im2 = im1 + kImgC * lp;
            if (a.lp > 0.0f && m != 0.0f) {
                const float ix = (float)p.x + fu, iy = (float)p.y + fv;
                float tu = 0.0f, tv = 0.0f;
#pragma unroll
                for (int c = 0; c < kImgC; ++c) {
                    float2 sl;
                    const float wv = sample_zeros(im2 + c * lp, v.h, v.w, ix, iy, &sl);
                    const float gw = -sgn(im1[c * lp + p.q] - wv) * m;   // d|im1 - warped| / d warped, times the mask
                    tu += gw * sl.x;
                    tv += gw * sl.y;
                }
                ou += gp * tu;
                ov += gp * tv;
            }
            if (a.ls > 0.0f) {
                float tx[2] = {0.0f, 0.0f}, ty[2] = {0.0f, 0.0f};
                const float ex = p.x < v.w - 1 ? edge_weight(im1, lp, p.q, 1) : 0.0f;
                const float exl = p.x > 0 ? edge_weight(im1, lp, p.q - 1, 1) : 0.0f;
                const float ey = p.y < v.h - 1 ? edge_weight(im1, lp, p.q, v.w) : 0.0f;
                const float eyu = p.y > 0 ? edge_weight(im1, lp, p.q - v.w, v.w) : 0.0f;
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const float *fp = f + ch * lp;
                    const float fc = fp[p.q];
                    if (p.x < v.w - 1) tx[ch] += sgn(fc - fp[p.q + 1]) * ex;
                    if (p.x > 0) tx[ch] -= sgn(fp[p.q - 1] - fc) * exl;
                    if (p.y < v.h - 1) ty[ch] += sgn(fc - fp[p.q + v.w]) * ey;
                    if (p.y > 0) ty[ch] -= sgn(fp[p.q - v.w] - fc) * eyu;
                }
                ou += gsx * tx[0] + gsy * ty[0];
                ov += gsx * tx[1] + gsy * ty[1];
            }
        }
        float *o = v.grad + (int64_t)p.b * 2 * lp + p.q;
        o[0] = ou;
        o[lp] = ov;
    }
}

// ------------------------------------------------------------------------------------------------ host side
int64_t blocks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }
int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

int64_t flow_fwd_bytes(int B, int H, int W) { return align256(blocks_of((int64_t)B * H * W) * 2 * 8); }
int64_t flow_bwd_bytes(int B, int H, int w) { return align256((int64_t)B * 2 * H * w * 8); }

bool geometry_ok(int H, int W, int h, int w) { return h >= 2 && w >= 2 && h <= H && w <= W; }

int check_flow_args(const char *who, const void *pred, const void *gt, const void *mask, int mask_u8, int rule, const void *out,
                    const void *workspace, int64_t workspace_bytes, int64_t need, int B, int H, int W, int h, int w, double eps,
                    int64_t bs_p, int64_t bs_g, int64_t bs_m) {
    if (!pred || !gt || !out || !workspace) PWC_FAIL(PWC_EINVAL, "%s: null pointer", who);
    if (B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0)
        PWC_FAIL(PWC_EINVAL, "%s: bad shape B=%d H=%d W=%d h=%d w=%d", who, B, H, W, h, w);
    if (rule != 0 && rule != 1) PWC_FAIL(PWC_EINVAL, "%s: mask rule must be 0 (> 0.5, max(., 1)) or 1 (raw, + 1e-8)", who);
    if (!(eps >= 0.0)) PWC_FAIL(PWC_EINVAL, "%s: eps must be >= 0", who);
    const int64_t plane = (int64_t)H * W;
    if (bs_p < 2LL * h * w || bs_g < 2 * plane || (mask && bs_m < plane))
        PWC_FAIL(PWC_EINVAL, "%s: batch stride smaller than the tensor", who);
    if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u))
        PWC_FAIL(PWC_EINVAL, "%s: workspace needs %lld bytes, 8-byte aligned", who, (long long)need);
    if (!geometry_ok(H, W, h, w)) {
        pwc::set_error("%s: declined geometry H=%d W=%d h=%d w=%d (needs 2 <= h <= H, 2 <= w <= W)", who, H, W, h, w);
        return PWC_EUNSUPPORTED;
    }
    if (misaligned({pred, gt, out}) || (mask && !mask_u8 && misaligned({mask})) || 2 * plane >= 0x7fffffffLL || B > 65535) {
        pwc::set_error("%s: needs 4-byte aligned operands, 2*H*W < 2^31 and B <= 65535", who);
        return PWC_EUNSUPPORTED;
    }
    return PWC_OK;
}

FlowArgs make_flow_args(const void *pred, const void *gt, const void *mask, int mask_u8, int rule, int B, int H, int W, int h,
                        int w, double eps, int64_t bs_p, int64_t bs_g, int64_t bs_m) {
    FlowArgs a{};
    a.pred = static_cast<const float *>(pred);
    a.gt = static_cast<const float *>(gt);
    a.mask = mask;
    a.mask_u8 = mask_u8 ? 1 : 0;
    a.rule = rule;
    a.eps2 = (float)(eps * eps);             // self.eps ** 2, a Python float added to a float32 tensor
    a.B = B; a.H = H; a.W = W; a.h = h; a.w = w;
    a.rh = (float)h / (float)H;
    a.rw = (float)w / (float)W;
    a.vx = (float)((double)W / (double)w);
    a.vy = (float)((double)H / (double)h);
    a.bs_p = bs_p; a.bs_g = bs_g; a.bs_m = bs_m;
    return a;
}

// level table from the host arrays; returns PWC_OK, or fails with the reason
int make_levels(const char *who, MsArgs &a, const void *const *preds, const int64_t *pred_bstrides, const int *level_hw,
                const float *weights, void *const *grads, int L, int B, int H, int W) {
    if (L < 1 || !level_hw) PWC_FAIL(PWC_EINVAL, "%s: needs 1 or more levels and their sizes", who);
    if (L > kMaxLevels) {
        pwc::set_error("%s: %d levels, at most %d", who, L, kMaxLevels);
        return PWC_EUNSUPPORTED;
    }
    a.L = L;
    int64_t blk = 0, ims = 0;
    for (int l = 0; l < L; ++l) {
        Level &v = a.lv[l];
        v.h = level_hw[2 * l];
        v.w = level_hw[2 * l + 1];
        if (v.h <= 0 || v.w <= 0) PWC_FAIL(PWC_EINVAL, "%s: level %d has size %d x %d", who, l, v.h, v.w);
        if (preds) {
            if (!preds[l]) PWC_FAIL(PWC_EINVAL, "%s: null pointer (level %d)", who, l);
            v.pred = static_cast<const float *>(preds[l]);
            v.bs_p = pred_bstrides ? pred_bstrides[l] : 2LL * v.h * v.w;
            if (v.bs_p < 2LL * v.h * v.w) PWC_FAIL(PWC_EINVAL, "%s: level %d batch stride smaller than the tensor", who, l);
        }
        if (grads) {
            if (!grads[l]) PWC_FAIL(PWC_EINVAL, "%s: null pointer (gradient of level %d)", who, l);
            v.grad = static_cast<float *>(grads[l]);
        }
        v.weight = weights ? weights[l] : 0.0f;
        v.sh = (float)H / (float)v.h;
        v.sw = (float)W / (float)v.w;
        v.ivx = 1.0f / (float)((double)W / (double)v.w);
        v.ivy = 1.0f / (float)((double)H / (double)v.h);
        v.blk0 = blk;
        v.nblk = blocks_of((int64_t)B * v.h * v.w);
        v.ims = ims;
        blk += v.nblk;
        ims += (int64_t)B * 2 * kImgC * v.h * v.w;
    }
    return PWC_OK;
}

int64_t ms_part_bytes(const MsArgs &a) { return align256((a.lv[a.L - 1].blk0 + a.lv[a.L - 1].nblk) * 6 * 8); }
int64_t ms_img_bytes(const MsArgs &a) {
    const Level &v = a.lv[a.L - 1];
    return align256((v.ims + (int64_t)a.B * 2 * kImgC * v.h * v.w) * 4);
}

int check_ms_args(const char *who, MsArgs &a, const void *const *preds, const int64_t *pred_bstrides, const int *level_hw,
                  const float *weights, void *const *grads, int L, const void *gt, const void *mask, int mask_u8,
                  const void *images, const void *out, int B, int H, int W, double eps, float lambda_photo, float lambda_smooth,
                  int64_t bs_g, int64_t bs_m, int64_t bs_i, const void *workspace, int64_t workspace_bytes) {
    if (!preds || !weights || !gt || !out || !workspace) PWC_FAIL(PWC_EINVAL, "%s: null pointer", who);
    if (B <= 0 || H <= 0 || W <= 0) PWC_FAIL(PWC_EINVAL, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    if (!(eps >= 0.0) || !(lambda_photo >= 0.0f) || !(lambda_smooth >= 0.0f))
        PWC_FAIL(PWC_EINVAL, "%s: eps and the lambdas must be >= 0", who);
    const bool with_images = lambda_photo > 0.0f || lambda_smooth > 0.0f;
    if (with_images && !images) PWC_FAIL(PWC_EINVAL, "%s: null pointer (images, needed by lambda_photo / lambda_smooth > 0)", who);
    const int64_t plane = (int64_t)H * W;
    if (bs_g < 2 * plane || (mask && bs_m < plane) || (with_images && bs_i < 2 * kImgC * plane))
        PWC_FAIL(PWC_EINVAL, "%s: batch stride smaller than the tensor", who);
    a.gt = static_cast<const float *>(gt);
    a.img = static_cast<const float *>(images);
    a.mask = mask;
    a.mask_u8 = mask_u8 ? 1 : 0;
    a.B = B; a.H = H; a.W = W;
    a.bs_g = bs_g; a.bs_m = bs_m; a.bs_i = bs_i;
    a.eps2 = (float)(eps * eps);
    a.lp = lambda_photo;
    a.ls = lambda_smooth;
    const int rc = make_levels(who, a, preds, pred_bstrides, level_hw, weights, grads, L, B, H, W);
    if (rc != PWC_OK) return rc;
    const int64_t need = ms_part_bytes(a) + (with_images ? ms_img_bytes(a) : 0);
    if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u))
        PWC_FAIL(PWC_EINVAL, "%s: workspace needs %lld bytes, 8-byte aligned", who, (long long)need);
    for (int l = 0; l < L; ++l) {
        if (!geometry_ok(H, W, a.lv[l].h, a.lv[l].w)) {
            pwc::set_error("%s: declined geometry of level %d: H=%d W=%d h=%d w=%d (needs 2 <= h <= H, 2 <= w <= W)", who, l, H, W,
                           a.lv[l].h, a.lv[l].w);
            return PWC_EUNSUPPORTED;
        }
        if (misaligned({a.lv[l].pred}) || (grads && misaligned({a.lv[l].grad}))) {
            pwc::set_error("%s: level %d: needs 4-byte aligned operands", who, l);
            return PWC_EUNSUPPORTED;
        }
    }
    if (misaligned({gt, out}) || (images && misaligned({images})) || (mask && !mask_u8 && misaligned({mask})) ||
        2 * kImgC * plane >= 0x7fffffffLL || B > 65535) {
        pwc::set_error("%s: needs 4-byte aligned operands, 6*H*W < 2^31 and B <= 65535", who);
        return PWC_EUNSUPPORTED;
    }
    char *ws = static_cast<char *>(const_cast<void *>(workspace));
    a.part = reinterpret_cast<double *>(ws);
    a.ims = with_images ? reinterpret_cast<float *>(ws + ms_part_bytes(a)) : nullptr;
    return PWC_OK;
}

void launch_resize(const MsArgs &a, hipStream_t st) {
    int64_t most = 0;
    for (int l = 0; l < a.L; ++l) {
        const int64_t n = (int64_t)a.B * 2 * kImgC * a.lv[l].h * a.lv[l].w;
        most = n > most ? n : most;
    }
    hipLaunchKernelGGL(ms_resize_kernel, dim3((unsigned)((most + kThreads - 1) / kThreads), (unsigned)a.L), dim3(kThreads), 0, st,
                       a);
}

}  // namespace

extern "C" int64_t pwc_sup_flow_loss_workspace_bytes(int B, int H, int W, int h, int w, int backward) {
    if (B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return -1;
    const int64_t f = flow_fwd_bytes(B, H, W);
    if (!backward) return f;
    const int64_t b = flow_bwd_bytes(B, H, w);
    return f > b ? f : b;
}

extern "C" int pwc_sup_flow_loss_fwd(const void *pred, const void *gt, const void *mask, int mask_u8, int mask_rule, void *out,
                                     int B, int H, int W, int h, int w, double eps, int64_t pred_bstride, int64_t gt_bstride,
                                     int64_t mask_bstride, void *workspace, int64_t workspace_bytes, void *stream) {
    const int rc = check_flow_args("pwc_sup_flow_loss_fwd", pred, gt, mask, mask_u8, mask_rule, out, workspace, workspace_bytes,
                                   pwc_sup_flow_loss_workspace_bytes(B, H, W, h, w, 0), B, H, W, h, w, eps, pred_bstride,
                                   gt_bstride, mask_bstride);
    if (rc != PWC_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    FlowArgs a = make_flow_args(pred, gt, mask, mask_u8, mask_rule, B, H, W, h, w, eps, pred_bstride, gt_bstride, mask_bstride);
    a.part = static_cast<double *>(workspace);
    const int64_t nblk = blocks_of((int64_t)B * H * W);
    hipLaunchKernelGGL(flow_fwd_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(flow_finish_kernel, dim3(1), dim3(kThreads), 0, st, static_cast<const double *>(workspace), nblk,
                       mask ? 1 : 0, mask_rule, static_cast<float *>(out));
    return pwc::check_launch("flow_fwd_kernel");
}

extern "C" int pwc_sup_flow_loss_bwd(const void *pred, const void *gt, const void *mask, int mask_u8, int mask_rule,
                                     const void *fwd_out, const void *grad_out, void *grad_pred, int B, int H, int W, int h, int w,
                                     double eps, int64_t pred_bstride, int64_t gt_bstride, int64_t mask_bstride, void *workspace,
                                     int64_t workspace_bytes, void *stream) {
    if (!fwd_out || !grad_out) PWC_FAIL(PWC_EINVAL, "pwc_sup_flow_loss_bwd: null pointer");
    const int rc = check_flow_args("pwc_sup_flow_loss_bwd", pred, gt, mask, mask_u8, mask_rule, grad_pred, workspace,
                                   workspace_bytes, pwc_sup_flow_loss_workspace_bytes(B, H, W, h, w, 1), B, H, W, h, w, eps,
                                   pred_bstride, gt_bstride, mask_bstride);
    if (rc != PWC_OK) return rc;
    if (misaligned({fwd_out, grad_out})) {
        pwc::set_error("pwc_sup_flow_loss_bwd: needs 4-byte aligned operands");
        return PWC_EUNSUPPORTED;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    FlowArgs a = make_flow_args(pred, gt, mask, mask_u8, mask_rule, B, H, W, h, w, eps, pred_bstride, gt_bstride, mask_bstride);
    a.fwd_out = static_cast<const float *>(fwd_out);
    a.gout = static_cast<const float *>(grad_out);
    a.rows = static_cast<double *>(workspace);
    a.gpred = static_cast<float *>(grad_pred);
    const int64_t nrow = (int64_t)B * H * w, nlow = (int64_t)B * h * w;
    hipLaunchKernelGGL(flow_rows_kernel, dim3((unsigned)((nrow + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(flow_cols_kernel, dim3((unsigned)((nlow + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
    return pwc::check_launch("flow_rows_kernel");
}

extern "C" int64_t pwc_sup_multiscale_loss_workspace_bytes(int B, int H, int W, int L, const int *level_hw, int with_images) {
    if (B <= 0 || H <= 0 || W <= 0 || L < 1 || L > kMaxLevels || !level_hw) return -1;
    MsArgs a{};
    a.B = B;
    if (make_levels("pwc_sup_multiscale_loss_workspace_bytes", a, nullptr, nullptr, level_hw, nullptr, nullptr, L, B, H, W) != PWC_OK)
        return -1;
    return ms_part_bytes(a) + (with_images ? ms_img_bytes(a) : 0);
}

extern "C" int pwc_sup_multiscale_loss_fwd(const void *const *preds, const int64_t *pred_bstrides, const int *level_hw,
                                           const float *weights, int L, const void *gt, const void *mask, int mask_u8,
                                           const void *images, void *out, int B, int H, int W, double eps, float lambda_photo,
                                           float lambda_smooth, int64_t gt_bstride, int64_t mask_bstride, int64_t img_bstride,
                                           void *workspace, int64_t workspace_bytes, void *stream) {
    MsArgs a{};
    const int rc = check_ms_args("pwc_sup_multiscale_loss_fwd", a, preds, pred_bstrides, level_hw, weights, nullptr, L, gt, mask,
                                 mask_u8, images, out, B, H, W, eps, lambda_photo, lambda_smooth, gt_bstride, mask_bstride,
                                 img_bstride, workspace, workspace_bytes);
    if (rc != PWC_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.ims) launch_resize(a, st);
    const int64_t nblk = a.lv[L - 1].blk0 + a.lv[L - 1].nblk;
    hipLaunchKernelGGL(ms_fwd_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(ms_finish_kernel, dim3(1), dim3(kThreads), 0, st, a, static_cast<float *>(out));
    return pwc::check_launch("ms_fwd_kernel");
}

extern "C" int pwc_sup_multiscale_loss_bwd(const void *const *preds, const int64_t *pred_bstrides, const int *level_hw,
                                           const float *weights, int L, const void *gt, const void *mask, int mask_u8,
                                           const void *images, const void *fwd_out, const void *grad_out, void *const *grads,
                                           int B, int H, int W, double eps, float lambda_photo, float lambda_smooth,
                                           int64_t gt_bstride, int64_t mask_bstride, int64_t img_bstride, void *workspace,
                                           int64_t workspace_bytes, void *stream) {
    if (!fwd_out || !grad_out || !grads) PWC_FAIL(PWC_EINVAL, "pwc_sup_multiscale_loss_bwd: null pointer");
    MsArgs a{};
    const int rc = check_ms_args("pwc_sup_multiscale_loss_bwd", a, preds, pred_bstrides, level_hw, weights, grads, L, gt, mask,
                                 mask_u8, images, fwd_out, B, H, W, eps, lambda_photo, lambda_smooth, gt_bstride, mask_bstride,
                                 img_bstride, workspace, workspace_bytes);
    if (rc != PWC_OK) return rc;
    if (misaligned({grad_out})) {
        pwc::set_error("pwc_sup_multiscale_loss_bwd: needs 4-byte aligned operands");
        return PWC_EUNSUPPORTED;
    }
    a.fwd_out = static_cast<const float *>(fwd_out);
    a.gout = static_cast<const float *>(grad_out);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.ims) launch_resize(a, st);
    const int64_t nblk = a.lv[L - 1].blk0 + a.lv[L - 1].nblk;
    hipLaunchKernelGGL(ms_bwd_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, st, a);
    return pwc::check_launch("ms_bwd_kernel");
}
