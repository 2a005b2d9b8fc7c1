// Self-supervised proxy-label loss of the reference's train_pseudo.py:65-164 / train_fundamental.py:62-166, forward and backward,
// plus the stand-alone image warp of the same scripts (warp / warp_image, forward only):
//   up      = bilinear_align_corners(flow) * (W/w, H/h)          (flow itself when (h,w) == (H,W))
//   y_c     = bilinear(img2_c, clamp(x + up_x, 0, W-1), clamp(y + up_y, 0, H-1))      (grid_sample, border, align_corners)
//   s_c     = clamp((1 - SSIM(img1_c, y_c)) / 2, 0, 1)          SSIM on zero-padded 3x3 /9 box moments, C1 = 1e-4, C2 = 9e-4, + eps
//   map     = 0.85 mean_c s_c + 0.15 mean_c |img1_c - y_c|
//   photo   = mean(map)  |  sum(map * m) / max(sum m, 1)         m = mask > 0.5
//   smooth  = mean|flow[..., 1:] - flow[..., :-1]| + mean|flow[..., 1:, :] - flow[..., :-1, :]|   (low resolution)
//   total   = alpha_photo * photo + alpha_smooth * smooth
//
// fp32 coordinate arithmetic (compiled with -ffp-contract=off, so no operation below is fused; restated by the tests):
//   rh = (float)(h-1) / (float)(H-1), rw = (float)(w-1) / (float)(W-1)          (torch's align_corners source scale)
//   sy = (float)((double)H / h),       sx = (float)((double)W / w)              (the scripts' Python-float vector scales)
//   per output pixel (Y, X):  fy = rh * (float)Y, y0 = (int)fy, y1 = y0 + (y0 < h-1), ly1 = fy - (float)y0, ly0 = 1 - ly1
//                             (x alike);  u = ly0 * (lx0 * f[y0,x0] + lx1 * f[y0,x1]) + ly1 * (lx0 * f[y1,x0] + lx1 * f[y1,x1]),
//                             up_x = u * sx   (v alike, * sy)
//   px = (float)X + up_x, py = (float)Y + up_y;  clamped ix = fminf(fmaxf(px, 0), W-1), iy alike
//   x0 = floorf(ix), tx = ix - x0 (y alike);  value = (1-ty) * ((1-tx) * v00 + tx * v01) + ty * ((1-tx) * v10 + tx * v11),
//   taps past the last row / column read as 0 (their weight is 0 then).
// This is the reference's sample point without its linspace + normalise + unnormalise round trip: x + up_x is what that chain
// computes in exact arithmetic; in fp32 the two differ by a few ulp.
//
// Gradient semantics = autograd on the reference expression: d(ix)/d(up_x) = 1 for 0 < px < W-1 and 0 otherwise (PyTorch's border
// clip counts <= 0 and >= size-1 as outside), clamp passes on its closed interval, |0| has gradient 0, the upsampling's adjoint
// takes d/d(up) back to flow; images and mask get none.
//
// Work split.  One workgroup = one 16 x 64 tile of one image, 256 lanes, each owning the column tid % 64 of the rows
// tid / 64 + 4 k (k = 0..3).  Channels are processed one at a time through LDS:
//   forward : the window's sample points once into LDS; per channel img1_c and warped img2_c on tile + 1-pixel halo (18 x 66, zeros outside the image = avg_pool's padding), then per
//             pixel the 3x3 moments -- the variances in centred form, (1/9) sum (v - mu)^2 over the nine taps padded zeros
//             included, which equals E[v^2] - mu^2 without its cancellation -- SSIM and |x - y|.  Per-pixel sums stay in registers;
//             each workgroup writes {sum map*m, sum m, sum |dx|, sum |dy|} (fp64, fixed tree order) to the workspace, and one
//             final workgroup adds those partials in workgroup order.  The smoothness sums are a grid-stride pass of the same
//             launch over the low-resolution flow.
//   backward: nothing is saved by the forward; each tile recomputes.  The sample points of tile + 2-pixel halo (20 x 68) go to
//             LDS once (as in the forward: a 16-byte tap per pixel, registers stay free for the channel loop); per channel img1_c and warped img2_c go to LDS on that window, then on tile + 1 halo the SSIM partials
//             g_mu = G dS/dmu_y, g_sy = G dS/dsigma_y, g_sxy = G dS/dsigma_xy (G = dL/dmap * 0.85/C * clamp') together with mu_x,
//             mu_y go to LDS, and each tile pixel q takes the box filter's adjoint
//                 dL/dy_c(q) = (1/9) sum_{p in 3x3(q)} [g_mu(p) + 2 (y(q) - mu_y(p)) g_sy(p) + (x(q) - mu_x(p)) g_sxy(p)]
//                              + dL/dmap(q) * 0.15/C * sgn(y(q) - x(q))
//             (centred again), times the bilinear slope of img2_c at its sample point, summed over channels: grad_up [B,2,H,W]
//             goes to the workspace.  A gather kernel then gives every low-resolution flow pixel the fixed-order sum of the
//             full-resolution pixels whose interpolation uses it, times the vector scale, plus the smoothness term.
// No atomics on floats: every result is bit-reproducible.  The mask count of the backward is an integer sum (one 64-bit integer
// atomic per workgroup; integer addition is associative).
#include "pwc_block_reduce.h"
#include "pwc_common.h"
#include "pwc_flow_up.h"

namespace {

constexpr int kTH = 16, kTW = 64, kThreads = 256;
constexpr int kRowStep = kThreads / kTW;      // 4
constexpr int kPix = kTH / kRowStep;          // 4 pixels per lane
constexpr int kFH = kTH + 2, kFW = kTW + 2;   // forward window: tile + 1 halo (18 x 66)
constexpr int kFN = kFH * kFW;
constexpr int kBH = kTH + 4, kBW = kTW + 4;   // backward image window: tile + 2 halo (20 x 68)
constexpr int kBN = kBH * kBW;
constexpr float kC1 = 1e-4f, kC2 = 9e-4f;     // 0.01^2, 0.03^2 (train_pseudo.py:89, train_fundamental.py:142)

struct Geo : pwc::UpGeo {
    int B, C, tiles_x, tiles_y;
    int64_t bs_f, bs_1, bs_2, bs_m;
};

Geo make_geo(int B, int C, int H, int W, int h, int w, int64_t bs_f, int64_t bs_1, int64_t bs_2, int64_t bs_m) {
    Geo g;
    static_cast<pwc::UpGeo &>(g) = pwc::up_geo_make(H, W, h, w);
    g.B = B; g.C = C;
    g.tiles_x = (W + kTW - 1) / kTW;
    g.tiles_y = (H + kTH - 1) / kTH;
    g.bs_f = bs_f; g.bs_1 = bs_1; g.bs_2 = bs_2; g.bs_m = bs_m;
    return g;
}

using pwc::misaligned;
using pwc::up_flow;   // pwc_flow_up.h: upsampled flow (u, v) at full-resolution pixel (Y, X)

struct Sample {
    float ix, iy;   // clamped sample point
    bool gx, gy;    // the clip passes the gradient (0 < p < size-1)
};

__device__ __forceinline__ Sample sample_point(const float *f, const Geo &g, int Y, int X) {
    const float2 d = up_flow(f, g, Y, X);
    const float px = (float)X + d.x, py = (float)Y + d.y;
    const float lx = (float)(g.W - 1), ly = (float)(g.H - 1);
    Sample s;
    s.gx = px > 0.0f && px < lx;
    s.gy = py > 0.0f && py < ly;
    s.ix = fminf(fmaxf(px, 0.0f), lx);
    s.iy = fminf(fmaxf(py, 0.0f), ly);
    return s;
}

// bilinear taps of a clamped sample point, 16 bytes, kept in LDS per window pixel for the whole channel loop:
// off = y0 * W + x0 (-1: no sample), bit 0 / bit 1 of fl: the column x0+1 / row y0+1 is inside the image (bits 2 / 3, backward:
// the border clip passes d/dx / d/dy)
struct Tap {
    int off, fl;
    float tx, ty;
};

__device__ __forceinline__ int4 pack_tap(const Tap &t) {
    return make_int4(t.off, t.fl, __float_as_int(t.tx), __float_as_int(t.ty));
}
__device__ __forceinline__ Tap unpack_tap(int4 v) {
    Tap t;
    t.off = v.x;
    t.fl = v.y;
    t.tx = __int_as_float(v.z);
    t.ty = __int_as_float(v.w);
    return t;
}

__device__ __forceinline__ Tap make_tap(float ix, float iy, int H, int W) {
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    Tap t;
    t.off = y0 * W + x0;
    t.fl = (x0 + 1 < W ? 1 : 0) | (y0 + 1 < H ? 2 : 0);
    t.tx = ix - fx;
    t.ty = iy - fy;
    return t;
}

// bilinear value of plane p at a tap (taps past the last column / row read as 0); with slope != nullptr also d/d(ix), d/d(iy)
__device__ __forceinline__ float bilinear(const float *p, const Tap &t, int W, float2 *slope) {
    const bool ox = (t.fl & 1) != 0, oy = (t.fl & 2) != 0;
    const int off = t.off < 0 ? 0 : t.off;   // no sample (a tile pixel past the image edge): read pixel 0, the value is discarded
    const float v00 = p[off];
    const float v01 = ox ? p[off + 1] : 0.0f;
    const float v10 = oy ? p[off + W] : 0.0f;
    const float v11 = (ox && oy) ? p[off + W + 1] : 0.0f;
    const float tx = t.tx, ty = t.ty;
    if (slope) {
        slope->x = (1.0f - ty) * (v01 - v00) + ty * (v11 - v10);
        slope->y = (1.0f - tx) * (v10 - v00) + tx * (v11 - v01);
    }
    return (1.0f - ty) * ((1.0f - tx) * v00 + tx * v01) + ty * ((1.0f - tx) * v10 + tx * v11);
}

__device__ __forceinline__ bool mask_on(const void *mask, int mask_u8, int64_t off) {
    return pwc::mask_val(mask, mask_u8, off) > 0.5f;
}

// centred 3x3 moments of window arrays xs, ys (row stride ld) around the element at index c
struct Moments { float mx, my, vx, vy, cxy; };
__device__ __forceinline__ Moments moments(const float *xs, const float *ys, int c, int ld) {
    float sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            sx += xs[c + dy * ld + dx];
            sy += ys[c + dy * ld + dx];
        }
    Moments m;
    m.mx = sx / 9.0f;
    m.my = sy / 9.0f;
    float vx = 0.0f, vy = 0.0f, cxy = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float a = xs[c + dy * ld + dx] - m.mx, b = ys[c + dy * ld + dx] - m.my;
            vx += a * a;
            vy += b * b;
            cxy += a * b;
        }
    m.vx = vx / 9.0f;
    m.vy = vy / 9.0f;
    m.cxy = cxy / 9.0f;
    return m;
}

struct FwdArgs {
    const float *flow, *img1, *img2;
    const void *mask;
    int mask_u8;
    float eps;
    double *part;        // [nblk][4]
    Geo g;
};

__global__ __launch_bounds__(kThreads) void proxy_fwd_kernel(FwdArgs a) {
    __shared__ float sx_[kFN], sy_[kFN];
    __shared__ int4 s_tap[kFN];
    __shared__ pwc::TreeLds<kThreads, 4> red;
    const Geo &g = a.g;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int Y0 = blockIdx.y * kTH - 1, X0 = blockIdx.x * kTW - 1;
    const float *f = a.flow + (int64_t)b * g.bs_f;
    const int64_t plane = (int64_t)g.H * g.W;

    // sample points of the window, once, into LDS (reused by every channel)
#pragma unroll 1
    for (int i = tid; i < kFN; i += kThreads) {
        const int Y = Y0 + i / kFW, X = X0 + i % kFW;
        Tap t;
        t.off = -1;                                 // outside the image
        t.fl = 0;
        t.tx = t.ty = 0.0f;
        if (Y >= 0 && Y < g.H && X >= 0 && X < g.W) {
            const Sample sp = sample_point(f, g, Y, X);
            t = make_tap(sp.ix, sp.iy, g.H, g.W);
        }
        s_tap[i] = pack_tap(t);
    }
    float acc_s[kPix], acc_l[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) acc_s[k] = acc_l[k] = 0.0f;
    const int col = tid % kTW, row0 = tid / kTW;

#pragma unroll 1
    for (int c = 0; c < g.C; ++c) {
        const float *p1 = a.img1 + (int64_t)b * g.bs_1 + c * plane;
        const float *p2 = a.img2 + (int64_t)b * g.bs_2 + c * plane;
        __syncthreads();                             // taps written (c = 0), or the previous channel's reads done
#pragma unroll 1
        for (int i = tid; i < kFN; i += kThreads) {
            const Tap t = unpack_tap(s_tap[i]);
            float xv = 0.0f, yv = 0.0f;
            if (t.off >= 0) {
                const int Y = Y0 + i / kFW, X = X0 + i % kFW;
                xv = p1[Y * g.W + X];
                yv = bilinear(p2, t, g.W, nullptr);
            }
            sx_[i] = xv;
            sy_[i] = yv;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const int r = row0 + k * kRowStep;
            const int ci = (r + 1) * kFW + col + 1;
            const Moments m = moments(sx_, sy_, ci, kFW);
            const float A1 = 2.0f * m.mx * m.my + kC1, A2 = 2.0f * m.cxy + kC2;
            const float B1 = m.mx * m.mx + m.my * m.my + kC1, B2 = m.vx + m.vy + kC2;
            const float s = (A1 * A2) / (B1 * B2 + a.eps);
            acc_s[k] += fminf(fmaxf((1.0f - s) / 2.0f, 0.0f), 1.0f);
            acc_l[k] += fabsf(sy_[ci] - sx_[ci]);
        }
    }
    double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        const int Y = Y0 + 1 + row0 + k * kRowStep, X = X0 + 1 + col;
        if (Y < g.H && X < g.W && mask_on(a.mask, a.mask_u8, (int64_t)b * g.bs_m + (int64_t)Y * g.W + X)) {
            const float map = 0.85f * (acc_s[k] / (float)g.C) + 0.15f * (acc_l[k] / (float)g.C);
            v[0] += (double)map;
            v[1] += 1.0;
        }
    }
    // smoothness: grid-stride over the low-resolution flow, the same assignment on every call
    const int64_t lin = blockIdx.x + (int64_t)g.tiles_x * (blockIdx.y + (int64_t)g.tiles_y * blockIdx.z);
    const int64_t nblk = (int64_t)g.tiles_x * g.tiles_y * g.B;
    const int64_t lp = (int64_t)g.h * g.w, nf = (int64_t)g.B * 2 * lp;
    for (int64_t e = lin * kThreads + tid; e < nf; e += nblk * kThreads) {
        const int64_t bb = e / (2 * lp), r = e - bb * 2 * lp;
        const int64_t pl = r / lp, q = r - pl * lp;
        const int i = (int)(q / g.w), jx = (int)(q - (int64_t)i * g.w);
        const float *fp = a.flow + bb * g.bs_f + pl * lp;
        const float fv = fp[q];
        if (jx < g.w - 1) v[2] += (double)fabsf(fv - fp[q + 1]);
        if (i < g.h - 1) v[3] += (double)fabsf(fv - fp[q + g.w]);
    }
    pwc::tree_sum(red, v, nullptr);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a.part[lin * 4 + k] = v[k];
    }
}

__global__ __launch_bounds__(kThreads) void proxy_finish_kernel(const double *part, int64_t nblk, int masked, double npix,
                                                                double nx, double ny, float ap, float as, float *out) {
    __shared__ pwc::TreeLds<kThreads, 4> red;
    const int tid = threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = tid; i < nblk; i += kThreads)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += part[i * 4 + k];
    pwc::tree_sum(red, v, nullptr);
    if (tid == 0) {
        const double den = masked ? (v[1] > 1.0 ? v[1] : 1.0) : npix;
        const float photo = (float)(v[0] / den);
        const float smooth = (float)(v[2] / nx + v[3] / ny);
        out[0] = ap * photo + as * smooth;
        out[1] = photo;
        out[2] = smooth;
    }
}

__global__ __launch_bounds__(kThreads) void mask_count_kernel(const void *mask, int mask_u8, int B, int64_t plane, int64_t bs_m,
                                                              unsigned long long *count) {
    __shared__ pwc::TreeLds<kThreads, 0, 1> red;
    const int tid = threadIdx.x;
    long long n = 0;
    const int64_t tot = (int64_t)B * plane;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + tid; e < tot; e += (int64_t)gridDim.x * kThreads) {
        const int64_t bb = e / plane;
        n += mask_on(mask, mask_u8, bb * bs_m + (e - bb * plane)) ? 1 : 0;
    }
    pwc::tree_sum(red, nullptr, &n);
    if (tid == 0 && n) atomicAdd(count, (unsigned long long)n);
}

struct BwdArgs {
    const float *flow, *img1, *img2;
    const void *mask;
    int mask_u8;
    float eps, ap, as;
    const float *gout;                   // {g_total, g_photo, g_smooth}
    const unsigned long long *count;     // mask count (masked calls)
    float *gup;                          // [B][2][H][W]
    float *gflow;                        // [B][2][h][w]
    Geo g;
};

__global__ __launch_bounds__(kThreads) void proxy_bwd_kernel(BwdArgs a) {
    __shared__ float sx_[kBN], sy_[kBN];
    __shared__ float s_gmap[kFN], s_gmu[kFN], s_gsy[kFN], s_gsxy[kFN], s_mux[kFN], s_muy[kFN];
    __shared__ int4 s_tap[kBN];
    const Geo &g = a.g;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int Y0 = blockIdx.y * kTH - 2, X0 = blockIdx.x * kTW - 2;     // image window origin
    const float *f = a.flow + (int64_t)b * g.bs_f;
    const int64_t plane = (int64_t)g.H * g.W;
    const float gp = a.gout[0] * a.ap + a.gout[1];
    float den;
    if (a.mask) {
        const unsigned long long n = *a.count;
        den = n > 1ull ? (float)n : 1.0f;
    } else {
        den = (float)((double)g.B * (double)plane);
    }
    const float gq = gp / den;

    // sample points of the window, once, into LDS (registers would have to hold 6 window taps + 4 tile taps across the channel
    // loop); fl bits 2 / 3: the border clip passes d/dx / d/dy
#pragma unroll 1
    for (int i = tid; i < kBN; i += kThreads) {
        const int Y = Y0 + i / kBW, X = X0 + i % kBW;
        Tap t;
        t.off = -1;
        t.fl = 0;
        t.tx = t.ty = 0.0f;
        if (Y >= 0 && Y < g.H && X >= 0 && X < g.W) {
            const Sample sp = sample_point(f, g, Y, X);
            t = make_tap(sp.ix, sp.iy, g.H, g.W);
            t.fl |= (sp.gx ? 4 : 0) | (sp.gy ? 8 : 0);
        }
        s_tap[i] = pack_tap(t);
    }
    // dL/dmap on tile + 1 halo (0 outside the image and where the mask is off)
#pragma unroll 1
    for (int i = tid; i < kFN; i += kThreads) {
        const int Y = Y0 + 1 + i / kFW, X = X0 + 1 + i % kFW;
        float gm = 0.0f;
        if (Y >= 0 && Y < g.H && X >= 0 && X < g.W && mask_on(a.mask, a.mask_u8, (int64_t)b * g.bs_m + (int64_t)Y * g.W + X)) gm = gq;
        s_gmap[i] = gm;
    }
    const int col = tid % kTW, row0 = tid / kTW;
    float gux[kPix], guy[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) gux[k] = guy[k] = 0.0f;
    const float wssim = 0.85f / (float)g.C, wl1 = 0.15f / (float)g.C;

#pragma unroll 1
    for (int c = 0; c < g.C; ++c) {
        const float *p1 = a.img1 + (int64_t)b * g.bs_1 + c * plane;
        const float *p2 = a.img2 + (int64_t)b * g.bs_2 + c * plane;
        __syncthreads();                             // taps / dL/dmap written (c = 0), or the previous channel's reads done
#pragma unroll 1
        for (int i = tid; i < kBN; i += kThreads) {
            const Tap t = unpack_tap(s_tap[i]);
            float xv = 0.0f, yv = 0.0f;
            if (t.off >= 0) {
                const int Y = Y0 + i / kBW, X = X0 + i % kBW;
                xv = p1[Y * g.W + X];
                yv = bilinear(p2, t, g.W, nullptr);
            }
            sx_[i] = xv;
            sy_[i] = yv;
        }
        __syncthreads();
        // SSIM partials on tile + 1 halo
#pragma unroll 1
        for (int i = tid; i < kFN; i += kThreads) {
            const int wy = i / kFW, wx = i % kFW;
            const float gm = s_gmap[i];
            float gmu = 0.0f, gsy = 0.0f, gsxy = 0.0f, mux = 0.0f, muy = 0.0f;
            if (gm != 0.0f) {
                const Moments m = moments(sx_, sy_, (wy + 1) * kBW + wx + 1, kBW);
                const float A1 = 2.0f * m.mx * m.my + kC1, A2 = 2.0f * m.cxy + kC2;
                const float B1 = m.mx * m.mx + m.my * m.my + kC1, B2 = m.vx + m.vy + kC2;
                const float D = B1 * B2 + a.eps;
                const float sv = (A1 * A2) / D;
                const float t = (1.0f - sv) / 2.0f;
                const float G = (t >= 0.0f && t <= 1.0f) ? gm * wssim * -0.5f : 0.0f;
                gmu = G * ((2.0f * m.mx * A2 - sv * 2.0f * m.my * B2) / D);
                gsy = G * (-sv * B1 / D);
                gsxy = G * (2.0f * A1 / D);
                mux = m.mx;
                muy = m.my;
            }
            s_gmu[i] = gmu;
            s_gsy[i] = gsy;
            s_gsxy[i] = gsxy;
            s_mux[i] = mux;
            s_muy[i] = muy;
        }
        __syncthreads();
        // box adjoint + L1 term at the tile pixels, then through the bilinear slope of img2_c
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const int r = row0 + k * kRowStep;
            const int Y = Y0 + 2 + r, X = X0 + 2 + col;
            if (Y < g.H && X < g.W) {
                const int qi = (r + 2) * kBW + col + 2;
                const float xq = sx_[qi], yq = sy_[qi];
                const int pc = (r + 1) * kFW + col + 1;
                float acc = 0.0f;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int pi = pc + dy * kFW + dx;
                        acc += s_gmu[pi] + 2.0f * (yq - s_muy[pi]) * s_gsy[pi] + (xq - s_mux[pi]) * s_gsxy[pi];
                    }
                const float d = yq - xq;
                const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
                const float gy = acc / 9.0f + s_gmap[pc] * wl1 * sg;
                float2 sl;
                bilinear(p2, unpack_tap(s_tap[qi]), g.W, &sl);
                gux[k] += gy * sl.x;
                guy[k] += gy * sl.y;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        const int r = row0 + k * kRowStep;
        const int Y = Y0 + 2 + r, X = X0 + 2 + col;
        if (Y < g.H && X < g.W) {
            const int fl = s_tap[(r + 2) * kBW + col + 2].y;
            float *o = a.gup + (int64_t)b * 2 * plane + (int64_t)Y * g.W + X;
            o[0] = (fl & 4) ? gux[k] : 0.0f;
            o[plane] = (fl & 8) ? guy[k] : 0.0f;
        }
    }
}

// full-resolution rows (or columns) whose align_corners interpolation uses low-resolution row i, and the weight it gets.
// One lane per low-resolution pixel walks about (2H/h) x (2W/w) full-resolution pixels: the total work is ~4 H W per image at any
// ratio, but at extreme ratios (h or w = 2 is accepted) it sits in a handful of lanes -- correct, and slow (milliseconds at
// 384 x 512 with a 2 x 2 flow).  The training scripts upsample by 4.
__device__ __forceinline__ int first_user(int i, float r, int n_out) {
    // smallest Y with (int)(r * Y) >= i - 1; the estimate is within ulps of it, walked to the exact value
    int Y = (int)floorf((float)(i - 1) / r) - 2;
    Y = Y < 0 ? 0 : Y;
    while (Y > 0 && (int)(r * (float)(Y - 1)) >= i - 1) --Y;
    while (Y < n_out && (int)(r * (float)Y) < i - 1) ++Y;
    return Y;
}
__device__ __forceinline__ float user_weight(int i, float r, int Y, int n_in) {
    const float fy = r * (float)Y;
    const int y0 = (int)fy, y1 = y0 + (y0 < n_in - 1 ? 1 : 0);
    const float l1 = fy - (float)y0, l0 = 1.0f - l1;
    return (y0 == i ? l0 : 0.0f) + (y1 == i ? l1 : 0.0f);
}

__global__ __launch_bounds__(kThreads) void proxy_gather_kernel(BwdArgs a) {
    const Geo &g = a.g;
    const int64_t lp = (int64_t)g.h * g.w;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)g.B * lp) return;
    const int b = (int)(e / lp);
    const int q = (int)(e - (int64_t)b * lp);
    const int i = q / g.w, j = q - i * g.w;
    const int64_t plane = (int64_t)g.H * g.W;
    const float *gu = a.gup + (int64_t)b * 2 * plane;
    // fp64 sums: the full-resolution gradients of a rough flow have mixed signs and cancel, fp32 would lose ~1e-4 of the result
    double acc0 = 0.0, acc1 = 0.0;
    if (g.same) {
        acc0 = gu[(int64_t)i * g.W + j];
        acc1 = gu[plane + (int64_t)i * g.W + j];
    } else {
        const int ylo = first_user(i, g.rh, g.H), xlo = first_user(j, g.rw, g.W);
        for (int Y = ylo; Y < g.H && (int)(g.rh * (float)Y) <= i; ++Y) {
            const double wy = user_weight(i, g.rh, Y, g.h);
            double r0 = 0.0, r1 = 0.0;
            for (int X = xlo; X < g.W && (int)(g.rw * (float)X) <= j; ++X) {
                const double wx = user_weight(j, g.rw, X, g.w);
                r0 += wx * gu[(int64_t)Y * g.W + X];
                r1 += wx * gu[plane + (int64_t)Y * g.W + X];
            }
            acc0 += wy * r0;
            acc1 += wy * r1;
        }
        acc0 *= g.sx;
        acc1 *= g.sy;
    }
    // smoothness: d/df of mean|f[j] - f[j+1]| + mean|f[i] - f[i+1]| over the low-resolution flow
    const float gs = a.gout[0] * a.as + a.gout[2];
    const float nx = (float)((double)g.B * 2.0 * g.h * (g.w - 1)), ny = (float)((double)g.B * 2.0 * (g.h - 1) * g.w);
    float out[2] = {(float)acc0, (float)acc1};
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        const float *fp = a.flow + (int64_t)b * g.bs_f + pl * lp;
        const float fv = fp[q];
        float tx = 0.0f, ty = 0.0f;
        if (j < g.w - 1) { const float d = fv - fp[q + 1]; tx += d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }
        if (j > 0) { const float d = fp[q - 1] - fv; tx -= d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }
        if (i < g.h - 1) { const float d = fv - fp[q + g.w]; ty += d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }
        if (i > 0) { const float d = fp[q - g.w] - fv; ty -= d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }
        out[pl] += gs * (tx / nx + ty / ny);
    }
    float *o = a.gflow + (int64_t)b * 2 * lp + q;
    o[0] = out[0];
    o[lp] = out[1];
}

__global__ __launch_bounds__(kThreads) void warp_image_kernel(const float *img, const float *flow, float *out, Geo g,
                                                              int64_t bs_o) {
    const int64_t plane = (int64_t)g.H * g.W;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)g.B * plane) return;
    const int b = (int)(e / plane);
    const int64_t q = e - (int64_t)b * plane;
    const int Y = (int)(q / g.W), X = (int)(q - (int64_t)Y * g.W);
    const Sample s = sample_point(flow + (int64_t)b * g.bs_f, g, Y, X);
    const Tap t = make_tap(s.ix, s.iy, g.H, g.W);
    const float *src = img + (int64_t)b * g.bs_1;
    float *dst = out + (int64_t)b * bs_o + q;
    for (int c = 0; c < g.C; ++c) dst[c * plane] = bilinear(src + c * plane, t, g.W, nullptr);
}

int64_t fwd_bytes(int B, int H, int W) {
    return (int64_t)B * ((H + kTH - 1) / kTH) * ((W + kTW - 1) / kTW) * 4 * 8;
}
int64_t gup_bytes(int B, int H, int W) {
    return ((int64_t)B * 2 * H * W * 4 + 255) / 256 * 256;
}

// shared validation of the two loss entries; returns PWC_OK to launch
int check_loss_args(const char *who, const void *flow, const void *img1, const void *img2, const void *mask, int mask_u8,
                    const void *out, const void *workspace, int64_t workspace_bytes, int64_t need, int B, int C, int H, int W,
                    int h, int w, int64_t bs_f, int64_t bs_1, int64_t bs_2, int64_t bs_m) {
    if (!flow || !img1 || !img2 || !out || !workspace) PWC_FAIL(PWC_EINVAL, "%s: null pointer", who);
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0)
        PWC_FAIL(PWC_EINVAL, "%s: bad shape B=%d C=%d H=%d W=%d h=%d w=%d", who, B, C, H, W, h, w);
    const int64_t plane = (int64_t)H * W;
    if (bs_f < 2LL * h * w || bs_1 < C * plane || bs_2 < C * plane || (mask && bs_m < plane))
        PWC_FAIL(PWC_EINVAL, "%s: batch stride smaller than the tensor", who);
    if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u))
        PWC_FAIL(PWC_EINVAL, "%s: workspace needs %lld bytes, 8-byte aligned", who, (long long)need);
    if (H < 2 || W < 2 || h < 2 || w < 2 || H < h || W < w) {
        pwc::set_error("%s: declined geometry H=%d W=%d h=%d w=%d (needs 2 <= h <= H, 2 <= w <= W)", who, H, W, h, w);
        return PWC_EUNSUPPORTED;
    }
    if (misaligned({flow, img1, img2, out}) || (mask && !mask_u8 && misaligned({mask})) || (int64_t)C * plane >= 0x7fffffffLL ||
        ((H + kTH - 1) / kTH) > 65535 || B > 65535) {
        pwc::set_error("%s: needs 4-byte aligned operands, C*H*W < 2^31 and B <= 65535", who);
        return PWC_EUNSUPPORTED;
    }
    return PWC_OK;
}

}  // namespace

extern "C" int64_t pwc_proxy_loss_fwd_workspace_bytes(int B, int C, int H, int W, int h, int w) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return -1;
    return fwd_bytes(B, H, W);
}

extern "C" int64_t pwc_proxy_loss_workspace_bytes(int B, int C, int H, int W, int h, int w) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return -1;
    const int64_t f = fwd_bytes(B, H, W), bw = gup_bytes(B, H, W) + 256;
    return f > bw ? f : bw;
}

extern "C" int pwc_proxy_loss_fwd(const void *flow, const void *img1, const void *img2, const void *mask, int mask_u8,
                                  void *out, int B, int C, int H, int W, int h, int w,
                                  float alpha_photo, float alpha_smooth, float ssim_eps,
                                  int64_t flow_bstride, int64_t img1_bstride, int64_t img2_bstride, int64_t mask_bstride,
                                  void *workspace, int64_t workspace_bytes, void *stream) {
    const int rc = check_loss_args("pwc_proxy_loss_fwd", flow, img1, img2, mask, mask_u8, out, workspace, workspace_bytes,
                                   pwc_proxy_loss_fwd_workspace_bytes(B, C, H, W, h, w),
                                   B, C, H, W, h, w, flow_bstride, img1_bstride, img2_bstride, mask_bstride);
    if (rc != PWC_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    FwdArgs a{static_cast<const float *>(flow), static_cast<const float *>(img1), static_cast<const float *>(img2), mask,
              mask_u8 ? 1 : 0, ssim_eps, static_cast<double *>(workspace),
              make_geo(B, C, H, W, h, w, flow_bstride, img1_bstride, img2_bstride, mask_bstride)};
    const int64_t nblk = (int64_t)a.g.tiles_x * a.g.tiles_y * B;
    hipLaunchKernelGGL(proxy_fwd_kernel, dim3(a.g.tiles_x, a.g.tiles_y, B), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(proxy_finish_kernel, dim3(1), dim3(kThreads), 0, st, static_cast<const double *>(workspace), nblk,
                       mask ? 1 : 0, (double)B * H * W, (double)B * 2 * h * (w - 1), (double)B * 2 * (h - 1) * w,
                       alpha_photo, alpha_smooth, static_cast<float *>(out));
    return pwc::check_launch("proxy_fwd_kernel");
}

extern "C" int pwc_proxy_loss_bwd(const void *flow, const void *img1, const void *img2, const void *mask, int mask_u8,
                                  const void *grad_out, void *grad_flow, int B, int C, int H, int W, int h, int w,
                                  float alpha_photo, float alpha_smooth, float ssim_eps,
                                  int64_t flow_bstride, int64_t img1_bstride, int64_t img2_bstride, int64_t mask_bstride,
                                  void *workspace, int64_t workspace_bytes, void *stream) {
    if (!grad_out) PWC_FAIL(PWC_EINVAL, "pwc_proxy_loss_bwd: null pointer");
    const int rc = check_loss_args("pwc_proxy_loss_bwd", flow, img1, img2, mask, mask_u8, grad_flow, workspace, workspace_bytes,
                                   pwc_proxy_loss_workspace_bytes(B, C, H, W, h, w),
                                   B, C, H, W, h, w, flow_bstride, img1_bstride, img2_bstride, mask_bstride);
    if (rc != PWC_OK) return rc;
    if (misaligned({grad_out})) {
        pwc::set_error("pwc_proxy_loss_bwd: needs 4-byte aligned operands");
        return PWC_EUNSUPPORTED;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    unsigned long long *count = reinterpret_cast<unsigned long long *>(ws + gup_bytes(B, H, W));
    BwdArgs a{static_cast<const float *>(flow), static_cast<const float *>(img1), static_cast<const float *>(img2), mask,
              mask_u8 ? 1 : 0, ssim_eps, alpha_photo, alpha_smooth, static_cast<const float *>(grad_out), count,
              reinterpret_cast<float *>(ws), static_cast<float *>(grad_flow),
              make_geo(B, C, H, W, h, w, flow_bstride, img1_bstride, img2_bstride, mask_bstride)};
    if (mask) {
        hipError_t e = hipMemsetAsync(count, 0, 8, st);
        if (e != hipSuccess) { pwc::set_error("pwc_proxy_loss_bwd: hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
        const int64_t tot = (int64_t)B * H * W;
        const int64_t nb = (tot + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(kThreads), 0, st, mask, a.mask_u8, B,
                           (int64_t)H * W, mask_bstride, count);
    }
    hipLaunchKernelGGL(proxy_bwd_kernel, dim3(a.g.tiles_x, a.g.tiles_y, B), dim3(kThreads), 0, st, a);
    const int64_t nlow = (int64_t)B * h * w;
    hipLaunchKernelGGL(proxy_gather_kernel, dim3((unsigned)((nlow + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
    return pwc::check_launch("proxy_bwd_kernel");
}

extern "C" int pwc_flow_warp_image_fwd(const void *img, const void *flow, void *out, int B, int C, int H, int W, int h, int w,
                                       int64_t img_bstride, int64_t flow_bstride, int64_t out_bstride, void *stream) {
    if (!img || !flow || !out) PWC_FAIL(PWC_EINVAL, "pwc_flow_warp_image_fwd: null pointer");
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0)
        PWC_FAIL(PWC_EINVAL, "pwc_flow_warp_image_fwd: bad shape B=%d C=%d H=%d W=%d h=%d w=%d", B, C, H, W, h, w);
    const int64_t plane = (int64_t)H * W;
    if (img_bstride < C * plane || out_bstride < C * plane || flow_bstride < 2LL * h * w)
        PWC_FAIL(PWC_EINVAL, "pwc_flow_warp_image_fwd: batch stride smaller than the tensor");
    if (H < 2 || W < 2 || h < 2 || w < 2 || H < h || W < w) {
        pwc::set_error("pwc_flow_warp_image_fwd: declined geometry H=%d W=%d h=%d w=%d (needs 2 <= h <= H, 2 <= w <= W)", H, W, h, w);
        return PWC_EUNSUPPORTED;
    }
    if (misaligned({img, flow, out}) || (int64_t)C * plane >= 0x7fffffffLL || ((int64_t)B * plane + kThreads - 1) / kThreads > 0x7fffffffLL) {
        pwc::set_error("pwc_flow_warp_image_fwd: needs 4-byte aligned operands and C*H*W < 2^31");
        return PWC_EUNSUPPORTED;
    }
    const Geo g = make_geo(B, C, H, W, h, w, flow_bstride, img_bstride, 0, 0);
    hipLaunchKernelGGL(warp_image_kernel, dim3((unsigned)(((int64_t)B * plane + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), static_cast<const float *>(img), static_cast<const float *>(flow),
                       static_cast<float *>(out), g, out_bstride);
    return pwc::check_launch("warp_image_kernel");
}
