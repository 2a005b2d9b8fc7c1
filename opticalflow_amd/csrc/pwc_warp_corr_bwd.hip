// Backward of the fused warp + correlation + LeakyReLU of a PWC-Net decoder level (pwc_warp_corr81_fwd, and pwc_corr_fwd's
// PWC configuration when flo == NULL), in one pass:
//   y[p,d] = act(scale * sum_c c1[p,c] * w2[p+d,c]),   w2 = warp(c2, flow_scale * flo)   (pad 4, max displacement 4, strides 1)
// gives, with g[p,d] = scale * act'(y[p,d]) * gy[p,d]   (act' = 1 where y > 0, slope elsewhere: y > 0 <=> x > 0 for slope > 0),
//   grad_c1[p] = sum_d g[p,d] * w2[p+d]
//   gw2[q]     = sum_d g[q-d,d] * c1[q-d]                     (gradient of the warped tensor; never written to HBM)
//   grad_c2    = scatter of gw2 through the bilinear taps     (the only cross-workgroup sum)
//   grad_flo   = sum_c gw2 * d w2 / d (u, v)                  (as pwc_warp_bwd; the validity mask is a constant)
//
// Work split: one workgroup = one 8 x 32 tile of one image and a slice of its chunks of kCC channels (all of them when the tiles
// fill the chip), one lane per pixel p (and q = p).  Per chunk, the c1 window and the warped-c2 window of the tile (16 x 40 pixels, the tile plus the 4-pixel displacement halo, zero outside
// the image as the correlation's padding) are built in LDS, then every lane walks the 81 displacements once, reading g[p,d] and
// g[p-d,d] (a shifted tile-sized slice of plane d) from gy and y, and accumulates grad_c1 and gw2 of the chunk in registers: both
// are gathers with a fixed summation order.  The activated output y is READ for the LeakyReLU mask rather than the pre-activation
// recomputed: recomputing costs the forward's whole 81 x C dot-product pass (~90 us at level 2, batch 16), reading y one more
// stream of the size of gy (~25 us at HBM rate), which the same lanes read anyway in the same order.
//
// grad_c2 scatter, deterministic: each contribution gw2 * w is rounded to a 64-bit fixed-point integer (integer addition is
// associative, so the order in which workgroups add does not matter) and summed first in LDS over a 16 x 48 source window
// anchored at the smallest tap row / column of the tile (two channel buffers; a smooth flow puts a tile's taps in about
// 9 x 33 pixels), then flushed with one 64-bit global atomic per non-zero window element, row-contiguous (384 B per window row).
// Taps outside the window (rough or diverging flow) add their integer straight to the global workspace from the lane.  A final
// pass converts the workspace to float.
// Fixed-point scale: |gw2| <= 81 * max|g| * max|c1| =: M with max|g| = max|gy| * |scale| * max(1, |slope|), and every bilinear
// weight is <= 1, so one contribution is < 2^(e+1) for e = floor(log2 M).  The scale 2^(39 - e) keeps a contribution below 2^40
// (resolution 2^-39 of M); an int64 element then holds 2^23 (8 388 608) such contributions before it could wrap -- more output
// pixels than that would have to sample ONE source pixel.  max|gy| and max|c1| come from one prepass over both tensors.
// Non-finite gy or c1 (or an M that overflows float) has no fixed-point form: the call then falls back, on the device and without
// synchronising, to float atomics for the whole grad_c2 (summed in the workspace viewed as float, copied out by the final pass),
// so Inf / NaN reach grad_c2 as in pwc_warp_bwd's fallback.
#include "pwc_common.h"
#include "pwc_warp_taps.h"
#include "pwc_absmax.h"

namespace {

using pwc_warp::Taps;
using pwc_warp::make_taps;
using pwc_warp::tap4;

constexpr int kD = 4;
constexpr int kND = 2 * kD + 1;          // 9
constexpr int kTH = 8, kTW = 32;         // tile
constexpr int kThreads = kTH * kTW;      // 256: one lane per pixel
constexpr int kWinH = kTH + 2 * kD;      // 16
constexpr int kWinW = kTW + 2 * kD;      // 40
constexpr int kWinPix = kWinH * kWinW;   // 640
constexpr int kWinPerLane = (kWinPix + kThreads - 1) / kThreads;   // 3
constexpr int kCC = 16;                  // channels per chunk (2 x 40 KB of windows; the kernel holds one workgroup per CU anyway)
constexpr int kSrcH = 16, kSrcW = 48;    // grad_c2 source window (2 x 6 KB of int64)
constexpr int kSrcPix = kSrcH * kSrcW;
constexpr unsigned kNonFiniteBits = pwc::kAbsmaxNonFinite;

struct Args {
    const float *c1, *c2, *flo, *y, *gy;
    float *gc1, *gc2;
    float *gfp;                          // [B][gridDim.y][2][H*W] per-slice sums of d/d(ix, iy) (warp form; summed by flo_reduce_kernel)
    unsigned long long *acc;             // [B*C*H*W] fixed-point grad_c2 (warp form only)
    const unsigned *mbits;               // [0] = max|gy| bits, [1] = max|c1| bits
    int C, H, W, tiles_x, tiles_y;
    int64_t bs_c1, bs_c2, bs_flo, bs_y, bs_gy;
    float flow_scale, thr, scale, slope;
    int align_corners, leaky;
};

// fixed-point mode and scale of this call (uniform over the grid; the same in every kernel that asks)
__device__ __forceinline__ bool fixed_mode(const unsigned *mbits, float gmul, float *fscale) {
    const unsigned bg = mbits[0], bc = mbits[1];
    if (bg >= kNonFiniteBits || bc >= kNonFiniteBits) return false;
    const float m = 81.0f * __uint_as_float(bg) * gmul * __uint_as_float(bc);
    if (!(m <= 3.0e38f)) return false;
    const int e = (int)(__float_as_uint(m) >> 23) - 127;      // floor(log2 M); -127 for zero / subnormal
    *fscale = __uint_as_float((unsigned)(min(max(39 - e, -126), 127) + 127) << 23);
    return true;
}

// g = scale * act'(y) * gy; without the activation the entry passes y = gy and slope = 1 (no branch in the loop)
__device__ __forceinline__ float gval(float g, float yv, float scale, float slope) {
    return (yv > 0.0f ? g : g * slope) * scale;
}

template <bool WARP>
__global__ void __launch_bounds__(kThreads)
warp_corr81_bwd_kernel(Args a) {
    __shared__ float s1[kCC][kWinPix];                        // c1 window of the chunk
    __shared__ float s2[kCC][kWinPix];                        // warped c2 window of the chunk
    __shared__ unsigned long long sacc[WARP ? 2 : 1][WARP ? kSrcPix : 1];
    __shared__ int sorg[2];

    const int t = threadIdx.x;
    int tile = blockIdx.x;
    const int tx = tile % a.tiles_x;
    tile /= a.tiles_x;
    const int ty = tile % a.tiles_y;
    const int b = tile / a.tiles_y;
    const int H = a.H, W = a.W, C = a.C;
    const int ly = t / kTW, lx = t % kTW;
    const int ty0 = ty * kTH, tx0 = tx * kTW;
    const int py = ty0 + ly, px = tx0 + lx;
    const bool inside = (py < H) && (px < W);
    const int64_t plane = (int64_t)H * W;
    const int pix = py * W + px;
    const int pin = inside ? pix : 0;                          // clamped for the unconditional loads
    const float *c1b = a.c1 + (int64_t)b * a.bs_c1;
    const float *c2b = a.c2 + (int64_t)b * a.bs_c2;
    const float *gyb = a.gy + (int64_t)b * a.bs_gy;
    const float *yb = a.y + (int64_t)b * a.bs_y;
    const int64_t obase = (int64_t)b * C * plane;              // grad_c1 / grad_c2 / workspace: dense [B,C,H,W]

    // ---- warp taps: of the window pixels this lane fills (forward's make_taps), and the lane's own pixel (pwc_warp_bwd's form)
    Taps wt[kWinPerLane];
    bool wok[kWinPerLane];
    float ax0 = 0.f, ax1 = 0.f, ay0 = 0.f, ay1 = 0.f;
    bool v00 = false, v01 = false, v10 = false, v11 = false, keep = false;
    int o00 = 0, o01 = 0, o10 = 0, o11 = 0;
    float w00 = 0.f, w01 = 0.f, w10 = 0.f, w11 = 0.f;
    bool fixed = true;
    float fscale = 0.f;
    if constexpr (WARP) {
        const float *fb = a.flo + (int64_t)b * a.bs_flo;
#pragma unroll
        for (int k = 0; k < kWinPerLane; ++k) {
            const int i = t + k * kThreads;
            const int gy = ty0 - kD + i / kWinW, gx = tx0 - kD + i % kWinW;
            wok[k] = (i < kWinPix) && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int o = wok[k] ? gy * W + gx : 0;
            const float u = fb[o] * a.flow_scale, v = fb[plane + o] * a.flow_scale;
            wt[k] = make_taps((float)gx + u, (float)gy + v, H, W, a.align_corners, a.thr);
        }
        if (t < 2) sorg[t] = 0x7fffffff;
        if (inside) {
            const float u = fb[pix] * a.flow_scale, v = fb[plane + pix] * a.flow_scale;
            const float fpx = (float)px + u, fpy = (float)py + v;
            const float gxn = 2.0f * fpx / (float)max(W - 1, 1) - 1.0f;
            const float gyn = 2.0f * fpy / (float)max(H - 1, 1) - 1.0f;
            float ix, iy;
            if (a.align_corners) {
                ix = (gxn + 1.0f) / 2.0f * (float)(W - 1);
                iy = (gyn + 1.0f) / 2.0f * (float)(H - 1);
            } else {
                ix = ((gxn + 1.0f) * (float)W - 1.0f) / 2.0f;
                iy = ((gyn + 1.0f) * (float)H - 1.0f) / 2.0f;
            }
            const bool wild = (ix < -16.0f) || (ix > (float)W + 16.0f) || (iy < -16.0f) || (iy > (float)H + 16.0f);
            ix = fminf(fmaxf(ix, -16.0f), (float)W + 16.0f);
            iy = fminf(fmaxf(iy, -16.0f), (float)H + 16.0f);
            const float fx = floorf(ix), fy = floorf(iy);
            const int x0 = (int)fx, y0 = (int)fy;
            ax1 = ix - fx; ay1 = iy - fy; ax0 = 1.0f - ax1; ay0 = 1.0f - ay1;
            const bool vx0 = (x0 >= 0) && (x0 < W), vx1 = (x0 + 1 >= 0) && (x0 + 1 < W);
            const bool vy0 = (y0 >= 0) && (y0 < H), vy1 = (y0 + 1 >= 0) && (y0 + 1 < H);
            v00 = vx0 && vy0; v01 = vx1 && vy0; v10 = vx0 && vy1; v11 = vx1 && vy1;
            w00 = v00 ? ay0 * ax0 : 0.f; w01 = v01 ? ay0 * ax1 : 0.f;
            w10 = v10 ? ay1 * ax0 : 0.f; w11 = v11 ? ay1 * ax1 : 0.f;
            const float msum = ((w00 + w01) + w10) + w11;
            keep = (msum >= a.thr) && !wild;
            const int xc0 = min(max(x0, 0), W - 1), xc1 = min(max(x0 + 1, 0), W - 1);
            const int yc0 = min(max(y0, 0), H - 1), yc1 = min(max(y0 + 1, 0), H - 1);
            o00 = yc0 * W + xc0; o01 = yc0 * W + xc1; o10 = yc1 * W + xc0; o11 = yc1 * W + xc1;
            if (!keep) { w00 = w01 = w10 = w11 = 0.f; }
        }
        fixed = fixed_mode(a.mbits, fabsf(a.scale) * fmaxf(1.0f, fabsf(a.slope)), &fscale);
        for (int i = t; i < 2 * kSrcPix; i += kThreads) (&sacc[0][0])[i] = 0ull;
        __syncthreads();
        if (keep) {                                           // source window origin: smallest row / column a tap adds to
            atomicMin(&sorg[0], (w00 != 0.f || w01 != 0.f) ? o00 / W : o10 / W);
            atomicMin(&sorg[1], (w00 != 0.f || w10 != 0.f) ? o00 % W : o01 % W);
        }
        __syncthreads();
    }
    // each tap's element in the source window, -1 outside it (taken by the lane's own global atomic)
    int lidx[4] = {-1, -1, -1, -1};
    const int sr0 = WARP ? sorg[0] : 0, sc0 = WARP ? sorg[1] : 0;
    if constexpr (WARP) {
        if (keep) {
            const int rt = o00 / W, rb = o10 / W, cl = o00 - rt * W, cr = o01 - rt * W;
            const int rr[4] = {rt - sr0, rt - sr0, rb - sr0, rb - sr0}, cc[4] = {cl - sc0, cr - sc0, cl - sc0, cr - sc0};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                lidx[k] = (rr[k] >= 0 && rr[k] < kSrcH && cc[k] >= 0 && cc[k] < kSrcW) ? rr[k] * kSrcW + cc[k] : -1;
        }
    }

    float dix = 0.f, diy = 0.f;
    // the channel chunks are spread over gridDim.y (see the entry for how many): grad_c1, gw2 and the grad_c2 scatter are per
    // channel; grad_flo, the one sum over channels, leaves one partial sum per y-slice for flo_reduce_kernel
    for (int c0 = kCC * blockIdx.y; c0 < C; c0 += kCC * gridDim.y) {
        const int nc = min(kCC, C - c0);
        __syncthreads();                                      // the previous chunk's window readers are done
        static_assert((kCC * kWinPix) % kThreads == 0, "window fill");
        float v1[kCC * kWinPix / kThreads], v2[kCC * kWinPix / kThreads];
#pragma unroll
        for (int j = 0; j < kCC * kWinPix / kThreads; ++j) {   // all loads first, then the LDS writes
            const int i = t + j * kThreads;
            const int c = i / kWinPix, pos = i - c * kWinPix;
            const int gy = ty0 - kD + pos / kWinW, gx = tx0 - kD + pos % kWinW;
            const bool ok = c < nc && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int64_t off = (int64_t)min(c0 + c, C - 1) * plane + min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
            v1[j] = c1b[off];
            if constexpr (!WARP) v2[j] = c2b[off];
            if (!ok) { v1[j] = 0.0f; v2[j] = 0.0f; }
        }
#pragma unroll
        for (int j = 0; j < kCC * kWinPix / kThreads; ++j) {
            const int i = t + j * kThreads;
            const int c = i / kWinPix, pos = i - c * kWinPix;
            s1[c][pos] = v1[j];
            if constexpr (!WARP) s2[c][pos] = v2[j];
        }
        if constexpr (WARP) {
#pragma unroll
            for (int k = 0; k < kWinPerLane; ++k) {
                const int i = t + k * kThreads;
                if (i >= kWinPix) continue;                       // the last position exists for the first lanes only
                const Taps &q = wt[k];
                float v[kCC];
#pragma unroll
                for (int c = 0; c < kCC; ++c) {
                    const float *src = c2b + (int64_t)min(c0 + c, C - 1) * plane;
                    v[c] = tap4(q, src[q.o00], src[q.o01], src[q.o10], src[q.o11]);
                }
#pragma unroll
                for (int c = 0; c < kCC; ++c) s2[c][i] = (wok[k] && c < nc) ? v[c] : 0.0f;
            }
        }
        __syncthreads();

        float a1[kCC], a2[kCC];
#pragma unroll
        for (int c = 0; c < kCC; ++c) a1[c] = a2[c] = 0.0f;
        for (int dy = -kD; dy <= kD; ++dy) {
            const int sy = py - dy;                                   // q - d, row
            const bool oky = inside && sy >= 0 && sy < H;
            const int syc = min(max(sy, 0), H - 1);
            float go[kND], gs[kND];
#pragma unroll
            for (int dx = -kD; dx <= kD; ++dx) {                      // 36 independent loads in flight, clamped addresses
                const int64_t dpl = (int64_t)((dy + kD) * kND + (dx + kD)) * plane;
                const int sx = px - dx;
                const int64_t so = dpl + syc * W + min(max(sx, 0), W - 1);
                const float g0 = gyb[dpl + pin], y0 = yb[dpl + pin], g1 = gyb[so], y1 = yb[so];
                go[dx + kD] = inside ? gval(g0, y0, a.scale, a.slope) : 0.0f;
                gs[dx + kD] = (oky && sx >= 0 && sx < W) ? gval(g1, y1, a.scale, a.slope) : 0.0f;
            }
#pragma unroll
            for (int dx = -kD; dx <= kD; ++dx) {
                const int ow = (ly + dy + kD) * kWinW + (lx + dx + kD);   // p + d in the window
                const int sw = (ly - dy + kD) * kWinW + (lx - dx + kD);   // q - d in the window
#pragma unroll
                for (int c = 0; c < kCC; ++c) {
                    a1[c] = fmaf(go[dx + kD], s2[c][ow], a1[c]);
                    a2[c] = fmaf(gs[dx + kD], s1[c][sw], a2[c]);
                }
            }
        }

        if (inside) {
#pragma unroll
            for (int c = 0; c < kCC; ++c)
                if (c < nc) {
                    a.gc1[obase + (int64_t)(c0 + c) * plane + pix] = a1[c];
                    if constexpr (!WARP) a.gc2[obase + (int64_t)(c0 + c) * plane + pix] = a2[c];
                }
        }
        if constexpr (WARP) {
#pragma unroll
            for (int c = 0; c < kCC; ++c) {
                if (c >= nc) continue;                        // uniform
                const int cg = c0 + c;
                unsigned long long *buf = sacc[cg & 1];
                if (keep) {
                    const float g = a2[c];
                    const float *src = c2b + (int64_t)cg * plane;
                    const float s00 = v00 ? src[o00] : 0.f, s01 = v01 ? src[o01] : 0.f;
                    const float s10 = v10 ? src[o10] : 0.f, s11 = v11 ? src[o11] : 0.f;
                    dix += g * (ay0 * (s01 - s00) + ay1 * (s11 - s10));
                    diy += g * (ax0 * (s10 - s00) + ax1 * (s11 - s01));
                    const int64_t cb = obase + (int64_t)cg * plane;
                    const int ot[4] = {o00, o01, o10, o11};
                    const float wv[4] = {w00, w01, w10, w11};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (wv[k] == 0.f) continue;
                        const float v = g * wv[k];
                        if (fixed) {
                            const unsigned long long iv = (unsigned long long)__double2ll_rn((double)v * (double)fscale);
                            if (lidx[k] >= 0) atomicAdd(&buf[lidx[k]], iv);
                            else atomicAdd(a.acc + cb + ot[k], iv);
                        } else {
                            atomicAdd(reinterpret_cast<float *>(a.acc) + cb + ot[k], v);
                        }
                    }
                }
                __syncthreads();
                if (fixed) {                                  // flush: one 64-bit add per touched element, row-contiguous
                    const int64_t cb = obase + (int64_t)cg * plane;
                    for (int i = t; i < kSrcPix; i += kThreads) {
                        const unsigned long long v = buf[i];
                        if (v) {
                            const int r = sr0 + i / kSrcW, cc = sc0 + i % kSrcW;
                            if (r < H && cc < W) atomicAdd(a.acc + cb + (int64_t)r * W + cc, v);
                            buf[i] = 0ull;
                        }
                    }
                }
            }
        }
    }
    if constexpr (WARP) {
        if (inside) {
            float *gp = a.gfp + ((int64_t)b * gridDim.y + blockIdx.y) * 2 * plane + pix;
            gp[0] = keep ? dix : 0.f;
            gp[plane] = keep ? diy : 0.f;
        }
    }
}

// grad_flo = flow_scale * d(ix, iy)/d(u, v) * sum over the chunks' partial sums, in chunk order (deterministic)
__global__ void __launch_bounds__(256)
flo_reduce_kernel(const float *__restrict__ gfp, int nchunk, int64_t plane, int64_t n, float fx, float fy, float flow_scale,
                  float *__restrict__ gflo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t b = i / plane, p = i - b * plane;
    const float *src = gfp + b * nchunk * 2 * plane + p;
    float u = 0.f, v = 0.f;
    for (int k = 0; k < nchunk; ++k, src += 2 * plane) {
        u += src[0];
        v += src[plane];
    }
    gflo[b * 2 * plane + p] = u * flow_scale * fx;
    gflo[b * 2 * plane + plane + p] = v * flow_scale * fy;
}

// workspace -> grad_c2: fixed-point integers / scale, or (non-finite fallback) the float sums kept in the workspace's first half
__global__ void __launch_bounds__(256)
fixed_to_float_kernel(const unsigned long long *__restrict__ acc, const unsigned *__restrict__ mbits, float gmul,
                      float *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float fscale;
    if (fixed_mode(mbits, gmul, &fscale)) out[i] = (float)((double)(long long)acc[i] / (double)fscale);
    else out[i] = reinterpret_cast<const float *>(acc)[i];
}

}  // namespace

extern "C" int64_t pwc_warp_corr81_bwd_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return -1;
    // int64 accumulators + max|gy|, max|c1| + the per-chunk grad_flo partial sums
    return (int64_t)B * C * H * W * 8 + 16 + (int64_t)B * ((C + kCC - 1) / kCC) * 2 * H * W * 4;
}

extern "C" int pwc_warp_corr81_bwd(const void *c1, const void *c2, const void *flo, const void *y, const void *gy,
                                   void *grad_c1, void *grad_c2, void *grad_flo, int B, int C, int H, int W,
                                   float flow_scale, int align_corners, float mask_threshold, float corr_multiply,
                                   unsigned flags, float leaky_slope,
                                   int64_t c1_bstride, int64_t c2_bstride, int64_t flo_bstride, int64_t y_bstride, int64_t gy_bstride,
                                   void *workspace, int64_t workspace_bytes, void *stream) {
    const bool warp = flo != nullptr, leaky = (flags & PWC_ACT_LEAKY) != 0;
    if (!c1 || !c2 || !gy || !grad_c1 || !grad_c2 || (leaky && !y) || (warp && (!grad_flo || !workspace)))
        PWC_FAIL(PWC_EINVAL, "pwc_warp_corr81_bwd: null pointer (y is needed with PWC_ACT_LEAKY, grad_flo and workspace with flo)");
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) PWC_FAIL(PWC_EINVAL, "pwc_warp_corr81_bwd: bad shape %dx%dx%dx%d", B, C, H, W);
    const int64_t plane = (int64_t)H * W;
    if (c1_bstride < C * plane || c2_bstride < C * plane || gy_bstride < 81 * plane || (leaky && y_bstride < 81 * plane) ||
        (warp && flo_bstride < 2 * plane))
        PWC_FAIL(PWC_EINVAL, "pwc_warp_corr81_bwd: batch stride smaller than the tensor");
    const int64_t nel = (int64_t)B * C * plane;
    if (warp && (workspace_bytes < pwc_warp_corr81_bwd_workspace_bytes(B, C, H, W) || (reinterpret_cast<uintptr_t>(workspace) & 7u)))
        PWC_FAIL(PWC_EINVAL, "pwc_warp_corr81_bwd: workspace needs %lld bytes, 8-byte aligned",
                 (long long)pwc_warp_corr81_bwd_workspace_bytes(B, C, H, W));
    const uintptr_t al = reinterpret_cast<uintptr_t>(c1) | reinterpret_cast<uintptr_t>(c2) | reinterpret_cast<uintptr_t>(flo) |
                         reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(grad_c1) |
                         reinterpret_cast<uintptr_t>(grad_c2) | reinterpret_cast<uintptr_t>(grad_flo);
    if ((al & 3u) || (int64_t)(C > 81 ? C : 81) * plane >= 0x7fffffffLL) {
        pwc::set_error("pwc_warp_corr81_bwd: needs 4-byte aligned operands and max(C, 81)*H*W < 2^31 (use pwc_warp_fwd + pwc_corr_bwd + pwc_warp_bwd)");
        return PWC_EUNSUPPORTED;
    }
    const int tiles_x = (W + kTW - 1) / kTW, tiles_y = (H + kTH - 1) / kTH;
    const int64_t nblk = (int64_t)B * tiles_x * tiles_y;
    const int nchunk = (C + kCC - 1) / kCC;
    if (nblk > 0x7fffffffLL || (nel + 255) / 256 > 0x7fffffffLL || nchunk > 65535) {
        pwc::set_error("pwc_warp_corr81_bwd: grid too large (use pwc_warp_fwd + pwc_corr_bwd + pwc_warp_bwd)");
        return PWC_EUNSUPPORTED;
    }
    // channel chunks spread over grid.y until the launch has ~1024 workgroups (4 per CU at one per CU at a time): levels with few
    // tiles (5..3, small batches) no longer run 8-13 chunks in series in a handful of workgroups, while a launch that fills the
    // chip (level 2 at batch 16: 1792 tiles) keeps its chunks in one workgroup and pays the taps / window origin once per tile
    const int ny = nblk >= 1024 ? 1 : (int)((1024 + nblk - 1) / nblk < nchunk ? (1024 + nblk - 1) / nblk : nchunk);
    const float scale = (flags & PWC_CORR_NORMALIZE) ? 1.0f / (float)C : corr_multiply;
    if (!leaky) {                                             // act' = 1: the kernel's mask select then keeps gy everywhere
        y = gy;
        y_bstride = gy_bstride;
        leaky_slope = 1.0f;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    Args a{static_cast<const float *>(c1), static_cast<const float *>(c2), static_cast<const float *>(flo),
           static_cast<const float *>(y), static_cast<const float *>(gy), static_cast<float *>(grad_c1),
           static_cast<float *>(grad_c2), nullptr, nullptr, nullptr, C, H, W, tiles_x, tiles_y,
           c1_bstride, c2_bstride, flo_bstride, y_bstride, gy_bstride, flow_scale, mask_threshold, scale, leaky_slope,
           align_corners ? 1 : 0, leaky ? 1 : 0};
    if (!warp) {                                              // level 6: gw2 IS grad_c2, no scatter
        hipLaunchKernelGGL(warp_corr81_bwd_kernel<false>, dim3((unsigned)nblk, (unsigned)ny), dim3(kThreads), 0, st, a);
        return pwc::check_launch("warp_corr81_bwd_kernel<nowarp>");
    }
    unsigned long long *acc = static_cast<unsigned long long *>(workspace);
    unsigned *mbits = reinterpret_cast<unsigned *>(acc + nel);
    a.acc = acc;
    a.mbits = mbits;
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)nel * 8 + 16, st);
    if (e != hipSuccess) { pwc::set_error("pwc_warp_corr81_bwd: hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
    a.gfp = reinterpret_cast<float *>(mbits + 4);              // 16 bytes after the accumulators: the grad_flo partials
    pwc::launch_absmax_bits(static_cast<const float *>(gy), (int64_t)81 * plane, gy_bstride, B, mbits, st);
    pwc::launch_absmax_bits(static_cast<const float *>(c1), (int64_t)C * plane, c1_bstride, B, mbits + 1, st);
    hipLaunchKernelGGL(warp_corr81_bwd_kernel<true>, dim3((unsigned)nblk, (unsigned)ny), dim3(kThreads), 0, st, a);
    const float fx = align_corners ? (float)(W - 1) / (float)(W > 1 ? W - 1 : 1) : (float)W / (float)(W > 1 ? W - 1 : 1);
    const float fy = align_corners ? (float)(H - 1) / (float)(H > 1 ? H - 1 : 1) : (float)H / (float)(H > 1 ? H - 1 : 1);
    hipLaunchKernelGGL(flo_reduce_kernel, dim3((unsigned)(((int64_t)B * plane + 255) / 256)), dim3(256), 0, st,
                       static_cast<const float *>(a.gfp), ny, plane, (int64_t)B * plane, fx, fy, flow_scale,
                       static_cast<float *>(grad_flo));
    const float gmul = fabsf(scale) * fmaxf(1.0f, fabsf(leaky_slope));
    hipLaunchKernelGGL(fixed_to_float_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, st,
                       static_cast<const unsigned long long *>(acc), static_cast<const unsigned *>(mbits), gmul,
                       static_cast<float *>(grad_c2), nel);
    return pwc::check_launch("warp_corr81_bwd_kernel");
}
