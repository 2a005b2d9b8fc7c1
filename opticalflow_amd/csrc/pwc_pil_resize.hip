// Pillow-exact bilinear resize on the device (opticalflow_amd/pil_resize.py): the first stage of train_pseudo.py / train_fundamental.py /
// inference.py (transforms.Resize -> ToTensor -> Normalize on 8-bit RGB frames) and inference.py's resize_flow (mode "F" planes).
//
// Pillow's BILINEAR is a separable triangle filter whose support widens with the scale factor.  Per axis the host makes a bounds
// table [O][2] (first tap, number of taps) and a coefficient table [O][ksize]; the kernels only apply them:
//   frames : sample = clip8((2^21 + sum_t src[first + t] * k[t]) >> 22) in int32, the horizontal pass first and ROUNDED TO BYTES,
//            the vertical pass on those bytes, then lut[c][byte] (ToTensor + Normalize as a 3 x 256 float table made with torch).
//   planes : ss = 0.0; ss += (double)src[first + t] * w[t] in tap order (separate multiply and add: -ffp-contract=off), (float)ss;
//            horizontal first with a float intermediate; an optional per-channel float factor after the second pass.
// Image.resize takes no pass on an axis whose length does not change (and copies when neither does).  The planes kernel does the
// same: with iw == ow its horizontal stage copies the source sample, with ih == oh its vertical stage copies the staged one (both
// conditions hold for a whole launch, so the host picks one of four instantiations), so -0.0, infinities and NaN stay where they are -- the identity table (0 * left + 1 * x
// on top of ss = 0.0) would turn -0.0 into +0.0 and spread an inf or a NaN to the neighbour as NaN.  The frames kernel needs no such
// branch: the identity coefficient is exactly 2^22 and (2^21 + v * 2^22) >> 22 == v for every byte, so applying the table IS the copy.
// Image.resize also takes the VERTICAL pass first when H > 100 * W and h < H.  The kernels here are single-order, horizontal first;
// opticalflow_amd/pil_resize.py composes that regime from two launches, (H, W) -> (h, W) and (h, W) -> (h, w), each a one-axis resize.
// One launch.  A workgroup owns a 16 x 64 output tile of one image: it resamples the source rows its tile needs (they follow from the
// vertical bounds of the tile's first and last row) horizontally into LDS and takes the vertical pass from there.  Frames: the
// source bytes of a batch of rows come in as aligned dwords with the lanes along x (the taps of neighbouring outputs overlap, and a
// byte load per tap from global memory took 2.2x the time at 1080x1920 -> 384x512), the taps are then byte reads of LDS; the resampled rows are staged as
// interleaved RGB bytes, so a thread of the vertical pass reads 12 contiguous bytes (4 pixels x 3 channels) per tap and ends with
// three 16-byte stores, one per output plane.  The LDS of a launch is sized by its scale factors (dynamic), not by the largest one.
#include <stdint.h>
#include <math.h>

#include "pwc_block_reduce.h"
#include "pwc_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTH = 16, kTW = 64;          // output tile
constexpr int kMaxScale = 8;               // supported: in <= 8 * out per axis (an upscale has 3-tap rows whatever its factor), see axis_fits
constexpr int kMaxK = 2 * kMaxScale + 1;   // ksize at that downscale: a tile's table slice holds kTW (kTH) rows of it
// staged rows of a tile: the centres of 16 output rows span 15 * scale <= 120 source rows, the support adds <= 8 on each side and the
// two roundings of the bounds at most 1 more: 137
constexpr int kMaxRows = 144;
constexpr int kPitchB = kTW * 3 + 4;       // frame staging: 192 bytes of a row + one dword, so rows start on different banks
constexpr int kMaxDim = 1 << 20;

// bounds of a table row as the kernel uses them: whatever the table holds, no tap leaves [0, in)
__device__ __forceinline__ int2 safe_bounds(const int32_t *__restrict__ b, int i, int in, int ksize) {
    const int first = min(max(b[2 * i], 0), in - 1);
    const int cnt = min(min(max(b[2 * i + 1], 0), ksize), in - first);
    return make_int2(first, cnt);
}

__device__ __forceinline__ int clip8(int v) { return min(max(v >> 22, 0), 255); }

// unaligned source bytes as aligned dwords: the dword at `p`, and where it is not wholly inside [lo, hi) its inside bytes alone
__device__ __forceinline__ uint32_t load_dword_within(const uint8_t *p, const uint8_t *lo, const uint8_t *hi) {
    if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t *>(p);
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (p + i >= lo && p + i < hi) v |= (uint32_t)p[i] << (8 * i);
    return v;
}

// dynamic LDS: [rows_cap][kPitchB] horizontally resampled rows of the tile, then [raw_rows][raw_pitch] source bytes of one row batch
__global__ void __launch_bounds__(256)
pil_frames_kernel(const uint8_t *__restrict__ src, float *__restrict__ out, uint8_t *__restrict__ out8, int H, int W, int h, int w,
                  const int32_t *__restrict__ xb, const int32_t *__restrict__ xk, int xks, const int32_t *__restrict__ yb,
                  const int32_t *__restrict__ yk, int yks, const float *__restrict__ lut, int64_t bso, int group, int vec,
                  int rows_cap, int raw_pitch, int raw_rows, int64_t src_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    __shared__ int32_t s_xk[kTW * kMaxK], s_yk[kTH * kMaxK];
    __shared__ int2 s_xb[kTW], s_yb[kTH];
    __shared__ float s_lut[768];
    uint8_t *s_rows = s_dyn, *s_raw = s_dyn + rows_cap * kPitchB;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH, f = blockIdx.z;
    const int tw = min(kTW, w - x0), th = min(kTH, h - y0);

    for (int i = tid; i < 768; i += 256) s_lut[i] = lut[i];
    if (tid < tw) s_xb[tid] = safe_bounds(xb, x0 + tid, W, xks);
    if (tid >= 64 && tid < 64 + th) s_yb[tid - 64] = safe_bounds(yb, y0 + tid - 64, H, yks);
    for (int i = tid; i < tw * xks; i += 256) s_xk[i] = xk[(int64_t)x0 * xks + i];
    for (int i = tid; i < th * yks; i += 256) s_yk[i] = yk[(int64_t)y0 * yks + i];
    __syncthreads();

    // source rows of this tile: first tap of its first row .. last tap of its last row (both bounds grow with y), and its source
    // columns likewise.  A column keeps only the taps a raw row has room for (all of them, with tables the host made).
    const int r0 = s_yb[0].x;
    const int rows = min(max(s_yb[th - 1].x + s_yb[th - 1].y - r0, 0), rows_cap);
    const int xlo = s_xb[0].x;
    const int2 mine = s_xb[min(tid, tw - 1)];
    __syncthreads();
    if (tid < tw) s_xb[tid] = make_int2(max(mine.x - xlo, 0), max(min(mine.y, (raw_pitch - 3) / 3 - max(mine.x - xlo, 0)), 0));
    __syncthreads();
    const int span = (s_xb[tw - 1].x + s_xb[tw - 1].y) * 3;      // source bytes of a row, <= raw_pitch - 3
    const int pd = raw_pitch >> 2;
    const uint8_t *img = src + (int64_t)f * H * W * 3 + (int64_t)xlo * 3;

    for (int rb = 0; rb < rows; rb += raw_rows) {
        const int nr = min(raw_rows, rows - rb);
        // the batch's source bytes as aligned dwords, lanes along x
        for (int it = tid; it < nr * pd; it += 256) {
            const int r = it / pd, d = it - r * pd;
            const uint8_t *row = img + (int64_t)(r0 + rb + r) * W * 3;
            const int shift = (int)(reinterpret_cast<uintptr_t>(row) & 3);
            if (4 * d < shift + span)
                *reinterpret_cast<uint32_t *>(s_raw + r * raw_pitch + 4 * d) = load_dword_within(row - shift + 4 * d, src, src + src_bytes);
        }
        __syncthreads();
        // horizontal pass: one thread = one dword of a staged row = 4 interleaved bytes (x, c) = (j / 3, j % 3)
        for (int it = tid; it < nr * (kTW * 3 / 4); it += 256) {
            const int r = it / (kTW * 3 / 4), q = it - r * (kTW * 3 / 4);
            const int shift = (int)(reinterpret_cast<uintptr_t>(img + (int64_t)(r0 + rb + r) * W * 3) & 3);
            const uint8_t *row = s_raw + r * raw_pitch + shift;
            uint32_t packed = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = 4 * q + i, xl = j / 3, c = j - 3 * xl;
                if (xl < tw) {
                    const int2 b = s_xb[xl];
                    const uint8_t *p = row + b.x * 3 + c;
                    const int32_t *k = s_xk + xl * xks;
                    int ss = 1 << 21;
                    for (int t = 0; t < b.y; ++t) ss += (int)p[3 * t] * k[t];
                    packed |= (uint32_t)clip8(ss) << (8 * i);
                }
            }
            *reinterpret_cast<uint32_t *>(s_rows + (rb + r) * kPitchB + 4 * q) = packed;
        }
        __syncthreads();
    }

    // vertical pass: one thread = 4 pixels x 3 channels of one output row
    const int yl = tid >> 4, xq = tid & 15;
    if (yl >= th || 4 * xq >= tw) return;
    const int2 b = s_yb[yl];
    int ss[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) ss[i] = 1 << 21;
    for (int t = 0; t < b.y; ++t) {
        const int r = min(b.x - r0 + t, rows_cap - 1);
        const uint32_t *p = reinterpret_cast<const uint32_t *>(s_rows + r * kPitchB + 12 * xq);
        const int k = s_yk[yl * yks + t];
        const uint32_t d[3] = {p[0], p[1], p[2]};
#pragma unroll
        for (int i = 0; i < 12; ++i) ss[i] += (int)((d[i >> 2] >> (8 * (i & 3))) & 255u) * k;
    }
    int v[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = clip8(ss[i]);

    const int y = y0 + yl, x = x0 + 4 * xq;
    const int b_out = f % group, half = f / group;
    float *o = out + (int64_t)b_out * bso + ((int64_t)(3 * half) * h + y) * w + x;
    const int64_t plane = (int64_t)h * w;
    if (vec) {                                   // w % 4 == 0 and every plane row 16-byte aligned: the quad is whole
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<f32x4 *>(o + c * plane) =
                (f32x4){s_lut[c * 256 + v[c]], s_lut[c * 256 + v[3 + c]], s_lut[c * 256 + v[6 + c]], s_lut[c * 256 + v[9 + c]]};
    } else {
        for (int px = 0; px < 4 && x + px < w; ++px)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c * plane + px] = s_lut[c * 256 + v[3 * px + c]];
    }
    if (out8) {
        uint8_t *o8 = out8 + (((int64_t)f * h + y) * w + x) * 3;
        const int nb = 3 * min(4, w - x);
        for (int i = 0; i < 12; ++i)
            if (i < nb) o8[i] = (uint8_t)v[i];
    }
}

// The planes kernel and the flow-evaluation kernel share their three steps: the tile's slices of the tables, the horizontal stage
// into LDS and the vertical stage of one output pixel.
// kCopyX / kCopyY: the axis keeps its length (iw == ow / ih == oh), so Pillow takes no pass on it and the stage copies.  Compile-time,
// so that the instantiation with both passes is the code it was before the copies existed.
struct PlaneTables {
    double *xk, *yk;                           // [kTW][xks], [kTH][yks]
    int2 *xb, *yb;                             // [kTW], [kTH]
};

// the tile's table slices into LDS; ends with a barrier
__device__ __forceinline__ void planes_load_tables(const PlaneTables &s, const int32_t *__restrict__ xb, const double *__restrict__ xk,
                                                   int xks, const int32_t *__restrict__ yb, const double *__restrict__ yk, int yks, int iw,
                                                   int ih, int x0, int y0, int tw, int th) {
    const int tid = threadIdx.x;
    if (tid < tw) s.xb[tid] = safe_bounds(xb, x0 + tid, iw, xks);
    if (tid >= 64 && tid < 64 + th) s.yb[tid - 64] = safe_bounds(yb, y0 + tid - 64, ih, yks);
    for (int i = tid; i < tw * xks; i += 256) s.xk[i] = xk[(int64_t)x0 * xks + i];
    for (int i = tid; i < th * yks; i += 256) s.yk[i] = yk[(int64_t)y0 * yks + i];
    __syncthreads();
}

// horizontal stage: source rows r0 .. r0 + rows of one plane, resampled to the tile's columns, into s_rows[rows][kTW]
template <bool kCopyX>
__device__ __forceinline__ void planes_stage_rows(const float *__restrict__ img, float *s_rows, const PlaneTables &s, int xks, int iw, int x0,
                                                  int tw, int r0, int rows) {
    for (int it = threadIdx.x; it < rows * kTW; it += 256) {
        const int r = it >> 6, xl = it & 63;
        float o = 0.f;
        if (kCopyX) {                            // unchanged axis: Pillow takes no horizontal pass, the sample is copied
            if (xl < tw) o = img[(int64_t)(r0 + r) * iw + x0 + xl];
        } else if (xl < tw) {
            const int2 b = s.xb[xl];
            const float *p = img + (int64_t)(r0 + r) * iw + b.x;
            const double *k = s.xk + xl * xks;
            double ss = 0.0;
            for (int t = 0; t < b.y; ++t) ss += (double)p[t] * k[t];
            o = (float)ss;
        }
        s_rows[it] = o;
    }
}

// vertical stage of output pixel (yl, xl) of the tile, from the staged rows
template <bool kCopyY>
__device__ __forceinline__ float planes_finish(const float *s_rows, const PlaneTables &s, int yks, int y0, int yl, int xl, int r0, int rows_cap) {
    if (kCopyY)                                  // unchanged axis: no vertical pass, output row y is staged row y - r0
        return s_rows[min(max(y0 + yl - r0, 0), rows_cap - 1) * kTW + xl];
    const int2 b = s.yb[yl];
    const double *k = s.yk + yl * yks;
    double ss = 0.0;
    for (int t = 0; t < b.y; ++t) ss += (double)s_rows[min(b.x - r0 + t, rows_cap - 1) * kTW + xl] * k[t];
    return (float)ss;
}

template <bool kCopyX, bool kCopyY>
__global__ void __launch_bounds__(256)
pil_planes_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int ih, int iw, int oh, int ow,
                  const int32_t *__restrict__ xb, const double *__restrict__ xk, int xks, const int32_t *__restrict__ yb,
                  const double *__restrict__ yk, int yks, const float *__restrict__ factors, int64_t bss, int rows_cap) {
    extern __shared__ __attribute__((aligned(16))) float s_rows[];          // [rows_cap][kTW]
    __shared__ double s_xk[kTW * kMaxK], s_yk[kTH * kMaxK];
    __shared__ int2 s_xb[kTW], s_yb[kTH];
    const PlaneTables s{s_xk, s_yk, s_xb, s_yb};
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int n = blockIdx.z / C, c = blockIdx.z - n * C;
    const int tw = min(kTW, ow - x0), th = min(kTH, oh - y0);
    planes_load_tables(s, xb, xk, xks, yb, yk, yks, iw, ih, x0, y0, tw, th);

    const int r0 = s_yb[0].x;
    const int rows = min(max(s_yb[th - 1].x + s_yb[th - 1].y - r0, 0), rows_cap);
    planes_stage_rows<kCopyX>(src + (int64_t)n * bss + (int64_t)c * ih * iw, s_rows, s, xks, iw, x0, tw, r0, rows);
    __syncthreads();

    const float fac = factors ? factors[c] : 1.0f;
    float *o = dst + ((int64_t)blockIdx.z * oh + y0) * ow + x0;
    for (int it = tid; it < th * kTW; it += 256) {
        const int yl = it >> 6, xl = it & 63;
        if (xl >= tw) continue;
        const float v = planes_finish<kCopyY>(s_rows, s, yks, y0, yl, xl, r0, rows_cap);
        o[(int64_t)yl * ow + xl] = factors ? v * fac : v;
    }
}

// ---- inference.py's resized flow, scored and / or encoded where it is made (include/pwc_hip.h pwc_pil_flow_eval) ----
// One workgroup makes BOTH channels of its tile: u is staged and finished into registers (lane tid owns column tid % 64 of the rows
// tid / 64 + 4 k, the planes kernel's own mapping), then the same LDS stages v.  What follows per pixel is pwc_kitti_score's
// arithmetic (csrc/pwc_kitti_score.hip) on a prediction that never leaves the registers.
constexpr int kPix = kTH * kTW / 256;          // 4 pixels per lane
using EvalRec = pwc::TilePartial<2>;           // {double sum_epe, int64 {valid, outliers}}: one per sample, then one per tile
static_assert(sizeof(pwc::TreeLds<256, 1, 2>) <= sizeof(double) * kTW * kMaxK, "the tile reduction reuses the x coefficient slice");

struct EvalOut {
    const void *gt;
    const uint8_t *valid;
    float *flow;
    uint16_t *enc;
    EvalRec *part;
    int enc_order;
};

// three consecutive uint16 at a 2-byte aligned address as one dword and one short, the dword wherever the address allows it
__device__ __forceinline__ void store3_u16(uint16_t *p, uint32_t s0, uint32_t s1, uint32_t s2) {
    if ((reinterpret_cast<uintptr_t>(p) & 2u) == 0) {
        *reinterpret_cast<uint32_t *>(p) = s0 | (s1 << 16);
        p[2] = (uint16_t)s2;
    } else {
        p[0] = (uint16_t)s0;
        *reinterpret_cast<uint32_t *>(p + 1) = s1 | (s2 << 16);
    }
}

// save_flow's sample: (uint16)(int)(x * 64 + 2^15) in float32, truncated toward zero; clamped to [0, 65535], NaN -> 0
__device__ __forceinline__ uint32_t encode16(float x) {
    const float t = x * 64.0f + 32768.0f;
    return (uint32_t)(int)(t > 0.0f ? fminf(t, 65535.0f) : 0.0f);
}

// KIND: -1 no ground truth, 0 float planes (+ uint8 validity), 1 uint16 {u, v, valid}, 2 uint16 {valid, v, u}
template <bool kCopyX, bool kCopyY, int KIND>
__global__ void __launch_bounds__(256)
pil_flow_eval_kernel(const float *__restrict__ src, int ih, int iw, int oh, int ow, const int32_t *__restrict__ xb,
                     const double *__restrict__ xk, int xks, const int32_t *__restrict__ yb, const double *__restrict__ yk, int yks,
                     const float *__restrict__ factors, int64_t bss, int rows_cap, EvalOut e) {
    extern __shared__ __attribute__((aligned(16))) float s_rows[];          // [rows_cap][kTW]
    __shared__ double s_xk[kTW * kMaxK], s_yk[kTH * kMaxK];
    __shared__ int2 s_xb[kTW], s_yb[kTH];
    const PlaneTables s{s_xk, s_yk, s_xb, s_yb};
    const int tid = threadIdx.x, n = blockIdx.z;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int tw = min(kTW, ow - x0), th = min(kTH, oh - y0);
    const int xl = tid & 63, yl0 = tid >> 6;
    const bool in_x = xl < tw;
    const int64_t npix = (int64_t)oh * ow;

    planes_load_tables(s, xb, xk, xks, yb, yk, yks, iw, ih, x0, y0, tw, th);

    const int r0 = s_yb[0].x;
    const int rows = min(max(s_yb[th - 1].x + s_yb[th - 1].y - r0, 0), rows_cap);
    float p[2][kPix];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        planes_stage_rows<kCopyX>(src + (int64_t)n * bss + (int64_t)c * ih * iw, s_rows, s, xks, iw, x0, tw, r0, rows);
        __syncthreads();
        const float fac = factors ? factors[c] : 1.0f;
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const int yl = yl0 + 4 * k;
            float v = 0.f;
            if (in_x && yl < th) {
                v = planes_finish<kCopyY>(s_rows, s, yks, y0, yl, xl, r0, rows_cap);
                if (factors) v = v * fac;
            }
            p[c][k] = v;
        }
        __syncthreads();                         // the staged rows of u are read; v (or the reduction) may take the LDS
    }

    double sum = 0.0;
    long long cnt[2] = {0, 0};                   // valid, outliers
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        const int yl = yl0 + 4 * k;
        if (!in_x || yl >= th) continue;
        const int64_t pix = (int64_t)(y0 + yl) * ow + x0 + xl;
        const float pu = p[0][k], pv = p[1][k];
        if (e.flow) {
            e.flow[(int64_t)n * 2 * npix + pix] = pu;
            e.flow[((int64_t)n * 2 + 1) * npix + pix] = pv;
        }
        if (e.enc) {
            const uint32_t eu = encode16(pu), ev = encode16(pv);
            uint16_t *o = e.enc + ((int64_t)n * npix + pix) * 3;
            if (e.enc_order == 0) store3_u16(o, 1u, ev, eu);
            else store3_u16(o, eu, ev, 1u);
        }
        if (KIND >= 0) {
            // a uint16 pixel is three 2-byte loads: a wave's 64 pixels are 384 contiguous bytes and the loads share their cache lines
            // (as in pwc_kitti_score)
            float gu, gv;
            bool ok;
            if (KIND == 0) {
                const float *f = static_cast<const float *>(e.gt) + (int64_t)n * 2 * npix + pix;
                gu = f[0];
                gv = f[npix];
                ok = e.valid ? e.valid[(int64_t)n * npix + pix] != 0 : true;
            } else {
                const uint16_t *q = static_cast<const uint16_t *>(e.gt) + ((int64_t)n * npix + pix) * 3;
                gu = ((float)q[KIND == 1 ? 0 : 2] - 32768.0f) / 64.0f;
                gv = ((float)q[1] - 32768.0f) / 64.0f;
                ok = q[KIND == 1 ? 2 : 0] != 0;
            }
            if (!ok) continue;
            const float du = pu - gu, dv = pv - gv;
            const float epe = sqrtf(du * du + dv * dv);
            const float mag = sqrtf(gu * gu + gv * gv);
            sum += (double)epe;
            ++cnt[0];
            if (epe > fmaxf(3.0f, 0.05f * mag)) ++cnt[1];
        }
    }
    if (KIND >= 0) {
        // the x coefficient slice was last read before the barriers above
        pwc::TreeLds<256, 1, 2> &red = *reinterpret_cast<pwc::TreeLds<256, 1, 2> *>(s_xk);
        pwc::tree_sum(red, &sum, cnt);
        if (tid == 0) e.part[blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z)] = EvalRec{sum, {cnt[0], cnt[1]}};
    }
}

// workgroup b adds the tiles of sample b in tile order (as pwc_kitti_score's finish does)
__global__ __launch_bounds__(256) void pil_flow_eval_finish_kernel(EvalRec *__restrict__ ws, int n, int64_t tiles, float *__restrict__ out) {
    __shared__ pwc::TreeLds<256, 1, 2> red;
    const int tid = threadIdx.x, b = blockIdx.x;
    const EvalRec *part = ws + n + (int64_t)b * tiles;
    double s = 0.0;
    long long cnt[2] = {0, 0};
    for (int64_t i = tid; i < tiles; i += 256) {
        s += part[i].sum;
        cnt[0] += part[i].count[0];
        cnt[1] += part[i].count[1];
    }
    pwc::tree_sum(red, &s, cnt);
    if (tid == 0) {
        ws[b] = EvalRec{s, {cnt[0], cnt[1]}};
        const long long nv = cnt[0], no = cnt[1];
        const float nan = __builtin_nanf("");
        out[2 * b] = nv ? (float)(s / (double)nv) : nan;
        out[2 * b + 1] = nv ? (float)(100.0 * (double)no / (double)nv) : nan;
    }
}

// ksize of Pillow's coefficient rows for one axis, whatever the scale; 0 for sizes that are not positive or above 2^20
int axis_ksize(int in, int out) {
    if (in <= 0 || out <= 0 || in > kMaxDim || out > kMaxDim) return 0;
    const double scale = (double)in / (double)out;
    const double k = 2.0 * ceil(scale < 1.0 ? 1.0 : scale) + 1.0;
    return k > (double)(1 << 22) ? 0 : (int)k;
}

// upper bound of the source samples under `tile` consecutive outputs of one axis: the first tap is >= c0 - support - 0.5, the end of
// the last <= c1 + support + 0.5 and c1 - c0 = (tile - 1) * scale
int span_bound(int in, int out, int tile) {
    const double scale = (double)in / (double)out;
    const int64_t b = (int64_t)ceil((tile - 1) * scale) + 2 * (int64_t)ceil(scale < 1.0 ? 1.0 : scale) + 2;
    return (int)(b < in ? b : in);
}
constexpr int kMaxCols = (kTW - 1) * kMaxScale + 2 * kMaxScale + 2;          // source columns under a tile at the largest downscale
static_assert((kTH - 1) * kMaxScale + 2 * kMaxScale + 2 <= kMaxRows, "a tile's staged rows fit the LDS budget at the largest downscale");

// What the kernels stage per tile decides the range: the tile's slice of the coefficient table (`tile` rows of kMaxK entries) and the
// source span under it (`max_span` samples).  Every in <= kMaxScale * out fits (ksize <= kMaxK and the spans above); so does a
// stronger downscale to an output shorter than a tile whose few, longer coefficient rows and short source still fit, e.g. 16 -> 1.
bool axis_fits(int in, int out, int tile, int max_span) {
    const int ks = axis_ksize(in, out);
    if (!ks) return false;
    return (int64_t)(out < tile ? out : tile) * ks <= (int64_t)tile * kMaxK && span_bound(in, out, tile) <= max_span;
}

constexpr int kRawBudget = 8192;           // bytes of source rows staged at a time

}  // namespace

extern "C" int pwc_pil_resize_ksize(int in_size, int out_size) {
    return axis_fits(in_size, out_size, kTW, kMaxCols) ? axis_ksize(in_size, out_size) : PWC_EINVAL;
}

extern "C" int pwc_pil_resize_supported(int in_h, int in_w, int out_h, int out_w) {
    return axis_fits(in_h, out_h, kTH, kMaxRows) && axis_fits(in_w, out_w, kTW, kMaxCols) && (out_h + kTH - 1) / kTH <= 65535;
}

extern "C" int pwc_pil_resize_frames_u8(const void *frames_u8, void *out_f32, void *out_u8, int n, int H, int W, int h, int w,
                                        const int32_t *xbounds, const int32_t *xcoef, int xksize, const int32_t *ybounds,
                                        const int32_t *ycoef, int yksize, const float *lut768, int64_t out_bstride, int out_group,
                                        void *stream) {
    if (!frames_u8 || !out_f32 || !xbounds || !xcoef || !ybounds || !ycoef || !lut768)
        PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_frames_u8: null pointer");
    if (n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || out_group <= 0) PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_frames_u8: bad shape");
    if (!pwc_pil_resize_supported(H, W, h, w))
        PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_frames_u8: %dx%d -> %dx%d is outside the supported scale range (downscale <= 8 per axis, more only to outputs shorter than a tile)", H, W, h, w);
    if (xksize != axis_ksize(W, w) || yksize != axis_ksize(H, h))
        PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_frames_u8: ksize (%d, %d) disagrees with the sizes (%d, %d expected)", xksize, yksize,
                 axis_ksize(W, w), axis_ksize(H, h));
    const int halves = (n + out_group - 1) / out_group;
    if (out_bstride < (int64_t)3 * halves * h * w) PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_frames_u8: batch stride smaller than the tensor");
    if (n > 65535) PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_frames_u8: grid too large (n > 65535)");
    if (pwc::misaligned({out_f32, xbounds, xcoef, ybounds, ycoef, lut768}))
        PWC_FAIL(PWC_EALIGN, "pwc_pil_resize_frames_u8: out / tables must be 4-byte aligned");
    const int vec = (w % 4 == 0) && pwc::aligned16(out_f32) && (out_bstride % 4 == 0);
    const int rows_cap = span_bound(H, h, kTH);                              // <= kMaxRows inside the supported range
    int raw_pitch = (span_bound(W, w, kTW) * 3 + 3 + 3) / 4 * 4;             // a row's bytes + the 3 an unaligned start can add
    if ((raw_pitch / 4) % 2 == 0) raw_pitch += 4;                           // odd dword pitch: rows start on different banks
    const int raw_rows = kRawBudget / raw_pitch < 1 ? 1 : (kRawBudget / raw_pitch < rows_cap ? kRawBudget / raw_pitch : rows_cap);
    const int lds = rows_cap * kPitchB + raw_rows * raw_pitch;               // <= 144 * 196 + 8192 bytes
    hipLaunchKernelGGL(pil_frames_kernel, dim3((w + kTW - 1) / kTW, (h + kTH - 1) / kTH, n), dim3(256), lds, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t *>(frames_u8), static_cast<float *>(out_f32), static_cast<uint8_t *>(out_u8), H, W, h, w,
                       xbounds, xcoef, xksize, ybounds, ycoef, yksize, lut768, out_bstride, out_group, vec, rows_cap, raw_pitch, raw_rows,
                       (int64_t)n * H * W * 3);
    return pwc::check_launch("pil_frames_kernel");
}

extern "C" int pwc_pil_resize_planes_f32(const void *src, void *dst, int n, int c, int in_h, int in_w, int out_h, int out_w,
                                         const int32_t *xbounds, const double *xcoef, int xksize, const int32_t *ybounds,
                                         const double *ycoef, int yksize, const float *factors, int64_t src_bstride, void *stream) {
    if (!src || !dst || !xbounds || !xcoef || !ybounds || !ycoef) PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_planes_f32: null pointer");
    if (n <= 0 || c <= 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_planes_f32: bad shape");
    if (!pwc_pil_resize_supported(in_h, in_w, out_h, out_w))
        PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_planes_f32: %dx%d -> %dx%d is outside the supported scale range (downscale <= 8 per axis, more only to outputs shorter than a tile)", in_h, in_w,
                 out_h, out_w);
    if (xksize != axis_ksize(in_w, out_w) || yksize != axis_ksize(in_h, out_h))
        PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_planes_f32: ksize (%d, %d) disagrees with the sizes (%d, %d expected)", xksize, yksize,
                 axis_ksize(in_w, out_w), axis_ksize(in_h, out_h));
    if (src_bstride < (int64_t)c * in_h * in_w) PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_planes_f32: batch stride smaller than the tensor");
    if ((int64_t)n * c > 65535) PWC_FAIL(PWC_EINVAL, "pwc_pil_resize_planes_f32: grid too large (n * c > 65535)");
    if (pwc::misaligned({src, dst, xbounds, ybounds, factors}) || pwc::misaligned({xcoef, ycoef}, 8))
        PWC_FAIL(PWC_EALIGN, "pwc_pil_resize_planes_f32: planes / bounds must be 4-byte, coefficients 8-byte aligned");
    const int rows_cap = span_bound(in_h, out_h, kTH);
    const bool copy_x = in_w == out_w, copy_y = in_h == out_h;
    const auto kernel = copy_x ? (copy_y ? pil_planes_kernel<true, true> : pil_planes_kernel<true, false>)
                               : (copy_y ? pil_planes_kernel<false, true> : pil_planes_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((out_w + kTW - 1) / kTW, (out_h + kTH - 1) / kTH, n * c), dim3(256),
                       rows_cap * kTW * sizeof(float), static_cast<hipStream_t>(stream), static_cast<const float *>(src),
                       static_cast<float *>(dst), c, in_h, in_w, out_h, out_w, xbounds, xcoef, xksize, ybounds, ycoef, yksize, factors,
                       src_bstride, rows_cap);
    return pwc::check_launch("pil_planes_kernel");
}

extern "C" int64_t pwc_pil_flow_eval_workspace_bytes(int n, int out_h, int out_w) {
    if (n <= 0 || out_h <= 0 || out_w <= 0) return -1;
    return (int64_t)sizeof(EvalRec) * n * (1 + (int64_t)((out_h + kTH - 1) / kTH) * ((out_w + kTW - 1) / kTW));
}

namespace {

template <int KIND, typename... Args>
void launch_flow_eval(bool copy_x, bool copy_y, dim3 grid, size_t lds, hipStream_t st, Args... args) {
    const auto kernel = copy_x ? (copy_y ? pil_flow_eval_kernel<true, true, KIND> : pil_flow_eval_kernel<true, false, KIND>)
                               : (copy_y ? pil_flow_eval_kernel<false, true, KIND> : pil_flow_eval_kernel<false, false, KIND>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, args...);
}

}  // namespace

extern "C" int pwc_pil_flow_eval(const void *src, int n, int in_h, int in_w, int out_h, int out_w, const int32_t *xbounds,
                                 const double *xcoef, int xksize, const int32_t *ybounds, const double *ycoef, int yksize,
                                 const float *factors, int64_t src_bstride, const void *gt, int gt_kind, const void *valid, void *flow_out,
                                 void *enc_out, int enc_order, void *workspace, int64_t workspace_bytes, void *out, void *stream) {
    if (!src || !xbounds || !xcoef || !ybounds || !ycoef) PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: null pointer");
    if (!gt && !flow_out && !enc_out) PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: nothing requested (gt, flow_out and enc_out are all NULL)");
    if (gt && (!workspace || !out)) PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: scoring needs workspace and out");
    if (n <= 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: bad shape");
    if (!pwc_pil_resize_supported(in_h, in_w, out_h, out_w))
        PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: %dx%d -> %dx%d is outside the supported scale range (downscale <= 8 per axis, more only to outputs shorter than a tile)", in_h, in_w,
                 out_h, out_w);
    if (xksize != axis_ksize(in_w, out_w) || yksize != axis_ksize(in_h, out_h))
        PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: ksize (%d, %d) disagrees with the sizes (%d, %d expected)", xksize, yksize,
                 axis_ksize(in_w, out_w), axis_ksize(in_h, out_h));
    if (src_bstride < (int64_t)2 * in_h * in_w) PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: batch stride smaller than the tensor");
    if (gt && (gt_kind < 0 || gt_kind > 2))
        PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: unknown gt_kind %d (0 = float planes, 1 = uint16 {u, v, valid}, 2 = uint16 {valid, v, u})", gt_kind);
    if (enc_out && (enc_order < 0 || enc_order > 1))
        PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: unknown enc_order %d (0 = {1, v, u}, 1 = {u, v, 1})", enc_order);
    if (valid && (!gt || gt_kind != 0))
        PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: valid must be NULL without float ground truth (a uint16 ground truth carries its validity)");
    if (n > 65535) PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: grid too large (n > 65535)");
    if (gt) {
        const int64_t need = pwc_pil_flow_eval_workspace_bytes(n, out_h, out_w);
        if (workspace_bytes < need)
            PWC_FAIL(PWC_EINVAL, "pwc_pil_flow_eval: workspace needs %lld bytes, got %lld", (long long)need, (long long)workspace_bytes);
        if (reinterpret_cast<uintptr_t>(workspace) & 7u) PWC_FAIL(PWC_EALIGN, "pwc_pil_flow_eval: workspace must be 8-byte aligned");
    }
    if (pwc::misaligned({src, xbounds, ybounds, factors, flow_out, gt ? out : nullptr}) || pwc::misaligned({xcoef, ycoef}, 8) ||
        pwc::misaligned({enc_out}, 2) || pwc::misaligned({gt}, gt_kind == 0 ? 4 : 2))
        PWC_FAIL(PWC_EALIGN, "pwc_pil_flow_eval: needs 4-byte aligned float operands and bounds, 8-byte aligned coefficients and 2-byte aligned uint16 operands");
    const int rows_cap = span_bound(in_h, out_h, kTH);
    const bool copy_x = in_w == out_w, copy_y = in_h == out_h;
    const dim3 grid((out_w + kTW - 1) / kTW, (out_h + kTH - 1) / kTH, n);
    const size_t lds = rows_cap * kTW * sizeof(float);
    hipStream_t st = static_cast<hipStream_t>(stream);
    EvalRec *ws = static_cast<EvalRec *>(workspace);
    const EvalOut e{gt, static_cast<const uint8_t *>(valid), static_cast<float *>(flow_out), static_cast<uint16_t *>(enc_out),
                    gt ? ws + n : nullptr, enc_order};
    const float *s = static_cast<const float *>(src);
#define PWC_EVAL_ARGS s, in_h, in_w, out_h, out_w, xbounds, xcoef, xksize, ybounds, ycoef, yksize, factors, src_bstride, rows_cap, e
    if (!gt) launch_flow_eval<-1>(copy_x, copy_y, grid, lds, st, PWC_EVAL_ARGS);
    else if (gt_kind == 0) launch_flow_eval<0>(copy_x, copy_y, grid, lds, st, PWC_EVAL_ARGS);
    else if (gt_kind == 1) launch_flow_eval<1>(copy_x, copy_y, grid, lds, st, PWC_EVAL_ARGS);
    else launch_flow_eval<2>(copy_x, copy_y, grid, lds, st, PWC_EVAL_ARGS);
#undef PWC_EVAL_ARGS
    if (gt) hipLaunchKernelGGL(pil_flow_eval_finish_kernel, dim3(n), dim3(256), 0, st, ws, n, (int64_t)grid.x * grid.y, static_cast<float *>(out));
    return pwc::check_launch("pil_flow_eval_kernel");
}
