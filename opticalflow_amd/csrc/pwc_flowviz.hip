// Flow pictures on the device: the colour-wheel image of pwc_extract_flow.py:58-123 (flow_to_color), the dominant direction of
// topview.py:122-134 (calculate_dominant_direction) and the arrow grid of pwc_extract_flow_video.py:94-135 (create_quiver_frame) and
// topview.py:137-178 (draw_flow_arrows).  All three kernels read the top-left crop_h x crop_w of a [n][2][Hq][Wq] float flow with a
// free batch stride; fp32 with no contraction, the arithmetic spelled out in include/pwc_hip.h.
//
//   pwc_flow_stats   one workgroup = one 16 x 64 tile of one sample (the split of pwc_kitti_score.hip), 256 lanes; each leaves {fp64
//                    sum u, fp64 sum v, int64 count, fp32 max radius} in the workspace, the sums in tree_sum's fixed order; one final
//                    workgroup per sample adds that sample's tiles in tile order and writes the 16-byte record.  No atomics.
//   pwc_flow_color   the output is a byte stream of 3 bytes per pixel whose samples start at any byte address.  One lane owns one
//                    ALIGNED dword of that stream (counted from `out` rounded down to 4 bytes): its 4 bytes belong to at most two
//                    pixels, whose colours the lane computes; a dword that lies wholly inside the stream is one 4-byte store (a wave
//                    writes 256 contiguous bytes), the at most two dwords that straddle its ends are written byte by byte.  Nothing
//                    outside [out, out + n*crop_h*crop_w*3) is touched and no store is misaligned, whatever `out` and the sample size
//                    are.  The 55-entry wheel is built in LDS by each workgroup (integer arithmetic, then / 255.f).
//   pwc_flow_quiver  one lane per grid point: the four taps of cv2.resize's INTER_LINEAR float path at that point only, so the
//                    frame-sized flow never exists.
#include "pwc_block_reduce.h"
#include "pwc_common.h"

namespace {

constexpr int kTH = 16, kTW = 64, kThreads = 256;
constexpr int kRowStep = kThreads / kTW;      // 4
constexpr int kPix = kTH / kRowStep;          // 4 pixels per lane
constexpr int kWheel = 55;
constexpr float kPi = 3.14159274101257324f;   // (float)M_PI: numpy divides a float32 array by np.pi in float32

struct StatPart {                              // one per tile in the workspace
    double su, sv;
    long long cnt;
    float mx, pad;
};
static_assert(sizeof(StatPart) == 32, "flow stats workspace layout");

struct Src {                                   // the cropped flow
    const float *flow;
    int64_t bstride, plane;                    // elements between samples / between u and v
    int Wq, crop_h, crop_w;
    int use_clip;
    float clip;
};

// (u, v) of pixel (y, x) of sample b after the optional clip_flow rescale (flow_to_color lines 65-69)
__device__ __forceinline__ float2 load_uv(const Src &s, int b, int y, int x, bool clip) {
    const float *p = s.flow + (int64_t)b * s.bstride + (int64_t)y * s.Wq + x;
    float u = p[0], v = p[s.plane];
    if (clip) {
        const float rad = sqrtf(u * u + v * v);
        const float den = fmaxf(fmaxf(rad, 1e-5f), s.clip);
        const float k = s.clip / den;
        u = u * k;
        v = v * k;
    }
    return make_float2(u, v);
}

__global__ __launch_bounds__(kThreads) void stats_tile_kernel(Src s, float threshold, int tiles_x, int tiles_y, StatPart *__restrict__ part) {
    __shared__ pwc::TreeLds<kThreads, 2, 1> red;
    __shared__ pwc::WaveLds<float, kThreads, 1> redm;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int col = tid % kTW, row0 = tid / kTW;
    const int x = blockIdx.x * kTW + col;
    double sum[2] = {0.0, 0.0};
    long long cnt[1] = {0};
    float mx = 0.0f;
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        const int y = blockIdx.y * kTH + row0 + k * kRowStep;
        if (y >= s.crop_h || x >= s.crop_w) continue;
        const float2 raw = load_uv(s, b, y, x, false);
        if (sqrtf(raw.x * raw.x + raw.y * raw.y) > threshold) {
            sum[0] += (double)raw.x;
            sum[1] += (double)raw.y;
            ++cnt[0];
        }
        const float2 c = s.use_clip ? load_uv(s, b, y, x, true) : raw;
        mx = fmaxf(mx, sqrtf(c.x * c.x + c.y * c.y));
    }
    pwc::tree_sum(red, sum, cnt);
    mx = pwc::wave_block_max(redm, mx);
    if (tid == 0) {
        const int64_t lin = blockIdx.x + (int64_t)tiles_x * (blockIdx.y + (int64_t)tiles_y * blockIdx.z);
        part[lin] = StatPart{sum[0], sum[1], cnt[0], mx, 0.0f};
    }
}

// workgroup b adds the tiles of sample b in tile order; record = {max radius, count (int32), mean u, mean v}
__global__ __launch_bounds__(kThreads) void stats_finish_kernel(const StatPart *__restrict__ ws, int64_t tiles, float *__restrict__ rec) {
    __shared__ pwc::TreeLds<kThreads, 2, 1> red;
    __shared__ pwc::WaveLds<float, kThreads, 1> redm;
    const int tid = threadIdx.x, b = blockIdx.x;
    const StatPart *part = ws + (int64_t)b * tiles;
    double sum[2] = {0.0, 0.0};
    long long cnt[1] = {0};
    float mx = 0.0f;
    for (int64_t i = tid; i < tiles; i += kThreads) {
        sum[0] += part[i].su;
        sum[1] += part[i].sv;
        cnt[0] += part[i].cnt;
        mx = fmaxf(mx, part[i].mx);
    }
    pwc::tree_sum(red, sum, cnt);
    mx = pwc::wave_block_max(redm, mx);
    if (tid == 0) {
        float *r = rec + 4 * (int64_t)b;
        r[0] = mx;
        reinterpret_cast<int *>(r)[1] = (int)cnt[0];
        r[2] = cnt[0] ? (float)(sum[0] / (double)cnt[0]) : 0.0f;
        r[3] = cnt[0] ? (float)(sum[1] / (double)cnt[0]) : 0.0f;
    }
}

// wheel entry i, channel c (0 R, 1 G, 2 B) as make_colorwheel builds it: RY 15, YG 6, GC 4, CB 11, BM 13, MR 6
__device__ __forceinline__ int wheel_entry(int i, int c) {
    int rgb[3] = {0, 0, 0};
    if (i < 15) { rgb[0] = 255; rgb[1] = 255 * i / 15; }
    else if (i < 21) { rgb[0] = 255 - 255 * (i - 15) / 6; rgb[1] = 255; }
    else if (i < 25) { rgb[1] = 255; rgb[2] = 255 * (i - 21) / 4; }
    else if (i < 36) { rgb[1] = 255 - 255 * (i - 25) / 11; rgb[2] = 255; }
    else if (i < 49) { rgb[2] = 255; rgb[0] = 255 * (i - 36) / 13; }
    else { rgb[2] = 255 - 255 * (i - 49) / 6; rgb[0] = 255; }
    return rgb[c];
}

// colour of pixel p (counted over all samples) as R | G << 8 | B << 16
__device__ __forceinline__ uint32_t pixel_color(const Src &s, const float *__restrict__ rec, const float (*wheel)[3], int64_t p) {
    const int64_t per = (int64_t)s.crop_h * s.crop_w;
    const int b = (int)(p / per);
    const int r = (int)(p - (int64_t)b * per);
    const int y = r / s.crop_w, x = r - y * s.crop_w;
    const float2 f = load_uv(s, b, y, x, s.use_clip != 0);
    const float rad = sqrtf(f.x * f.x + f.y * f.y);
    const float ang = atan2f(-f.y, -f.x) / kPi;                    // the sign of a zero v reaches atan2f: the wheel is not continuous there
    const float fk = (ang + 1.0f) / 2.0f * (float)(kWheel - 1) + 1.0f;
    const float kf = floorf(fk);
    const float fr = fk - kf;                                      // exact, and so is 1 - fr: fk >= 1
    const int k0 = ((int)kf - 1) % kWheel, k1 = (k0 + 1) % kWheel;
    const float rn = fminf(fmaxf(rad / (rec[4 * (int64_t)b] + 1e-5f), 0.0f), 1.0f);
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float col = (1.0f - fr) * wheel[k0][c] + fr * wheel[k1][c];
        col = 1.0f - rn * (1.0f - col);
        const float lv = fminf(fmaxf(col, 0.0f), 1.0f) * 255.0f;
        out |= (uint32_t)(int)lv << (8 * c);
    }
    return out;
}

__global__ __launch_bounds__(kThreads) void color_kernel(Src s, const float *__restrict__ rec, uint8_t *__restrict__ out, int head, int64_t total) {
    __shared__ float wheel[kWheel][3];
    const int tid = threadIdx.x;
    if (tid < kWheel * 3) wheel[tid / 3][tid % 3] = (float)wheel_entry(tid / 3, tid % 3) / 255.0f;
    __syncthreads();
    // this lane's dword covers stream bytes g0 .. g0 + 3; `out - head` is 4-byte aligned
    const int64_t g0 = ((int64_t)blockIdx.x * kThreads + tid) * 4 - head;
    if (g0 >= total || g0 + 3 < 0) return;
    const int64_t lo = g0 < 0 ? 0 : g0, hi = g0 + 3 < total ? g0 + 3 : total - 1;
    const int64_t pa = lo / 3, pb = hi / 3;
    const uint32_t ca = pixel_color(s, rec, wheel, pa);
    const uint32_t cb = pb != pa ? pixel_color(s, rec, wheel, pb) : ca;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t g = g0 + k;
        if (g < lo || g > hi) continue;
        const int64_t p = g / 3;
        const int c = (int)(g - p * 3);
        word |= (((p == pa ? ca : cb) >> (8 * c)) & 0xffu) << (8 * k);
    }
    if (lo == g0 && hi == g0 + 3) {
        *reinterpret_cast<uint32_t *>(out + g0) = word;
    } else {
        for (int64_t g = lo; g <= hi; ++g) out[g] = (uint8_t)(word >> (8 * (int)(g - g0)));
    }
}

struct Axis { int s0, s1; float f; };

// xofs / alpha of cv::resize INTER_LINEAR for destination index d (harness._cv2_axis): geometry in double, then float
__device__ __forceinline__ Axis cv2_axis(int d, double scale, int src) {
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    const float sf = floorf(fx);
    fx = fx - sf;
    int sx = (int)sf;
    if (sx < 0) { sx = 0; fx = 0.0f; }
    else if (sx >= src - 1) { sx = src - 1; fx = 0.0f; }
    return Axis{sx, sx + 1 < src - 1 ? sx + 1 : src - 1, fx};
}

struct Quiver {
    int H, W, step, Gy, Gx, same, tip_rule;
    double scale_y, scale_x;
    float vec_sx, vec_sy, gain, min_mag, angle_threshold;
    const float *dom;
    int64_t dom_stride;
};

__device__ __forceinline__ float resize_tap(const float *__restrict__ p, int Wq, Axis ay, Axis ax) {
    const float a0 = 1.0f - ax.f, b0 = 1.0f - ay.f;
    const float *r0 = p + (int64_t)ay.s0 * Wq, *r1 = p + (int64_t)ay.s1 * Wq;
    const float h0 = r0[ax.s0] * a0 + r0[ax.s1] * ax.f;          // HResizeLinear
    const float h1 = r1[ax.s0] * a0 + r1[ax.s1] * ax.f;
    return h0 * b0 + h1 * ay.f;                                   // VResizeLinear
}

__global__ __launch_bounds__(kThreads) void quiver_kernel(Src s, Quiver q, float2 *__restrict__ vec, int2 *__restrict__ tip,
                                                          uint8_t *__restrict__ flags) {
    const int gx = blockIdx.x * kThreads + threadIdx.x, gy = blockIdx.y, b = blockIdx.z;
    if (gx >= q.Gx) return;
    const int x = gx * q.step, y = gy * q.step;
    const float *p = s.flow + (int64_t)b * s.bstride;
    float dx, dy;
    if (q.same) {
        dx = p[(int64_t)y * s.Wq + x];
        dy = p[s.plane + (int64_t)y * s.Wq + x];
    } else {
        const Axis ay = cv2_axis(y, q.scale_y, s.crop_h), ax = cv2_axis(x, q.scale_x, s.crop_w);
        dx = resize_tap(p, s.Wq, ay, ax);
        dy = resize_tap(p + s.plane, s.Wq, ay, ax);
    }
    dx = dx * q.vec_sx;
    dy = dy * q.vec_sy;
    const float mag = sqrtf(dx * dx + dy * dy);
    const float tx = (float)x + dx * q.gain, ty = (float)y + dy * q.gain;
    int2 t;
    if (q.tip_rule == 0) { t.x = (int)rintf(tx); t.y = (int)rintf(ty); }          // int(round(.)): half to even
    else { t.x = (int)tx; t.y = (int)ty; }                                       // int(.): toward zero
    int aligned = 1;
    if (q.dom) {
        const float du = q.dom[(int64_t)b * q.dom_stride], dv = q.dom[(int64_t)b * q.dom_stride + 1];
        const float dn = sqrtf(du * du + dv * dv);
        if (dn > 0.0f) {
            const float c = (dx / mag) * (du / dn) + (dy / mag) * (dv / dn);
            const float deg = acosf(fminf(fmaxf(c, -1.0f), 1.0f)) * 180.0f / kPi;
            aligned = deg < q.angle_threshold;                                    // false for the NaN of a zero vector
        }
    }
    const int64_t o = ((int64_t)b * q.Gy + gy) * q.Gx + gx;
    vec[o] = make_float2(dx, dy);
    tip[o] = t;
    flags[o] = (uint8_t)((mag < q.min_mag ? 0 : 1) | (aligned << 1));
}

// argument checks shared by the three entry points; fills s
int make_src(const char *who, const void *flow, int n, int Hq, int Wq, int crop_h, int crop_w, int64_t bstride, int use_clip, float clip,
             Src *s) {
    if (!flow) PWC_FAIL(PWC_EINVAL, "%s: null pointer", who);
    if (n <= 0 || Hq <= 0 || Wq <= 0 || crop_h <= 0 || crop_w <= 0)
        PWC_FAIL(PWC_EINVAL, "%s: bad shape n=%d Hq=%d Wq=%d crop=%dx%d", who, n, Hq, Wq, crop_h, crop_w);
    if (crop_h > Hq || crop_w > Wq) PWC_FAIL(PWC_EINVAL, "%s: crop %dx%d larger than the map %dx%d", who, crop_h, crop_w, Hq, Wq);
    if (bstride < (int64_t)2 * Hq * Wq) PWC_FAIL(PWC_EINVAL, "%s: batch stride smaller than the tensor", who);
    if ((int64_t)n * crop_h * crop_w * 3 >= 0x80000000LL || n > 65535 || (int64_t)2 * Hq * Wq >= 0x80000000LL)
        PWC_FAIL(PWC_EINVAL, "%s: needs n*crop_h*crop_w*3 < 2^31, 2*Hq*Wq < 2^31 and n <= 65535", who);
    if (use_clip && !(clip > 0.0f)) PWC_FAIL(PWC_EINVAL, "%s: clip_flow must be positive", who);
    if (pwc::misaligned({flow})) PWC_FAIL(PWC_EALIGN, "%s: flow must be 4-byte aligned", who);
    s->flow = static_cast<const float *>(flow);
    s->bstride = bstride;
    s->plane = (int64_t)Hq * Wq;
    s->Wq = Wq; s->crop_h = crop_h; s->crop_w = crop_w;
    s->use_clip = use_clip ? 1 : 0;
    s->clip = clip;
    return PWC_OK;
}

}  // namespace

extern "C" int64_t pwc_flow_stats_workspace_bytes(int n, int crop_h, int crop_w) {
    if (n <= 0 || crop_h <= 0 || crop_w <= 0) return -1;
    return (int64_t)sizeof(StatPart) * n * ((crop_h + kTH - 1) / kTH) * ((crop_w + kTW - 1) / kTW);
}

extern "C" int pwc_flow_stats(const void *flow, int n, int Hq, int Wq, int crop_h, int crop_w, int64_t bstride, int use_clip, float clip_flow,
                              float threshold, void *workspace, int64_t workspace_bytes, void *rec, void *stream) {
    Src s;
    if (int rc = make_src("pwc_flow_stats", flow, n, Hq, Wq, crop_h, crop_w, bstride, use_clip, clip_flow, &s)) return rc;
    if (!workspace || !rec) PWC_FAIL(PWC_EINVAL, "pwc_flow_stats: null pointer");
    const int tiles_x = (crop_w + kTW - 1) / kTW, tiles_y = (crop_h + kTH - 1) / kTH;
    if (tiles_y > 65535) PWC_FAIL(PWC_EINVAL, "pwc_flow_stats: crop_h must be <= 16 * 65535");
    const int64_t need = pwc_flow_stats_workspace_bytes(n, crop_h, crop_w);
    if (workspace_bytes < need)
        PWC_FAIL(PWC_EINVAL, "pwc_flow_stats: workspace needs %lld bytes, got %lld", (long long)need, (long long)workspace_bytes);
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) PWC_FAIL(PWC_EALIGN, "pwc_flow_stats: workspace must be 8-byte aligned");
    if (pwc::misaligned({rec})) PWC_FAIL(PWC_EALIGN, "pwc_flow_stats: the record must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    StatPart *ws = static_cast<StatPart *>(workspace);
    hipLaunchKernelGGL(stats_tile_kernel, dim3(tiles_x, tiles_y, n), dim3(kThreads), 0, st, s, threshold, tiles_x, tiles_y, ws);
    hipLaunchKernelGGL(stats_finish_kernel, dim3(n), dim3(kThreads), 0, st, ws, (int64_t)tiles_x * tiles_y, static_cast<float *>(rec));
    return pwc::check_launch("stats_tile_kernel");
}

extern "C" int pwc_flow_color(const void *flow, int n, int Hq, int Wq, int crop_h, int crop_w, int64_t bstride, int use_clip, float clip_flow,
                              const void *rec, void *out, void *stream) {
    Src s;
    if (int rc = make_src("pwc_flow_color", flow, n, Hq, Wq, crop_h, crop_w, bstride, use_clip, clip_flow, &s)) return rc;
    if (!rec || !out) PWC_FAIL(PWC_EINVAL, "pwc_flow_color: null pointer");
    if (pwc::misaligned({rec})) PWC_FAIL(PWC_EALIGN, "pwc_flow_color: the record must be 4-byte aligned");
    const int head = (int)(reinterpret_cast<uintptr_t>(out) & 3u);
    const int64_t total = (int64_t)n * crop_h * crop_w * 3;
    const int64_t dwords = (head + total + 3) / 4;
    const int64_t blocks = (dwords + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(color_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), s,
                       static_cast<const float *>(rec), static_cast<uint8_t *>(out), head, total);
    return pwc::check_launch("color_kernel");
}

extern "C" int pwc_flow_quiver(const void *flow, int n, int Hq, int Wq, int crop_h, int crop_w, int64_t bstride, int frame_h, int frame_w,
                               int step, float vec_sx, float vec_sy, float gain, int tip_rule, float min_mag, const void *dominant,
                               int64_t dom_stride, float angle_threshold, void *vec, void *tip, void *flags, void *stream) {
    Src s;
    if (int rc = make_src("pwc_flow_quiver", flow, n, Hq, Wq, crop_h, crop_w, bstride, 0, 0.0f, &s)) return rc;
    if (!vec || !tip || !flags) PWC_FAIL(PWC_EINVAL, "pwc_flow_quiver: null pointer");
    if (frame_h <= 0 || frame_w <= 0 || step < 1)
        PWC_FAIL(PWC_EINVAL, "pwc_flow_quiver: bad frame %dx%d or step %d", frame_h, frame_w, step);
    if (tip_rule != 0 && tip_rule != 1) PWC_FAIL(PWC_EINVAL, "pwc_flow_quiver: unknown tip_rule %d (0 = round half to even, 1 = truncate)", tip_rule);
    if (dominant && dom_stride < 2) PWC_FAIL(PWC_EINVAL, "pwc_flow_quiver: dominant stride must be >= 2");
    Quiver q;
    q.H = frame_h; q.W = frame_w; q.step = step;
    q.Gy = (frame_h + step - 1) / step;
    q.Gx = (frame_w + step - 1) / step;
    if (q.Gy > 65535) PWC_FAIL(PWC_EINVAL, "pwc_flow_quiver: more than 65535 grid rows");
    if (pwc::misaligned({vec, tip}, 8) || pwc::misaligned({dominant}))
        PWC_FAIL(PWC_EALIGN, "pwc_flow_quiver: vec and tip must be 8-byte aligned, dominant 4-byte aligned");
    q.same = (crop_h == frame_h && crop_w == frame_w) ? 1 : 0;
    q.tip_rule = tip_rule;
    q.scale_y = 1.0 / ((double)frame_h / (double)crop_h);          // scale = 1. / inv_scale, in double like cv::resize
    q.scale_x = 1.0 / ((double)frame_w / (double)crop_w);
    q.vec_sx = vec_sx; q.vec_sy = vec_sy; q.gain = gain; q.min_mag = min_mag; q.angle_threshold = angle_threshold;
    q.dom = static_cast<const float *>(dominant);
    q.dom_stride = dom_stride;
    hipLaunchKernelGGL(quiver_kernel, dim3((q.Gx + kThreads - 1) / kThreads, q.Gy, n), dim3(kThreads), 0, static_cast<hipStream_t>(stream), s,
                       q, static_cast<float2 *>(vec), static_cast<int2 *>(tip), static_cast<uint8_t *>(flags));
    return pwc::check_launch("quiver_kernel");
}
