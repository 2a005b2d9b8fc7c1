// Flow-comparison report on the device (reference onnx_pth_compare.py:133-201 compare_flows and :225-230 print_flow_stats): two float32
// flow fields a ("pth", the reference side) and b, [n][2][H][W] each, go straight to one fp64 record per sample plus one for the whole
// batch; nothing image-sized is written unless the caller asks for the per-pixel EPE map.  Per pixel, fp32 with no contraction:
//   du = a_u - b_u;  dv = a_v - b_v;  epe = sqrtf(du*du + dv*dv)            (bit for bit the reference's float32 np.linalg.norm)
// Per scalar (u, then v), widened to fp64 before it is added: d^2, |d|, a^2, b^2, |a|, a, b, a*b; per pixel the fp64 sum of epe.
// Exact float32 reductions: max |d|, max epe, min / max of a and of b.  Integer counts: epe <= tau_k (inclusive, as the reference).
//
// Work split as in pwc_kitti_score.hip, with a larger tile: one workgroup = one 32 x 128 tile of one sample, 256 lanes.  Two load
// forms, chosen by the launcher as pwc_aug::launch chooses vec / scalar: with W % 4 == 0 and 16-byte aligned planes each lane owns four
// neighbouring pixels of the rows tid / 32 + 8 k (four 16-byte loads per pass: a_u, a_v, b_u, b_v); otherwise each lane owns the column
// tid % 128 of the rows tid / 128 + 2 k with guarded 4-byte loads.  Each workgroup leaves one Part (tree_sum's fixed order for the
// sums; a maximum has no order) in the workspace; the finish kernel has n + 1 workgroups: workgroup s < n adds the tiles of sample s
// in tile order, workgroup n adds every tile in (sample, tile) order -- the report of the samples stacked along H.  No atomics: two
// runs give the same bits.
//
// Why 32 x 128 and not pwc_kitti_score's 16 x 64: the batch row is ONE workgroup reading every Part, and a workgroup's reduction is a
// fixed cost per tile.  Measured at 16 x 375 x 1242: 102 us for the launch pair with 16 x 64 tiles (7680 Parts), 50 us with 32 x 128
// (1920 Parts; tile kernel 36 us, finish kernel 16 us).  A tile of 4096 pixels still fits the 16-bit fields in
// which the tile kernel carries its eight counts (two 64-bit words instead of eight through the workgroup sum).
//
// NaN / Inf are not special-cased.  The sums carry them as IEEE arithmetic dictates; epe <= tau is false for a NaN epe; the extrema
// go through fmaxf, which returns the other operand when one is NaN, so a NaN never becomes an extremum (np.max would return NaN).
#include "pwc_block_reduce.h"
#include "pwc_common.h"

namespace {

constexpr int kTH = 32, kTW = 128, kThreads = 256;
constexpr int kRowStep = kThreads / kTW;            // 2: scalar form, rows per pass
constexpr int kVecRowStep = kThreads / (kTW / 4);   // 8: 16-byte form, rows per pass
constexpr int kPix = kTH / kRowStep;                // 16 pixels per lane in either form
constexpr int kND = 9;                        // d^2, |d|, a^2, b^2, |a|, a, b, a*b, epe
constexpr int kNI = PWC_FLOW_COMPARE_MAX_TAUS;
constexpr int kNX = 6;                        // max |d|, max epe, max -a, max a, max -b, max b
enum { S_D2, S_ABSD, S_A2, S_B2, S_ABSA, S_A, S_B, S_AB, S_EPE };
enum { X_ABSD, X_EPE, X_NEG_A, X_A, X_NEG_B, X_B };

// what one tile leaves in the workspace
struct Part {
    double sum[kND];
    int cnt[kNI];
    float ext[kNX];
};
static_assert(sizeof(Part) == 128, "flow compare workspace layout");
static_assert(kTH * kTW < 65536 && kNI == 8, "the tile kernel packs four 16-bit counts into a 64-bit word");

struct Geo {
    int H, W, tiles_x, tiles_y;
    int64_t bsa, bsb;
    int ntau, map_vec;
    float tau[kNI];
};

// NC = 2: four 16-bit counts per word (tile kernel); NC = 8: one count per word (finish kernel)
template <int NC> struct Acc {
    double s[kND];
    long long c[NC];
    float x[kNX];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < kND; ++k) s[k] = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) c[k] = 0;
#pragma unroll
        for (int k = 0; k < kNX; ++k) x[k] = -INFINITY;
    }
};

__device__ __forceinline__ void add_scalar(Acc<2> &r, float a, float b) {
    const float d = a - b;
    const double dd = (double)d, da = (double)a, db = (double)b;
    r.s[S_D2] += dd * dd;
    r.s[S_ABSD] += fabs(dd);
    r.s[S_A2] += da * da;
    r.s[S_B2] += db * db;
    r.s[S_ABSA] += fabs(da);
    r.s[S_A] += da;
    r.s[S_B] += db;
    r.s[S_AB] += da * db;
    r.x[X_ABSD] = fmaxf(r.x[X_ABSD], fabsf(d));
    r.x[X_NEG_A] = fmaxf(r.x[X_NEG_A], -a);
    r.x[X_A] = fmaxf(r.x[X_A], a);
    r.x[X_NEG_B] = fmaxf(r.x[X_NEG_B], -b);
    r.x[X_B] = fmaxf(r.x[X_B], b);
}

// one pixel: both scalars, then the endpoint error; returns the epe
__device__ __forceinline__ float add_pixel(Acc<2> &r, const Geo &g, float au, float av, float bu, float bv) {
    add_scalar(r, au, bu);
    add_scalar(r, av, bv);
    const float du = au - bu, dv = av - bv;
    const float epe = sqrtf(du * du + dv * dv);
    r.s[S_EPE] += (double)epe;
    r.x[X_EPE] = fmaxf(r.x[X_EPE], epe);
#pragma unroll
    for (int k = 0; k < kNI; ++k) r.c[k / 4] += (long long)((k < g.ntau && epe <= g.tau[k]) ? 1 : 0) << (16 * (k % 4));
    return epe;
}

template <int NC> struct Lds {
    pwc::TreeLds<kThreads, kND, NC> sum;
    pwc::WaveLds<float, kThreads, 1> ext;
};

// workgroup totals of r, in every lane
template <int NC> __device__ __forceinline__ void block_reduce(Lds<NC> &lds, Acc<NC> &r) {
    pwc::tree_sum(lds.sum, r.s, r.c);
#pragma unroll
    for (int k = 0; k < kNX; ++k) r.x[k] = pwc::wave_block_max(lds.ext, r.x[k]);
}

template <bool VEC, bool WRITE>
__global__ __launch_bounds__(kThreads) void compare_tile_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                                float *__restrict__ epe_map, Part *__restrict__ part, Geo g) {
    __shared__ Lds<2> lds;
    const int tid = threadIdx.x, s = blockIdx.z;
    const int64_t npix = (int64_t)g.H * g.W;
    const float *pa = a + (int64_t)s * g.bsa, *pb = b + (int64_t)s * g.bsb;
    Acc<2> r;
    r.clear();
    if (VEC) {
        // W % 4 == 0: a lane's four pixels are all inside the row or all outside it
        const int x = blockIdx.x * kTW + (tid % (kTW / 4)) * 4, row0 = tid / (kTW / 4);
#pragma unroll
        for (int k = 0; k < kTH / kVecRowStep; ++k) {
            const int y = blockIdx.y * kTH + row0 + k * kVecRowStep;
            if (y >= g.H || x >= g.W) continue;
            const int64_t pix = (int64_t)y * g.W + x;
            const float4 au = *reinterpret_cast<const float4 *>(pa + pix), av = *reinterpret_cast<const float4 *>(pa + npix + pix);
            const float4 bu = *reinterpret_cast<const float4 *>(pb + pix), bv = *reinterpret_cast<const float4 *>(pb + npix + pix);
            float4 e;
            e.x = add_pixel(r, g, au.x, av.x, bu.x, bv.x);
            e.y = add_pixel(r, g, au.y, av.y, bu.y, bv.y);
            e.z = add_pixel(r, g, au.z, av.z, bu.z, bv.z);
            e.w = add_pixel(r, g, au.w, av.w, bu.w, bv.w);
            if (WRITE) {
                float *m = epe_map + (int64_t)s * npix + pix;
                if (g.map_vec) {
                    *reinterpret_cast<float4 *>(m) = e;
                } else {
                    m[0] = e.x; m[1] = e.y; m[2] = e.z; m[3] = e.w;
                }
            }
        }
    } else {
        const int x = blockIdx.x * kTW + tid % kTW, row0 = tid / kTW;
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const int y = blockIdx.y * kTH + row0 + k * kRowStep;
            if (y >= g.H || x >= g.W) continue;
            const int64_t pix = (int64_t)y * g.W + x;
            const float e = add_pixel(r, g, pa[pix], pa[npix + pix], pb[pix], pb[npix + pix]);
            if (WRITE) epe_map[(int64_t)s * npix + pix] = e;
        }
    }
    block_reduce(lds, r);
    if (tid == 0) {
        Part &p = part[blockIdx.x + (int64_t)g.tiles_x * (blockIdx.y + (int64_t)g.tiles_y * blockIdx.z)];
#pragma unroll
        for (int k = 0; k < kND; ++k) p.sum[k] = r.s[k];
#pragma unroll
        for (int k = 0; k < kNI; ++k) p.cnt[k] = (int)((r.c[k / 4] >> (16 * (k % 4))) & 0xffff);
#pragma unroll
        for (int k = 0; k < kNX; ++k) p.ext[k] = r.x[k];
    }
}

// workgroup s < n adds the tiles of sample s in tile order, workgroup n adds every tile in (sample, tile) order; lane 0 forms the
// derived metrics in fp64 from the totals and writes the row
__global__ __launch_bounds__(kThreads) void compare_finish_kernel(const Part *__restrict__ part, int n, int64_t tiles, int64_t pix_per_sample,
                                                                  int ntau, double *__restrict__ out) {
    __shared__ Lds<kNI> lds;
    const int tid = threadIdx.x, row = blockIdx.x;
    const int64_t first = row < n ? row * tiles : 0, count = row < n ? tiles : n * tiles;
    const int samples = row < n ? 1 : n;
    Acc<kNI> r;
    r.clear();
#pragma unroll 4
    for (int64_t i = tid; i < count; i += kThreads) {
        const Part &p = part[first + i];
#pragma unroll
        for (int k = 0; k < kND; ++k) r.s[k] += p.sum[k];
#pragma unroll
        for (int k = 0; k < kNI; ++k) r.c[k] += p.cnt[k];
#pragma unroll
        for (int k = 0; k < kNX; ++k) r.x[k] = fmaxf(r.x[k], p.ext[k]);
    }
    block_reduce(lds, r);
    if (tid != 0) return;
    double *o = out + (int64_t)row * PWC_FLOW_COMPARE_FIELDS;
    const double P = (double)(pix_per_sample * samples), N = 2.0 * P;
    const double min_a = -(double)r.x[X_NEG_A], max_a = (double)r.x[X_A], min_b = -(double)r.x[X_NEG_B], max_b = (double)r.x[X_B];
    o[PWC_FC_N] = N;
    o[PWC_FC_P] = P;
    o[PWC_FC_SUM_D2] = r.s[S_D2];
    o[PWC_FC_SUM_ABS_D] = r.s[S_ABSD];
    o[PWC_FC_SUM_A2] = r.s[S_A2];
    o[PWC_FC_SUM_B2] = r.s[S_B2];
    o[PWC_FC_SUM_ABS_A] = r.s[S_ABSA];
    o[PWC_FC_SUM_A] = r.s[S_A];
    o[PWC_FC_SUM_B] = r.s[S_B];
    o[PWC_FC_SUM_AB] = r.s[S_AB];
    o[PWC_FC_SUM_EPE] = r.s[S_EPE];
    o[PWC_FC_MAX_ABS] = (double)r.x[X_ABSD];
    o[PWC_FC_EPE_MAX] = (double)r.x[X_EPE];
    o[PWC_FC_MIN_A] = min_a;
    o[PWC_FC_MAX_A] = max_a;
    o[PWC_FC_MIN_B] = min_b;
    o[PWC_FC_MAX_B] = max_b;
    const double nan = __builtin_nan("");
    for (int k = 0; k < kNI; ++k) {
        o[PWC_FC_COUNT0 + k] = k < ntau ? (double)r.c[k] : 0.0;
        o[PWC_FC_AGREE0 + k] = k < ntau ? (double)r.c[k] / P * 100.0 : nan;
    }
    const double l2 = sqrt(r.s[S_D2]), mae = r.s[S_ABSD] / N;
    const double na = sqrt(r.s[S_A2]), nb = sqrt(r.s[S_B2]);
    o[PWC_FC_L2] = l2;
    o[PWC_FC_MAE] = mae;
    o[PWC_FC_REL_L2] = l2 / (na + 1e-8);
    o[PWC_FC_REL_MAE] = mae / (r.s[S_ABSA] / N + 1e-8);
    o[PWC_FC_COSINE] = r.s[S_AB] / (na * nb + 1e-8);
    const bool flat_a = min_a == max_a, flat_b = min_b == max_b;
    double pearson = nan;
    if (!flat_a && !flat_b) {
        const double cov = r.s[S_AB] - r.s[S_A] * r.s[S_B] / N;
        const double va = r.s[S_A2] - r.s[S_A] * r.s[S_A] / N, vb = r.s[S_B2] - r.s[S_B] * r.s[S_B] / N;
        pearson = cov / sqrt(va * vb);
        pearson = pearson > 1.0 ? 1.0 : pearson < -1.0 ? -1.0 : pearson;      // np.corrcoef clips its result the same way
    }
    o[PWC_FC_PEARSON] = pearson;
    o[PWC_FC_EPE_MEAN] = r.s[S_EPE] / P;
    const double mean_a = r.s[S_A] / N, mean_b = r.s[S_B] / N;
    const double var_a = r.s[S_A2] / N - mean_a * mean_a, var_b = r.s[S_B2] / N - mean_b * mean_b;
    o[PWC_FC_MEAN_A] = mean_a;
    o[PWC_FC_STD_A] = flat_a ? 0.0 : sqrt(var_a > 0.0 ? var_a : 0.0);
    o[PWC_FC_MEAN_B] = mean_b;
    o[PWC_FC_STD_B] = flat_b ? 0.0 : sqrt(var_b > 0.0 ? var_b : 0.0);
}

}  // namespace

extern "C" int64_t pwc_flow_compare_workspace_bytes(int n, int H, int W) {
    if (n <= 0 || H <= 0 || W <= 0) return -1;
    return (int64_t)sizeof(Part) * n * ((int64_t)((H + kTH - 1) / kTH) * ((W + kTW - 1) / kTW));
}

extern "C" int pwc_flow_compare(const void *a, const void *b, int n, int H, int W, int64_t a_bstride, int64_t b_bstride, const float *taus,
                                int ntau, void *epe_map, void *workspace, int64_t workspace_bytes, void *out, void *stream) {
    if (!a || !b || !taus || !workspace || !out) PWC_FAIL(PWC_EINVAL, "pwc_flow_compare: null pointer");
    if (n <= 0 || H <= 0 || W <= 0) PWC_FAIL(PWC_EINVAL, "pwc_flow_compare: bad shape n=%d H=%d W=%d", n, H, W);
    if (ntau < 1 || ntau > kNI) PWC_FAIL(PWC_EINVAL, "pwc_flow_compare: ntau %d outside 1..%d", ntau, kNI);
    for (int k = 0; k < ntau; ++k)
        if (!(taus[k] >= 0.0f) || taus[k] == INFINITY)
            PWC_FAIL(PWC_EINVAL, "pwc_flow_compare: threshold %d is not a finite non-negative number (%g)", k, (double)taus[k]);
    if ((int64_t)n * 2 * H * W >= 0x80000000LL || n > 65535 || (H + kTH - 1) / kTH > 65535)
        PWC_FAIL(PWC_EINVAL, "pwc_flow_compare: needs n*2*H*W < 2^31, n <= 65535 and H <= 32 * 65535");
    if (a_bstride < (int64_t)2 * H * W || b_bstride < (int64_t)2 * H * W)
        PWC_FAIL(PWC_EINVAL, "pwc_flow_compare: batch stride smaller than the tensor");
    const int64_t need = pwc_flow_compare_workspace_bytes(n, H, W);
    if (workspace_bytes < need)
        PWC_FAIL(PWC_EINVAL, "pwc_flow_compare: workspace needs %lld bytes, got %lld", (long long)need, (long long)workspace_bytes);
    if (pwc::misaligned({workspace, out}, 8)) PWC_FAIL(PWC_EINVAL, "pwc_flow_compare: workspace and out must be 8-byte aligned");
    if (pwc::misaligned({a, b, epe_map})) PWC_FAIL(PWC_EINVAL, "pwc_flow_compare: a, b and epe_map must be 4-byte aligned");
    Geo g;
    g.H = H; g.W = W;
    g.tiles_x = (W + kTW - 1) / kTW;
    g.tiles_y = (H + kTH - 1) / kTH;
    g.bsa = a_bstride; g.bsb = b_bstride;
    g.ntau = ntau;
    for (int k = 0; k < kNI; ++k) g.tau[k] = k < ntau ? taus[k] : 0.0f;
    g.map_vec = pwc::aligned16(epe_map);
    // 16-byte loads need every plane of every sample on a 16-byte boundary: W % 4 == 0 puts the rows and the v plane there
    const bool vec = W % 4 == 0 && pwc::aligned16(a) && pwc::aligned16(b) && a_bstride % 4 == 0 && b_bstride % 4 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float *fa = static_cast<const float *>(a), *fb = static_cast<const float *>(b);
    float *fm = static_cast<float *>(epe_map);
    Part *part = static_cast<Part *>(workspace);
    const dim3 grid(g.tiles_x, g.tiles_y, n), block(kThreads);
    if (vec) {
        if (fm) hipLaunchKernelGGL((compare_tile_kernel<true, true>), grid, block, 0, st, fa, fb, fm, part, g);
        else hipLaunchKernelGGL((compare_tile_kernel<true, false>), grid, block, 0, st, fa, fb, fm, part, g);
    } else {
        if (fm) hipLaunchKernelGGL((compare_tile_kernel<false, true>), grid, block, 0, st, fa, fb, fm, part, g);
        else hipLaunchKernelGGL((compare_tile_kernel<false, false>), grid, block, 0, st, fa, fb, fm, part, g);
    }
    hipLaunchKernelGGL(compare_finish_kernel, dim3(n + 1), block, 0, st, part, n, (int64_t)g.tiles_x * g.tiles_y, (int64_t)H * W, ntau,
                       static_cast<double *>(out));
    return pwc::check_launch("compare_tile_kernel");
}
