// Epipolar hard mask and soft Sampson penalty of the reference's train_fundamental.py:169-382, as used at :459-483:
//   pairs    _flow_to_pairs (:169-194): grid points (x, y) = mgrid[0:H:s, 0:W:s] row-major, endpoints (x + fu, y + fv) in fp64,
//            dropped when an endpoint is not finite or the image mask is 0 there; order kept, so N varies per sample.
//   ransac   _ransac_F (:236-258): hypothesis i fits the eight points of row i of the host-drawn index table
//            (rng.choice(N, 8, replace=False) per iteration, numpy's generator, drawn by the caller), counts the points with
//            Sampson d < thresh, keeps the first strictly largest count, fails when N < 8 or that count < 8, and refits on the
//            winner's inliers.
//   8-point  _eight_point_F (:211-225): Hartley normalisation (after x / (x_2 + 1e-12)), rows [u u', v u', u', v' u, v' v, v', u, v, 1],
//            the right singular vector of the min(n, 9)-th largest singular value (numpy's thin SVD of an 8 x 9 matrix returns 8
//            right vectors, so VT[-1] is NOT the null vector there: restated, not fixed), rank 2 by zeroing the smallest singular
//            value, T2^T F T1, then / F[2,2] when |F[2,2]| > 1e-12, else / ||F||_F, only when ||F||_F > 0.
//   mask     build_epipolar_mask_from_flow (:261-327): d of every pixel from the refit F; thr = min(tau, quantile(d_finite,
//            keep_ratio)); keep = finite & d <= thr; when mean(keep) < min_keep, thr = min(tau, quantile(d_finite, min_keep)) (which
//            can tighten; restated).  All true when the fit failed or no d is finite.
//   loss     epipolar_sampson_loss (:331-382): d per pixel with x1 = (x, y, 1), x2 = (x + fu, y + fv, 1) (no homogeneous
//            division there; the endpoint is the reference's fp32 sum (xs + flow).float(), d(x2)/d(flow) = 1) and F rounded to
//            fp32, the rest in fp64; huber / l1 / mean over pixels with mask > 0.5, times weight.
//
// Every geometric quantity is fp64 (the library is built with -ffp-contract=off: no operation below is fused).  Reductions are
// integer or fixed-order fp64; there are no float atomics, so every entry is bit-reproducible.
//
// Singular vectors.  Hestenes' one-sided Jacobi on the ROWS of a matrix M (R x 9): plane rotations from the left make the rows
// mutually orthogonal, after which row i is sigma_i v_i^T -- the right singular vectors without accumulating any rotation
// (registers hold M only).  The k-th largest row norm gives the k-th right singular vector, accurate to about eps sigma_1 / gap.
// Hypotheses: M = the 8 x 9 sample matrix, k = 8.  Refit: M = the 9 x 9 Gram matrix A^T A of the n inlier rows (rows become
// sigma_i^2 v_i^T), k = min(n, 9); accurate to about eps (sigma_1 / sigma_8)^2, far inside the 1e-8 the tests ask on F.
// Rank 2: the same on the 3 x 3 F, then F - (F v3) v3^T, which is U diag(s1, s2, 0) V^T.
//
// Quantiles.  For d >= 0 the fp64 bit pattern orders like the value, so numpy's linear quantile (virtual index (n-1) q, then
// _lerp(a, b, g) = a + (b-a) g, or b - (b-a)(1-g) when g >= 0.5) takes two order statistics, found by an 8-bit radix select over
// the finite d of one sample in one workgroup (four ranks at once: keep_ratio's and min_keep's two each).
#include "pwc_block_reduce.h"
#include "pwc_common.h"

#include <math.h>

namespace {

constexpr double kEps12 = 1e-12;
constexpr int kScoreThreads = 256, kScorePts = 4, kScoreHyps = 64;
constexpr int kRefitThreads = 256;
constexpr int kSelThreads = 1024;
constexpr int kMapThreads = 256;
constexpr int kLossThreads = 256, kLossPer = 8, kLossChunk = kLossThreads * kLossPer;

__device__ __forceinline__ bool finite64(double v) {
    return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}

// Sampson distance of train_fundamental.py:228-233 for homogeneous points (x1a, x1b, x1c) / (x2a, x2b, x2c), F row-major
__device__ __forceinline__ double sampson(const double *F, double x1a, double x1b, double x1c, double x2a, double x2b, double x2c) {
    const double f0 = F[0] * x1a + F[1] * x1b + F[2] * x1c;
    const double f1 = F[3] * x1a + F[4] * x1b + F[5] * x1c;
    const double f2 = F[6] * x1a + F[7] * x1b + F[8] * x1c;
    const double t0 = F[0] * x2a + F[3] * x2b + F[6] * x2c;
    const double t1 = F[1] * x2a + F[4] * x2b + F[7] * x2c;
    const double n = x2a * f0 + x2b * f1 + x2c * f2;
    const double den = f0 * f0 + f1 * f1 + t0 * t0 + t1 * t1 + kEps12;
    return (n * n) / den;
}

// one-sided Jacobi on the rows of m (R x C), fully unrolled (compile-time indices: m stays in registers)
template <int R, int C> __device__ __forceinline__ void row_jacobi(double (&m)[R][C]) {
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < R - 1; ++p) {
#pragma unroll
            for (int q = p + 1; q < R; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    al += m[p][j] * m[p][j];
                    be += m[q][j] * m[q][j];
                    ga += m[p][j] * m[q][j];
                }
                if (fabs(ga) > 2.220446049250313e-16 * sqrt(al * be) && ga != 0.0) {
                    rotated = true;
                    const double zeta = (be - al) / (2.0 * ga);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int j = 0; j < C; ++j) {
                        const double a = m[p][j], b = m[q][j];
                        m[p][j] = c * a - s * b;
                        m[q][j] = s * a + c * b;
                    }
                }
            }
        }
        if (!rotated) break;
    }
}

// unit vector of the row with the k-th largest norm (k 1-based; ties: lower row first) of a row-orthogonalised m
template <int R, int C> __device__ __forceinline__ double kth_row(const double (&m)[R][C], int k, double (&v)[C]) {
    double nr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < C; ++j) s += m[r][j] * m[r][j];
        nr[r] = s;
    }
    double sel = 0.0;
#pragma unroll
    for (int j = 0; j < C; ++j) v[j] = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int rank = 0;
#pragma unroll
        for (int o = 0; o < R; ++o) rank += (nr[o] > nr[r] || (nr[o] == nr[r] && o < r)) ? 1 : 0;
        if (rank == k - 1) {
            sel = sqrt(nr[r]);
#pragma unroll
            for (int j = 0; j < C; ++j) v[j] = m[r][j];
        }
    }
    if (sel > 0.0) {
#pragma unroll
        for (int j = 0; j < C; ++j) v[j] = v[j] / sel;
    }
    return sel;
}

// rank 2 (zero the smallest singular value), T2^T F T1, scale: the tail of _eight_point_F (:218-225)
__device__ __forceinline__ void finish_F(const double (&fv)[9], double s1, double m1x, double m1y, double s2, double m2x, double m2y,
                                         double *out) {
    double m[3][3], F[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) m[r][c] = F[r][c] = fv[3 * r + c];
    row_jacobi<3, 3>(m);
    double v3[3];
    if (kth_row<3, 3>(m, 3, v3) > 0.0) {
        double Fv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) Fv[r] = F[r][0] * v3[0] + F[r][1] * v3[1] + F[r][2] * v3[2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) F[r][c] = F[r][c] - Fv[r] * v3[c];
    }
    // T = [[s, 0, -s mx], [0, s, -s my], [0, 0, 1]];  G = T2^T F,  Fm = G T1
    const double T1[3][3] = {{s1, 0.0, -s1 * m1x}, {0.0, s1, -s1 * m1y}, {0.0, 0.0, 1.0}};
    const double T2[3][3] = {{s2, 0.0, -s2 * m2x}, {0.0, s2, -s2 * m2y}, {0.0, 0.0, 1.0}};
    double G[3][3], Fm[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[r][c] = T2[0][r] * F[0][c] + T2[1][r] * F[1][c] + T2[2][r] * F[2][c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Fm[r][c] = G[r][0] * T1[0][c] + G[r][1] * T1[1][c] + G[r][2] * T1[2][c];
    double ss = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) ss += Fm[r][c] * Fm[r][c];
    const double nrm = sqrt(ss);
    if (nrm > 0.0) {
        const double dv = fabs(Fm[2][2]) > kEps12 ? Fm[2][2] : nrm;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Fm[r][c] = Fm[r][c] / dv;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * r + c] = Fm[r][c];
}

// the normalised design row of _eight_point_F from homogeneous-divided points (x1 = (a, b, c), x2 alike) and the two T's
__device__ __forceinline__ void design_row(double x1a, double x1b, double x2a, double x2b, double c, double s1, double m1x,
                                           double m1y, double s2, double m2x, double m2y, double (&r)[9]) {
    // (T @ x.T).T restated: s x_0 + 0 x_1 + (-s mx) x_2
    const double u = s1 * x1a + 0.0 * x1b + (-s1 * m1x) * c;
    const double v = 0.0 * x1a + s1 * x1b + (-s1 * m1y) * c;
    const double up = s2 * x2a + 0.0 * x2b + (-s2 * m2x) * c;
    const double vp = 0.0 * x2a + s2 * x2b + (-s2 * m2y) * c;
    r[0] = u * up; r[1] = v * up; r[2] = up; r[3] = vp * u; r[4] = vp * v; r[5] = vp; r[6] = u; r[7] = v; r[8] = 1.0;
}

__device__ __forceinline__ double hom_w() { return 1.0 + kEps12; }

using pwc::misaligned;
using pwc::wave_block_sum;   // pwc_block_reduce.h: per wave xor tree, then the waves in order: fixed order, bit-reproducible

// ------------------------------------------------------------------------------------------------------------ compaction
// one workgroup per sample; chunks of 1024 grid points in row-major order, ballot + wave prefix for the order-preserving write
__global__ __launch_bounds__(1024) void epi_pairs_kernel(const float *__restrict__ flow, const void *__restrict__ mask, int mask_u8,
                                                         double *__restrict__ pts, int *__restrict__ npts, int H, int W, int stride,
                                                         int Ws, int cap, int64_t flow_bs, int64_t mask_bs) {
    __shared__ int wtot[16];
    __shared__ int base_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float *fu = flow + (int64_t)b * flow_bs, *fv = fu + (int64_t)H * W;
    double *out = pts + (int64_t)b * cap * 4;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int c0 = 0; c0 < cap; c0 += 1024) {
        const int g = c0 + tid;
        bool valid = false;
        double u = 0.0, v = 0.0, u2 = 0.0, v2 = 0.0;
        if (g < cap) {
            const int y = (g / Ws) * stride, x = (g % Ws) * stride;
            const int64_t o = (int64_t)y * W + x;
            u = (double)x; v = (double)y;
            u2 = u + (double)fu[o];
            v2 = v + (double)fv[o];
            valid = finite64(u2) && finite64(v2);
            valid = valid && pwc::mask_val(mask, mask_u8, (int64_t)b * mask_bs + o) != 0.0f;
        }
        const unsigned long long bal = __ballot(valid);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wv] = __popcll(bal);
        __syncthreads();
        int off = base_s;
        for (int k = 0; k < wv; ++k) off += wtot[k];
        if (valid) {
            double *p = out + (int64_t)(off + before) * 4;
            p[0] = u; p[1] = v; p[2] = u2; p[3] = v2;
        }
        __syncthreads();
        if (tid == 0) {
            int s = base_s;
            for (int k = 0; k < 16; ++k) s += wtot[k];
            base_s = s;
        }
        __syncthreads();
    }
    if (tid == 0) npts[b] = base_s;
}

// ------------------------------------------------------------------------------------------------------------ hypotheses
// one lane per (sample, hypothesis): gather 8 points, Hartley-normalise, 8 x 9 row-Jacobi, k = 8, rank 2, denormalise, scale
__global__ __launch_bounds__(64) void epi_hyp_kernel(const double *__restrict__ pts, const int *__restrict__ npts, int cap,
                                                     const int *__restrict__ idx, int64_t idx_bs, int iters, double *__restrict__ Fh) {
    const int b = blockIdx.y, i = blockIdx.x * 64 + threadIdx.x;
    if (i >= iters) return;
    double *out = Fh + ((int64_t)b * iters + i) * 9;
    const int N = npts[b];
    const int *ix = idx + (int64_t)b * idx_bs + (int64_t)i * 8;
    bool bad = N < 8;
    double x1[8][2], x2[8][2];
    const double w = hom_w(), c = 1.0 / w;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int j = bad ? 0 : ix[k];
        if (j < 0 || j >= N) { bad = true; j = 0; }
        const double *p = pts + ((int64_t)b * cap + j) * 4;
        x1[k][0] = p[0] / w; x1[k][1] = p[1] / w; x2[k][0] = p[2] / w; x2[k][1] = p[3] / w;
    }
    if (bad) {
        for (int k = 0; k < 9; ++k) out[k] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    // means: sequential over the 8 rows; mean distance: numpy's 8-way pairwise sum
    double m1x = 0.0, m1y = 0.0, m2x = 0.0, m2y = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { m1x += x1[k][0]; m1y += x1[k][1]; m2x += x2[k][0]; m2y += x2[k][1]; }
    m1x /= 8.0; m1y /= 8.0; m2x /= 8.0; m2y /= 8.0;
    double r1[8], r2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double a = x1[k][0] - m1x, bb = x1[k][1] - m1y, e = x2[k][0] - m2x, f = x2[k][1] - m2y;
        r1[k] = sqrt(a * a + bb * bb) + kEps12;
        r2[k] = sqrt(e * e + f * f) + kEps12;
    }
    const double md1 = (((r1[0] + r1[1]) + (r1[2] + r1[3])) + ((r1[4] + r1[5]) + (r1[6] + r1[7]))) / 8.0;
    const double md2 = (((r2[0] + r2[1]) + (r2[2] + r2[3])) + ((r2[4] + r2[5]) + (r2[6] + r2[7]))) / 8.0;
    const double s1 = 1.4142135623730951 / md1, s2 = 1.4142135623730951 / md2;
    double A[8][9];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double r[9];
        design_row(x1[k][0], x1[k][1], x2[k][0], x2[k][1], c, s1, m1x, m1y, s2, m2x, m2y, r);
#pragma unroll
        for (int j = 0; j < 9; ++j) A[k][j] = r[j];
    }
    row_jacobi<8, 9>(A);
    double fv[9];
    kth_row<8, 9>(A, 8, fv);
    finish_F(fv, s1, m1x, m1y, s2, m2x, m2y, out);
}

// ------------------------------------------------------------------------------------------------------------ scoring
// workgroup = (chunk of 1024 points, block of 64 hypotheses, sample); each lane keeps 4 points in registers, F is uniform
__global__ __launch_bounds__(kScoreThreads) void epi_score_kernel(const double *__restrict__ pts, const int *__restrict__ npts, int cap,
                                                                 const double *__restrict__ Fh, int iters, double thresh,
                                                                 int *__restrict__ counts) {
    __shared__ int wc[kScoreThreads / 64][kScoreHyps];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = npts[b];
    const int p0 = blockIdx.x * kScoreThreads * kScorePts;
    if (p0 >= N || N < 8) return;
    const double w = hom_w(), c = 1.0 / w;
    double q[kScorePts][4];
    bool has[kScorePts];
#pragma unroll
    for (int k = 0; k < kScorePts; ++k) {
        const int j = p0 + k * kScoreThreads + tid;
        has[k] = j < N;
        const double *p = pts + ((int64_t)b * cap + (has[k] ? j : 0)) * 4;
        q[k][0] = p[0] / w; q[k][1] = p[1] / w; q[k][2] = p[2] / w; q[k][3] = p[3] / w;
    }
    const int h0 = blockIdx.y * kScoreHyps;
    const int nh = iters - h0 < kScoreHyps ? iters - h0 : kScoreHyps;
    for (int h = 0; h < nh; ++h) {
        const double *F = Fh + ((int64_t)b * iters + h0 + h) * 9;
        double Fr[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) Fr[j] = F[j];
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < kScorePts; ++k) {
            const double d = sampson(Fr, q[k][0], q[k][1], c, q[k][2], q[k][3], c);
            cnt += __popcll(__ballot(has[k] && d < thresh));
        }
        if (lane == 0) wc[wv][h] = cnt;
    }
    __syncthreads();
    if (tid < nh) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < kScoreThreads / 64; ++k) s += wc[k][tid];
        if (s) atomicAdd(counts + (int64_t)b * iters + h0 + tid, s);   // integer: order-free
    }
}

// ------------------------------------------------------------------------------------------------------------ best + refit
__global__ __launch_bounds__(kRefitThreads) void epi_refit_kernel(const double *__restrict__ pts, const int *__restrict__ npts, int cap,
                                                                 const double *__restrict__ Fh, const int *__restrict__ counts,
                                                                 int iters, double thresh, double *__restrict__ F_out,
                                                                 int *__restrict__ ok_out, int *__restrict__ best_out) {
    __shared__ pwc::WaveLds<double, kRefitThreads, 45> red;
    __shared__ int bc[kRefitThreads / 64], bi[kRefitThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = npts[b];
    // argmax, first index on ties
    int mc = -1, mi = 0x7fffffff;
    if (N >= 8)
        for (int i = tid; i < iters; i += kRefitThreads) {
            const int c = counts[(int64_t)b * iters + i];
            if (c > mc) { mc = c; mi = i; }
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int oc = __shfl_xor(mc, o, 64), oi = __shfl_xor(mi, o, 64);
        if (oc > mc || (oc == mc && oi < mi)) { mc = oc; mi = oi; }
    }
    if (lane == 0) { bc[wv] = mc; bi[wv] = mi; }
    __syncthreads();
    mc = bc[0]; mi = bi[0];
    for (int k = 1; k < kRefitThreads / 64; ++k)
        if (bc[k] > mc || (bc[k] == mc && bi[k] < mi)) { mc = bc[k]; mi = bi[k]; }
    double *Fo = F_out + (int64_t)b * 9;
    if (N < 8 || mc < 8) {
        if (tid < 9) Fo[tid] = 0.0;
        if (tid == 0) { ok_out[b] = 0; if (best_out) best_out[b] = N < 8 ? -1 : mi; }
        return;
    }
    double Fb[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) Fb[j] = Fh[((int64_t)b * iters + mi) * 9 + j];
    const double w = hom_w(), c = 1.0 / w;
    const double *P = pts + (int64_t)b * cap * 4;
    // pass 1: inlier count and coordinate sums
    double s4[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < N; j += kRefitThreads) {
        const double a = P[4 * j] / w, bb = P[4 * j + 1] / w, e = P[4 * j + 2] / w, f = P[4 * j + 3] / w;
        if (sampson(Fb, a, bb, c, e, f, c) < thresh) { s4[0] += a; s4[1] += bb; s4[2] += e; s4[3] += f; s4[4] += 1.0; }
    }
    wave_block_sum(red, s4);
    const double n = s4[4];
    const double m1x = s4[0] / n, m1y = s4[1] / n, m2x = s4[2] / n, m2y = s4[3] / n;
    // pass 2: mean distances
    double s2v[2] = {0.0, 0.0};
    for (int j = tid; j < N; j += kRefitThreads) {
        const double a = P[4 * j] / w, bb = P[4 * j + 1] / w, e = P[4 * j + 2] / w, f = P[4 * j + 3] / w;
        if (sampson(Fb, a, bb, c, e, f, c) < thresh) {
            const double dx = a - m1x, dy = bb - m1y, ex = e - m2x, ey = f - m2y;
            s2v[0] += sqrt(dx * dx + dy * dy) + kEps12;
            s2v[1] += sqrt(ex * ex + ey * ey) + kEps12;
        }
    }
    wave_block_sum(red, s2v);
    const double s1 = 1.4142135623730951 / (s2v[0] / n), s2 = 1.4142135623730951 / (s2v[1] / n);
    // pass 3: Gram matrix of the normalised rows (upper triangle, 45 sums)
    double g[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) g[k] = 0.0;
    for (int j = tid; j < N; j += kRefitThreads) {
        const double a = P[4 * j] / w, bb = P[4 * j + 1] / w, e = P[4 * j + 2] / w, f = P[4 * j + 3] / w;
        if (sampson(Fb, a, bb, c, e, f, c) < thresh) {
            double r[9];
            design_row(a, bb, e, f, c, s1, m1x, m1y, s2, m2x, m2y, r);
            int k = 0;
#pragma unroll
            for (int p = 0; p < 9; ++p)
#pragma unroll
                for (int q = p; q < 9; ++q) g[k++] += r[p] * r[q];
        }
    }
    wave_block_sum(red, g);
    if (tid != 0) return;
    double G[9][9];
    {
        int k = 0;
#pragma unroll
        for (int p = 0; p < 9; ++p)
#pragma unroll
            for (int q = p; q < 9; ++q) { G[p][q] = g[k]; G[q][p] = g[k]; ++k; }
    }
    row_jacobi<9, 9>(G);
    double fv[9];
    kth_row<9, 9>(G, n < 9.0 ? (int)n : 9, fv);
    finish_F(fv, s1, m1x, m1y, s2, m2x, m2y, Fo);
    ok_out[b] = 1;
    if (best_out) best_out[b] = mi;
}

// ------------------------------------------------------------------------------------------------------------ distance map
// d over all H x W pixels, x1 = (x, y, 1) / (1 + 1e-12), x2 = (x + fu, y + fv, 1) / (1 + 1e-12) (train_fundamental.py:285-296)
__global__ __launch_bounds__(kMapThreads) void epi_dist_kernel(const float *__restrict__ flow, const double *__restrict__ Fm,
                                                              int64_t F_bs, double *__restrict__ dist, int H, int W, int64_t flow_bs) {
    const int64_t plane = (int64_t)H * W;
    const int b = blockIdx.y;
    const int64_t o = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
    if (o >= plane) return;
    const double *F = Fm + b * F_bs;
    double Fr[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) Fr[j] = F[j];
    const int y = (int)(o / W), x = (int)(o % W);
    const float *fu = flow + (int64_t)b * flow_bs;
    const double w = hom_w(), c = 1.0 / w;
    const double u2 = (double)x + (double)fu[o], v2 = (double)y + (double)fu[plane + o];
    dist[(int64_t)b * plane + o] = sampson(Fr, (double)x / w, (double)y / w, c, u2 / w, v2 / w, c);
}

// ------------------------------------------------------------------------------------------------------------ threshold
struct SelCfg {
    double tau, keep_ratio, min_keep;
    int use_keep, use_min;
};

// numpy's linear quantile from the order statistics lo = x[k], hi = x[k+1] (hi = lo past the end), gamma = vi - k
__device__ __forceinline__ double np_lerp(double a, double bv, double g) {
    const double diff = bv - a;
    return g >= 0.5 ? bv - diff * (1.0 - g) : a + diff * g;
}

// one workgroup per sample: finite count, radix select of up to four ranks, lerp, keep count, relaxation decision
__global__ __launch_bounds__(kSelThreads) void epi_select_kernel(const double *__restrict__ dist, const int *__restrict__ ok,
                                                                int64_t plane, SelCfg cfg, double *__restrict__ thr_out,
                                                                int *__restrict__ all_out) {
    __shared__ unsigned hist[4][256];
    __shared__ pwc::WaveLds<long long, kSelThreads> redi;
    __shared__ unsigned long long pre_s[4];
    __shared__ int64_t rank_s[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double *d = dist + (int64_t)b * plane;
    const unsigned long long *key = reinterpret_cast<const unsigned long long *>(d);
    if (!ok[b]) {
        if (tid == 0) { thr_out[b] = __longlong_as_double(0x7ff8000000000000LL); all_out[b] = 1; }
        return;
    }
    long long nf[1] = {0};
    for (int64_t o = tid; o < plane; o += kSelThreads) nf[0] += finite64(d[o]) ? 1 : 0;
    wave_block_sum(redi, nf);
    const int64_t nfin = nf[0];
    if (nfin == 0) {
        if (tid == 0) { thr_out[b] = __longlong_as_double(0x7ff8000000000000LL); all_out[b] = 1; }
        return;
    }
    // ranks: 0/1 -> keep_ratio's (k, k+1), 2/3 -> min_keep's
    int64_t rk[4];
    double gam[2];
    const double qs[2] = {cfg.keep_ratio, cfg.min_keep};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const double vi = (double)(nfin - 1) * qs[t];
        int64_t k0, k1;
        if (vi >= (double)(nfin - 1)) { k0 = k1 = nfin - 1; gam[t] = vi - (-1.0); }
        else { const double fl = floor(vi); k0 = (int64_t)fl; k1 = k0 + 1; gam[t] = vi - fl; }
        rk[2 * t] = k0; rk[2 * t + 1] = k1;
    }
    if (tid < 4) { pre_s[tid] = 0ull; rank_s[tid] = rk[tid]; }
    __syncthreads();
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int k = tid; k < 4 * 256; k += kSelThreads) (&hist[0][0])[k] = 0u;
        __syncthreads();
        const unsigned long long hmask = shift == 56 ? 0ull : (~0ull << (shift + 8));
        unsigned long long pre[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) pre[t] = pre_s[t];
        for (int64_t o = tid; o < plane; o += kSelThreads) {
            const unsigned long long kv = key[o];
            if (!finite64(__longlong_as_double((long long)kv))) continue;
            const unsigned dg = (unsigned)(kv >> shift) & 255u;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if ((kv & hmask) == pre[t]) atomicAdd(&hist[t][dg], 1u);
        }
        __syncthreads();
        if (wv < 4) {
            // wave wv resolves target wv: inclusive scan of its 256 bins, 4 per lane
            const int t = wv;
            unsigned c4[4], loc = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { c4[k] = hist[t][lane * 4 + k]; loc += c4[k]; }
            unsigned inc = loc;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned v = __shfl_up(inc, o, 64);
                if (lane >= o) inc += v;
            }
            const int64_t r = rank_s[t];
            int64_t run = (int64_t)(inc - loc);
            int hit = -1;
            int64_t below = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (hit < 0 && r >= run && r < run + (int64_t)c4[k]) { hit = lane * 4 + k; below = run; }
                run += c4[k];
            }
            const unsigned long long hb = __ballot(hit >= 0);
            const int src = hb ? __ffsll((long long)hb) - 1 : 0;
            const int hd = __shfl(hit, src, 64);
            const long long bl = __shfl((long long)below, src, 64);
            if (lane == 0 && hb) {
                pre_s[t] = pre_s[t] | ((unsigned long long)hd << shift);
                rank_s[t] = r - bl;
            }
        }
        __syncthreads();
    }
    double val[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) val[t] = __longlong_as_double((long long)pre_s[t]);
    const double qk = np_lerp(val[0], val[1], gam[0]), qm = np_lerp(val[2], val[3], gam[1]);
    double thr = cfg.tau;
    if (cfg.use_keep && qk < thr) thr = qk;
    if (cfg.use_min) {
        long long keep[1] = {0};
        for (int64_t o = tid; o < plane; o += kSelThreads) {
            const double v = d[o];
            keep[0] += (finite64(v) && v <= thr) ? 1 : 0;
        }
        wave_block_sum(redi, keep);
        if ((double)keep[0] / (double)plane < cfg.min_keep) thr = qm < cfg.tau ? qm : cfg.tau;
    }
    if (tid == 0) { thr_out[b] = thr; all_out[b] = 0; }
}

__global__ __launch_bounds__(kMapThreads) void epi_mask_kernel(const double *__restrict__ dist, const double *__restrict__ thr,
                                                              const int *__restrict__ all, unsigned char *__restrict__ mask,
                                                              int64_t plane) {
    const int b = blockIdx.y;
    const int64_t o = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
    if (o >= plane) return;
    const int64_t i = (int64_t)b * plane + o;
    const double v = dist[i];
    mask[i] = (all[b] || (finite64(v) && v <= thr[b])) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ soft loss
struct LossArgs {
    const float *flow;
    const double *F;
    int64_t F_bs;
    const int *ok;
    int64_t ok_bs;
    const void *mask;
    int mask_u8;
    int H, W, robust;
    double delta, weight;
    int64_t flow_bs, mask_bs;
};

__device__ __forceinline__ bool loss_sel(const LossArgs &a, int b, int64_t o) {
    if (a.ok && !a.ok[b * a.ok_bs]) return false;
    if (!a.mask) return true;
    if (a.mask_u8) return static_cast<const unsigned char *>(a.mask)[(int64_t)b * a.mask_bs + o] != 0;
    return static_cast<const float *>(a.mask)[(int64_t)b * a.mask_bs + o] > 0.5f;
}

__device__ __forceinline__ void loss_F(const LossArgs &a, int b, double (&Fr)[9]) {
    const double *F = a.F + b * a.F_bs;
#pragma unroll
    for (int j = 0; j < 9; ++j) Fr[j] = (double)(float)F[j];   // F_np cast to the flow dtype (:355)
}

// per-pixel loss term and its derivative dL/dd
__device__ __forceinline__ double robust_term(int robust, double d, double delta, double *dldd) {
    if (robust == 0) {
        const double r = sqrt(d + kEps12);
        if (r <= delta) { *dldd = 0.5 / delta; return 0.5 * (r * r) / delta; }
        *dldd = 0.5 / r;
        return r - 0.5 * delta;
    }
    if (robust == 1) {
        const double r = sqrt(d + kEps12);
        *dldd = 0.5 / r;
        return r;
    }
    *dldd = 1.0;
    return d;
}

// workgroup (chunk, sample) writes {sum, count} of its 2048 pixels; fixed sequential-then-tree order.  wave_block_sum starts the
// sum over the waves at the first wave's value and not at +0.0: the same bits, because a sum is -0.0 only when both terms are, every
// lane (here and in the finish kernel) starts from +0.0, and so no lane's sum, no wave's and no partial is ever -0.0.
__global__ __launch_bounds__(kLossThreads) void epi_loss_partial_kernel(LossArgs a, double *__restrict__ part) {
    __shared__ pwc::WaveLds<double, kLossThreads, 2> red;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t plane = (int64_t)a.H * a.W;
    double Fr[9];
    loss_F(a, b, Fr);
    const float *fu = a.flow + (int64_t)b * a.flow_bs;
    double v[2] = {0.0, 0.0};   // sum, count
    for (int k = 0; k < kLossPer; ++k) {
        const int64_t o = (int64_t)blockIdx.x * kLossChunk + k * kLossThreads + tid;
        if (o >= plane || !loss_sel(a, b, o)) continue;
        const int y = (int)(o / a.W), x = (int)(o % a.W);
        const double d = sampson(Fr, (double)x, (double)y, 1.0, (double)((float)x + fu[o]), (double)((float)y + fu[plane + o]), 1.0);
        double g;
        v[0] += robust_term(a.robust, d, a.delta, &g);
        v[1] += 1.0;
    }
    wave_block_sum(red, v);
    if (tid == 0) {
        const int64_t pi = (int64_t)b * gridDim.x + blockIdx.x;
        part[2 * pi] = v[0];
        part[2 * pi + 1] = v[1];
    }
}

// one workgroup: partials in a fixed order -> out (float loss) and tot = {sum, count} (fp64, for the backward)
__global__ __launch_bounds__(kLossThreads) void epi_loss_finish_kernel(const double *__restrict__ part, int64_t np, double weight,
                                                                      float *__restrict__ out, double *__restrict__ tot) {
    __shared__ pwc::WaveLds<double, kLossThreads, 2> red;
    const int tid = threadIdx.x;
    double v[2] = {0.0, 0.0};
    for (int64_t i = tid; i < np; i += kLossThreads) { v[0] += part[2 * i]; v[1] += part[2 * i + 1]; }
    wave_block_sum(red, v);
    if (tid == 0) {
        const double S = v[0], C = v[1];
        if (out) out[0] = C > 0.0 ? (float)(weight * (S / C)) : 0.0f;
        if (tot) { tot[0] = S; tot[1] = C; }
    }
}

// grad_flow = g * weight / count * dL/dd * dd/dflow on selected pixels, 0 elsewhere
__global__ __launch_bounds__(kLossThreads) void epi_loss_bwd_kernel(LossArgs a, const double *__restrict__ tot,
                                                                   const float *__restrict__ grad_out, float *__restrict__ gflow) {
    const int b = blockIdx.y;
    const int64_t plane = (int64_t)a.H * a.W;
    const int64_t o = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    if (o >= plane) return;
    float *gu = gflow + (int64_t)b * 2 * plane;
    const double C = tot[1];
    if (C <= 0.0 || !loss_sel(a, b, o)) { gu[o] = 0.0f; gu[plane + o] = 0.0f; return; }
    double F[9];
    loss_F(a, b, F);
    const float *fu = a.flow + (int64_t)b * a.flow_bs;
    const int y = (int)(o / a.W), x = (int)(o % a.W);
    const double X = (double)x, Y = (double)y, u2 = (double)((float)x + fu[o]), v2 = (double)((float)y + fu[plane + o]);
    const double f0 = F[0] * X + F[1] * Y + F[2];
    const double f1 = F[3] * X + F[4] * Y + F[5];
    const double f2 = F[6] * X + F[7] * Y + F[8];
    const double t0 = F[0] * u2 + F[3] * v2 + F[6];
    const double t1 = F[1] * u2 + F[4] * v2 + F[7];
    const double n = u2 * f0 + v2 * f1 + f2;
    const double den = f0 * f0 + f1 * f1 + t0 * t0 + t1 * t1 + kEps12;
    const double d = (n * n) / den;
    double dl;
    robust_term(a.robust, d, a.delta, &dl);
    const double sc = (double)grad_out[0] * a.weight / C * dl;
    const double q = (n * n) / (den * den);
    const double gx = 2.0 * n * f0 / den - q * (2.0 * t0 * F[0] + 2.0 * t1 * F[1]);
    const double gy = 2.0 * n * f1 / den - q * (2.0 * t0 * F[3] + 2.0 * t1 * F[4]);
    gu[o] = (float)(sc * gx);
    gu[plane + o] = (float)(sc * gy);
}

int64_t pad8(int64_t n) { return (n + 7) & ~7LL; }

int64_t loss_parts(int B, int H, int W) { return (int64_t)B * (((int64_t)H * W + kLossChunk - 1) / kLossChunk); }

}  // namespace

extern "C" int pwc_epipolar_pairs(const void *flow, const void *mask, int mask_u8, void *pts, void *npts, int B, int H, int W,
                                  int stride, int64_t flow_bstride, int64_t mask_bstride, void *stream) {
    if (!flow || !pts || !npts) PWC_FAIL(PWC_EINVAL, "pwc_epipolar_pairs: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || stride <= 0)
        PWC_FAIL(PWC_EINVAL, "pwc_epipolar_pairs: bad shape B=%d H=%d W=%d stride=%d", B, H, W, stride);
    const int64_t plane = (int64_t)H * W;
    if (flow_bstride < 2 * plane || (mask && mask_bstride < plane))
        PWC_FAIL(PWC_EINVAL, "pwc_epipolar_pairs: batch stride smaller than the tensor");
    if (misaligned({flow, npts}, 4) || (mask && !mask_u8 && misaligned({mask}, 4)) || misaligned({pts}, 8) ||
        2 * plane >= 0x7fffffffLL || B > 65535) {
        pwc::set_error("pwc_epipolar_pairs: needs aligned operands, 2*H*W < 2^31 and B <= 65535");
        return PWC_EUNSUPPORTED;
    }
    const int Ws = (W + stride - 1) / stride, Hs = (H + stride - 1) / stride;
    hipLaunchKernelGGL(epi_pairs_kernel, dim3(B), dim3(1024), 0, static_cast<hipStream_t>(stream), static_cast<const float *>(flow),
                       mask, mask_u8 ? 1 : 0, static_cast<double *>(pts), static_cast<int *>(npts), H, W, stride, Ws, Hs * Ws,
                       flow_bstride, mask_bstride);
    return pwc::check_launch("epi_pairs_kernel");
}

extern "C" int64_t pwc_epipolar_ransac_workspace_bytes(int B, int iters) {
    if (B <= 0 || iters <= 0) return -1;
    return pad8((int64_t)B * iters * 9 * 8);
}

extern "C" int pwc_epipolar_ransac(const void *pts, const void *npts, int cap, const void *idx, int64_t idx_bstride, int B, int iters,
                                   double thresh, void *F_out, void *ok_out, void *best_out, void *counts, void *workspace,
                                   int64_t workspace_bytes, void *stream) {
    if (!pts || !npts || !idx || !F_out || !ok_out || !counts || !workspace)
        PWC_FAIL(PWC_EINVAL, "pwc_epipolar_ransac: null pointer");
    if (B <= 0 || iters <= 0 || cap <= 0) PWC_FAIL(PWC_EINVAL, "pwc_epipolar_ransac: bad shape B=%d iters=%d cap=%d", B, iters, cap);
    if (idx_bstride != 0 && idx_bstride < 8LL * iters) PWC_FAIL(PWC_EINVAL, "pwc_epipolar_ransac: index batch stride < 8*iters");
    const int64_t need = pwc_epipolar_ransac_workspace_bytes(B, iters);
    if (workspace_bytes < need || misaligned({workspace}, 8))
        PWC_FAIL(PWC_EINVAL, "pwc_epipolar_ransac: workspace needs %lld bytes, 8-byte aligned", (long long)need);
    if (misaligned({pts, F_out}, 8) || misaligned({npts, idx, ok_out, best_out, counts}, 4) || B > 65535 ||
        (int64_t)cap * 4 >= 0x7fffffffLL || iters > 65535 * 64 || !(thresh == thresh)) {
        pwc::set_error("pwc_epipolar_ransac: needs aligned operands, B <= 65535, iters <= 4194240 and a finite threshold");
        return PWC_EUNSUPPORTED;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *Fh = static_cast<double *>(workspace);
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)B * iters * 4, st);
    if (e != hipSuccess) { pwc::set_error("pwc_epipolar_ransac: hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
    const int *np_ = static_cast<const int *>(npts);
    const double *P = static_cast<const double *>(pts);
    hipLaunchKernelGGL(epi_hyp_kernel, dim3((iters + 63) / 64, B), dim3(64), 0, st, P, np_, cap, static_cast<const int *>(idx),
                       idx_bstride, iters, Fh);
    hipLaunchKernelGGL(epi_score_kernel, dim3((cap + kScoreThreads * kScorePts - 1) / (kScoreThreads * kScorePts),
                       (iters + kScoreHyps - 1) / kScoreHyps, B), dim3(kScoreThreads), 0, st, P, np_, cap, Fh, iters, thresh,
                       static_cast<int *>(counts));
    hipLaunchKernelGGL(epi_refit_kernel, dim3(B), dim3(kRefitThreads), 0, st, P, np_, cap, Fh, static_cast<const int *>(counts),
                       iters, thresh, static_cast<double *>(F_out), static_cast<int *>(ok_out), static_cast<int *>(best_out));
    return pwc::check_launch("epi_ransac");
}

extern "C" int pwc_epipolar_distance(const void *flow, const void *F, int64_t F_bstride, void *dist, int B, int H, int W,
                                     int64_t flow_bstride, void *stream) {
    if (!flow || !F || !dist) PWC_FAIL(PWC_EINVAL, "pwc_epipolar_distance: null pointer");
    if (B <= 0 || H <= 0 || W <= 0) PWC_FAIL(PWC_EINVAL, "pwc_epipolar_distance: bad shape B=%d H=%d W=%d", B, H, W);
    const int64_t plane = (int64_t)H * W;
    if (flow_bstride < 2 * plane || (F_bstride != 0 && F_bstride < 9))
        PWC_FAIL(PWC_EINVAL, "pwc_epipolar_distance: batch stride smaller than the tensor");
    if (misaligned({flow}, 4) || misaligned({F, dist}, 8) || 2 * plane >= 0x7fffffffLL || B > 65535) {
        pwc::set_error("pwc_epipolar_distance: needs aligned operands, 2*H*W < 2^31 and B <= 65535");
        return PWC_EUNSUPPORTED;
    }
    hipLaunchKernelGGL(epi_dist_kernel, dim3((unsigned)((plane + kMapThreads - 1) / kMapThreads), B), dim3(kMapThreads), 0,
                       static_cast<hipStream_t>(stream), static_cast<const float *>(flow), static_cast<const double *>(F), F_bstride,
                       static_cast<double *>(dist), H, W, flow_bstride);
    return pwc::check_launch("epi_dist_kernel");
}

extern "C" int64_t pwc_epipolar_mask_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    return pad8((int64_t)B * H * W * 8) + pad8((int64_t)B * 4);
}

extern "C" int pwc_epipolar_mask(const void *flow, const void *F, const void *ok, void *mask_out, void *thr_out, void *dist_out,
                                 int B, int H, int W, double tau, double keep_ratio, double min_keep, int64_t flow_bstride,
                                 void *workspace, int64_t workspace_bytes, void *stream) {
    if (!flow || !F || !ok || !mask_out || !thr_out || !workspace) PWC_FAIL(PWC_EINVAL, "pwc_epipolar_mask: null pointer");
    if (B <= 0 || H <= 0 || W <= 0) PWC_FAIL(PWC_EINVAL, "pwc_epipolar_mask: bad shape B=%d H=%d W=%d", B, H, W);
    const int64_t plane = (int64_t)H * W;
    if (flow_bstride < 2 * plane) PWC_FAIL(PWC_EINVAL, "pwc_epipolar_mask: batch stride smaller than the tensor");
    const int64_t need = pwc_epipolar_mask_workspace_bytes(B, H, W);
    if (workspace_bytes < need || misaligned({workspace}, 8))
        PWC_FAIL(PWC_EINVAL, "pwc_epipolar_mask: workspace needs %lld bytes, 8-byte aligned", (long long)need);
    if (misaligned({flow, ok}, 4) || misaligned({F, thr_out, dist_out}, 8) || 2 * plane >= 0x7fffffffLL || B > 65535 ||
        !(tau == tau)) {
        pwc::set_error("pwc_epipolar_mask: needs aligned operands, 2*H*W < 2^31, B <= 65535 and tau not NaN");
        return PWC_EUNSUPPORTED;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    double *dist = dist_out ? static_cast<double *>(dist_out) : reinterpret_cast<double *>(ws);
    int *all = reinterpret_cast<int *>(ws + pad8((int64_t)B * plane * 8));
    const dim3 grid((unsigned)((plane + kMapThreads - 1) / kMapThreads), B);
    hipLaunchKernelGGL(epi_dist_kernel, grid, dim3(kMapThreads), 0, st, static_cast<const float *>(flow), static_cast<const double *>(F),
                       (int64_t)9, dist, H, W, flow_bstride);
    SelCfg cfg{tau, keep_ratio, min_keep, (keep_ratio > 0.0 && keep_ratio < 1.0) ? 1 : 0, (min_keep > 0.0 && min_keep < 1.0) ? 1 : 0};
    hipLaunchKernelGGL(epi_select_kernel, dim3(B), dim3(kSelThreads), 0, st, dist, static_cast<const int *>(ok), plane, cfg,
                       static_cast<double *>(thr_out), all);
    hipLaunchKernelGGL(epi_mask_kernel, grid, dim3(kMapThreads), 0, st, dist, static_cast<const double *>(thr_out), all,
                       static_cast<unsigned char *>(mask_out), plane);
    return pwc::check_launch("epi_mask");
}

extern "C" int64_t pwc_epipolar_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    return 16 * loss_parts(B, H, W) + 16;
}

static int loss_args(const char *who, const void *flow, const void *F, int64_t F_bstride, int64_t ok_bstride, const void *mask,
                     int mask_u8, const void *out, int B, int H, int W, int robust, double delta, int64_t flow_bstride,
                     int64_t mask_bstride, const void *workspace, int64_t workspace_bytes) {
    if (!flow || !F || !out || !workspace) PWC_FAIL(PWC_EINVAL, "%s: null pointer", who);
    if (B <= 0 || H <= 0 || W <= 0) PWC_FAIL(PWC_EINVAL, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    if (robust < 0 || robust > 2) PWC_FAIL(PWC_EINVAL, "%s: robust must be 0 (huber), 1 (l1) or 2 (mean)", who);
    const int64_t plane = (int64_t)H * W;
    if (flow_bstride < 2 * plane || (mask && mask_bstride < plane) || (F_bstride != 0 && F_bstride < 9) || ok_bstride < 0)
        PWC_FAIL(PWC_EINVAL, "%s: batch stride smaller than the tensor", who);
    const int64_t need = pwc_epipolar_loss_workspace_bytes(B, H, W);
    if (workspace_bytes < need || misaligned({workspace}, 8))
        PWC_FAIL(PWC_EINVAL, "%s: workspace needs %lld bytes, 8-byte aligned", who, (long long)need);
    if (misaligned({flow, out}, 4) || (mask && !mask_u8 && misaligned({mask}, 4)) || misaligned({F}, 8) ||
        2 * plane >= 0x7fffffffLL || B > 65535 || !(delta > 0.0)) {
        pwc::set_error("%s: needs aligned operands, 2*H*W < 2^31, B <= 65535 and delta > 0", who);
        return PWC_EUNSUPPORTED;
    }
    return PWC_OK;
}

extern "C" int pwc_epipolar_loss_fwd(const void *flow, const void *F, int64_t F_bstride, const void *ok, int64_t ok_bstride,
                                     const void *mask, int mask_u8, void *out, int B, int H, int W, int robust, double delta,
                                     double weight, int64_t flow_bstride, int64_t mask_bstride, void *workspace,
                                     int64_t workspace_bytes, void *stream) {
    const int rc = loss_args("pwc_epipolar_loss_fwd", flow, F, F_bstride, ok_bstride, mask, mask_u8, out, B, H, W, robust, delta,
                             flow_bstride, mask_bstride, workspace, workspace_bytes);
    if (rc != PWC_OK) return rc;
    if (misaligned({ok}, 4)) { pwc::set_error("pwc_epipolar_loss_fwd: needs aligned operands"); return PWC_EUNSUPPORTED; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    LossArgs a{static_cast<const float *>(flow), static_cast<const double *>(F), F_bstride, static_cast<const int *>(ok), ok_bstride,
               mask, mask_u8 ? 1 : 0, H, W, robust, delta, weight, flow_bstride, mask_bstride};
    double *part = static_cast<double *>(workspace);
    const int64_t nbx = ((int64_t)H * W + kLossChunk - 1) / kLossChunk, np = loss_parts(B, H, W);
    hipLaunchKernelGGL(epi_loss_partial_kernel, dim3((unsigned)nbx, B), dim3(kLossThreads), 0, st, a, part);
    hipLaunchKernelGGL(epi_loss_finish_kernel, dim3(1), dim3(kLossThreads), 0, st, part, np, weight, static_cast<float *>(out),
                       part + 2 * np);
    return pwc::check_launch("epi_loss_fwd");
}

extern "C" int pwc_epipolar_loss_bwd(const void *flow, const void *F, int64_t F_bstride, const void *ok, int64_t ok_bstride,
                                     const void *mask, int mask_u8, const void *grad_out, void *grad_flow, int B, int H, int W,
                                     int robust, double delta, double weight, int64_t flow_bstride, int64_t mask_bstride,
                                     void *workspace, int64_t workspace_bytes, void *stream) {
    if (!grad_out) PWC_FAIL(PWC_EINVAL, "pwc_epipolar_loss_bwd: null pointer");
    const int rc = loss_args("pwc_epipolar_loss_bwd", flow, F, F_bstride, ok_bstride, mask, mask_u8, grad_flow, B, H, W, robust, delta,
                             flow_bstride, mask_bstride, workspace, workspace_bytes);
    if (rc != PWC_OK) return rc;
    if (misaligned({ok, grad_out}, 4)) { pwc::set_error("pwc_epipolar_loss_bwd: needs aligned operands"); return PWC_EUNSUPPORTED; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    LossArgs a{static_cast<const float *>(flow), static_cast<const double *>(F), F_bstride, static_cast<const int *>(ok), ok_bstride,
               mask, mask_u8 ? 1 : 0, H, W, robust, delta, weight, flow_bstride, mask_bstride};
    double *part = static_cast<double *>(workspace);
    const int64_t plane = (int64_t)H * W, nbx = (plane + kLossChunk - 1) / kLossChunk, np = loss_parts(B, H, W);
    hipLaunchKernelGGL(epi_loss_partial_kernel, dim3((unsigned)nbx, B), dim3(kLossThreads), 0, st, a, part);
    hipLaunchKernelGGL(epi_loss_finish_kernel, dim3(1), dim3(kLossThreads), 0, st, part, np, weight, static_cast<float *>(nullptr),
                       part + 2 * np);
    hipLaunchKernelGGL(epi_loss_bwd_kernel, dim3((unsigned)((plane + kLossThreads - 1) / kLossThreads), B), dim3(kLossThreads), 0, st,
                       a, static_cast<const double *>(part + 2 * np), static_cast<const float *>(grad_out),
                       static_cast<float *>(grad_flow));
    return pwc::check_launch("epi_loss_bwd");
}
