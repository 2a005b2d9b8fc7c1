// Vanishing point of a flow field on the device: estimate_vanishing_point_from_flow of pwc_extract_flow_video_vanishpoint.py:93-255,
// batched, from the arrow grid pwc_flow_quiver leaves (vec float [n][Gy][Gx][2] = (dx, dy) at x = gx*step, y = gy*step).  All
// arithmetic is fp64 with no contraction, the expressions spelled out in include/pwc_hip.h.  Three launches per call:
//
//   select_kernel  one workgroup per frame: zeroes the frame's histogram, counts the cells with a finite hypot(dx, dy) >= min_mag (N), and
//                  writes the selected cells in order: all of them row-major when N <= max_points (as the reference does), else the
//                  first max_points kept cells in the sequence of `order` (a permutation of the cells; the reference draws from
//                  NumPy's global state there, which nobody can reproduce).  The compaction is a ballot scan over 256 positions at a
//                  time, so the selected order does not depend on scheduling.  Also leaves the largest selected magnitude.
//   pair_kernel    kPairGroups workgroups per frame, workgroup g takes rows i = g, g + kPairGroups, ... (interleaved: row i has
//                  N - 1 - i pairs, contiguous blocks of rows would leave the last workgroup idle) and the lanes take j = i + 1 ...
//                  Each kept intersection adds its weight to its bin with a 64-bit INTEGER atomicAdd (into the workgroup's own
//                  histogram in LDS for grid <= 64, whose non-empty bins are then added to the frame's; straight into the frame's
//                  for a larger grid): the weight is
//                  mag_i * mag_j with both magnitudes divided by the frame's largest selected one, so w' in (0, 1], stored as
//                  llrint(w' * 2^40).  Integer addition commutes, so two runs give the same bits whatever the order of the atomics.
//                  At most 1024 * 1023 / 2 < 2^19 pairs of at most 2^40 each: the sum stays below 2^59.
//                  Bound on prob (best bin / total): one rounding of w' * 2^40 to an integer is an absolute 2^-41 of w'.  With
//                  max(mag) / min(mag) <= R, w' >= R^-2, so the relative error per weight, and hence per sum of weights, is at most
//                  R^2 * 2^-41 (4.5e-9 for R = 100); the two products and the division by maxmag add a few 2^-53.  prob inherits
//                  twice that.
//   finish_kernel  one workgroup per frame: arg-max of the histogram over the flat index gx * grid + gy (lowest index wins a tie, as
//                  np.argmax), the bin centre, prob, the distances of all N lines to the centre rounded to fp32 (the reference builds
//                  the candidate as a float32 array), their median by counting ranks in LDS, the inliers, and the 2 x 2 normal
//                  equations of the inlier lines summed lane-strided and then in tree_sum's fixed order (no atomics).  The right-hand
//                  side is taken about the bin centre (c - n . centre), which leaves the solution unchanged and keeps the sums small.
//
// The kernels are latency-sized: a frame is a few hundred cells and at most 2^19 pairs.  Nothing allocates or synchronises.
#include <math.h>

#include "pwc_block_reduce.h"
#include "pwc_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxPoints = 1024, kMaxGrid = 128, kMaxCells = 65536;
constexpr int kPairGroups = 16;
constexpr int kLdsGrid = 64;                   // largest grid whose histogram a pair workgroup keeps in LDS
constexpr double kFix = 1099511627776.0;      // 2^40

struct Head {                                  // first bytes of a frame's workspace
    int n_kept, n_used;
    double maxmag;
    long long pairs;
};
static_assert(sizeof(Head) == 24, "vanishing workspace layout");

struct Vp {
    const float2 *vec;
    const int *order;
    char *ws;
    int64_t frame_bytes;
    int gy, gx, cells, step, max_points, grid, min_pairs;
    double min_mag;
    double xlo, xhi, xstep, ylo, yhi, ystep;     // histogram range and (hi - lo) / grid, as np.linspace computes them
};

__device__ __forceinline__ Head *frame_head(const Vp &p, int b) { return reinterpret_cast<Head *>(p.ws + (int64_t)b * p.frame_bytes); }
__device__ __forceinline__ long long *frame_hist(const Vp &p, int b) {
    return reinterpret_cast<long long *>(p.ws + (int64_t)b * p.frame_bytes + sizeof(Head));
}
__device__ __forceinline__ int *frame_sel(const Vp &p, int b) {
    return reinterpret_cast<int *>(p.ws + (int64_t)b * p.frame_bytes + sizeof(Head) + (int64_t)8 * p.grid * p.grid);
}

__device__ __forceinline__ double cell_mag(const Vp &p, int b, int cell, double *dx, double *dy) {
    const float2 v = p.vec[(int64_t)b * p.cells + cell];
    *dx = (double)v.x;
    *dy = (double)v.y;
    return hypot(*dx, *dy);
}

// the selection's one predicate: at least min_mag and finite.  A NaN magnitude fails the first test by itself; an infinite one would
// pass it, become the frame's largest magnitude and turn every weight of the frame into 0 or NaN.
__device__ __forceinline__ bool mag_kept(double mag, double min_mag) { return mag >= min_mag && isfinite(mag); }

// edge k of np.linspace(lo, hi, grid + 1): k * step + lo in two roundings, the last edge hi itself
__device__ __forceinline__ double edge(int k, int grid, double lo, double hi, double step) { return k < grid ? (double)k * step + lo : hi; }

// bin of lo <= v <= hi as np.histogram2d places it: e[k] <= v < e[k + 1], v == hi in the last bin.  A guess, corrected against the edges.
__device__ __forceinline__ int bin_of(double v, int grid, double lo, double hi, double step) {
    int g = (int)floor((v - lo) / step);
    g = g < 0 ? 0 : (g > grid - 1 ? grid - 1 : g);
    while (g > 0 && v < edge(g, grid, lo, hi, step)) --g;
    while (g < grid - 1 && v >= edge(g + 1, grid, lo, hi, step)) ++g;
    return g;
}

__global__ __launch_bounds__(kThreads) void select_kernel(Vp p) {
    __shared__ pwc::TreeLds<kThreads, 0, 1> redn;
    __shared__ double redm[kThreads];
    __shared__ int wave_cnt[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
    long long *hist = frame_hist(p, b);
    int *sel = frame_sel(p, b);
    for (int i = tid; i < p.grid * p.grid; i += kThreads) hist[i] = 0;
    long long cnt[1] = {0};
    double dx, dy;
    for (int c = tid; c < p.cells; c += kThreads) cnt[0] += mag_kept(cell_mag(p, b, c, &dx, &dy), p.min_mag) ? 1 : 0;
    pwc::tree_sum(redn, static_cast<double *>(nullptr), cnt);
    const int n_kept = (int)cnt[0];
    const bool by_order = n_kept > p.max_points;             // the entry point has made sure that `order` is there when this can happen
    int n_used = by_order ? p.max_points : n_kept;
    int offset = 0;
    for (int base = 0; base < p.cells && offset < n_used; base += kThreads) {
        const int pos = base + tid;
        int cell = -1;
        bool keep = false;
        if (pos < p.cells) {
            cell = by_order ? p.order[pos] : pos;
            keep = (unsigned)cell < (unsigned)p.cells && mag_kept(cell_mag(p, b, cell, &dx, &dy), p.min_mag);
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int c = wave_cnt[w];
            before += w < wv ? c : 0;
            total += c;
        }
        const int r = offset + before + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && r < n_used) sel[r] = cell;
        offset += total;
        __syncthreads();
    }
    n_used = offset < n_used ? offset : n_used;              // an `order` that is no permutation may name fewer kept cells
    double mx = 0.0;
    for (int r = tid; r < n_used; r += kThreads) mx = fmax(mx, cell_mag(p, b, sel[r], &dx, &dy));
    redm[tid] = mx;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) redm[tid] = fmax(redm[tid], redm[tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        Head *h = frame_head(p, b);
        h->n_kept = n_kept;
        h->n_used = n_used;
        h->maxmag = redm[0];
        h->pairs = 0;
    }
}

struct Points {                                 // the selected lines of one frame in LDS; x = cx * step, y = cy * step
    unsigned short cx[kMaxPoints], cy[kMaxPoints];   // grid indices: at most 65536 cells, so each index fits 16 bits
    double dxn[kMaxPoints], dyn[kMaxPoints];
};
static_assert(kMaxCells <= 65536, "grid indices are kept in 16 bits");

// kLdsHist: the workgroup votes into its own histogram in LDS (grid <= kLdsGrid: 32 KB) and adds its non-empty bins to the frame's
// histogram at the end, so the atomics of the many pairs that fall into the best bin do not queue up on one address in L2.  A larger
// grid does not fit next to the lines and votes into the frame's histogram directly.  Integer sums: the result is the same either way.
template <bool kLdsHist>
__global__ __launch_bounds__(kThreads) void pair_kernel(Vp p) {
    __shared__ Points pt;
    __shared__ double wn[kMaxPoints];
    __shared__ pwc::TreeLds<kThreads, 0, 1> redn;
    __shared__ unsigned long long lh[kLdsHist ? kLdsGrid * kLdsGrid : 1];
    const int tid = threadIdx.x, b = blockIdx.y;
    const Head *h = frame_head(p, b);
    const int N = h->n_used;
    if (N < 5) return;
    const double maxmag = h->maxmag;
    const int *sel = frame_sel(p, b);
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(frame_hist(p, b));
    for (int r = tid; r < N; r += kThreads) {
        const int cell = sel[r];
        double dx, dy;
        const double mag = cell_mag(p, b, cell, &dx, &dy);
        pt.cx[r] = (unsigned short)(cell % p.gx);
        pt.cy[r] = (unsigned short)(cell / p.gx);
        pt.dxn[r] = dx / mag;
        pt.dyn[r] = dy / mag;
        wn[r] = mag / maxmag;
    }
    if constexpr (kLdsHist)
        for (int i = tid; i < p.grid * p.grid; i += kThreads) lh[i] = 0;
    __syncthreads();
    long long kept[1] = {0};
    for (int i = blockIdx.x; i < N - 1; i += kPairGroups) {
        const double p1x = (double)((int)pt.cx[i] * p.step), p1y = (double)((int)pt.cy[i] * p.step);
        const double d1x = pt.dxn[i], d1y = pt.dyn[i], w1 = wn[i];
        for (int j = i + 1 + tid; j < N; j += kThreads) {
            const double d2x = pt.dxn[j], d2y = pt.dyn[j];
            const double denom = d1x * d2y - d1y * d2x;
            if (fabs(denom) < 1e-6) continue;
            const double dpx = (double)((int)pt.cx[j] * p.step) - p1x, dpy = (double)((int)pt.cy[j] * p.step) - p1y;
            const double t1 = (dpx * d2y - dpy * d2x) / denom;
            const double ix = p1x + t1 * d1x, iy = p1y + t1 * d1y;
            if (!(p.xlo <= ix && ix <= p.xhi && p.ylo <= iy && iy <= p.yhi)) continue;
            const int bx = bin_of(ix, p.grid, p.xlo, p.xhi, p.xstep), by = bin_of(iy, p.grid, p.ylo, p.yhi, p.ystep);
            const long long q = llrint((w1 * wn[j]) * kFix);
            if constexpr (kLdsHist) atomicAdd(&lh[bx * p.grid + by], (unsigned long long)q);
            else atomicAdd(&hist[bx * p.grid + by], (unsigned long long)q);
            ++kept[0];
        }
    }
    if constexpr (kLdsHist) {
        __syncthreads();
        for (int i = tid; i < p.grid * p.grid; i += kThreads)
            if (lh[i]) atomicAdd(&hist[i], lh[i]);
    }
    pwc::tree_sum(redn, static_cast<double *>(nullptr), kept);
    if (tid == 0 && kept[0]) atomicAdd(reinterpret_cast<unsigned long long *>(&frame_head(p, b)->pairs), (unsigned long long)kept[0]);
}

__global__ __launch_bounds__(kThreads) void finish_kernel(Vp p, double *__restrict__ out_vp, int *__restrict__ out_info) {
    __shared__ Points pt;
    __shared__ double dist[kMaxPoints];
    __shared__ pwc::TreeLds<kThreads, 5, 1> red;
    __shared__ pwc::TreeLds<kThreads, 0, 1> redn;            // a sum of counts alone takes the LDS type without doubles: tree_sum reads
                                                             // as many doubles per lane as its LDS type holds
    __shared__ long long bestv[kThreads];
    __shared__ int besti[kThreads];
    __shared__ double med[2];
    const int tid = threadIdx.x, b = blockIdx.x;
    const Head *h = frame_head(p, b);
    const int N = h->n_used;
    const long long pairs = h->pairs;
    const long long *hist = frame_hist(p, b);
    double *vp = out_vp + 5 * (int64_t)b;
    int *info = out_info + 6 * (int64_t)b;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    // best bin: every lane walks its bins in ascending order and keeps the first largest; the tree prefers the lower index on a tie
    long long bv = -1, tot[1] = {0};
    int bi = 0x7fffffff;
    for (int i0 = tid; i0 < p.grid * p.grid; i0 += 8 * kThreads) {       // eight loads in flight, then compared in ascending order
        long long v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = i0 + k * kThreads;
            v[k] = i < p.grid * p.grid ? hist[i] : 0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            tot[0] += v[k];
            if (v[k] > bv && i0 + k * kThreads < p.grid * p.grid) { bv = v[k]; bi = i0 + k * kThreads; }
        }
    }
    bestv[tid] = bv;
    besti[tid] = bi;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const long long ov = bestv[tid + s];
            const int oi = besti[tid + s];
            if (ov > bestv[tid] || (ov == bestv[tid] && oi < besti[tid])) { bestv[tid] = ov; besti[tid] = oi; }
        }
        __syncthreads();
    }
    bv = bestv[0];
    bi = besti[0];
    pwc::tree_sum(redn, static_cast<double *>(nullptr), tot);

    int status = 0;
    if (N < 5) status = 2;
    else if (pairs < (long long)p.min_pairs) status = 3;
    else if (bv <= 0) status = 4;
    if (status) {                                             // uniform: every lane read the same values
        if (tid == 0) {
            vp[0] = nan; vp[1] = nan; vp[2] = 0.0; vp[3] = nan; vp[4] = nan;
            info[0] = status; info[1] = N; info[2] = status == 2 ? 0 : (int)pairs; info[3] = -1; info[4] = -1; info[5] = 0;
        }
        return;
    }
    const int gx = bi / p.grid, gy = bi - gx * p.grid;
    const double cx = 0.5 * (edge(gx, p.grid, p.xlo, p.xhi, p.xstep) + edge(gx + 1, p.grid, p.xlo, p.xhi, p.xstep));
    const double cy = 0.5 * (edge(gy, p.grid, p.ylo, p.yhi, p.ystep) + edge(gy + 1, p.grid, p.ylo, p.yhi, p.ystep));
    // hist of the reference = sum * maxmag^2 / 2^40, so its 1e-9 is 1e-9 * 2^40 / maxmag^2 here
    const double prob = (double)bv / ((double)tot[0] + 1e-9 * kFix / (h->maxmag * h->maxmag));
    const double cxf = (double)(float)cx, cyf = (double)(float)cy;

    const int *sel = frame_sel(p, b);
    for (int r = tid; r < N; r += kThreads) {
        const int cell = sel[r];
        double dx, dy;
        const double mag = cell_mag(p, b, cell, &dx, &dy);
        pt.cx[r] = (unsigned short)(cell % p.gx);
        pt.cy[r] = (unsigned short)(cell / p.gx);
        pt.dxn[r] = dx / mag;
        pt.dyn[r] = dy / mag;
        const double nx = -pt.dyn[r], ny = pt.dxn[r];
        const double c = nx * (double)((int)pt.cx[r] * p.step) + ny * (double)((int)pt.cy[r] * p.step);
        dist[r] = fabs(nx * cxf + ny * cyf - c);
    }
    if (tid == 0) { med[0] = nan; med[1] = nan; }
    __syncthreads();
    // median by rank: rank(r) = how many distances sort before dist[r] (ties by index); the ranks (N-1)/2 and N/2 are the middle
    for (int r = tid; r < N; r += kThreads) {
        const double d = dist[r];
        int rank = 0;
        for (int m = 0; m < N; ++m) {
            const double e = dist[m];
            rank += (e < d || (e == d && m < r)) ? 1 : 0;
        }
        if (rank == (N - 1) / 2) med[0] = d;
        if (rank == N / 2) med[1] = d;
    }
    __syncthreads();
    const double thresh = ((med[0] + med[1]) / 2.0) * 3.0 + 1e-6;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    long long cnt[1] = {0};
    for (int r = tid; r < N; r += kThreads) {
        if (!(dist[r] < thresh)) continue;
        const double nx = -pt.dyn[r], ny = pt.dxn[r];
        const double c = nx * (double)((int)pt.cx[r] * p.step) + ny * (double)((int)pt.cy[r] * p.step);
        const double cc = c - (nx * cx + ny * cy);
        s[0] += nx * nx;
        s[1] += nx * ny;
        s[2] += ny * ny;
        s[3] += nx * cc;
        s[4] += ny * cc;
        ++cnt[0];
    }
    pwc::tree_sum(red, s, cnt);
    if (tid != 0) return;
    double vx = cx, vy = cy;
    status = 1;
    if (cnt[0] >= 5) {
        const double det = s[0] * s[2] - s[1] * s[1], tr = s[0] + s[2];
        if (isfinite(det) && det > 1e-12 * (tr * tr)) {
            vx = cx + (s[2] * s[3] - s[1] * s[4]) / det;
            vy = cy + (s[0] * s[4] - s[1] * s[3]) / det;
            status = 0;
        }
    }
    vp[0] = vx; vp[1] = vy; vp[2] = prob; vp[3] = cx; vp[4] = cy;
    info[0] = status; info[1] = N; info[2] = (int)pairs; info[3] = gx; info[4] = gy; info[5] = (int)cnt[0];
}

int64_t frame_bytes_of(int grid) { return (int64_t)sizeof(Head) + (int64_t)8 * grid * grid + (int64_t)4 * kMaxPoints; }

}  // namespace

extern "C" int64_t pwc_vanishing_workspace_bytes(int n, int gy, int gx, int grid) {
    if (n <= 0 || gy <= 0 || gx <= 0 || (int64_t)gy * gx > kMaxCells || grid < 2 || grid > kMaxGrid) return -1;
    return (int64_t)n * frame_bytes_of(grid);
}

extern "C" int pwc_vanishing_point(const void *vec, int n, int gy, int gx, int frame_h, int frame_w, int step, double min_mag, int max_points,
                                   int grid, int min_pairs, const void *order, void *out_vp, void *out_info, void *workspace,
                                   int64_t workspace_bytes, void *stream) {
    if (!vec || !out_vp || !out_info || !workspace) PWC_FAIL(PWC_EINVAL, "pwc_vanishing_point: null pointer");
    if (step < 1) PWC_FAIL(PWC_EINVAL, "pwc_vanishing_point: step %d < 1", step);
    if (n <= 0 || n > 65535 || gy <= 0 || gx <= 0 || frame_h <= 0 || frame_w <= 0)
        PWC_FAIL(PWC_EINVAL, "pwc_vanishing_point: bad shape n=%d grid=%dx%d frame=%dx%d (n <= 65535)", n, gy, gx, frame_h, frame_w);
    if ((int64_t)gy * gx > kMaxCells) PWC_FAIL(PWC_EINVAL, "pwc_vanishing_point: %dx%d cells, at most %d", gy, gx, kMaxCells);
    if (gy != (frame_h + step - 1) / step || gx != (frame_w + step - 1) / step)
        PWC_FAIL(PWC_EINVAL, "pwc_vanishing_point: %dx%d cells are not the grid of a %dx%d frame at step %d", gy, gx, frame_h, frame_w, step);
    if (grid < 2 || grid > kMaxGrid) PWC_FAIL(PWC_EINVAL, "pwc_vanishing_point: grid %d outside 2..%d", grid, kMaxGrid);
    if (max_points < 5 || max_points > kMaxPoints) PWC_FAIL(PWC_EINVAL, "pwc_vanishing_point: max_points %d outside 5..%d", max_points, kMaxPoints);
    const int cells = gy * gx;
    if (cells > max_points && !order)
        PWC_FAIL(PWC_EINVAL, "pwc_vanishing_point: %d cells can exceed max_points %d: an order table is needed", cells, max_points);
    const int64_t need = pwc_vanishing_workspace_bytes(n, gy, gx, grid);
    if (workspace_bytes < need)
        PWC_FAIL(PWC_EINVAL, "pwc_vanishing_point: workspace needs %lld bytes, got %lld", (long long)need, (long long)workspace_bytes);
    if (pwc::misaligned({vec, out_vp, workspace}, 8) || pwc::misaligned({order, out_info}))
        PWC_FAIL(PWC_EALIGN, "pwc_vanishing_point: vec, out_vp and workspace must be 8-byte aligned, order and out_info 4-byte aligned");
    Vp p;
    p.vec = static_cast<const float2 *>(vec);
    p.order = static_cast<const int *>(order);
    p.ws = static_cast<char *>(workspace);
    p.frame_bytes = frame_bytes_of(grid);
    p.gy = gy; p.gx = gx; p.cells = cells; p.step = step; p.max_points = max_points; p.grid = grid; p.min_pairs = min_pairs;
    p.min_mag = min_mag;
    p.xlo = -0.5 * (double)frame_w; p.xhi = 1.5 * (double)frame_w; p.xstep = (p.xhi - p.xlo) / (double)grid;
    p.ylo = -0.5 * (double)frame_h; p.yhi = 1.5 * (double)frame_h; p.ystep = (p.yhi - p.ylo) / (double)grid;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(select_kernel, dim3(n), dim3(kThreads), 0, st, p);
    if (grid <= kLdsGrid) hipLaunchKernelGGL(pair_kernel<true>, dim3(kPairGroups, n), dim3(kThreads), 0, st, p);
    else hipLaunchKernelGGL(pair_kernel<false>, dim3(kPairGroups, n), dim3(kThreads), 0, st, p);
    hipLaunchKernelGGL(finish_kernel, dim3(n), dim3(kThreads), 0, st, p, static_cast<double *>(out_vp), static_cast<int *>(out_info));
    return pwc::check_launch("pwc_vanishing_point");
}
