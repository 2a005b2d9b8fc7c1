// First pyramid level of the fp32 plan: Conv2d(16 -> 16, 3x3, pad 1) + LeakyReLU (conv1aa, conv1b; PWCNet.py:53-54) by Winograd
// F(2x2,3x3) on v_mfma_f32_16x16x4_f32.
//
// Why a kernel of its own: the two Winograd kernels of the library are K-loop pipelines around 32-cout wave pairs.  A 16 -> 16 layer
// has no K loop (K = 16 is four MFMA steps per Winograd position) and its whole transformed filter bank is 16 positions x 16 x 16
// floats = 16 KB, which stays in LDS for the life of the workgroup.  As a direct convolution the layer is MFMA-bound (16.9 GFLOP at
// batch 16, 108 us at peak, 180 us measured); with 16 multiplications per 2x2 outputs instead of 36 it is 7.5 GFLOP next to 235 MB in +
// 235 MB out: 125 us measured, 1.2-1.3x the floor of the memory stream (profiles/r09_pyr1_notes.md: what remains is SIMD time, the
// transforms' VALU work adds to the matrix cycles instead of hiding under them).
//
// Shape of the kernel:
//   * a workgroup (4 waves) owns 8 x 64 output pixels of one image at a time and walks over tiles (persistent: the grid is at most two
//     workgroups per CU, the filter bank is read once).  The 10 x 66 x 16 input patch is staged in LDS with 16-byte loads; the loads of
//     the NEXT tile are issued into registers before the arithmetic of the current one, and two workgroups per CU (61 KB of LDS, 224
//     VGPRs) cover each other's barriers.
//   * a wave owns a strip of 2 rows x 64 pixels = 32 Winograd tiles = two MFMA column blocks.  Lane (t = lane & 15, q = lane >> 4) holds
//     tiles 2t and 2t+1 (four adjacent pixels, so the result leaves in 16-byte stores) and the input channels 4s + q, s = 0..3, which is
//     the B operand of 16x16x4 (k = lane >> 4, column = lane & 15) with no data movement; the A operand is U[pos][cout = lane & 15]
//     [cin = 4s + q], one ds_read_b128 per position.  D has cout = 4q + reg, tile = t.
//   * the 16 positions are walked in four rows of four: a row's four positions need ONE signed sum of two input rows (Bt d), then the
//     column transform; its four accumulators (x 2 blocks) are folded into the 2x2 outputs (At M A, row by row) as soon as the row is
//     done, so 32 accumulator registers are live instead of 128.
//   * the six pixels a lane needs per row are one ds_read_b128 (its own four) and the neighbours' edge pixels by DPP row shifts (a DPP
//     row is 16 lanes = the 16 lanes that share q); only t = 0 / t = 15 take the strip's halo pixel, from one conflict-free ds_read_b32.
#include "pwc_common.h"

namespace pwc {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTH = 8, kTW = 64;                 // output pixels of a workgroup tile
constexpr int kRows = kTH + 2;                   // staged input rows
constexpr int kRS = 72;                          // LDS row stride (floats): pixel x0 - 4 + i at index i, used 3 .. 68
constexpr int kCS = kRows * kRS;                 // 720 = 16 (mod 64): the four channels of a ds_read_b128 fall on disjoint banks
constexpr int kXF = 16 * kCS;                    // floats of the input patch
constexpr int kUF = 16 * 256;                    // floats of the filter bank [pos][lane][s]
constexpr int kBF = 16;                          // bias, behind its filter bank
constexpr int kThreads = 256;
static_assert(kThreads == 16 * (kTW / 4) && 16 * kRows <= kThreads, "loader split: thread = (channel, 16-byte piece of a row)");
static_assert(kCS % 64 == 16 && kRS % 4 == 0, "LDS layout");

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// lane t of a 16-lane row <- lane t-1 (row_shr:1) / t+1 (row_shl:1); the lane without a source keeps `edge`
__device__ __forceinline__ float from_left(float v, float edge) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_right(float v, float edge) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x101, 0xf, 0xf, false));
}

// One strip (2 output rows x 64 pixels, 16 couts) from four staged rows.  src: LDS, element (channel c, row r, pixel p) at
// src[c * cs + r * rs + p] with p = 0 the pixel left of the strip (src + 1 is 16-byte aligned), p = 65 the one right of it.
// Y[row][block]: the lane's couts 4q .. 4q+3 at pixel 4t + 2 * block + {0, 1} -> Y[row][block * 2 + {0, 1}].
__device__ __forceinline__ void wino_strip(const float *src, int rs, int cs, const float *U, int lane, f32x4 (&Y)[2][4]) {
    const int t = lane & 15, q = lane >> 4;
    const float *lp = src + q * cs + 1 + 4 * t;                 // the lane's own four pixels
    const float *hp = src + q * cs + (t == 15 ? 65 : 0);        // halo pixel: t = 0 left, t = 15 right (other lanes: broadcast of the left one)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) Y[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // Bt d, row i: d0 - d2 | d1 + d2 | d2 - d1 | d1 - d3
        const int ra = (i == 0) ? 0 : (i == 2) ? 2 : 1;
        const int rb = (i == 0) ? 2 : (i == 1) ? 2 : (i == 2) ? 1 : 3;
        f32x4 u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = *reinterpret_cast<const f32x4 *>(U + (i * 4 + j) * 256 + lane * 4);
        f32x4 acc[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(lp + 4 * s * cs + ra * rs);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(lp + 4 * s * cs + rb * rs);
            const float ha = hp[4 * s * cs + ra * rs], hb = hp[4 * s * cs + rb * rs];
            float r1, r2, r3, r4, h;
            if (i == 1) { r1 = a.x + b.x; r2 = a.y + b.y; r3 = a.z + b.z; r4 = a.w + b.w; h = ha + hb; }
            else        { r1 = a.x - b.x; r2 = a.y - b.y; r3 = a.z - b.z; r4 = a.w - b.w; h = ha - hb; }
            const float r0 = from_left(r4, h), r5 = from_right(r1, h);
            const float us[4] = {u[0][s], u[1][s], u[2][s], u[3][s]};
            // (Bt d) B, tiles 2t (pixels r0..r3) and 2t+1 (r2..r5)
            acc[0][0] = mfma4(us[0], r0 - r2, acc[0][0]);
            acc[0][1] = mfma4(us[0], r2 - r4, acc[0][1]);
            acc[1][0] = mfma4(us[1], r1 + r2, acc[1][0]);
            acc[1][1] = mfma4(us[1], r3 + r4, acc[1][1]);
            acc[2][0] = mfma4(us[2], r2 - r1, acc[2][0]);
            acc[2][1] = mfma4(us[2], r4 - r3, acc[2][1]);
            acc[3][0] = mfma4(us[3], r1 - r3, acc[3][0]);
            acc[3][1] = mfma4(us[3], r3 - r5, acc[3][1]);
        }
        // At M A: columns first (m0 + m1 + m2 | m1 - m2 - m3), then this row's share of the two output rows (1 1 1 0 | 0 1 -1 -1)
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const f32x4 c0 = acc[0][blk] + acc[1][blk] + acc[2][blk];
            const f32x4 c1 = acc[1][blk] - acc[2][blk] - acc[3][blk];
            if (i < 3) { Y[0][2 * blk] += c0; Y[0][2 * blk + 1] += c1; }
            if (i == 1) { Y[1][2 * blk] += c0; Y[1][2 * blk + 1] += c1; }
            if (i >= 2) { Y[1][2 * blk] -= c0; Y[1][2 * blk + 1] -= c1; }
        }
        __builtin_amdgcn_sched_barrier(0);                      // keep the next row's LDS reads out of this one: 32 live accumulators, not 128
    }
}

struct Tile { int img, y0, x0; };
template <int TH = kTH, int TW = kTW> __device__ __forceinline__ Tile tile_of(int id, int tiles_x, int tiles_y) {
    Tile t;
    t.img = id / (tiles_x * tiles_y);
    const int r = id - t.img * tiles_x * tiles_y;
    t.y0 = (r / tiles_x) * TH;
    t.x0 = (r - (r / tiles_x) * tiles_x) * TW;
    return t;
}

// The loads of one tile, held in registers until the LDS patch is free.  Thread (ch = tid >> 4, c4 = tid & 15) takes the 16-byte piece
// c4 of every row of channel ch, so that a load's address is one per-thread offset plus a wave-uniform row pointer, and threads
// 0 .. 159 take the two halo pixels of (channel tid / kRows, row tid % kRows).  Addresses are clamped into the image so that every load
// is unconditional; what lies outside is stored as zero (the convolution's padding) when the registers go to LDS.
struct Patch { f32x4 v[kRows]; float h[2]; int y0; bool col_ok, hl_ok, hr_ok; };

__device__ __forceinline__ void load_patch(Patch &p, const float *x, const Tile tl, int H, int W, int64_t bs, int tid) {
    const float *xi = x + (int64_t)tl.img * bs;
    const int ch = tid >> 4, gx = tl.x0 + 4 * (tid & 15);
    p.y0 = tl.y0;
    p.col_ok = gx < W;                                                   // W % 4 == 0: a 16-byte piece is inside or outside as a whole
    const unsigned off = (unsigned)(ch * H * W + min(gx, W - 4));
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const float *rowp = xi + min(max(tl.y0 - 1 + k, 0), H - 1) * W;  // wave-uniform
        p.v[k] = *reinterpret_cast<const f32x4 *>(rowp + off);
    }
    const int hid = min(tid, 16 * kRows - 1), hch = hid / kRows, hrow = hid - hch * kRows;
    const int gy = tl.y0 - 1 + hrow, xl = tl.x0 - 1, xr = tl.x0 + kTW;
    const bool row_ok = tid < 16 * kRows && gy >= 0 && gy < H;
    p.hl_ok = row_ok && xl >= 0;
    p.hr_ok = row_ok && xr < W;
    const float *hp = xi + (hch * H + min(max(gy, 0), H - 1)) * W;
    p.h[0] = hp[max(xl, 0)];
    p.h[1] = hp[min(xr, W - 1)];
}

__device__ __forceinline__ void store_patch(const Patch &p, float *X, int H, int tid) {
    float *dst = X + (tid >> 4) * kCS + 4 + 4 * (tid & 15);
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int gy = p.y0 - 1 + k;
        const bool ok = p.col_ok && gy >= 0 && gy < H;
        *reinterpret_cast<f32x4 *>(dst + k * kRS) = ok ? p.v[k] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (tid < 16 * kRows) {
        float *hd = X + (tid / kRows) * kCS + (tid % kRows) * kRS;
        hd[3] = p.hl_ok ? p.h[0] : 0.f;
        hd[4 + kTW] = p.hr_ok ? p.h[1] : 0.f;
    }
}

__global__ __launch_bounds__(kThreads, 2) void pyr1_wino2_kernel(const float *__restrict__ x, const float *__restrict__ up,
                                                                 const float *__restrict__ bias, float *__restrict__ y, int H, int W,
                                                                 int tiles_x, int tiles_y, int ntiles, int64_t bsx, int64_t bsy, float slope) {
    __shared__ __attribute__((aligned(16))) float lds[kXF + kUF + kBF];
    float *X = lds, *U = lds + kXF;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = lane & 15, q = lane >> 4;
    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    Patch p;
    load_patch(p, x, tile_of(tile, tiles_x, tiles_y), H, W, bsx, tid);
#pragma unroll
    for (int k = 0; k < kUF / 4 / kThreads; ++k)
        reinterpret_cast<f32x4 *>(U)[tid + kThreads * k] = reinterpret_cast<const f32x4 *>(up)[tid + kThreads * k];
    // the bias goes through LDS too: a register loaded from memory here and first used inside the loop would put its s_waitcnt there,
    // where it also waits for the NEXT tile's loads (the counter retires in order)
    if (tid < kBF) U[kUF + tid] = bias[tid];
    for (; tile < ntiles; tile += gridDim.x) {
        const Tile tl = tile_of(tile, tiles_x, tiles_y);
        store_patch(p, X, H, tid);
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) load_patch(p, x, tile_of(tile + gridDim.x, tiles_x, tiles_y), H, W, bsx, tid);
        const int gy = tl.y0 + 2 * wave, gx = tl.x0 + 4 * t;
        if (gy < H) {                                                     // wave-uniform
            f32x4 Y[2][4];
            wino_strip(X + 2 * wave * kRS + 3, kRS, kCS, U, lane, Y);
            if (gx < W) {
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(U + kUF + 4 * q);
                float *yo = y + (int64_t)tl.img * bsy + ((int64_t)(4 * q) * H + gy) * W + gx;
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (gy + r < H) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            f32x4 o;
#pragma unroll
                            for (int c = 0; c < 4; ++c) o[c] = leaky(Y[r][c][j] + bv[j], slope);
                            *reinterpret_cast<f32x4 *>(yo + ((int64_t)j * H + r) * W) = o;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---- conv1aa and conv1b in one launch ---------------------------------------------------------------------------------------------
// The same strip arithmetic twice per workgroup: conv1aa on the output tile plus a one-pixel ring, kept in LDS, then conv1b from
// LDS; the 16-channel map between the two layers is neither written nor read.  One workgroup of 8 waves per CU (113 KB of LDS):
//   * output tile 14 rows x 60 columns.  conv1aa is evaluated on 16 rows x 64 columns (8 strips = one per wave) from an 18 x 68
//     input patch; conv1b on 14 x 64 (7 strips), of which the last four columns are not stored.  Recomputed halo: conv1aa runs
//     16 * 64 / (14 * 60) = 1.22x the pixels of the tile, conv1b 1.07x.
//   * every wave holds its conv1aa strip in registers across a barrier and then stores it OVER the input patch (which is dead by
//     then), so the patch and the intermediate map share their LDS.  Ring pixels outside the image are stored as ZERO: conv1b pads
//     conv1aa's output, it does not see conv1aa evaluated outside the map.
//   * columns: the conv1aa strip starts at x0 - 2, which is 8-byte but not 16-byte aligned in memory, so the staged pieces go to LDS as
//     two ds_write_b64 each, at the offset that gives every lane its own four pixels 16-byte aligned -- in both passes (pixel p of the
//     patch at index p - x0 + 6, pixel p of the intermediate map at p - x0 + 4).
constexpr int kFTH = 14, kFTW = 60;
constexpr int kFRows = kFTH + 4;                 // staged input rows; the intermediate map has kFTH + 2
constexpr int kFCS = kFRows * kRS;               // 1296 = 16 (mod 64)
constexpr int kFXF = 16 * kFCS;
constexpr int kFThreads = 512;
constexpr int kFLd = kFRows / 2;                 // 16-byte loads per thread and tile, + 1 for the 17th piece of a row
constexpr int kFSmem = (kFXF + 2 * (kUF + kBF)) * 4;
static_assert(kFCS % 64 == 16 && kFRows % 2 == 0 && 16 * kFRows <= kFThreads && (kFTH + 2) / 2 == kFThreads / 64, "fused geometry");

// thread (half = tid >> 8, ch = (tid >> 4) & 15, c = tid & 15): piece c (pixels x0 - 4 + 4c ..) of rows 9 half .. 9 half + 8 of channel ch;
// threads 0 .. 287: the 17th piece (x0 + 60 ..) of (channel tid / 18, row tid % 18)
struct PatchF { f32x4 v[kFLd]; f32x4 e; int y0; bool col_ok, e_ok; };

__device__ __forceinline__ void load_patch_f(PatchF &p, const float *x, const Tile tl, int H, int W, int64_t bs, int tid) {
    const float *xi = x + (int64_t)tl.img * bs;
    const int half = __builtin_amdgcn_readfirstlane(tid >> 8), ch = (tid >> 4) & 15, gx = tl.x0 - 4 + 4 * (tid & 15);
    p.y0 = tl.y0;
    p.col_ok = gx >= 0 && gx < W;
    const unsigned off = (unsigned)(ch * H * W + min(max(gx, 0), W - 4));
#pragma unroll
    for (int k = 0; k < kFLd; ++k) {
        const float *rowp = xi + min(max(tl.y0 - 2 + kFLd * half + k, 0), H - 1) * W;      // wave-uniform
        p.v[k] = *reinterpret_cast<const f32x4 *>(rowp + off);
    }
    const int eid = min(tid, 16 * kFRows - 1), ech = eid / kFRows, erow = eid - ech * kFRows;
    const int gy = tl.y0 - 2 + erow, ex = tl.x0 + 60;
    p.e_ok = tid < 16 * kFRows && gy >= 0 && gy < H && ex < W;
    p.e = *reinterpret_cast<const f32x4 *>(xi + (ech * H + min(max(gy, 0), H - 1)) * W + min(ex, W - 4));
}

__device__ __forceinline__ void st_lds4(float *dst, f32x4 v) {          // 8-byte aligned
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    reinterpret_cast<f32x2 *>(dst)[0] = f32x2{v.x, v.y};
    reinterpret_cast<f32x2 *>(dst)[1] = f32x2{v.z, v.w};
}

__device__ __forceinline__ void store_patch_f(const PatchF &p, float *X, int H, int tid) {
    const int half = __builtin_amdgcn_readfirstlane(tid >> 8);
    float *dst = X + ((tid >> 4) & 15) * kFCS + kFLd * half * kRS + 2 + 4 * (tid & 15);
#pragma unroll
    for (int k = 0; k < kFLd; ++k) {
        const int gy = p.y0 - 2 + kFLd * half + k;
        const bool ok = p.col_ok && gy >= 0 && gy < H;
        st_lds4(dst + k * kRS, ok ? p.v[k] : f32x4{0.f, 0.f, 0.f, 0.f});
    }
    if (tid < 16 * kFRows) st_lds4(X + (tid / kFRows) * kFCS + (tid % kFRows) * kRS + 66, p.e_ok ? p.e : f32x4{0.f, 0.f, 0.f, 0.f});
}

__global__ __launch_bounds__(kFThreads, 2) void pyr1_wino2_pair_kernel(const float *__restrict__ x, const float *__restrict__ up1,
                                                                      const float *__restrict__ bias1, const float *__restrict__ up2,
                                                                      const float *__restrict__ bias2, float *__restrict__ y, int H, int W,
                                                                      int tiles_x, int tiles_y, int ntiles, int64_t bsx, int64_t bsy, float slope) {
    extern __shared__ __attribute__((aligned(16))) float lds_f[];
    float *X = lds_f, *U1 = lds_f + kFXF, *U2 = U1 + kUF + kBF;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = lane & 15, q = lane >> 4;
    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    PatchF p;
    load_patch_f(p, x, tile_of<kFTH, kFTW>(tile, tiles_x, tiles_y), H, W, bsx, tid);
#pragma unroll
    for (int k = 0; k < kUF / 4 / kFThreads; ++k) {
        reinterpret_cast<f32x4 *>(U1)[tid + kFThreads * k] = reinterpret_cast<const f32x4 *>(up1)[tid + kFThreads * k];
        reinterpret_cast<f32x4 *>(U2)[tid + kFThreads * k] = reinterpret_cast<const f32x4 *>(up2)[tid + kFThreads * k];
    }
    if (tid < kBF) { U1[kUF + tid] = bias1[tid]; U2[kUF + tid] = bias2[tid]; }      // through LDS: see pyr1_wino2_kernel
    for (; tile < ntiles; tile += gridDim.x) {
        const Tile tl = tile_of<kFTH, kFTW>(tile, tiles_x, tiles_y);
        store_patch_f(p, X, H, tid);
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) load_patch_f(p, x, tile_of<kFTH, kFTW>(tile + gridDim.x, tiles_x, tiles_y), H, W, bsx, tid);
        f32x4 Y[2][4];
        // conv1aa: strip `wave` = rows y0 - 1 + 2 wave, + 1 of the intermediate map, columns x0 - 2 .. x0 + 61
        wino_strip(X + 2 * wave * kRS + 3, kRS, kFCS, U1, lane, Y);
        __syncthreads();                                                  // every wave has read its input rows: the patch is dead
        const f32x4 b1 = *reinterpret_cast<const f32x4 *>(U1 + kUF + 4 * q);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int gy = tl.y0 - 1 + 2 * wave + r;
            const bool row_ok = gy >= 0 && gy < H;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 o;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int gx = tl.x0 - 2 + 4 * t + c;
                    o[c] = (row_ok && gx >= 0 && gx < W) ? leaky(Y[r][c][j] + b1[j], slope) : 0.f;      // outside the map: conv1b's padding
                }
                st_lds4(X + (4 * q + j) * kFCS + (2 * wave + r) * kRS + 2 + 4 * t, o);
            }
        }
        __syncthreads();
        // conv1b: strip `wave` < 7 = output rows y0 + 2 wave, + 1, columns x0 .. x0 + 63 (60 stored)
        const int gy = tl.y0 + 2 * wave, gx = tl.x0 + 4 * t;
        if (wave < kFTH / 2 && gy < H) {
            wino_strip(X + 2 * wave * kRS + 3, kRS, kFCS, U2, lane, Y);
            if (t < kFTW / 4 && gx < W) {
                const f32x4 b2 = *reinterpret_cast<const f32x4 *>(U2 + kUF + 4 * q);
                float *yo = y + (int64_t)tl.img * bsy + ((int64_t)(4 * q) * H + gy) * W + gx;
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (gy + r < H) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            f32x4 o;
#pragma unroll
                            for (int c = 0; c < 4; ++c) o[c] = leaky(Y[r][c][j] + b2[j], slope);
                            *reinterpret_cast<f32x4 *>(yo + ((int64_t)j * H + r) * W) = o;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// G g Gt (F(2x2,3x3): G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]) in the kernel's LDS order [pos][q * 16 + cout][s], cin = 4s + q
__global__ void pyr1_wino2_pack_kernel(const float *__restrict__ w, float *__restrict__ up) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;               // pos * 256 + cout * 16 + cin
    if (id >= kUF) return;
    const int pos = id >> 8, cout = (id >> 4) & 15, cin = id & 15, i = pos >> 2, j = pos & 3;
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    double acc = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) acc += G[i][a] * (double)w[(cout * 16 + cin) * 9 + a * 3 + b] * G[j][b];
    up[pos * 256 + ((cin & 3) * 16 + cout) * 4 + (cin >> 2)] = (float)acc;
}

int cu_count() {
    static std::atomic<int> cus[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (!n) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

}  // namespace
}  // namespace pwc

using namespace pwc;

extern "C" int64_t pwc_pyr1_wino_packed_bytes(void) { return (int64_t)kUF * 4; }

extern "C" int pwc_pyr1_wino_preferred(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (W % 4) || option(OPT_PYR1_WINO) <= 0) return 0;
    const int64_t tiles = (int64_t)B * ((H + kTH - 1) / kTH) * ((W + kTW - 1) / kTW);
    if (tiles < option(OPT_PYR1_WINO_MIN_TILES)) return 0;
    return option(OPT_PYR1_WINO) >= 2 ? 2 : 1;
}

extern "C" int pwc_pyr1_wino_pack(const void *w, void *up, void *stream) {
    if (!w || !up) PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_pack: null pointer");
    if (!aligned16(up)) PWC_FAIL(PWC_EALIGN, "pwc_pyr1_wino_pack: packed filters must be 16-byte aligned");
    hipLaunchKernelGGL(pyr1_wino2_pack_kernel, dim3(kUF / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(w), static_cast<float *>(up));
    return check_launch("pyr1_wino2_pack_kernel");
}

extern "C" int pwc_pyr1_wino_fwd(const void *x, const void *up, const void *bias, void *y, int B, int H, int W, float leaky_slope,
                                 int64_t x_bstride, int64_t y_bstride, void *stream) {
    if (!x || !up || !bias || !y) PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_fwd: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || (int64_t)16 * H * W > 0x7fffffffLL) PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_fwd: bad shape");
    if (W % 4) PWC_FAIL(PWC_EUNSUPPORTED, "pwc_pyr1_wino_fwd: W must be a multiple of 4 (got %d)", W);
    if (x_bstride < (int64_t)16 * H * W || y_bstride < (int64_t)16 * H * W)
        PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_fwd: batch stride smaller than the tensor");
    if (!aligned16(x) || !aligned16(y) || !aligned16(up) || (x_bstride % 4) || (y_bstride % 4))
        PWC_FAIL(PWC_EALIGN, "pwc_pyr1_wino_fwd: x, y and the packed filters must be 16-byte aligned, batch strides multiples of 4");
    if (!(leaky_slope >= 0.f && leaky_slope <= 1.f)) PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_fwd: leaky_slope must be in [0, 1]");
    const int tiles_x = (W + kTW - 1) / kTW, tiles_y = (H + kTH - 1) / kTH;
    const int64_t ntiles = (int64_t)B * tiles_x * tiles_y;
    if (ntiles > 0x3fffffffLL) PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_fwd: too many tiles");
    const int64_t grid = ntiles < 2LL * cu_count() ? ntiles : 2LL * cu_count();
    note_kernel("pyr1_wino2", kTH, kTW, 0, 0, 0, 0);
    hipLaunchKernelGGL(pyr1_wino2_kernel, dim3((unsigned)grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(x), static_cast<const float *>(up), static_cast<const float *>(bias),
                       static_cast<float *>(y), H, W, tiles_x, tiles_y, (int)ntiles, x_bstride, y_bstride, leaky_slope);
    return check_launch("pyr1_wino2_kernel");
}

extern "C" int pwc_pyr1_wino_pair_fwd(const void *x, const void *up1, const void *bias1, const void *up2, const void *bias2, void *y,
                                      int B, int H, int W, float leaky_slope, int64_t x_bstride, int64_t y_bstride, void *stream) {
    if (!x || !up1 || !bias1 || !up2 || !bias2 || !y) PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_pair_fwd: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || (int64_t)16 * H * W > 0x7fffffffLL) PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_pair_fwd: bad shape");
    if (W % 4) PWC_FAIL(PWC_EUNSUPPORTED, "pwc_pyr1_wino_pair_fwd: W must be a multiple of 4 (got %d)", W);
    if (x_bstride < (int64_t)16 * H * W || y_bstride < (int64_t)16 * H * W)
        PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_pair_fwd: batch stride smaller than the tensor");
    if (!aligned16(x) || !aligned16(y) || !aligned16(up1) || !aligned16(up2) || (x_bstride % 4) || (y_bstride % 4))
        PWC_FAIL(PWC_EALIGN, "pwc_pyr1_wino_pair_fwd: x, y and the packed filters must be 16-byte aligned, batch strides multiples of 4");
    if (!(leaky_slope >= 0.f && leaky_slope <= 1.f)) PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_pair_fwd: leaky_slope must be in [0, 1]");
    if (x == y) PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_pair_fwd: in-place operation is not possible (tiles read their neighbours' input)");
    const int tiles_x = (W + kFTW - 1) / kFTW, tiles_y = (H + kFTH - 1) / kFTH;
    const int64_t ntiles = (int64_t)B * tiles_x * tiles_y;
    if (ntiles > 0x3fffffffLL) PWC_FAIL(PWC_EINVAL, "pwc_pyr1_wino_pair_fwd: too many tiles");
    static LdsAttrOnce attr;
    if (const int rc = ensure_lds_attr(attr, reinterpret_cast<const void *>(pyr1_wino2_pair_kernel), kFSmem, "pwc_pyr1_wino_pair_fwd")) return rc;
    const int64_t grid = ntiles < cu_count() ? ntiles : cu_count();
    note_kernel("pyr1_wino2_pair", kFTH, kFTW, 0, 0, 0, 0);
    hipLaunchKernelGGL(pyr1_wino2_pair_kernel, dim3((unsigned)grid), dim3(kFThreads), kFSmem, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(x), static_cast<const float *>(up1), static_cast<const float *>(bias1),
                       static_cast<const float *>(up2), static_cast<const float *>(bias2), static_cast<float *>(y), H, W, tiles_x, tiles_y,
                       (int)ntiles, x_bstride, y_bstride, leaky_slope);
    return check_launch("pyr1_wino2_pair_kernel");
}
