// Census of the fp32 direct 3x3 kernel's cost model (choose_tile of csrc/pwc_conv_mfma.h) on the host: which tile of each
// (stride, dilation) unit's table is picked where.  No GPU, no library:
//     hipcc --cuda-host-only -O2 -std=c++17 -Iopticalflow_amd/csrc -Iinclude tools/conv_tile_census.hip -o conv_tile_census
//
//   (default)  the box of DESIGN.md 4c, exhaustively: B 1..32, Cin up to 1001, Cout up to 384, input maps up to 256 x 512.  The model
//              sees a shape only as (chunks8 = ceil(Cin / 8), tiles32 = CoutP / 32, B * tiles_x, Ho), so the walk is over chunks8 1..126,
//              tiles32 1..12, every product B (1..32) x tiles_x (1..16 / stride) and Ho 1..256 / stride, in that nesting and ascending.
//              Per unit: the number of classes and an order-dependent 64-bit hash of all choices.  Per tile: the number of classes that
//              pick it and the cheapest shape that does, as a row of launch_audit.TILE_CASES.  Cheapest = fewest multiply-adds of the
//              float64 reference of the first and the last image; Cin is ragged against the 4- and 8-channel chunks, Cout against 32,
//              W against the 32-column tile and, wherever some picking class allows it, Ho against the tile's 4 NT rows with H above the
//              dilation, so that taps of all three rows reach the image (a tile picked only at lower maps or only at whole tiles is
//              marked; where dropping one of the two wishes gives a cheaper class, that one is printed too).
//   --list     the tables, as the labels pwc_last_conv_kernel reports.
//   --wide     a sampled walk far outside the box (Cin up to 2400, Cout up to 1024, B * tiles_x up to 16384, Ho up to 2048 / stride,
//              4 M classes per unit from a fixed seed): picks per tile and the shortest Cin at which each was picked.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pwc_conv_mfma.h"

using pwc_conv::TileChoice;

namespace {

template <int S, int D>
std::vector<TileChoice> table() {
    return std::vector<TileChoice>(std::begin(pwc_conv::Tiles<S, D>::list), std::end(pwc_conv::Tiles<S, D>::list));
}
template <int S, int D>
TileChoice pick(int B, int Cin, int Ho, int Wo, int CoutP) { return pwc_conv::choose_tile<S, D>(B, Cin, Ho, Wo, CoutP, -1); }

struct Shape {
    bool any = false;
    double macs = 0, elems = 0;
    int B = 0, Cin = 0, Cout = 0, H = 0, W = 0;
};

struct Stat {
    long long picks = 0;
    int min_chunks8 = 0;
    Shape full, ragged, any;    // cheapest class with Ho % (4 NT) != 0 and H > D / with Ho % (4 NT) != 0 / of all
};

// the shape a test would run for the class (chunks8, tiles32, B * tiles_x = prod, Ho): ragged in Cin, Cout and W, the factorisation
// of prod with the cheapest reference.  Widths stay multiples of four (16-byte staging, as the plans' maps) and above 16 columns, and
// Cout above 16, so that the launch reaches this kernel family and not the folded tile or the 16-cout kernel.
struct Split { int B, Wo; };
Split split_of(int prod, int max_tx) {
    Split best{0, 0};
    double best_macs = 0, best_elems = 0;
    for (int tx = 1; tx <= max_tx; ++tx) {
        if (prod % tx || prod / tx > 32) continue;
        const int B = prod / tx, Wo = tx == 1 ? 20 : 32 * (tx - 1) + 4;
        const double macs = (B > 1 ? 2.0 : 1.0) * Wo, elems = (double)B * Wo;
        if (!best.B || macs < best_macs || (macs == best_macs && elems < best_elems)) {
            best = {B, Wo};
            best_macs = macs; best_elems = elems;
        }
    }
    return best;
}
Shape shape_of(int S, int chunks8, int tiles32, Split sp, int Ho) {
    Shape s;
    s.any = true;
    s.B = sp.B;
    s.Cin = 8 * (chunks8 - 1) + 5;
    s.Cout = tiles32 == 1 ? 20 : 32 * (tiles32 - 1) + 4;
    s.H = S == 1 ? Ho : 2 * Ho - 1;
    s.W = S * sp.Wo;
    s.macs = (sp.B > 1 ? 2.0 : 1.0) * s.Cin * 9.0 * s.Cout * Ho * sp.Wo;
    s.elems = (double)s.B * s.Cin * s.H * s.W;
    return s;
}

void keep_cheaper(Shape &best, const Shape &s) {
    if (!best.any || s.macs < best.macs || (s.macs == best.macs && s.elems < best.elems)) best = s;
}

int index_of(const std::vector<TileChoice> &t, TileChoice c) {
    for (size_t i = 0; i < t.size(); ++i)
        if (t[i].mt == c.mt && t[i].nt == c.nt && t[i].two == c.two) return (int)i;
    return -1;
}

void print_label(int S, int D, TileChoice t) { printf("conv3x3_mfma_kernel<%d, %d, %d, %d, %d, 0>", t.mt, t.nt, S, D, t.two); }

void print_shape(const char *what, int S, int D, TileChoice t, const Shape &s) {
    printf("      %s %.3g MACs: (%d, %d, %d, %d, %d, %d, %d, \"", what, s.macs, s.B, s.Cin, s.Cout, s.H, s.W, S, D);
    print_label(S, D, t);
    printf("\"),\n");
}

template <int S, int D>
int box() {
    const std::vector<TileChoice> tiles = table<S, D>();
    std::vector<Stat> stat(tiles.size());
    const int max_tx = 16 / S, max_ho = 256 / S;
    std::vector<int> prods;
    for (int b = 1; b <= 32; ++b)
        for (int tx = 1; tx <= max_tx; ++tx) prods.push_back(b * tx);
    std::sort(prods.begin(), prods.end());
    prods.erase(std::unique(prods.begin(), prods.end()), prods.end());
    std::vector<Split> splits;
    for (int prod : prods) splits.push_back(split_of(prod, max_tx));
    uint64_t hash = 0xcbf29ce484222325ull;
    long long classes = 0;
    for (int chunks8 = 1; chunks8 <= 126; ++chunks8)
        for (int tiles32 = 1; tiles32 <= 12; ++tiles32)
            for (size_t p = 0; p < prods.size(); ++p)
                for (int Ho = 1; Ho <= max_ho; ++Ho) {
                    const int prod = prods[p];
                    const TileChoice c = pick<S, D>(prod, 8 * chunks8, Ho, 32, 32 * tiles32);
                    hash = (hash ^ (uint64_t)(c.mt * 16 + c.nt * 2 + c.two)) * 0x100000001b3ull;
                    ++classes;
                    const int i = index_of(tiles, c);
                    if (i < 0) {
                        fprintf(stderr, "s%dd%d: choice <%d, %d, %d> is not in the table\n", S, D, c.mt, c.nt, c.two);
                        return 1;
                    }
                    Stat &st = stat[i];
                    ++st.picks;
                    const Shape s = shape_of(S, chunks8, tiles32, splits[p], Ho);
                    const bool ragged_h = Ho % (4 * c.nt) != 0;
                    keep_cheaper(st.any, s);
                    if (ragged_h) keep_cheaper(st.ragged, s);
                    if (ragged_h && s.H > D) keep_cheaper(st.full, s);
                }
    printf("unit s%dd%d: %zu tiles, %lld classes, hash %016llx\n", S, D, tiles.size(), classes, (unsigned long long)hash);
    for (size_t i = 0; i < tiles.size(); ++i) {
        printf("  <%d, %d, %d, %d, %d> picks %lld\n", tiles[i].mt, tiles[i].nt, S, D, tiles[i].two, stat[i].picks);
        if (!stat[i].picks) continue;
        const Stat &st = stat[i];
        const Shape &first = st.full.any ? st.full : st.ragged.any ? st.ragged : st.any;
        print_shape(st.full.any ? "cheapest" : st.ragged.any ? "cheapest (H <= dilation)" : "cheapest (H whole tiles)", S, D, tiles[i], first);
        if (st.ragged.any && st.ragged.macs < first.macs) print_shape("cheaper with H <= dilation", S, D, tiles[i], st.ragged);
        if (st.any.macs < first.macs && st.any.macs < st.ragged.macs) print_shape("cheaper with H whole tiles", S, D, tiles[i], st.any);
    }
    return 0;
}

uint64_t next(uint64_t &s) {        // xorshift64*
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return s * 0x2545f4914f6cdd1dull;
}
// 1..hi, every octave equally likely
int log_uniform(uint64_t &s, int hi) {
    int bits = 0;
    while ((1 << bits) <= hi) ++bits;
    for (;;) {
        const int top = 1 + (int)(next(s) % bits);                          // magnitude: below 2^top
        const int v = (int)(next(s) % (1u << top)) | (1 << (top - 1));      // top bit set
        if (v <= hi) return v;
    }
}

template <int S, int D>
int wide() {
    const std::vector<TileChoice> tiles = table<S, D>();
    std::vector<Stat> stat(tiles.size());
    uint64_t seed = 0x9e3779b97f4a7c15ull, hash = 0xcbf29ce484222325ull;
    const int n = 4 << 20;
    for (int k = 0; k < n; ++k) {
        const int chunks8 = 1 + (int)(next(seed) % 300), tiles32 = 1 + (int)(next(seed) % 32);
        const int prod = log_uniform(seed, 16384), Ho = log_uniform(seed, 2048 / S);
        const TileChoice c = pick<S, D>(prod, 8 * chunks8, Ho, 32, 32 * tiles32);
        hash = (hash ^ (uint64_t)(c.mt * 16 + c.nt * 2 + c.two)) * 0x100000001b3ull;
        const int i = index_of(tiles, c);
        if (i < 0) {
            fprintf(stderr, "s%dd%d: choice <%d, %d, %d> is not in the table\n", S, D, c.mt, c.nt, c.two);
            return 1;
        }
        ++stat[i].picks;
        if (!stat[i].min_chunks8 || chunks8 < stat[i].min_chunks8) stat[i].min_chunks8 = chunks8;
    }
    printf("unit s%dd%d wide: %d sampled classes, hash %016llx\n", S, D, n, (unsigned long long)hash);
    for (size_t i = 0; i < tiles.size(); ++i) {
        printf("  <%d, %d, %d, %d, %d> picks %lld", tiles[i].mt, tiles[i].nt, S, D, tiles[i].two, stat[i].picks);
        if (stat[i].picks) printf(", Cin from %d", 8 * (stat[i].min_chunks8 - 1) + 1);
        printf("\n");
    }
    return 0;
}

template <int S, int D>
int list() {
    for (const TileChoice &t : table<S, D>()) {
        print_label(S, D, t);
        printf("\n");
    }
    return 0;
}

}  // namespace

#define EACH_UNIT(fn) (fn<1, 1>() || fn<1, 2>() || fn<1, 4>() || fn<1, 8>() || fn<1, 16>() || fn<2, 1>())

int main(int argc, char **argv) {
    if (argc == 1) return EACH_UNIT(box);
    if (argc == 2 && !strcmp(argv[1], "--list")) return EACH_UNIT(list);
    if (argc == 2 && !strcmp(argv[1], "--wide")) return EACH_UNIT(wide);
    fprintf(stderr, "usage: %s [--list | --wide]\n", argv[0]);
    return 2;
}
