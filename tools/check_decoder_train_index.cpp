// Host-only check of the training-mode decoder's index arithmetic (gdb-nerf_amd/csrc/gdb_decoder_train_index.h).  Build and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o check_decoder_train_index tools/check_decoder_train_index.cpp && ./check_decoder_train_index
// Every packed element of every layer form must name a source element inside its tensor (or padding), every real source element must
// be named exactly once, and every partial a weight-gradient wave writes must lie inside the partial buffer and be written once.
#include <cassert>
#include <cstdio>
#include <vector>
#include "../gdb-nerf_amd/csrc/gdb_decoder_train_index.h"

static size_t conv_floats(int cin, int nt) { return (size_t)((cin + 31) / 32) * 9 * 8 * 64 * 2 * nt; }

static void check_fwd(int cout, int cin, int nt) {
    std::vector<int> hit((size_t)cout * cin * 9, 0);
    const size_t n = conv_floats(cin, nt);
    for (size_t i = 0; i < n; ++i) {
        const long long k = dect_conv16_src((unsigned)i, (cin + 31) / 32, cout, cin);
        assert(k >= -1 && k < (long long)hit.size());
        if (k >= 0) ++hit[(size_t)k];
    }
    for (int h : hit) assert(h == 1);
}
static void check_t(int cout, int cin, int rows, int rs, int c0) {   // source W (rows = cin, rs, 3, 3)
    std::vector<int> hit((size_t)rows * rs * 9, 0);
    const size_t n = conv_floats(cin, cout > 32 ? 2 : 1);
    for (size_t i = 0; i < n; ++i) {
        const long long k = dect_conv16_src_t((unsigned)i, (cin + 31) / 32, cout, cin, rs, c0);
        assert(k >= -1 && k < (long long)hit.size());
        if (k >= 0) ++hit[(size_t)k];
    }
    for (int i = 0; i < rows; ++i)
        for (int c = 0; c < rs; ++c)
            for (int t = 0; t < 9; ++t) assert(hit[((size_t)i * rs + c) * 9 + t] == ((c >= c0 && c < c0 + cout) ? 1 : 0));
}
static void check_dw(int M, int N, int rows) {
    int tg, nslab, rps;
    dect_dw_plan(M, N, rows, &tg, &nslab, &rps);
    assert(nslab >= 1 && nslab <= 256 && (long long)nslab * rps >= rows && (long long)(nslab - 1) * rps < rows);
    const int nmt = (M + 15) / 16, nnt = (N + 15) / 16, nwaves = nmt * nnt * (9 / tg) * nslab;
    std::vector<int> hit((size_t)nslab * M * N * 9, 0);
    std::vector<int> rowhit(rows, 0);
    for (int w = 0; w < nwaves; ++w) {
        int mt, nt, g, slab, r0, r1;
        dect_dw_wave(w, nmt, nnt, 9 / tg, rps, rows, &mt, &nt, &g, &slab, &r0, &r1);
        assert(mt < nmt && nt < nnt && g < 9 / tg && slab < nslab && r0 >= 0 && r0 < r1 && r1 <= rows);
        if (mt == 0 && nt == 0 && g == 0)
            for (int r = r0; r < r1; ++r) ++rowhit[r];
        for (int lane = 0; lane < 64; ++lane)
            for (int q = 0; q < tg; ++q)
                for (int r = 0; r < 4; ++r) {
                    const long long k = dect_dw_part_index(slab, M, N, 16 * mt + 4 * (lane >> 4) + r, 16 * nt + (lane & 15), g * tg + q);
                    assert(k >= -1 && k < (long long)hit.size());
                    if (k >= 0) ++hit[(size_t)k];
                }
    }
    for (int h : hit) assert(h == 1);
    for (int h : rowhit) assert(h == 1);
}

int main() {
    check_fwd(64, 27, 2); check_fwd(32, 64, 1); check_fwd(32, 96, 1); check_fwd(64, 128, 2); check_fwd(12, 64, 1);
    check_t(64, 64, 64, 128, 0); check_t(64, 64, 64, 128, 64); check_t(64, 32, 32, 96, 0); check_t(32, 32, 32, 96, 64);
    check_t(64, 32, 32, 64, 0); check_t(27, 64, 64, 27, 0);
    const int dims[5][2] = {{12, 64}, {64, 128}, {32, 96}, {32, 64}, {64, 27}};
    const int rows[] = {1, 2, 3, 4, 5, 7, 8, 9, 17, 34, 70, 256, 257, 1000, 65536};
    for (const auto& d : dims)
        for (int r : rows) check_dw(d[0], d[1], r);
    printf("decoder-train index arithmetic ok\n");
    return 0;
}
