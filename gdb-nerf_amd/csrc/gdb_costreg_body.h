// The cost-regularisation U-Nets' layer plan, weight order, launch geometry and implicit-GEMM convolution body, shared by the eval-mode
// forward (gdb_costreg.hip) and the train-mode forward and backward (gdb_costreg_train.hip).  Each file wraps costreg_conv_body in a
// __global__ of its own, as gdb_costvol_body.h does for the plane sweep.
#pragma once
#include "gdb_internal.h"
#include <cmath>
#include <cstring>

typedef float F2 __attribute__((ext_vector_type(2)));
typedef float F4 __attribute__((ext_vector_type(4)));

enum { CR_S1 = 0, CR_S2 = 1, CR_UP = 2 };     // stride-1 conv, stride-2 conv, stride-2 transposed conv
enum { CR_BN = 0, CR_HEADS = 1, CR_RAW = 2 };  // epilogues: eval BN + ReLU, the two heads, the raw sums (train mode: z, or a gradient)

// ---- layer plan (packing, workspace and launches share it) ---------------------------------------------------------------
#define CR_MAX_LAYERS 11   // conv0 .. conv9 + the heads at depth 3
struct CrLayer {
    int mode, cin, cout, level_in, level_out;  // level l: resolution (D, H, W) >> l
    int nc;        // the input is the (B, C, D, H, W) cost volume (conv0)
    int zs;        // output planes per wave: 2 for an 8-channel stride-1 layer (rows = 2 planes x 8 channels), else 1
    int taps;      // 27, or 36 (4 input planes x 9) when zs == 2
    int e;         // floats per lane per k-chunk: 4 (16 channels per chunk) or 2 (8)
    int nchunk;    // k-chunks of the input channels
    int rows;      // GEMM rows: cout, zs * cout, or voxel_dim + 1 for the heads
    int nmt;       // 16-row tiles
    size_t w_off, ep_off;   // packed floats: weights, then [invstd | mean | weight | bias] x cout (BN layers)
};
struct CrPlan {
    int depth, cin, c, cout, nlayers;   // nlayers counts the heads (last)
    CrLayer L[CR_MAX_LAYERS];
    size_t total;
};

static void cr_layer_set(CrLayer& l, int mode, int ci, int co, int lin, int lout, int nc) {
    l.mode = mode; l.cin = ci; l.cout = co; l.level_in = lin; l.level_out = lout;
    l.nc = nc;
    l.zs = (mode == CR_S1 && co == 8) ? 2 : 1;
    l.taps = l.zs == 2 ? 36 : 27;
    l.e = (l.nc || ci % 16 == 0) ? 4 : 2;
    l.nchunk = l.nc ? (ci + 15) / 16 : ci / (4 * l.e);
    l.rows = l.zs * co;
    l.nmt = (l.rows + 15) / 16;
}

static int cr_plan(int depth, int cin, int c, int cout, CrPlan* P) {
    if (depth != 2 && depth != 3) return gdb_fail(GDB_E_BADARG, "cost reg: depth %d (2 or 3 are supported)", depth);
    if (cin < 8 || cin > 256 || cin % 8) return gdb_fail(GDB_E_BADARG, "cost reg: in_channels %d (a multiple of 8, at most 256)", cin);
    if (c < 8 || (c << depth) > 128 || c % 8)
        return gdb_fail(GDB_E_BADARG, "cost reg: base_channels %d (a multiple of 8 with base << depth <= 128)", c);
    if (cout < 1 || cout > 15) return gdb_fail(GDB_E_BADARG, "cost reg: out_channels %d (1 .. 15: both heads share one 16-row tile)", cout);
    P->depth = depth; P->cin = cin; P->c = c; P->cout = cout;
    int n = 0;
    auto add = [&](int mode, int ci, int co, int lin, int lout) {
        cr_layer_set(P->L[n], mode, ci, co, lin, lout, n == 0);
        ++n;
    };
    add(CR_S1, cin, c, 0, 0);                                                   // conv0
    for (int lvl = 0; lvl < depth; ++lvl) {
        add(CR_S2, c << lvl, c << (lvl + 1), lvl, lvl + 1);                     // conv(2 lvl + 1)
        add(CR_S1, c << (lvl + 1), c << (lvl + 1), lvl + 1, lvl + 1);           // conv(2 lvl + 2)
    }
    for (int lvl = depth - 1; lvl >= 0; --lvl) add(CR_UP, c << (lvl + 1), c << lvl, lvl + 1, lvl);
    add(CR_S1, c, cout, 0, 0);                                                  // the heads
    CrLayer& h = P->L[n - 1];
    h.zs = 1; h.taps = 27; h.rows = cout + 1; h.nmt = 1;
    P->nlayers = n;
    size_t o = 0;
    for (int i = 0; i < n; ++i) {
        CrLayer& l = P->L[i];
        l.w_off = o; o += (size_t)l.nmt * l.taps * l.nchunk * 64 * l.e;
        l.ep_off = o; o += (i == n - 1) ? 0 : (size_t)4 * l.cout;
        o = (o + 63) / 64 * 64;
    }
    P->total = o;
    return GDB_OK;
}

// Input channel of k-chunk cc, lane group kq, element e (the packing and the kernels' operand loads agree on it).
static inline int cr_ci(const CrLayer& l, int cc, int kq, int e) { return l.nc ? 16 * cc + 4 * e + kq : 4 * l.e * cc + l.e * kq + e; }

// Weight of GEMM row `row` of layer l at input channel ci and tap.  Conv weights are torch's (cout, cin, 3, 3, 3), transposed-conv
// weights (cin, cout, 3, 3, 3); tap = (kz 3 + ky) 3 + kx, or with zs == 2 (dz 3 + ky) 3 + kx over the 4 input planes dz.
static float cr_weight(const CrLayer& l, bool heads, const float* w, const float* w2, int row, int ci, int tap) {
    if (ci >= l.cin || row >= l.rows) return 0.f;
    if (heads)   // rows 0 .. cout - 1: feat_head (cout, c, 3, 3, 3); row cout: prob_head (1, c, 3, 3, 3)
        return row < l.cout ? w[((size_t)row * l.cin + ci) * 27 + tap] : w2[(size_t)ci * 27 + tap];
    if (l.zs == 2) {
        const int s = row / l.cout, co = row % l.cout, kz = tap / 9 - s;
        if (kz < 0 || kz > 2) return 0.f;
        return w[((size_t)co * l.cin + ci) * 27 + kz * 9 + tap % 9];
    }
    if (l.mode == CR_UP) return w[((size_t)ci * l.cout + row) * 27 + tap];
    return w[((size_t)row * l.cin + ci) * 27 + tap];
}

// ---- device ---------------------------------------------------------------------------------------------------------------
struct CrArgs {
    const float* in;     // nc: (B, cin, Di, Hi, Wi); else channel-last (B, Di, Hi, Wi, cin)
    const float* w;      // the layer's packed weights
    const float* ep;     // [invstd | mean | weight | bias] x cout
    float* out;          // channel-last (B, Do, Ho, Wo, cout); heads: the volume (B, cout, Do, Ho, Wo)
    float* prob;         // heads: the prob head's logits (B, Do, Ho, Wo)
    int skip;            // add out's previous contents after the ReLU (in place)
    int B, cin, cout, Di, Hi, Wi, Do, Ho, Wo;
    int taps, nchunk, nmt;
    int ncols, nct;      // columns (output x, or x / 2 for CR_UP) and column tiles per row
    int nz;              // output plane groups (Do / zs)
    int nwaves;
};

template <int E> struct Vec;
template <> struct Vec<2> { typedef F2 T; };
template <> struct Vec<4> { typedef F4 T; };
struct F4u { float x, y, z, w; } __attribute__((packed, aligned(4)));

// MODE: CR_S1 / CR_S2 / CR_UP; E: floats per lane per k-chunk; NC: the (B, C, D, H, W) input; ZS: output planes per wave; EPI: CR_BN /
// CR_HEADS.  NA accumulators of 16 columns each: NC -> 4 (x = x0 + 4 j + n), else 2 (x = x0 + 16 n + j).
template <int MODE, int E, bool NC, int ZS, int EPI>
__device__ __forceinline__ void costreg_conv_body(const CrArgs& a) {
    constexpr int NA = NC ? 4 : 2;
    typedef typename Vec<E>::T VE;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (wave >= a.nwaves) return;
    const int j = lane & 15, kq = lane >> 4;
    int t = wave;
    const int ct = t % a.nct; t /= a.nct;
    const int px = MODE == CR_UP ? (t & 1) : 0;
    if (MODE == CR_UP) t >>= 1;
    const int mt = t % a.nmt; t /= a.nmt;
    const int y = t % a.Ho; t /= a.Ho;
    const int zg = t % a.nz;
    const int b = t / a.nz;
    const int x0 = ct * 16 * NA;
    F4 acc[NA];
#pragma unroll
    for (int n = 0; n < NA; ++n) acc[n] = F4{0.f, 0.f, 0.f, 0.f};
    const size_t plane_in = (size_t)a.Hi * a.Wi;
    const float* wl = a.w + (size_t)mt * a.taps * a.nchunk * 64 * E + (size_t)lane * E;
    for (int tap = 0; tap < a.taps; ++tap) {
        const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        int iz, iy, xoff;   // input plane, input row; input x = column * (1 or 2) + xoff
        if (MODE == CR_S1) { iz = zg * ZS + kz - 1; iy = y + ky - 1; xoff = kx - 1; }
        else if (MODE == CR_S2) { iz = 2 * zg + kz - 1; iy = 2 * y + ky - 1; xoff = kx - 1; }
        else {   // o = 2 i - 1 + k: the tap belongs to the wave's parity class iff o + 1 - k is even
            if (((zg + 1 - kz) | (y + 1 - ky) | (px + 1 - kx)) & 1) continue;
            iz = (zg + 1 - kz) >> 1; iy = (y + 1 - ky) >> 1; xoff = (px + 1 - kx) >> 1;
        }
        if (iz < 0 || iz >= a.Di || iy < 0 || iy >= a.Hi) continue;   // zero padding: the tap adds nothing (wave-uniform)
        const float* wt = wl + (size_t)tap * a.nchunk * 64 * E;
        if constexpr (NC) {
            const int xs = x0 + 4 * j + xoff;   // this lane's four consecutive input x
            const bool whole = xs >= 0 && xs + 3 < a.Wi;
            for (int cc = 0; cc < a.nchunk; ++cc) {
                const F4 wv = *(const F4*)(wt + (size_t)cc * 64 * E);
                F4 bv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ci = 16 * cc + 4 * e + kq;
                    bv[e] = F4{0.f, 0.f, 0.f, 0.f};
                    if (ci < a.cin) {
                        const float* p = a.in + (((size_t)b * a.cin + ci) * a.Di + iz) * plane_in + (size_t)iy * a.Wi;
                        if (whole) {
                            const F4u v = *(const F4u*)(p + xs);
                            bv[e] = F4{v.x, v.y, v.z, v.w};
                        } else {
#pragma unroll
                            for (int q = 0; q < 4; ++q) bv[e][q] = (xs + q >= 0 && xs + q < a.Wi) ? p[xs + q] : 0.f;
                        }
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[e], bv[e][n], acc[n], 0, 0, 0);
            }
        } else {
            constexpr int xmul = MODE == CR_S2 ? 2 : 1;
            const float* rowp = a.in + (((size_t)b * a.Di + iz) * a.Hi + iy) * (size_t)a.Wi * a.cin + E * kq;
            int xi[NA];
            bool ok[NA];
#pragma unroll
            for (int n = 0; n < NA; ++n) {
                xi[n] = (x0 + 16 * n + j) * xmul + xoff;
                ok[n] = xi[n] >= 0 && xi[n] < a.Wi;
            }
            for (int cc = 0; cc < a.nchunk; ++cc) {
                const VE wv = *(const VE*)(wt + (size_t)cc * 64 * E);
                VE bv[NA];
#pragma unroll
                for (int n = 0; n < NA; ++n) {
                    if (ok[n]) {
                        bv[n] = *(const VE*)(rowp + (size_t)xi[n] * a.cin + 4 * E * cc);
                    } else {
#pragma unroll
                        for (int e = 0; e < E; ++e) bv[n][e] = 0.f;
                    }
                }
#pragma unroll
                for (int e = 0; e < E; ++e)
#pragma unroll
                    for (int n = 0; n < NA; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[e], bv[n][e], acc[n], 0, 0, 0);
            }
        }
    }
    // epilogue: register r of lane (j, kq) = GEMM row 4 kq + r of column j of accumulator n
#pragma unroll
    for (int n = 0; n < NA; ++n) {
        const int col = x0 + (NC ? 4 * j + n : 16 * n + j);
        if (col >= a.ncols) continue;
        const int x = MODE == CR_UP ? 2 * col + px : col;
        if constexpr (EPI == CR_HEADS) {
            const size_t ovol = (size_t)a.Do * a.Ho * a.Wo, p = ((size_t)zg * a.Ho + y) * a.Wo + x;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * kq + r;
                if (row < a.cout) a.out[((size_t)b * a.cout + row) * ovol + p] = acc[n][r];
                else if (row == a.cout) a.prob[(size_t)b * ovol + p] = acc[n][r];
            }
        } else {
            const int row0 = 4 * kq;
            const int s = ZS == 2 ? row0 / a.cout : 0, co = ZS == 2 ? row0 % a.cout : 16 * mt + row0;
            if (co >= a.cout) continue;   // (cout is a multiple of 4: a lane's four rows are one voxel's channels co .. co + 3)
            const int z = zg * ZS + s;
            float* o = a.out + ((((size_t)b * a.Do + z) * a.Ho + y) * a.Wo + x) * a.cout + co;
            F4 v;
            if constexpr (EPI == CR_RAW) {
                v = acc[n];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = co + r;
                    const float h = (acc[n][r] - a.ep[a.cout + c]) * a.ep[c] * a.ep[2 * a.cout + c] + a.ep[3 * a.cout + c];
                    v[r] = fmaxf(h, 0.f);
                }
            }
            if (a.skip) {
                const F4 sk = *(const F4*)o;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = sk[r] + v[r];
            }
            *(F4*)o = v;
        }
    }
}

// workspace: per level l = 0 .. depth the channel-last activation / skip S_l (c << l channels at (D, H, W) >> l) and, for
// l >= 1, the stride-2 convolution's output T_l of the same size
static size_t cr_level_floats(int B, int D, int H, int W, int c, int l) {
    return ((size_t)B * (D >> l) * (H >> l) * (W >> l) * (c << l) + 63) / 64 * 64;
}
static size_t cr_ws_floats(const CrPlan& P, int B, int D, int H, int W) {
    size_t s = 0;
    for (int l = 0; l <= P.depth; ++l) s += (l ? 2 : 1) * cr_level_floats(B, D, H, W, P.c, l);
    return s;
}

static int cr_check_shape(const CrPlan& P, int B, int D, int H, int W) {
    if (B < 1 || D < 1 || H < 1 || W < 1) return gdb_fail(GDB_E_SHAPE, "cost reg: bad volume shape B=%d D=%d H=%d W=%d", B, D, H, W);
    const int m = 1 << P.depth;
    if (D % m || H % m || W % m)
        return gdb_fail(GDB_E_SHAPE, "cost reg: volume D=%d H=%d W=%d is not divisible by 2^depth = %d (the skip adds would mismatch)", D, H, W, m);
    if ((double)B * D * H * W * (P.cin > P.c ? P.cin : P.c) >= 1e12) return gdb_fail(GDB_E_SHAPE, "cost reg: volume too large");
    return GDB_OK;
}

// the launch geometry of a layer; GDB_E_SHAPE when the grid would overflow
static int cr_geom(const CrLayer& l, int B, int D, int H, int W, CrArgs* pa) {
    CrArgs& a = *pa;
    a = CrArgs{};
    a.B = B; a.cin = l.cin; a.cout = l.cout;
    a.Di = D >> l.level_in; a.Hi = H >> l.level_in; a.Wi = W >> l.level_in;
    a.Do = D >> l.level_out; a.Ho = H >> l.level_out; a.Wo = W >> l.level_out;
    a.taps = l.taps; a.nchunk = l.nchunk; a.nmt = l.nmt;
    a.ncols = l.mode == CR_UP ? a.Wo / 2 : a.Wo;
    const int na = l.nc ? 4 : 2;
    a.nct = (a.ncols + 16 * na - 1) / (16 * na);
    a.nz = a.Do / l.zs;
    const long long nw = (long long)B * a.nz * a.Ho * l.nmt * (l.mode == CR_UP ? 2 : 1) * a.nct;
    if (nw >= (1LL << 31) - 4) return gdb_fail(GDB_E_SHAPE, "cost reg: volume too large for the launch grid");
    a.nwaves = (int)nw;
    return GDB_OK;
}

// the launch geometry of layer li of the forward plan
static int cr_args(const CrPlan& P, int li, int B, int D, int H, int W, CrArgs* pa) {
    const CrLayer& l = P.L[li];
    // After conv0 every stride-1 and every transposed BN layer reads c << (level + 1) channels, a multiple of 16, into at least 16
    // rows: E = 4 at one plane per wave is the only form cr_plan asks for, and the only one built (cr_layer).
    if (li > 0 && li < P.nlayers - 1 && l.mode != CR_S2 && (l.e != 4 || l.zs != 1))
        return gdb_fail(GDB_E_BADARG, "cost reg: layer %d (mode %d, %d -> %d channels) asks for a kernel that is not built (E = %d, %d planes per wave)",
                        li, l.mode, l.cin, l.cout, l.e, l.zs);
    return cr_geom(l, B, D, H, W, pa);
}
