// The feature pyramid network (`FeatureNet.forward`, networks/gdb_nerf/feature_net.py: conv0 / conv1 / conv2, each two
// conv_block2d, then out0 and the two top-down steps nearest-upsample + lateral 1x1 + add, then out1 and out2) as HIP kernels for
// gfx950, inference only (eval-mode BatchNorm).
//
// * Layout: the input is the (N, 3, H, W) image batch, read in place; every intermediate is channel-last (N, h, w, C) in the caller's
//   workspace; the pyramid levels are written in the module's layout, level 0 (N, out0, H/4, W/4), level 1 (N, out1, H/2, W/2),
//   level 2 (N, out2, H, W), where every halving is ceil(x / 2) (the 5x5 stride-2 convolutions' padding 2).
// * Every convolution is one implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate: k-ordered fmaf chains;
//   a channel-last layer keeps one chain per element e of a lane's E-float load and adds the E of them pairwise at the end, so that
//   a chain is at most cin / 4 x taps / 4 MFMAs long: one chain over the 864 .. 1600 products of the 96- and 128-channel layers
//   strayed further from float64 than 4 x the fp32 PyTorch module does, tests/test_fpn_referee.py):
//   output channels on the MFMA rows, 32 consecutive pixels of one output row on the columns (2 accumulators of 16), K = (tap, input
//   channel).  One wave owns one 16-row tile.  Operands come straight from global memory (L1 / L2 hits: a pixel's channels are re-read
//   by the taps of neighbouring waves); the weights are packed on the host in operand order, one E-float load per lane per E k-steps.
//     - channel-last input: lane (j = l & 15, kq = l >> 4) loads E consecutive channels of pixel j (E = 4, or 2 for inputs whose
//       channel count is not a multiple of 16); element e feeds k-step e: channel 4 E cc + E kq + e of k-chunk cc;
//     - the first convolution (3 input channels, planar image): K = (ci, input row, kx) is folded into k-steps of 4 (27 or 36 of
//       them, zero-padded to a multiple of 4); lane (j, kq) loads the one image value of k = 4 s + kq for each of its columns.
// * 8-output-channel 3x3 layers (conv0.* at base_channels 8, out1 / out2 at 8 channels) would fill half a tile.  They run two output
//   rows per wave instead: rows 0-7 are the 8 channels at row y, rows 8-15 the same channels at y + 1, over K = 4 input rows x 3 x cin
//   (the row half's weights shifted by one input row, zeros outside): 4/3 of the K for twice the useful rows.
// * Epilogues fused: eval BatchNorm (x - running_mean) * invstd * weight + bias with invstd = 1 / sqrt(running_var + eps) formed on
//   the host in fp32, then ReLU (conv_block2d); the lateral 1x1 convolutions add their bias and then the nearest-upsampled coarser map
//   (torch's `nearest` with an explicit size: source index min(floor(dst * (float) in / out), in - 1), the index itself at equal sizes,
//   dst >> 1 at exactly twice the size); out0 adds its bias; out1 / out2 have none.  No atomics anywhere: the outputs are
//   deterministic, and every workspace buffer is written before it is read.
#include "gdb_internal.h"
#include <cmath>
#include <cstring>

typedef float F2 __attribute__((ext_vector_type(2)));
typedef float F4 __attribute__((ext_vector_type(4)));

enum { FP_BN = 0, FP_LAT = 1, FP_OUT = 2 };   // epilogues: BN + ReLU (channel-last), bias + upsampled add (channel-last), level (NCHW)
enum { FP_C00, FP_C01, FP_C10, FP_C11, FP_C20, FP_C21, FP_OUT0, FP_INNER1, FP_INNER2, FP_OUT1, FP_OUT2, FP_NLAYERS };

// ---- layer plan (packing, workspace and launches share it) ---------------------------------------------------------------
struct FpLayer {
    int ks, stride, pad, cin, cout;
    int lin, lout;   // resolution level of the input / output: 0 full (H, W), 1 half, 2 quarter
    int img;         // the input is the planar (N, 3, H, W) image (conv0.0)
    int zs;          // output rows per wave: 2 for an 8-channel 3x3 layer (rows = 2 image rows x 8 channels), else 1
    int taps;        // taps (ks^2, or 4 x 3 when zs == 2); for the image layer the number of 4-wide k-steps
    int e;           // floats per lane per k-chunk: 4 (16 channels per chunk), 2 (8), 1 for the image layer
    int nchunk;      // k-chunks of the input channels (1 for the image layer)
    int rows, nmt;   // GEMM rows (zs x cout) and 16-row tiles
    int epi, bias;   // epilogue; FP_OUT with a bias (out0)
    size_t w_off, ep_off;   // packed floats: weights, then [invstd | mean | weight | bias] x cout (BN) or bias x cout
};
struct FpPlan {
    int c, o0, o1, o2;
    FpLayer L[FP_NLAYERS];
    size_t total;
};

static int fp_plan(int c, int o0, int o1, int o2, FpPlan* P) {
    if (c < 8 || c > 32 || c % 8) return gdb_fail(GDB_E_BADARG, "fpn: base_channels %d (a multiple of 8, at most 32)", c);
    const int outs[3] = {o0, o1, o2};
    for (int i = 0; i < 3; ++i)
        if (outs[i] < 8 || outs[i] > 64 || outs[i] % 8)
            return gdb_fail(GDB_E_BADARG, "fpn: out_channels[%d] = %d (a multiple of 8, at most 64)", i, outs[i]);
    P->c = c; P->o0 = o0; P->o1 = o1; P->o2 = o2;
    auto set = [&](int i, int ks, int stride, int cin, int cout, int lin, int lout, int epi, int bias) {
        FpLayer& l = P->L[i];
        l.ks = ks; l.stride = stride; l.pad = ks / 2; l.cin = cin; l.cout = cout; l.lin = lin; l.lout = lout;
        l.epi = epi; l.bias = bias;
        l.img = (i == FP_C00);
        l.zs = (ks == 3 && stride == 1 && cout == 8) ? 2 : 1;
        if (l.img) {
            l.e = 1; l.nchunk = 1;
            l.taps = (9 * (l.zs == 2 ? 4 : 3) + 3) / 4;
        } else {
            l.e = cin % 16 == 0 ? 4 : 2;
            l.nchunk = cin / (4 * l.e);
            l.taps = l.zs == 2 ? 12 : ks * ks;
        }
        l.rows = l.zs * cout;
        l.nmt = (l.rows + 15) / 16;
    };
    set(FP_C00, 3, 1, 3, c, 0, 0, FP_BN, 0);
    set(FP_C01, 3, 1, c, c, 0, 0, FP_BN, 0);
    set(FP_C10, 5, 2, c, 2 * c, 0, 1, FP_BN, 0);
    set(FP_C11, 3, 1, 2 * c, 2 * c, 1, 1, FP_BN, 0);
    set(FP_C20, 5, 2, 2 * c, 4 * c, 1, 2, FP_BN, 0);
    set(FP_C21, 3, 1, 4 * c, 4 * c, 2, 2, FP_BN, 0);
    set(FP_OUT0, 1, 1, 4 * c, o0, 2, 2, FP_OUT, 1);
    set(FP_INNER1, 1, 1, 2 * c, 4 * c, 1, 1, FP_LAT, 1);
    set(FP_INNER2, 1, 1, c, 4 * c, 0, 0, FP_LAT, 1);
    set(FP_OUT1, 3, 1, 4 * c, o1, 1, 1, FP_OUT, 0);
    set(FP_OUT2, 3, 1, 4 * c, o2, 0, 0, FP_OUT, 0);
    size_t o = 0;
    for (int i = 0; i < FP_NLAYERS; ++i) {
        FpLayer& l = P->L[i];
        l.w_off = o; o += (size_t)l.nmt * l.taps * l.nchunk * 64 * l.e;
        o = (o + 63) / 64 * 64;
        l.ep_off = o; o += l.epi == FP_BN ? (size_t)4 * l.cout : l.bias ? (size_t)l.cout : 0;
        o = (o + 63) / 64 * 64;
    }
    P->total = o;
    return GDB_OK;
}

// Weight of GEMM row `row` of layer l at lane group kq, element e of k-chunk cc and tap (the packing and the kernels' operand loads
// agree on it).  Torch's Conv2d weights are (cout, cin, ks, ks).
static float fp_weight(const FpLayer& l, const float* w, int row, int tap, int cc, int kq, int e) {
    if (row >= l.rows) return 0.f;
    const int co = l.zs == 2 ? row % 8 : row, s = l.zs == 2 ? row / 8 : 0;
    int ci, ky, kx;
    if (l.img) {   // k = (ci TR + input row) 3 + kx, TR = 3 or 4 input rows
        const int TR = l.zs == 2 ? 4 : 3, k = 4 * tap + kq;
        if (k >= 9 * TR) return 0.f;
        ci = k / (3 * TR); ky = (k / 3) % TR - s; kx = k % 3;
    } else {
        ci = 4 * l.e * cc + l.e * kq + e;
        if (l.zs == 2) { ky = tap / 3 - s; kx = tap % 3; }
        else { ky = tap / l.ks; kx = tap % l.ks; }
    }
    if (ky < 0 || ky >= l.ks) return 0.f;
    return w[(((size_t)co * l.cin + ci) * l.ks + ky) * l.ks + kx];
}

// ---- device ---------------------------------------------------------------------------------------------------------------
struct FpArgs {
    const float* in;     // img: (N, 3, Hi, Wi); else channel-last (N, Hi, Wi, cin)
    const float* w;      // the layer's packed weights
    const float* ep;     // [invstd | mean | weight | bias] x cout, or bias x cout
    const float* top;    // FP_LAT: the coarser map, channel-last (N, Ht, Wt, cout)
    float* out;          // channel-last (N, Ho, Wo, cout), or FP_OUT: (N, cout, Ho, Wo)
    int N, cin, cout, Hi, Wi, Ho, Wo, ks, stride, pad, bias;
    int taps, nchunk, nmt, nct, nyg, nwaves;
    int Ht, Wt;
    float sy, sx;        // (float) Ht / Ho, (float) Wt / Wo
};

template <int E> struct Vec;
template <> struct Vec<1> { typedef float T; };
template <> struct Vec<2> { typedef F2 T; };
template <> struct Vec<4> { typedef F4 T; };

// torch's nearest source index for an explicit output size (aten/src/ATen/native/UpSample.h nearest_idx)
__device__ __forceinline__ int fp_nearest(int dst, int in, int out, float scale) {
    if (in == out) return dst;
    if (out == 2 * in) return dst >> 1;
    return min((int)floorf((float)dst * scale), in - 1);
}

// IMG: the planar 3-channel image input; ZS: output rows per wave; E: floats per lane per k-chunk; EPI: FP_BN / FP_LAT / FP_OUT.
// NA = 2 accumulators of 16 columns: x = x0 + 16 n + j.
template <bool IMG, int ZS, int E, int EPI>
__global__ void __launch_bounds__(256) k_fpn_conv(FpArgs a) {
    constexpr int NA = 2;
    typedef typename Vec<E>::T VE;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (wave >= a.nwaves) return;
    const int j = lane & 15, kq = lane >> 4;
    int t = wave;
    const int ct = t % a.nct; t /= a.nct;
    const int mt = t % a.nmt; t /= a.nmt;
    const int yg = t % a.nyg;
    const int n = t / a.nyg;
    const int x0 = ct * 16 * NA;
    F4 part[NA][E];   // one accumulation chain per element of the lane's load
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int e = 0; e < E; ++e) part[i][e] = F4{0.f, 0.f, 0.f, 0.f};
    const float* wl = a.w + (size_t)mt * a.taps * a.nchunk * 64 * E + (size_t)lane * E;
    if constexpr (IMG) {
        constexpr int TR = ZS == 2 ? 4 : 3, K = 9 * TR;
        const int ybase = ZS * yg - 1;   // input row of row index 0 (stride 1, padding 1)
        for (int s = 0; s < a.taps; ++s) {
            const float wv = wl[(size_t)s * 64];
            const int k = 4 * s + kq;
            const int ci = k / (3 * TR), iy = ybase + (k / 3) % TR, kx = k % 3;
            const bool rowok = k < K && iy >= 0 && iy < a.Hi;
            const size_t rbase = rowok ? (((size_t)n * 3 + ci) * a.Hi + iy) * a.Wi : 0;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int ix = x0 + 16 * i + j + kx - 1;
                const float b = (rowok && ix >= 0 && ix < a.Wi) ? a.in[rbase + ix] : 0.f;
                part[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, b, part[i][0], 0, 0, 0);
            }
        }
    } else {
        for (int tap = 0; tap < a.taps; ++tap) {
            int iy, kx;
            if (ZS == 2) { iy = 2 * yg - 1 + tap / 3; kx = tap % 3; }
            else { iy = yg * a.stride + tap / a.ks - a.pad; kx = tap % a.ks; }
            if (iy < 0 || iy >= a.Hi) continue;   // zero padding: the tap adds nothing (wave-uniform)
            const float* rowp = a.in + ((size_t)n * a.Hi + iy) * (size_t)a.Wi * a.cin + E * kq;
            const float* wt = wl + (size_t)tap * a.nchunk * 64 * E;
            int xi[NA];
            bool ok[NA];
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                xi[i] = (x0 + 16 * i + j) * a.stride + kx - a.pad;
                ok[i] = xi[i] >= 0 && xi[i] < a.Wi;
            }
            for (int cc = 0; cc < a.nchunk; ++cc) {
                const VE wv = *(const VE*)(wt + (size_t)cc * 64 * E);
                VE bv[NA];
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    if (ok[i]) {
                        bv[i] = *(const VE*)(rowp + (size_t)xi[i] * a.cin + 4 * E * cc);
                    } else {
#pragma unroll
                        for (int e = 0; e < E; ++e) bv[i][e] = 0.f;
                    }
                }
#pragma unroll
                for (int e = 0; e < E; ++e)
#pragma unroll
                    for (int i = 0; i < NA; ++i) part[i][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[e], bv[i][e], part[i][e], 0, 0, 0);
            }
        }
    }
    F4 acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        if constexpr (E == 4) acc[i] = (part[i][0] + part[i][1]) + (part[i][2] + part[i][3]);
        else if constexpr (E == 2) acc[i] = part[i][0] + part[i][1];
        else acc[i] = part[i][0];
    }
    // epilogue: register r of lane (j, kq) = GEMM row 4 kq + r of column j of accumulator i
    const int row0 = 4 * kq;
    const int s = ZS == 2 ? row0 / 8 : 0, co = ZS == 2 ? row0 % 8 : 16 * mt + row0;
    const int y = ZS * yg + s;
    if (co >= a.cout || y >= a.Ho) return;   // (cout is a multiple of 8: a lane's four rows are one pixel's channels co .. co + 3)
    int sy = 0;
    if constexpr (EPI == FP_LAT) sy = fp_nearest(y, a.Ht, a.Ho, a.sy);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int x = x0 + 16 * i + j;
        if (x >= a.Wo) continue;
        if constexpr (EPI == FP_OUT) {
            float* o = a.out + (((size_t)n * a.cout + co) * a.Ho + y) * a.Wo + x;
            const size_t plane = (size_t)a.Ho * a.Wo;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r * plane] = a.bias ? acc[i][r] + a.ep[co + r] : acc[i][r];
        } else {
            float* o = a.out + (((size_t)n * a.Ho + y) * a.Wo + x) * a.cout + co;
            F4 v;
            if constexpr (EPI == FP_BN) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = co + r;
                    const float h = (acc[i][r] - a.ep[a.cout + c]) * a.ep[c] * a.ep[2 * a.cout + c] + a.ep[3 * a.cout + c];
                    v[r] = fmaxf(h, 0.f);
                }
            } else {   // interpolate(top, size) + lateral(skip): the lateral's bias first, then the upsampled map
                const int sx = fp_nearest(x, a.Wt, a.Wo, a.sx);
                const F4 tp = *(const F4*)(a.top + (((size_t)n * a.Ht + sy) * a.Wt + sx) * a.cout + co);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = tp[r] + (acc[i][r] + a.ep[co + r]);
            }
            *(F4*)o = v;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
extern "C" int gdb_fpn_packed_floats(int32_t base_channels, int32_t out0, int32_t out1, int32_t out2, size_t* out_floats) {
    if (!out_floats) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    FpPlan P;
    int rc = fp_plan(base_channels, out0, out1, out2, &P);
    if (rc != GDB_OK) return rc;
    *out_floats = P.total;
    return GDB_OK;
}

// h_tensors: 0 .. 29 the six conv_block2d (weight, bn weight, bn bias, running_mean, running_var); 30 out0.weight, 31 out0.bias,
// 32 inner1.weight, 33 inner1.bias, 34 inner2.weight, 35 inner2.bias, 36 out1.weight, 37 out2.weight, 38 the BN eps
#define FP_NTENSORS 39
static const int fp_wt[FP_NLAYERS] = {0, 5, 10, 15, 20, 25, 30, 32, 34, 36, 37};
static const int fp_bias[FP_NLAYERS] = {-1, -1, -1, -1, -1, -1, 31, 33, 35, -1, -1};

extern "C" int gdb_pack_fpn_weights(int32_t base_channels, int32_t out0, int32_t out1, int32_t out2, const float* const* t, float* out) {
    if (!t || !out) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    FpPlan P;
    int rc = fp_plan(base_channels, out0, out1, out2, &P);
    if (rc != GDB_OK) return rc;
    for (int i = 0; i < FP_NTENSORS; ++i)
        if (!t[i]) return gdb_fail(GDB_E_BADARG, "NULL tensor %d of the FPN state dict", i);
    const float eps = t[FP_NTENSORS - 1][0];
    memset(out, 0, P.total * sizeof(float));
    for (int li = 0; li < FP_NLAYERS; ++li) {
        const FpLayer& l = P.L[li];
        const float* w = t[fp_wt[li]];
        float* o = out + l.w_off;
        for (int mt = 0; mt < l.nmt; ++mt)
            for (int tap = 0; tap < l.taps; ++tap)
                for (int cc = 0; cc < l.nchunk; ++cc)
                    for (int ln = 0; ln < 64; ++ln)
                        for (int e = 0; e < l.e; ++e)
                            o[((((size_t)mt * l.taps + tap) * l.nchunk + cc) * 64 + ln) * l.e + e] =
                                fp_weight(l, w, 16 * mt + (ln & 15), tap, cc, ln >> 4, e);
        float* ep = out + l.ep_off;
        if (l.epi == FP_BN) {
            const float *g = t[fp_wt[li] + 1], *bb = t[fp_wt[li] + 2], *mean = t[fp_wt[li] + 3], *var = t[fp_wt[li] + 4];
            for (int c = 0; c < l.cout; ++c) {
                ep[c] = 1.f / sqrtf(var[c] + eps);
                ep[l.cout + c] = mean[c];
                ep[2 * l.cout + c] = g[c];
                ep[3 * l.cout + c] = bb[c];
            }
        } else if (l.bias) {
            memcpy(ep, t[fp_bias[li]], sizeof(float) * l.cout);
        }
    }
    return GDB_OK;
}

// workspace: A (conv0.0's output, N H W c; placed in I2's space when level 2 is built: I2 is written after A is last read), F0
// (conv0, N H W c), T1 / H1 (conv1.0 / conv1, N h w 2c), T2 / Q (conv2.0 / conv2, N q wq 4c), I1 (the half-resolution top-down map,
// N h w 4c; levels 1 and 2), I2 (the full-resolution one, N H W 4c; level 2)
enum { WS_A, WS_F0, WS_T1, WS_H1, WS_T2, WS_Q, WS_I1, WS_I2, WS_N };
struct FpDims { int H[3], W[3]; };
static FpDims fp_dims(int H, int W) {
    FpDims d;
    d.H[0] = H; d.W[0] = W;
    for (int l = 1; l < 3; ++l) { d.H[l] = (d.H[l - 1] + 1) / 2; d.W[l] = (d.W[l - 1] + 1) / 2; }
    return d;
}
static int fp_levels_needed(int mask) {   // the top-down maps a mask needs: bit 1 = I1, bit 2 = I2
    return ((mask & 6) ? 2 : 0) | ((mask & 4) ? 4 : 0);
}
static void fp_ws_sizes(const FpPlan& P, int N, int H, int W, int mask, size_t sz[WS_N]) {
    const FpDims d = fp_dims(H, W);
    auto f = [&](int l, int ch) { return ((size_t)N * d.H[l] * d.W[l] * ch + 63) / 64 * 64; };
    const int need = fp_levels_needed(mask), c = P.c;
    sz[WS_F0] = f(0, c);
    sz[WS_T1] = sz[WS_H1] = f(1, 2 * c);
    sz[WS_T2] = sz[WS_Q] = f(2, 4 * c);
    sz[WS_I1] = (need & 2) ? f(1, 4 * c) : 0;
    sz[WS_I2] = (need & 4) ? f(0, 4 * c) : 0;
    sz[WS_A] = (need & 4) ? 0 : f(0, c);
}
static size_t fp_ws_bytes(const FpPlan& P, int N, int H, int W, int mask) {
    size_t sz[WS_N], s = 0;
    fp_ws_sizes(P, N, H, W, mask, sz);
    for (int i = 0; i < WS_N; ++i) s += sz[i];
    return s * sizeof(float);
}

static int fp_check(int N, int H, int W, int mask) {
    if (N < 1 || H < 1 || W < 1) return gdb_fail(GDB_E_SHAPE, "fpn: bad image shape N=%d H=%d W=%d", N, H, W);
    if ((mask & 7) == 0 || (mask & ~7)) return gdb_fail(GDB_E_BADARG, "fpn: level_mask 0x%x (a non-empty subset of bits 0..2)", mask);
    if ((double)N * H * W * 128 >= 1e12) return gdb_fail(GDB_E_SHAPE, "fpn: images too large");
    return GDB_OK;
}

extern "C" int gdb_fpn_workspace_bytes(int32_t base_channels, int32_t out0, int32_t out1, int32_t out2, int32_t N, int32_t H, int32_t W,
                                       int32_t level_mask, size_t* out_bytes) {
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    FpPlan P;
    int rc = fp_plan(base_channels, out0, out1, out2, &P);
    if (rc != GDB_OK) return rc;
    if ((rc = fp_check(N, H, W, level_mask)) != GDB_OK) return rc;
    *out_bytes = fp_ws_bytes(P, N, H, W, level_mask);
    return GDB_OK;
}

// the launch geometry of layer li; GDB_E_SHAPE when the grid would overflow
static int fp_args(const FpPlan& P, int li, int N, const FpDims& d, FpArgs* pa) {
    const FpLayer& l = P.L[li];
    FpArgs& a = *pa;
    a = FpArgs{};
    a.N = N; a.cin = l.cin; a.cout = l.cout;
    a.Hi = d.H[l.lin]; a.Wi = d.W[l.lin]; a.Ho = d.H[l.lout]; a.Wo = d.W[l.lout];
    a.ks = l.ks; a.stride = l.stride; a.pad = l.pad; a.bias = l.bias;
    a.taps = l.taps; a.nchunk = l.nchunk; a.nmt = l.nmt;
    a.nct = (a.Wo + 31) / 32;
    a.nyg = (a.Ho + l.zs - 1) / l.zs;
    if (l.epi == FP_LAT) {
        a.Ht = d.H[l.lout + 1]; a.Wt = d.W[l.lout + 1];
        a.sy = (float)a.Ht / (float)a.Ho; a.sx = (float)a.Wt / (float)a.Wo;
    }
    const long long nw = (long long)N * a.nyg * a.nmt * a.nct;
    if (nw >= (1LL << 31) - 4) return gdb_fail(GDB_E_SHAPE, "fpn: images too large for the launch grid");
    a.nwaves = (int)nw;
    return GDB_OK;
}

template <bool IMG, int ZS, int E, int EPI>
static int fp_launch(const FpArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((k_fpn_conv<IMG, ZS, E, EPI>), dim3((unsigned)((a.nwaves + 3) / 4)), dim3(256), 0, st, a);
    LAUNCH_CHECK("k_fpn_conv");
    return GDB_OK;
}

static int fp_layer(const FpLayer& l, const FpArgs& a, hipStream_t st) {
    if (l.img) return l.zs == 2 ? fp_launch<true, 2, 1, FP_BN>(a, st) : fp_launch<true, 1, 1, FP_BN>(a, st);
    switch (l.epi) {
        case FP_BN:
            if (l.zs == 2) return l.e == 4 ? fp_launch<false, 2, 4, FP_BN>(a, st) : fp_launch<false, 2, 2, FP_BN>(a, st);
            return l.e == 4 ? fp_launch<false, 1, 4, FP_BN>(a, st) : fp_launch<false, 1, 2, FP_BN>(a, st);
        case FP_LAT: return l.e == 4 ? fp_launch<false, 1, 4, FP_LAT>(a, st) : fp_launch<false, 1, 2, FP_LAT>(a, st);
        default:
            if (l.zs == 2) return l.e == 4 ? fp_launch<false, 2, 4, FP_OUT>(a, st) : fp_launch<false, 2, 2, FP_OUT>(a, st);
            return l.e == 4 ? fp_launch<false, 1, 4, FP_OUT>(a, st) : fp_launch<false, 1, 2, FP_OUT>(a, st);
    }
}

extern "C" int gdb_fpn(int32_t base_channels, int32_t out0, int32_t out1, int32_t out2, const float* d_images, int32_t N, int32_t H,
                       int32_t W, const float* d_packed, int32_t level_mask, void* d_ws, size_t ws_bytes, float* d_level0, float* d_level1,
                       float* d_level2, void* stream_) {
    FpPlan P;
    int rc = fp_plan(base_channels, out0, out1, out2, &P);
    if (rc != GDB_OK) return rc;
    if ((rc = fp_check(N, H, W, level_mask)) != GDB_OK) return rc;
    if (!d_images || !d_packed || !d_ws) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    float* outs[3] = {d_level0, d_level1, d_level2};
    for (int l = 0; l < 3; ++l)
        if ((level_mask >> l & 1) && !outs[l]) return gdb_fail(GDB_E_BADARG, "fpn: NULL output for level %d, which the mask asks for", l);
    const size_t need = fp_ws_bytes(P, N, H, W, level_mask);
    if (ws_bytes < need) return gdb_fail(GDB_E_WORKSPACE, "fpn: workspace of %zu bytes, %zu needed", ws_bytes, need);
    // the layers this mask runs, in order, and every one's geometry before the first launch: a refusal launches nothing
    const int tdn = fp_levels_needed(level_mask);
    int order[FP_NLAYERS], nl = 0;
    for (int li = FP_C00; li <= FP_C21; ++li) order[nl++] = li;
    if (level_mask & 1) order[nl++] = FP_OUT0;
    if (tdn & 2) order[nl++] = FP_INNER1;
    if (level_mask & 2) order[nl++] = FP_OUT1;
    if (tdn & 4) { order[nl++] = FP_INNER2; order[nl++] = FP_OUT2; }
    const FpDims d = fp_dims(H, W);
    FpArgs A[FP_NLAYERS];
    for (int k = 0; k < nl; ++k)
        if ((rc = fp_args(P, order[k], N, d, &A[order[k]])) != GDB_OK) return rc;
    size_t sz[WS_N];
    fp_ws_sizes(P, N, H, W, level_mask, sz);
    float* B[WS_N];
    float* p = (float*)d_ws;
    for (int i = 0; i < WS_N; ++i) { B[i] = p; p += sz[i]; }
    if (tdn & 4) B[WS_A] = B[WS_I2];
    auto io = [&](int li, const float* in, float* out, const float* top) {
        A[li].in = in; A[li].out = out; A[li].top = top;
        A[li].w = d_packed + P.L[li].w_off; A[li].ep = d_packed + P.L[li].ep_off;
    };
    io(FP_C00, d_images, B[WS_A], nullptr);
    io(FP_C01, B[WS_A], B[WS_F0], nullptr);
    io(FP_C10, B[WS_F0], B[WS_T1], nullptr);
    io(FP_C11, B[WS_T1], B[WS_H1], nullptr);
    io(FP_C20, B[WS_H1], B[WS_T2], nullptr);
    io(FP_C21, B[WS_T2], B[WS_Q], nullptr);
    io(FP_OUT0, B[WS_Q], d_level0, nullptr);
    io(FP_INNER1, B[WS_H1], B[WS_I1], B[WS_Q]);
    io(FP_OUT1, B[WS_I1], d_level1, nullptr);
    io(FP_INNER2, B[WS_F0], B[WS_I2], B[WS_I1]);
    io(FP_OUT2, B[WS_I2], d_level2, nullptr);
    hipStream_t st = (hipStream_t)stream_;
    for (int k = 0; k < nl; ++k)
        if ((rc = fp_layer(P.L[order[k]], A[order[k]], st)) != GDB_OK) return rc;
    return GDB_OK;
}
