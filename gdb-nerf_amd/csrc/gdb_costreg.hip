// The cascade's cost-regularisation 3-D U-Nets (`_UNet3d.forward`, networks/gdb_nerf/cost_reg_net.py:24-54: CostRegNet_small at
// depth 2, CostRegNet at depth 3) as HIP kernels for gfx950, inference only (eval-mode BatchNorm).
//
// * Layout: the input is the plane-sweep cost volume exactly as gdb_build_feature_volume writes it, (B, C, D, H, W), read in place;
//   every internal activation is channel-last (B, D, H, W, C) in the caller's workspace; the heads write the module's layouts,
//   volume (B, voxel_dim, D, H, W) and prob (B, D, H, W).
// * Every 3x3x3 layer is one implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate: a k-ordered fmaf chain):
//   output channels on the MFMA rows, consecutive W-voxels of one (b, z, y) row on the columns, K = (tap, input channel).  One wave
//   owns one 16-row tile and 64 (first layer) or 32 (channel-last layers) voxels: 4 or 2 independent accumulators.  Operands come
//   straight from global memory (L1 / L2 hits: a voxel's channels are re-read by the 27 taps of neighbouring waves); the weights are
//   packed on the host in operand order, one 16- or 8-byte load per lane per E MFMA k-steps.
//     - channel-last input: lane (j = l & 15, kq = l >> 4) loads E consecutive channels of voxel j (E = 4, or 2 for inputs whose
//       channel count is not a multiple of 16); element e feeds k-step e: channel 4 E cc + E kq + e of k-chunk cc;
//     - the (B, C, D, H, W) cost volume: lane (j, kq) loads four consecutive x of ONE channel (16 B) and element q feeds the
//       accumulator of the voxels x = x0 + 4 j + q; k-step e of chunk cc is channel 16 cc + 4 e + kq: four MFMAs per load.
// * 8-output-channel stride-1 layers (conv0 at base_channels 8) would fill half a tile.  They run two output planes per wave
//   instead: rows 0-7 are the 8 channels at plane z, rows 8-15 the same channels at plane z + 1, over K = 4 input planes x 9 x cin
//   (the row half's weights shifted by one plane, zeros outside): 4/3 of the K for twice the useful rows.
// * Transposed convolution (stride 2, padding 1, output_padding 1) without a scatter: output o = 2 i - 1 + k, so per dimension an
//   even output takes tap 1 (i = o / 2), an odd one taps 2 (i = (o - 1) / 2) and 0 (i = (o + 1) / 2).  A wave owns one output row
//   (z, y) and one x parity px: its columns are consecutive x / 2, its taps the 1, 2, 4 or 8 of its parity class.
// * Epilogue fused: eval BatchNorm (x - running_mean) * invstd * weight + bias with invstd = 1 / sqrt(running_var + eps) formed on
//   the host in fp32, ReLU, then the U-Net's skip add (skips.pop() + conv(y), :52) in place on the skip buffer.  The two heads
//   (feat_head c -> voxel_dim, prob_head c -> 1) are one GEMM of voxel_dim + 1 rows over y; the softmax over D (:54) is a small
//   kernel after it: max over D, exp, a sum in plane order, a division.  No atomics anywhere: the outputs are deterministic.
#include "gdb_internal.h"
#include <cmath>
#include <cstring>

int gdb_fail(int code, const char* fmt, ...);

#define LAUNCH_CHECK(name)                                                                    \
    do {                                                                                      \
        hipError_t e_ = hipGetLastError();                                                    \
        if (e_ != hipSuccess) return gdb_fail(GDB_E_HIP, "launch %s: %s", name, hipGetErrorString(e_)); \
    } while (0)

typedef float F2 __attribute__((ext_vector_type(2)));
typedef float F4 __attribute__((ext_vector_type(4)));

enum { CR_S1 = 0, CR_S2 = 1, CR_UP = 2 };     // stride-1 conv, stride-2 conv, stride-2 transposed conv
enum { CR_BN = 0, CR_HEADS = 1 };              // epilogues

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

static int cr_plan(int depth, int cin, int c, int cout, CrPlan* P) {
    if (depth != 2 && depth != 3) return gdb_fail(GDB_E_BADARG, "cost reg: depth %d (2 or 3 are supported)", depth);
    if (cin < 8 || cin > 256 || cin % 8) return gdb_fail(GDB_E_BADARG, "cost reg: in_channels %d (a multiple of 8, at most 256)", cin);
    if (c < 8 || (c << depth) > 128 || c % 8)
        return gdb_fail(GDB_E_BADARG, "cost reg: base_channels %d (a multiple of 8 with base << depth <= 128)", c);
    if (cout < 1 || cout > 15) return gdb_fail(GDB_E_BADARG, "cost reg: out_channels %d (1 .. 15: both heads share one 16-row tile)", cout);
    P->depth = depth; P->cin = cin; P->c = c; P->cout = cout;
    int n = 0;
    auto add = [&](int mode, int ci, int co, int lin, int lout) {
        CrLayer& l = P->L[n];
        l.mode = mode; l.cin = ci; l.cout = co; l.level_in = lin; l.level_out = lout;
        l.nc = (n == 0);
        l.zs = (mode == CR_S1 && co == 8) ? 2 : 1;
        l.taps = l.zs == 2 ? 36 : 27;
        l.e = (l.nc || ci % 16 == 0) ? 4 : 2;
        l.nchunk = l.nc ? (ci + 15) / 16 : ci / (4 * l.e);
        l.rows = l.zs * co;
        l.nmt = (l.rows + 15) / 16;
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
__global__ void __launch_bounds__(256) k_costreg_conv(CrArgs a) {
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
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = co + r;
                const float h = (acc[n][r] - a.ep[a.cout + c]) * a.ep[c] * a.ep[2 * a.cout + c] + a.ep[3 * a.cout + c];
                v[r] = fmaxf(h, 0.f);
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

// softmax over D of the prob head's logits, in place on (B, D, H, W): one thread per (b, y, x), the planes summed in order
__global__ void __launch_bounds__(256) k_costreg_softmax(float* __restrict__ p, int B, int D, size_t HW) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)B * HW) return;
    const size_t b = t / HW, q = t - b * HW;
    float* pb = p + b * D * HW + q;
    float m = pb[0];
    for (int d = 1; d < D; ++d) m = fmaxf(m, pb[d * HW]);
    float s = 0.f;
    for (int d = 0; d < D; ++d) {
        const float e = expf(pb[d * HW] - m);
        pb[d * HW] = e;
        s += e;
    }
    for (int d = 0; d < D; ++d) pb[d * HW] = pb[d * HW] / s;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
extern "C" int gdb_cost_reg_packed_floats(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, size_t* out_floats) {
    if (!out_floats) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    CrPlan P;
    int rc = cr_plan(depth, cin, base_channels, cout, &P);
    if (rc != GDB_OK) return rc;
    *out_floats = P.total;
    return GDB_OK;
}

extern "C" int gdb_pack_cost_reg_weights(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* const* t, float* out) {
    if (!t || !out) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    CrPlan P;
    int rc = cr_plan(depth, cin, base_channels, cout, &P);
    if (rc != GDB_OK) return rc;
    const int nconv = 3 * depth + 1, ntens = 5 * nconv + 3;
    for (int i = 0; i < ntens; ++i)
        if (!t[i]) return gdb_fail(GDB_E_BADARG, "NULL tensor %d of the cost-reg state dict", i);
    const float eps = t[ntens - 1][0];
    memset(out, 0, P.total * sizeof(float));
    for (int li = 0; li < P.nlayers; ++li) {
        const CrLayer& l = P.L[li];
        const bool heads = li == P.nlayers - 1;
        const float* w = heads ? t[5 * nconv] : t[5 * li];
        const float* w2 = heads ? t[5 * nconv + 1] : nullptr;
        float* o = out + l.w_off;
        for (int mt = 0; mt < l.nmt; ++mt)
            for (int tap = 0; tap < l.taps; ++tap)
                for (int cc = 0; cc < l.nchunk; ++cc)
                    for (int ln = 0; ln < 64; ++ln)
                        for (int e = 0; e < l.e; ++e)
                            o[((((size_t)mt * l.taps + tap) * l.nchunk + cc) * 64 + ln) * l.e + e] =
                                cr_weight(l, heads, w, w2, 16 * mt + (ln & 15), cr_ci(l, cc, ln >> 4, e), tap);
        if (heads) continue;
        const float *g = t[5 * li + 1], *bb = t[5 * li + 2], *mean = t[5 * li + 3], *var = t[5 * li + 4];
        float* ep = out + l.ep_off;
        for (int c = 0; c < l.cout; ++c) {
            ep[c] = 1.f / sqrtf(var[c] + eps);
            ep[l.cout + c] = mean[c];
            ep[2 * l.cout + c] = g[c];
            ep[3 * l.cout + c] = bb[c];
        }
    }
    return GDB_OK;
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

extern "C" int gdb_cost_reg_workspace_bytes(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, int32_t B, int32_t D, int32_t H,
                                            int32_t W, size_t* out_bytes) {
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    CrPlan P;
    int rc = cr_plan(depth, cin, base_channels, cout, &P);
    if (rc != GDB_OK) return rc;
    if ((rc = cr_check_shape(P, B, D, H, W)) != GDB_OK) return rc;
    *out_bytes = cr_ws_floats(P, B, D, H, W) * sizeof(float);
    return GDB_OK;
}

template <int MODE, int E, bool NC, int ZS, int EPI>
static int cr_launch(const CrArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((k_costreg_conv<MODE, E, NC, ZS, EPI>), dim3((unsigned)((a.nwaves + 3) / 4)), dim3(256), 0, st, a);
    LAUNCH_CHECK("k_costreg_conv");
    return GDB_OK;
}

// the launch geometry of layer li; GDB_E_SHAPE when the grid would overflow
static int cr_args(const CrPlan& P, int li, int B, int D, int H, int W, CrArgs* pa) {
    const CrLayer& l = P.L[li];
    // After conv0 every stride-1 and every transposed BN layer reads c << (level + 1) channels, a multiple of 16, into at least 16
    // rows: E = 4 at one plane per wave is the only form cr_plan asks for, and the only one built (cr_layer).
    if (li > 0 && li < P.nlayers - 1 && l.mode != CR_S2 && (l.e != 4 || l.zs != 1))
        return gdb_fail(GDB_E_BADARG, "cost reg: layer %d (mode %d, %d -> %d channels) asks for a kernel that is not built (E = %d, %d planes per wave)",
                        li, l.mode, l.cin, l.cout, l.e, l.zs);
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

static int cr_layer(const CrPlan& P, int li, const CrArgs& a, hipStream_t st) {
    const CrLayer& l = P.L[li];
    if (li == P.nlayers - 1) return l.e == 4 ? cr_launch<CR_S1, 4, false, 1, CR_HEADS>(a, st) : cr_launch<CR_S1, 2, false, 1, CR_HEADS>(a, st);
    if (l.nc) return l.zs == 2 ? cr_launch<CR_S1, 4, true, 2, CR_BN>(a, st) : cr_launch<CR_S1, 4, true, 1, CR_BN>(a, st);
    // After conv0 only the stride-2 layers meet 8-channel chunks (cr_args has refused everything else that is not built).
    if (l.mode == CR_S2) return l.e == 4 ? cr_launch<CR_S2, 4, false, 1, CR_BN>(a, st) : cr_launch<CR_S2, 2, false, 1, CR_BN>(a, st);
    return l.mode == CR_S1 ? cr_launch<CR_S1, 4, false, 1, CR_BN>(a, st) : cr_launch<CR_UP, 4, false, 1, CR_BN>(a, st);
}

// mode 1: the whole U-Net with the softmax over D (gdb_cost_reg).  mode 0: up to the prob head's logits, left in d_prob, for the
// cascade stage's fused softmax and depth regression (gdb_cascade.hip).  mode 2: the refusals alone, nothing is launched.
int gdb_cost_reg_run_(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B, int32_t D,
                      int32_t H, int32_t W, const float* d_packed, void* d_ws, size_t ws_bytes, float* d_volume, float* d_prob,
                      int mode, void* stream_) {
    CrPlan P;
    int rc = cr_plan(depth, cin, base_channels, cout, &P);
    if (rc != GDB_OK) return rc;
    if (!d_cost || !d_packed || !d_ws || !d_volume || !d_prob) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if ((rc = cr_check_shape(P, B, D, H, W)) != GDB_OK) return rc;
    const size_t need = cr_ws_floats(P, B, D, H, W) * sizeof(float);
    if (ws_bytes < need) return gdb_fail(GDB_E_WORKSPACE, "cost reg: workspace of %zu bytes, %zu needed", ws_bytes, need);
    // every layer's geometry before the first launch: a refusal launches nothing
    CrArgs A[CR_MAX_LAYERS];
    for (int li = 0; li < P.nlayers; ++li)
        if ((rc = cr_args(P, li, B, D, H, W, &A[li])) != GDB_OK) return rc;
    if (mode == 2) return GDB_OK;
    float* S[4] = {};
    float* T[4] = {};
    float* p = (float*)d_ws;
    for (int l = 0; l <= depth; ++l) {
        const size_t n = cr_level_floats(B, D, H, W, base_channels, l);
        S[l] = p; p += n;
        if (l) { T[l] = p; p += n; }
    }
    auto io = [&](int li, const float* in, float* out, int skip) {
        A[li].in = in; A[li].out = out; A[li].skip = skip;
        A[li].w = d_packed + P.L[li].w_off; A[li].ep = d_packed + P.L[li].ep_off;
    };
    int li = 0;
    io(li++, d_cost, S[0], 0);
    for (int l = 0; l < depth; ++l) {
        io(li++, S[l], T[l + 1], 0);
        io(li++, T[l + 1], S[l + 1], 0);
    }
    for (int l = depth - 1; l >= 0; --l) io(li++, S[l + 1], S[l], 1);   // y = skips.pop() + conv(y), written over that skip
    io(li, S[0], d_volume, 0);
    A[li].prob = d_prob;
    hipStream_t st = (hipStream_t)stream_;
    for (int i = 0; i < P.nlayers; ++i)
        if ((rc = cr_layer(P, i, A[i], st)) != GDB_OK) return rc;
    if (mode == 0) return GDB_OK;
    const size_t HW = (size_t)H * W, n = (size_t)B * HW;
    hipLaunchKernelGGL(k_costreg_softmax, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_prob, B, D, HW);
    LAUNCH_CHECK("k_costreg_softmax");
    return GDB_OK;
}

extern "C" int gdb_cost_reg(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B, int32_t D,
                            int32_t H, int32_t W, const float* d_packed, void* d_ws, size_t ws_bytes, float* d_volume, float* d_prob,
                            void* stream_) {
    return gdb_cost_reg_run_(depth, cin, base_channels, cout, d_cost, B, D, H, W, d_packed, d_ws, ws_bytes, d_volume, d_prob, 1, stream_);
}
