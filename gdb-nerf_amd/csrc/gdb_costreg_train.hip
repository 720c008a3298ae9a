// The cost-regularisation 3-D U-Nets (`_UNet3d`, networks/gdb_nerf/cost_reg_net.py) in TRAINING mode on gfx950: the forward with batch
// statistics and the backward that differentiates through them.  Exact fp32 on v_mfma_f32_16x16x4_f32 throughout.
//
// * Forward, per BN layer: the convolution of gdb_costreg.hip (same body, gdb_costreg_body.h) with the raw epilogue writes z,
//   channel-last, into the caller's saved buffer; k_crt_colsum sums z and z^2 per channel in double, one partial per workgroup, and
//   k_crt_stats_final adds the partials in workgroup order (mean, biased variance, invstd, running statistics, all formed in double
//   and rounded once); k_crt_bnrelu writes relu(gamma * xhat + beta) (+ the skip).  Weights are packed on the device, from the
//   parameters as they are, into the operand order of the convolution body: no host copy of a parameter, no synchronisation.
// * Backward, per layer in reverse: k_crt_colsum<1> (sum dzhat, sum dzhat * xhat in double), k_crt_bnb_final (dbeta, dgamma, the two
//   means), k_crt_bn_dz, then the weight gradient (k_crt_dw) and the data gradient, which is the forward body once more on repacked
//   weights: a stride-1 layer's is CR_S1 with flipped taps and swapped channel roles, a stride-2 layer's CR_UP, a transposed
//   layer's CR_S2.  The in-place skip add of the body sums the two paths into a skip's gradient.  The ReLU mask is recomputed from z
//   with the forward's own expression (ReLU'(0) = 0).
// * k_crt_dw: dW[m, n, tap] = sum over voxels o of P[o, m] * Q[s o + k - 1, n], a GEMM with K = voxels: rows m and columns n on the
//   MFMA tile, four consecutive x of one (b, z, y) row per k-step.  For a convolution P = dz, Q = the layer's input; for a transposed
//   one P = its input (coarse), Q = dz (fine): either way the result is the weight tensor's own layout.  A wave owns one 16 x 16
//   tile, TG of the 27 taps (27 accumulators, or 3) and a slab of rows; it writes one partial.  Two reduction kernels add the
//   partials in slab order in double.  No atomics: two runs are bit-identical.
#include "gdb_costreg_body.h"
#include <cstdio>

template <int MODE, int E, bool NC, int ZS, int EPI>
__global__ void __launch_bounds__(256) k_crt_conv(CrArgs a) { costreg_conv_body<MODE, E, NC, ZS, EPI>(a); }

// ---- weights into the body's operand order, on the device ----------------------------------------------------------------
// element (row, ci, tap) of the GEMM = src[row rs + ci cs + (flip ? 26 - tap : tap)]
struct CrtPack {
    const float* src;
    float* dst;
    long long rs, cs;
    int flip, rows, cout, cin, zs, taps, nchunk, e, nc;
    size_t n;
};
__global__ void __launch_bounds__(256) k_crt_pack(CrtPack p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int el = (int)(i % p.e);
    size_t t = i / p.e;
    const int ln = (int)(t % 64); t /= 64;
    const int cc = (int)(t % p.nchunk); t /= p.nchunk;
    const int tap = (int)(t % p.taps);
    const int mt = (int)(t / p.taps);
    const int row = 16 * mt + (ln & 15), kq = ln >> 4;
    const int ci = p.nc ? 16 * cc + 4 * el + kq : 4 * p.e * cc + p.e * kq + el;
    float v = 0.f;
    if (ci < p.cin && row < p.rows) {
        int co = row, k = tap;
        if (p.zs == 2) {   // rows 8 .. 15: the same channels one plane further (gdb_costreg_body.h, cr_weight)
            const int s = row / p.cout, kz = tap / 9 - s;
            co = row % p.cout;
            k = (kz < 0 || kz > 2) ? -1 : kz * 9 + tap % 9;
        }
        if (k >= 0) v = p.src[(long long)co * p.rs + (long long)ci * p.cs + (p.flip ? 26 - k : k)];
    }
    p.dst[i] = v;
}

// ---- per-channel sums over the voxels, in double ----------------------------------------------------------------------------
struct CrtBn {
    const float* z;        // (N, C) raw convolution output
    const float* dy;       // (N, C) upstream of the BN + ReLU (backward)
    float* out;            // (N, C)
    const float* skip;     // (N, C) or NULL
    const float *mean, *invstd, *gamma, *beta;
    const float* coef;     // backward: mean(dzhat) | mean(dzhat xhat)
    double* part;          // [nblk][2][C]
    size_t N, chunk;
    int C, nblk;
};

__device__ __forceinline__ float crt_xhat(float z, float mean, float invstd) { return (z - mean) * invstd; }
__device__ __forceinline__ float crt_bn(float xh, float g, float b) { return fmaf(xh, g, b); }

// BWD 0: sum z, sum z^2.  BWD 1: sum dzhat, sum dzhat * xhat with dzhat = dy [bn(z) > 0].
template <int BWD>
__global__ void __launch_bounds__(256) k_crt_colsum(CrtBn a) {
    __shared__ double sh[2][256];
    const int t = threadIdx.x, nv = 256 / a.C, c = t % a.C, v = t / a.C;
    double s1 = 0.0, s2 = 0.0;
    if (v < nv) {
        const size_t start = (size_t)blockIdx.x * a.chunk;
        size_t end = start + a.chunk;
        if (end > a.N) end = a.N;
        float mean = 0.f, invstd = 0.f, g = 0.f, b = 0.f;
        if (BWD) { mean = a.mean[c]; invstd = a.invstd[c]; g = a.gamma[c]; b = a.beta[c]; }
        for (size_t vox = start + v; vox < end; vox += nv) {
            const float z = a.z[vox * a.C + c];
            if (BWD) {
                const float xh = crt_xhat(z, mean, invstd);
                const float d = crt_bn(xh, g, b) > 0.f ? a.dy[vox * a.C + c] : 0.f;
                s1 += (double)d;
                s2 += (double)d * (double)xh;
            } else {
                s1 += (double)z;
                s2 += (double)z * (double)z;
            }
        }
    }
    sh[0][t] = s1; sh[1][t] = s2;
    __syncthreads();
    if (t < a.C) {
        double r1 = 0.0, r2 = 0.0;
        for (int q = 0; q < nv; ++q) { r1 += sh[0][q * a.C + t]; r2 += sh[1][q * a.C + t]; }
        a.part[((size_t)blockIdx.x * 2 + 0) * a.C + t] = r1;
        a.part[((size_t)blockIdx.x * 2 + 1) * a.C + t] = r2;
    }
}

struct CrtStats {
    const double* part;
    int nblk, C;
    double n, eps, momentum;
    float *mean, *invstd;            // saved buffer
    float* batch;                    // mean | biased variance (may be NULL)
    float *run_mean, *run_var;       // may be NULL
    long long* tracked;              // may be NULL
};
__global__ void __launch_bounds__(128) k_crt_stats_final(CrtStats a) {
    const int c = threadIdx.x;
    if (c == 0 && a.tracked) *a.tracked += 1;
    if (c >= a.C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < a.nblk; ++b) { s1 += a.part[((size_t)b * 2 + 0) * a.C + c]; s2 += a.part[((size_t)b * 2 + 1) * a.C + c]; }
    const double mean = s1 / a.n;
    double var = s2 / a.n - mean * mean;
    if (!(var > 0.0)) var = 0.0;
    a.mean[c] = (float)mean;
    a.invstd[c] = (float)(1.0 / sqrt(var + a.eps));
    if (a.batch) { a.batch[c] = (float)mean; a.batch[a.C + c] = (float)var; }
    if (a.run_mean) a.run_mean[c] = (float)((1.0 - a.momentum) * (double)a.run_mean[c] + a.momentum * mean);
    if (a.run_var) a.run_var[c] = (float)((1.0 - a.momentum) * (double)a.run_var[c] + a.momentum * var * (a.n / (a.n - 1.0)));
}

struct CrtBnbFinal {
    const double* part;
    int nblk, C;
    double n;
    float *g_gamma, *g_beta, *coef;
};
__global__ void __launch_bounds__(128) k_crt_bnb_final(CrtBnbFinal a) {
    const int c = threadIdx.x;
    if (c >= a.C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < a.nblk; ++b) { s1 += a.part[((size_t)b * 2 + 0) * a.C + c]; s2 += a.part[((size_t)b * 2 + 1) * a.C + c]; }
    a.g_beta[c] = (float)s1;
    a.g_gamma[c] = (float)s2;
    a.coef[c] = (float)(s1 / a.n);
    a.coef[a.C + c] = (float)(s2 / a.n);
}

// out = [skip +] relu(bn(z)); one thread per four channels of a voxel
__global__ void __launch_bounds__(256) k_crt_bnrelu(CrtBn a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N * (size_t)(a.C / 4)) return;
    const int c0 = (int)(i % (size_t)(a.C / 4)) * 4;
    const F4 z = *(const F4*)(a.z + 4 * i);
    F4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(crt_bn(crt_xhat(z[r], a.mean[c0 + r], a.invstd[c0 + r]), a.gamma[c0 + r], a.beta[c0 + r]), 0.f);
    if (a.skip) {
        const F4 s = *(const F4*)(a.skip + 4 * i);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = s[r] + v[r];
    }
    *(F4*)(a.out + 4 * i) = v;
}

// dz = gamma invstd (dzhat - mean(dzhat) - xhat mean(dzhat xhat))
__global__ void __launch_bounds__(256) k_crt_bn_dz(CrtBn a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N * (size_t)(a.C / 4)) return;
    const int c0 = (int)(i % (size_t)(a.C / 4)) * 4;
    const F4 z = *(const F4*)(a.z + 4 * i);
    const F4 dy = *(const F4*)(a.dy + 4 * i);
    F4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = c0 + r;
        const float xh = crt_xhat(z[r], a.mean[c], a.invstd[c]);
        const float d = crt_bn(xh, a.gamma[c], a.beta[c]) > 0.f ? dy[r] : 0.f;
        v[r] = a.gamma[c] * a.invstd[c] * (d - a.coef[c] - xh * a.coef[a.C + c]);
    }
    *(F4*)(a.out + 4 * i) = v;
}

// ---- softmax over D, forward (the logits in place, as k_costreg_softmax) and backward -------------------------------------------
__global__ void __launch_bounds__(256) k_crt_softmax(float* __restrict__ p, int B, int D, size_t HW) {
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
// dlogit = p (g - sum_d g p), written as channel `cout` of the planar upstream u (B, cout + 1, D, H, W)
__global__ void __launch_bounds__(256) k_crt_softmax_bwd(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ u,
                                                          int B, int D, size_t HW, int cout) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)B * HW) return;
    const size_t b = t / HW, q = t - b * HW;
    const float* pb = p + b * D * HW + q;
    const float* gb = g + b * D * HW + q;
    float* ub = u + (b * (cout + 1) + cout) * D * HW + q;
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += (double)gb[d * HW] * (double)pb[d * HW];
    const float sf = (float)s;
    for (int d = 0; d < D; ++d) ub[d * HW] = pb[d * HW] * (gb[d * HW] - sf);
}

// ---- the weight gradient ----------------------------------------------------------------------------------------------------
struct CrtDw {
    const float *P, *Q;    // element (b, voxel, channel) at b xB + voxel xV + channel xM
    float* part;           // [nslab][M][N][27]
    long long pB, pV, pM, qB, qV, qM;
    int M, N, s, Dp, Hp, Wp, Dq, Hq, Wq;
    int nmt, nnt, nslab, rps, rows, nwaves;
};
template <int TG>
__global__ void __launch_bounds__(256) k_crt_dw(CrtDw a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (wave >= a.nwaves) return;
    const int j = lane & 15, kq = lane >> 4;
    int t = wave;
    const int mt = t % a.nmt; t /= a.nmt;
    const int nt = t % a.nnt; t /= a.nnt;
    const int tg = t % (27 / TG);
    const int slab = t / (27 / TG);
    F4 acc[TG];
#pragma unroll
    for (int q = 0; q < TG; ++q) acc[q] = F4{0.f, 0.f, 0.f, 0.f};
    const int m = 16 * mt + j, n = 16 * nt + j;
    const bool mok = m < a.M, nok = n < a.N;
    const int r0 = slab * a.rps;
    const int r1 = r0 + a.rps < a.rows ? r0 + a.rps : a.rows;
    for (int r = r0; r < r1; ++r) {
        const int y = r % a.Hp, z = (r / a.Hp) % a.Dp, b = r / (a.Hp * a.Dp);
        unsigned mask = 0;   // the taps whose input row exists (wave-uniform)
#pragma unroll
        for (int q = 0; q < TG; ++q) {
            const int tap = tg * TG + q, iz = a.s * z + tap / 9 - 1, iy = a.s * y + (tap / 3) % 3 - 1;
            if (iz >= 0 && iz < a.Dq && iy >= 0 && iy < a.Hq) mask |= 1u << q;
        }
        if (!mask) continue;
        const float* prow = a.P + (long long)b * a.pB + ((long long)(z * a.Hp + y) * a.Wp) * a.pV + (long long)m * a.pM;
        const float* qb = a.Q + (long long)b * a.qB + (long long)n * a.qM;
        for (int x0 = 0; x0 < a.Wp; x0 += 4) {
            const int x = x0 + kq;
            const bool xok = x < a.Wp;
            const float av = (mok && xok) ? prow[(long long)x * a.pV] : 0.f;
#pragma unroll
            for (int q = 0; q < TG; ++q) {
                if (!((mask >> q) & 1)) continue;
                const int tap = tg * TG + q, iz = a.s * z + tap / 9 - 1, iy = a.s * y + (tap / 3) % 3 - 1, ix = a.s * x + tap % 3 - 1;
                float bv = 0.f;
                if (nok && xok && ix >= 0 && ix < a.Wq) bv = qb[((long long)(iz * a.Hq + iy) * a.Wq + ix) * a.qV];
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[q], 0, 0, 0);
            }
        }
    }
    // register r of lane (j, kq) = row 4 kq + r, column j of the tile
    float* o = a.part + (size_t)slab * a.M * a.N * 27;
    const int nn = 16 * nt + j;
#pragma unroll
    for (int q = 0; q < TG; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int mm = 16 * mt + 4 * kq + r;
            if (mm < a.M && nn < a.N) o[((size_t)mm * a.N + nn) * 27 + tg * TG + q] = acc[q][r];
        }
}

#define CRT_R1 16   // slabs per first-level group
__global__ void __launch_bounds__(256) k_crt_dw_reduce1(const float* __restrict__ part, double* __restrict__ p2, size_t wn, int nslab, int ng) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= wn * ng) return;
    const size_t g = i / wn, w = i - g * wn;
    const int s1 = (int)g * CRT_R1 + CRT_R1 < nslab ? (int)g * CRT_R1 + CRT_R1 : nslab;
    double s = 0.0;
    for (int q = (int)g * CRT_R1; q < s1; ++q) s += (double)part[(size_t)q * wn + w];
    p2[i] = s;
}
__global__ void __launch_bounds__(256) k_crt_dw_reduce2(const double* __restrict__ p2, float* __restrict__ out, size_t wn, int ng) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= wn) return;
    double s = 0.0;
    for (int g = 0; g < ng; ++g) s += p2[(size_t)g * wn + w];
    out[w] = (float)s;
}

// ---- host: layout ---------------------------------------------------------------------------------------------------------------
#define CRT_MAX_BN 10
#define CRT_MAX_REGIONS 64
#define CRT_STAT_BLOCKS 256
struct CrtLayout {
    int nreg;
    GdbCostRegTrainRegion R[CRT_MAX_REGIONS];
    size_t z[CRT_MAX_BN], out[CRT_MAX_BN], mean[CRT_MAX_BN], invstd[CRT_MAX_BN], prob, packed, wcat, statp;   // saved buffer
    size_t G[4], DZ[4], U, pdx, wcat_b, gcat, bnp, coef, dwp, dwp2;                                          // workspace
    size_t nvox[4];
    size_t saved_bytes, ws_bytes;
};

static size_t crt_add(CrtLayout* L, int buffer, size_t* cursor, const char* name, size_t bytes, int channels, int level) {
    const size_t off = *cursor;
    GdbCostRegTrainRegion& r = L->R[L->nreg++];
    memset(&r, 0, sizeof r);
    snprintf(r.name, sizeof r.name, "%s", name);
    r.offset = off; r.bytes = bytes; r.buffer = buffer; r.channels = channels; r.level = level;
    *cursor = (off + bytes + 255) / 256 * 256;
    return off;
}

// the weight gradient's split: TG taps per wave, slabs of output rows
static void crt_dw_plan(int M, int N, int rows, int* tg, int* nslab, int* rps) {
    const long long tiles = (long long)((M + 15) / 16) * ((N + 15) / 16);
    *tg = tiles * rows >= 1024 ? 27 : 3;
    const long long per = tiles * (27 / *tg);
    long long ns = (1024 + per - 1) / per;
    if (ns > 256) ns = 256;
    if (ns > rows) ns = rows;
    if (ns < 1) ns = 1;
    *rps = (int)((rows + ns - 1) / ns);
    *nslab = (rows + *rps - 1) / *rps;
}

// M, N and the level of P's grid of layer li's weight gradient (li == nlayers - 1: the heads)
static void crt_dw_dims(const CrPlan& P, int li, int* M, int* N, int* level) {
    const CrLayer& l = P.L[li];
    if (li == P.nlayers - 1) { *M = P.cout + 1; *N = l.cin; *level = 0; return; }
    *M = l.mode == CR_UP ? l.cin : l.cout;
    *N = l.mode == CR_UP ? l.cout : l.cin;
    *level = l.level_in > l.level_out ? l.level_in : l.level_out;
}

// the data gradient of forward layer li as a layer of the body (li >= 1; li == nlayers - 1: the heads, from the planar upstream)
static void crt_dx_layer(const CrPlan& P, int li, CrLayer* d) {
    const CrLayer& l = P.L[li];
    if (li == P.nlayers - 1) cr_layer_set(*d, CR_S1, P.cout + 1, l.cin, 0, 0, 1);
    else if (l.mode == CR_S1) cr_layer_set(*d, CR_S1, l.cout, l.cin, l.level_out, l.level_in, 0);
    else if (l.mode == CR_S2) cr_layer_set(*d, CR_UP, l.cout, l.cin, l.level_out, l.level_in, 0);
    else cr_layer_set(*d, CR_S2, l.cout, l.cin, l.level_out, l.level_in, 0);
}
static size_t crt_packed_floats(const CrLayer& l) { return (size_t)l.nmt * l.taps * l.nchunk * 64 * l.e; }
// the data gradient of conv0 - the cost volume's gradient - as a layer of the body: stride 1, flipped taps, roles swapped, base -> cin
// channels, channel-last in and out; one plane per wave whatever cin (an 8-channel result fills half a 16-row tile)
static void crt_dx0_layer(const CrPlan& P, CrLayer* d) {
    cr_layer_set(*d, CR_S1, P.c, P.cin, 0, 0, 0);
    d->zs = 1; d->taps = 27; d->rows = P.cin; d->nmt = (P.cin + 15) / 16;
}
// the scratch of the cost volume's gradient: conv0's repacked weights, then the gradient channel-last (B, D, H, W, cin)
// (the weights stand at offset 0)
struct CrtCostWs { size_t grad_off, total; };
static CrtCostWs crt_cost_ws(const CrPlan& P, size_t nvox0) {
    CrLayer d;
    crt_dx0_layer(P, &d);
    CrtCostWs w;
    w.grad_off = (crt_packed_floats(d) * sizeof(float) + 255) / 256 * 256;
    w.total = (w.grad_off + nvox0 * P.cin * sizeof(float) + 255) / 256 * 256;
    return w;
}

static int crt_layout(const CrPlan& P, int B, int D, int H, int W, CrtLayout* L) {
    int rc = cr_check_shape(P, B, D, H, W);
    if (rc != GDB_OK) return rc;
    for (int l = 0; l <= P.depth; ++l) L->nvox[l] = (size_t)B * (D >> l) * (H >> l) * (W >> l);
    if (L->nvox[P.depth] == 1)
        return gdb_fail(GDB_E_SHAPE, "cost reg train: one value per channel at level %d (B=%d D=%d H=%d W=%d): batch statistics need more", P.depth, B, D, H, W);
    if (L->nvox[0] * (size_t)(P.c / 4) / 256 >= (1u << 31) - 1 || (size_t)B * D * H >= (1u << 30))
        return gdb_fail(GDB_E_SHAPE, "cost reg train: volume too large for the launch grid");
    L->nreg = 0;
    const int nbn = P.nlayers - 1;
    char name[32];
    size_t o = 0;
    for (int i = 0; i < nbn; ++i) {
        const CrLayer& l = P.L[i];
        const size_t n = L->nvox[l.level_out] * l.cout * sizeof(float);
        snprintf(name, sizeof name, "conv%d.z", i);      L->z[i] = crt_add(L, 0, &o, name, n, l.cout, l.level_out);
        snprintf(name, sizeof name, "conv%d.out", i);    L->out[i] = crt_add(L, 0, &o, name, n, l.cout, l.level_out);
        snprintf(name, sizeof name, "conv%d.mean", i);   L->mean[i] = crt_add(L, 0, &o, name, l.cout * sizeof(float), l.cout, -1);
        snprintf(name, sizeof name, "conv%d.invstd", i); L->invstd[i] = crt_add(L, 0, &o, name, l.cout * sizeof(float), l.cout, -1);
    }
    L->prob = crt_add(L, 0, &o, "prob", L->nvox[0] * sizeof(float), 1, 0);
    L->packed = crt_add(L, 0, &o, "packed", P.total * sizeof(float), 0, -1);
    L->wcat = crt_add(L, 0, &o, "heads.weight", (size_t)(P.cout + 1) * P.c * 27 * sizeof(float), P.c, -1);
    L->statp = crt_add(L, 0, &o, "stat_partials", (size_t)CRT_STAT_BLOCKS * 2 * 128 * sizeof(double), 0, -1);
    L->saved_bytes = o;
    o = 0;
    for (int l = 0; l <= P.depth; ++l) {
        const size_t n = L->nvox[l] * (P.c << l) * sizeof(float);
        snprintf(name, sizeof name, "grad.l%d", l); L->G[l] = crt_add(L, 1, &o, name, n, P.c << l, l);
        snprintf(name, sizeof name, "dz.l%d", l);   L->DZ[l] = crt_add(L, 1, &o, name, n, P.c << l, l);
    }
    L->U = crt_add(L, 1, &o, "upstream", L->nvox[0] * (P.cout + 1) * sizeof(float), P.cout + 1, 0);
    size_t pdx = 0, dwp = 0, dwp2 = 0;
    for (int i = 0; i < P.nlayers; ++i) {
        if (i > 0) {
            CrLayer d;
            crt_dx_layer(P, i, &d);
            const size_t n = crt_packed_floats(d);
            pdx = n > pdx ? n : pdx;
        }
        int M, N, level, tg, nslab, rps;
        crt_dw_dims(P, i, &M, &N, &level);
        crt_dw_plan(M, N, B * (D >> level) * (H >> level), &tg, &nslab, &rps);
        const size_t wn = (size_t)M * N * 27, n1 = wn * nslab, n2 = wn * ((nslab + CRT_R1 - 1) / CRT_R1);
        dwp = n1 > dwp ? n1 : dwp;
        dwp2 = n2 > dwp2 ? n2 : dwp2;
    }
    L->pdx = crt_add(L, 1, &o, "packed_dx", pdx * sizeof(float), 0, -1);
    L->wcat_b = crt_add(L, 1, &o, "heads.weight_bwd", (size_t)(P.cout + 1) * P.c * 27 * sizeof(float), P.c, -1);
    L->gcat = crt_add(L, 1, &o, "heads.weight_grad", (size_t)(P.cout + 1) * P.c * 27 * sizeof(float), P.c, -1);
    L->bnp = crt_add(L, 1, &o, "bn_partials", (size_t)CRT_STAT_BLOCKS * 2 * 128 * sizeof(double), 0, -1);
    L->coef = crt_add(L, 1, &o, "bn_means", 2 * 128 * sizeof(float), 0, -1);
    L->dwp = crt_add(L, 1, &o, "dw_partials", dwp * sizeof(float), 0, -1);
    L->dwp2 = crt_add(L, 1, &o, "dw_partials2", dwp2 * sizeof(double), 0, -1);
    L->ws_bytes = o;
    return GDB_OK;
}

extern "C" int gdb_cost_reg_train_layout(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, int32_t B, int32_t D, int32_t H,
                                         int32_t W, GdbCostRegTrainRegion* out, int32_t capacity, int32_t* out_count, size_t* saved_bytes,
                                         size_t* ws_bytes) {
    CrPlan P;
    int rc = cr_plan(depth, cin, base_channels, cout, &P);
    if (rc != GDB_OK) return rc;
    CrtLayout L;
    if ((rc = crt_layout(P, B, D, H, W, &L)) != GDB_OK) return rc;
    if (out_count) *out_count = L.nreg;
    if (saved_bytes) *saved_bytes = L.saved_bytes;
    if (ws_bytes) *ws_bytes = L.ws_bytes;
    if (out) {
        if (capacity < L.nreg) return gdb_fail(GDB_E_BADARG, "cost reg train: %d regions, room for %d", L.nreg, capacity);
        memcpy(out, L.R, L.nreg * sizeof(GdbCostRegTrainRegion));
    }
    return GDB_OK;
}

// ---- host: launches ---------------------------------------------------------------------------------------------------------------
template <int MODE, int E, bool NC, int ZS, int EPI>
static int crt_launch(const CrArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((k_crt_conv<MODE, E, NC, ZS, EPI>), dim3((unsigned)((a.nwaves + 3) / 4)), dim3(256), 0, st, a);
    LAUNCH_CHECK("k_crt_conv");
    return GDB_OK;
}

// is the raw-epilogue form of this layer built?  (checked for every layer, forward and data gradient, before the first launch)
static bool crt_conv_built(const CrLayer& l) {
    if (l.nc) return l.mode == CR_S1 && l.e == 4;
    if (l.mode == CR_S2) return l.zs == 1;
    if (l.mode == CR_S1) return l.zs == 1;   // (E = 2: a stride-1 layer that reads 8 or 24 channels - conv0's data gradient)
    return l.e == 4 && l.zs == 1;
}
static int crt_conv(const CrLayer& l, const CrArgs& a, hipStream_t st) {
    if (l.nc) return l.zs == 2 ? crt_launch<CR_S1, 4, true, 2, CR_RAW>(a, st) : crt_launch<CR_S1, 4, true, 1, CR_RAW>(a, st);
    if (l.mode == CR_S2) return l.e == 4 ? crt_launch<CR_S2, 4, false, 1, CR_RAW>(a, st) : crt_launch<CR_S2, 2, false, 1, CR_RAW>(a, st);
    if (l.mode == CR_S1) return l.e == 4 ? crt_launch<CR_S1, 4, false, 1, CR_RAW>(a, st) : crt_launch<CR_S1, 2, false, 1, CR_RAW>(a, st);
    return crt_launch<CR_UP, 4, false, 1, CR_RAW>(a, st);
}

static int crt_pack(const CrLayer& l, const float* src, long long rs, long long cs, int flip, float* dst, hipStream_t st) {
    CrtPack p;
    p.src = src; p.dst = dst; p.rs = rs; p.cs = cs; p.flip = flip;
    p.rows = l.rows; p.cout = l.cout; p.cin = l.cin; p.zs = l.zs; p.taps = l.taps; p.nchunk = l.nchunk; p.e = l.e; p.nc = l.nc;
    p.n = crt_packed_floats(l);
    hipLaunchKernelGGL(k_crt_pack, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, st, p);
    LAUNCH_CHECK("k_crt_pack");
    return GDB_OK;
}

static void crt_bn_grid(CrtBn* a, size_t N, int C) {
    a->N = N; a->C = C;
    const size_t nv = 256 / C;
    size_t nblk = (N + 4 * nv - 1) / (4 * nv);
    if (nblk > CRT_STAT_BLOCKS) nblk = CRT_STAT_BLOCKS;
    if (nblk < 1) nblk = 1;
    a->chunk = (N + nblk - 1) / nblk;
    a->nblk = (int)((N + a->chunk - 1) / a->chunk);
}
static unsigned crt_elem_blocks(size_t N, int C) { return (unsigned)((N * (size_t)(C / 4) + 255) / 256); }

static int crt_dw(const CrPlan& P, int li, const CrtLayout& L, int B, int D, int H, int W, const float* Pp, int p_planar, const float* Qp,
                  int q_planar, char* ws, float* out, hipStream_t st) {
    int M, N, level, tg;
    CrtDw a;
    crt_dw_dims(P, li, &M, &N, &level);
    a.M = M; a.N = N;
    a.Dp = D >> level; a.Hp = H >> level; a.Wp = W >> level;
    a.rows = B * a.Dp * a.Hp;
    crt_dw_plan(M, N, a.rows, &tg, &a.nslab, &a.rps);
    const CrLayer& l = P.L[li];
    const int qlevel = l.level_in < l.level_out ? l.level_in : l.level_out;
    a.s = l.level_in == l.level_out ? 1 : 2;
    a.Dq = D >> qlevel; a.Hq = H >> qlevel; a.Wq = W >> qlevel;
    const long long pv = (long long)a.Dp * a.Hp * a.Wp, qv = (long long)a.Dq * a.Hq * a.Wq;
    a.pB = pv * M; a.pV = p_planar ? 1 : M; a.pM = p_planar ? pv : 1;
    a.qB = qv * N; a.qV = q_planar ? 1 : N; a.qM = q_planar ? qv : 1;
    a.P = Pp; a.Q = Qp;
    a.part = (float*)(ws + L.dwp);
    a.nmt = (M + 15) / 16; a.nnt = (N + 15) / 16;
    a.nwaves = a.nmt * a.nnt * (27 / tg) * a.nslab;
    const dim3 grid((unsigned)((a.nwaves + 3) / 4));
    if (tg == 27) hipLaunchKernelGGL(k_crt_dw<27>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_crt_dw<3>, grid, dim3(256), 0, st, a);
    LAUNCH_CHECK("k_crt_dw");
    const size_t wn = (size_t)M * N * 27;
    const int ng = (a.nslab + CRT_R1 - 1) / CRT_R1;
    double* p2 = (double*)(ws + L.dwp2);
    hipLaunchKernelGGL(k_crt_dw_reduce1, dim3((unsigned)((wn * ng + 255) / 256)), dim3(256), 0, st, a.part, p2, wn, a.nslab, ng);
    LAUNCH_CHECK("k_crt_dw_reduce1");
    hipLaunchKernelGGL(k_crt_dw_reduce2, dim3((unsigned)((wn + 255) / 256)), dim3(256), 0, st, p2, out, wn, ng);
    LAUNCH_CHECK("k_crt_dw_reduce2");
    return GDB_OK;
}

#define HIP_OK(call, what)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) return gdb_fail(GDB_E_HIP, "%s: %s", what, hipGetErrorString(e_)); \
    } while (0)

// source strides of forward layer li's weights as GEMM (row = output channel, ci = input channel)
static void crt_fwd_strides(const CrLayer& l, long long* rs, long long* cs) {
    if (l.mode == CR_UP) { *rs = 27; *cs = (long long)l.cout * 27; }   // (cin, cout, 3, 3, 3)
    else { *rs = (long long)l.cin * 27; *cs = 27; }                    // (cout, cin, 3, 3, 3)
}

extern "C" int gdb_cost_reg_train(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B, int32_t D,
                                  int32_t H, int32_t W, const void* const* d_params, float eps, float momentum, void* d_saved,
                                  size_t saved_bytes, float* d_volume, float* d_prob, float* d_batch_stats, void* stream_) {
    CrPlan P;
    int rc = cr_plan(depth, cin, base_channels, cout, &P);
    if (rc != GDB_OK) return rc;
    if (!d_cost || !d_params || !d_saved || !d_volume || !d_prob) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    const int nbn = P.nlayers - 1;
    for (int i = 0; i < nbn; ++i)
        for (int k = 0; k < 3; ++k)
            if (!d_params[6 * i + k]) return gdb_fail(GDB_E_BADARG, "cost reg train: NULL parameter %d of conv%d", k, i);
    if (!d_params[6 * nbn] || !d_params[6 * nbn + 1]) return gdb_fail(GDB_E_BADARG, "cost reg train: NULL head weight");
    CrtLayout L;
    if ((rc = crt_layout(P, B, D, H, W, &L)) != GDB_OK) return rc;
    if (saved_bytes < L.saved_bytes) return gdb_fail(GDB_E_WORKSPACE, "cost reg train: saved buffer of %zu bytes, %zu needed", saved_bytes, L.saved_bytes);
    CrArgs A[CR_MAX_LAYERS];
    for (int li = 0; li < P.nlayers; ++li) {
        if ((rc = cr_args(P, li, B, D, H, W, &A[li])) != GDB_OK) return rc;
        if (li < nbn && !crt_conv_built(P.L[li])) return gdb_fail(GDB_E_BADARG, "cost reg train: layer %d asks for a kernel that is not built", li);
    }
    hipStream_t st = (hipStream_t)stream_;
    char* sv = (char*)d_saved;
    float* packed = (float*)(sv + L.packed);
    float* wcat = (float*)(sv + L.wcat);
    const size_t nfeat = (size_t)cout * base_channels * 27, nprob = (size_t)base_channels * 27;
    HIP_OK(hipMemcpyAsync(wcat, d_params[6 * nbn], nfeat * sizeof(float), hipMemcpyDeviceToDevice, st), "copy feat_head.weight");
    HIP_OK(hipMemcpyAsync(wcat + nfeat, d_params[6 * nbn + 1], nprob * sizeof(float), hipMemcpyDeviceToDevice, st), "copy prob_head.weight");
    for (int li = 0; li < P.nlayers; ++li) {
        const CrLayer& l = P.L[li];
        long long rs, cs;
        crt_fwd_strides(l, &rs, &cs);
        if ((rc = crt_pack(l, li == nbn ? wcat : (const float*)d_params[6 * li], rs, cs, 0, packed + l.w_off, st)) != GDB_OK) return rc;
    }
    size_t stat_off = 0;
    for (int li = 0; li < nbn; ++li) {
        const CrLayer& l = P.L[li];
        float* z = (float*)(sv + L.z[li]);
        float* out = (float*)(sv + L.out[li]);
        A[li].in = li == 0 ? d_cost : (const float*)(sv + L.out[li - 1]);
        A[li].out = z; A[li].skip = 0; A[li].w = packed + l.w_off; A[li].ep = nullptr;
        if ((rc = crt_conv(l, A[li], st)) != GDB_OK) return rc;
        CrtBn b = {};
        crt_bn_grid(&b, L.nvox[l.level_out], l.cout);
        b.z = z; b.out = out; b.part = (double*)(sv + L.statp);
        b.mean = (float*)(sv + L.mean[li]); b.invstd = (float*)(sv + L.invstd[li]);
        b.gamma = (const float*)d_params[6 * li + 1]; b.beta = (const float*)d_params[6 * li + 2];
        if (l.mode == CR_UP) b.skip = (const float*)(sv + L.out[l.level_out == 0 ? 0 : 2 * l.level_out]);   // skips.pop() + conv(y)
        hipLaunchKernelGGL(k_crt_colsum<0>, dim3((unsigned)b.nblk), dim3(256), 0, st, b);
        LAUNCH_CHECK("k_crt_colsum");
        CrtStats s = {};
        s.part = b.part; s.nblk = b.nblk; s.C = l.cout; s.n = (double)b.N; s.eps = (double)eps; s.momentum = (double)momentum;
        s.mean = (float*)(sv + L.mean[li]); s.invstd = (float*)(sv + L.invstd[li]);
        s.batch = d_batch_stats ? d_batch_stats + stat_off : nullptr;
        s.run_mean = (float*)d_params[6 * li + 3]; s.run_var = (float*)d_params[6 * li + 4]; s.tracked = (long long*)d_params[6 * li + 5];
        stat_off += 2 * (size_t)l.cout;
        hipLaunchKernelGGL(k_crt_stats_final, dim3(1), dim3(128), 0, st, s);
        LAUNCH_CHECK("k_crt_stats_final");
        hipLaunchKernelGGL(k_crt_bnrelu, dim3(crt_elem_blocks(b.N, b.C)), dim3(256), 0, st, b);
        LAUNCH_CHECK("k_crt_bnrelu");
    }
    {
        const CrLayer& l = P.L[nbn];
        A[nbn].in = (const float*)(sv + L.out[nbn - 1]);
        A[nbn].out = d_volume; A[nbn].prob = d_prob; A[nbn].skip = 0; A[nbn].w = packed + l.w_off; A[nbn].ep = nullptr;
        rc = l.e == 4 ? crt_launch<CR_S1, 4, false, 1, CR_HEADS>(A[nbn], st) : crt_launch<CR_S1, 2, false, 1, CR_HEADS>(A[nbn], st);
        if (rc != GDB_OK) return rc;
    }
    const size_t HW = (size_t)H * W, n = (size_t)B * HW;
    hipLaunchKernelGGL(k_crt_softmax, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_prob, B, D, HW);
    LAUNCH_CHECK("k_crt_softmax");
    HIP_OK(hipMemcpyAsync(sv + L.prob, d_prob, L.nvox[0] * sizeof(float), hipMemcpyDeviceToDevice, st), "save prob");
    return GDB_OK;
}

// channel-last (B, n, C) -> planar (B, C, n): one lane per output element
__global__ void __launch_bounds__(256) k_crt_to_planar(const float* __restrict__ in, float* __restrict__ out, size_t n, int C, size_t total) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const size_t bc = t / n, p = t - bc * n, b = bc / C, c = bc - b * C;
    out[t] = in[(b * n + p) * C + c];
}

extern "C" int gdb_cost_reg_train_cost_grad_bytes(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, int32_t B, int32_t D,
                                                  int32_t H, int32_t W, size_t* out_bytes) {
    CrPlan P;
    int rc = cr_plan(depth, cin, base_channels, cout, &P);
    if (rc != GDB_OK) return rc;
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "out_bytes is NULL");
    CrtLayout L;
    if ((rc = crt_layout(P, B, D, H, W, &L)) != GDB_OK) return rc;
    *out_bytes = crt_cost_ws(P, L.nvox[0]).total;
    return GDB_OK;
}

static int crt_backward(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B,
                        int32_t D, int32_t H, int32_t W, const void* const* d_params, const float* d_g_volume,
                        const float* d_g_prob, const void* d_saved, size_t saved_bytes, void* d_ws, size_t ws_bytes,
                        float* const* d_grads, float* d_g_cost, void* d_cost_ws, size_t cost_ws_bytes, void* stream_);

extern "C" int gdb_cost_reg_train_backward(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B,
                                           int32_t D, int32_t H, int32_t W, const void* const* d_params, const float* d_g_volume,
                                           const float* d_g_prob, const void* d_saved, size_t saved_bytes, void* d_ws, size_t ws_bytes,
                                           float* const* d_grads, void* stream_) {
    return crt_backward(depth, cin, base_channels, cout, d_cost, B, D, H, W, d_params, d_g_volume, d_g_prob, d_saved, saved_bytes, d_ws, ws_bytes,
                        d_grads, nullptr, nullptr, 0, stream_);
}

extern "C" int gdb_cost_reg_train_backward_cost(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B,
                                                int32_t D, int32_t H, int32_t W, const void* const* d_params, const float* d_g_volume,
                                                const float* d_g_prob, const void* d_saved, size_t saved_bytes, void* d_ws, size_t ws_bytes,
                                                float* const* d_grads, float* d_g_cost, void* d_cost_ws, size_t cost_ws_bytes, void* stream_) {
    return crt_backward(depth, cin, base_channels, cout, d_cost, B, D, H, W, d_params, d_g_volume, d_g_prob, d_saved, saved_bytes, d_ws, ws_bytes,
                        d_grads, d_g_cost, d_cost_ws, cost_ws_bytes, stream_);
}

static int crt_backward(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B,
                        int32_t D, int32_t H, int32_t W, const void* const* d_params, const float* d_g_volume,
                        const float* d_g_prob, const void* d_saved, size_t saved_bytes, void* d_ws, size_t ws_bytes,
                        float* const* d_grads, float* d_g_cost, void* d_cost_ws, size_t cost_ws_bytes, void* stream_) {
    CrPlan P;
    int rc = cr_plan(depth, cin, base_channels, cout, &P);
    if (rc != GDB_OK) return rc;
    if (!d_cost || !d_params || !d_saved || !d_ws || !d_grads) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    const int nbn = P.nlayers - 1;
    for (int i = 0; i < nbn; ++i)
        for (int k = 0; k < 3; ++k)
            if (!d_params[6 * i + k] || !d_grads[3 * i + k]) return gdb_fail(GDB_E_BADARG, "cost reg train: NULL parameter or gradient %d of conv%d", k, i);
    if (!d_params[6 * nbn] || !d_params[6 * nbn + 1] || !d_grads[3 * nbn] || !d_grads[3 * nbn + 1])
        return gdb_fail(GDB_E_BADARG, "cost reg train: NULL head weight or gradient");
    CrtLayout L;
    if ((rc = crt_layout(P, B, D, H, W, &L)) != GDB_OK) return rc;
    if (saved_bytes < L.saved_bytes) return gdb_fail(GDB_E_WORKSPACE, "cost reg train: saved buffer of %zu bytes, %zu needed", saved_bytes, L.saved_bytes);
    if (ws_bytes < L.ws_bytes) return gdb_fail(GDB_E_WORKSPACE, "cost reg train: workspace of %zu bytes, %zu needed", ws_bytes, L.ws_bytes);
    CrLayer DX[CR_MAX_LAYERS];
    CrArgs A[CR_MAX_LAYERS];
    for (int li = 1; li < P.nlayers; ++li) {
        crt_dx_layer(P, li, &DX[li]);
        if (!crt_conv_built(DX[li])) return gdb_fail(GDB_E_BADARG, "cost reg train: the data gradient of layer %d asks for a kernel that is not built", li);
        if ((rc = cr_geom(DX[li], B, D, H, W, &A[li])) != GDB_OK) return rc;
    }
    CrtCostWs CW = {};
    if (d_g_cost) {   // the cost volume's gradient: conv0's data gradient, out of a scratch of its own
        CW = crt_cost_ws(P, L.nvox[0]);
        if (!d_cost_ws) return gdb_fail(GDB_E_BADARG, "cost reg train: the cost volume's gradient needs its scratch");
        if (cost_ws_bytes < CW.total) return gdb_fail(GDB_E_WORKSPACE, "cost reg train: cost-gradient scratch of %zu bytes, %zu needed", cost_ws_bytes, CW.total);
        crt_dx0_layer(P, &DX[0]);
        if (!crt_conv_built(DX[0])) return gdb_fail(GDB_E_BADARG, "cost reg train: the data gradient of layer 0 asks for a kernel that is not built");
        if ((rc = cr_geom(DX[0], B, D, H, W, &A[0])) != GDB_OK) return rc;
        if (L.nvox[0] * (size_t)cin / 256 >= (1u << 31) - 1) return gdb_fail(GDB_E_SHAPE, "cost reg train: volume too large for the launch grid");
    }
    hipStream_t st = (hipStream_t)stream_;
    const char* sv = (const char*)d_saved;
    char* ws = (char*)d_ws;
    float* pdx = (float*)(ws + L.pdx);
    float* G[4];
    float* DZ[4];
    for (int l = 0; l <= depth; ++l) { G[l] = (float*)(ws + L.G[l]); DZ[l] = (float*)(ws + L.DZ[l]); }
    const size_t nv0 = L.nvox[0], HW = (size_t)H * W;
    const size_t nfeat = (size_t)cout * base_channels * 27, nprob = (size_t)base_channels * 27;

    // the heads: upstream (B, cout + 1, D, H, W) = [g_volume | softmax backward of g_prob]
    float* U = (float*)(ws + L.U);
    for (int b = 0; b < B; ++b) {
        float* ub = U + (size_t)b * (cout + 1) * (nv0 / B);
        if (d_g_volume) HIP_OK(hipMemcpyAsync(ub, d_g_volume + (size_t)b * cout * (nv0 / B), (size_t)cout * (nv0 / B) * sizeof(float), hipMemcpyDeviceToDevice, st), "copy g_volume");
        else HIP_OK(hipMemsetAsync(ub, 0, (size_t)cout * (nv0 / B) * sizeof(float), st), "zero g_volume");
        if (!d_g_prob) HIP_OK(hipMemsetAsync(ub + (size_t)cout * (nv0 / B), 0, (nv0 / B) * sizeof(float), st), "zero g_prob");
    }
    if (d_g_prob) {
        const size_t n = (size_t)B * HW;
        hipLaunchKernelGGL(k_crt_softmax_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)(sv + L.prob), d_g_prob, U, B, D, HW, cout);
        LAUNCH_CHECK("k_crt_softmax_bwd");
    }
    float* wcat = (float*)(ws + L.wcat_b);
    float* gcat = (float*)(ws + L.gcat);
    HIP_OK(hipMemcpyAsync(wcat, d_params[6 * nbn], nfeat * sizeof(float), hipMemcpyDeviceToDevice, st), "copy feat_head.weight");
    HIP_OK(hipMemcpyAsync(wcat + nfeat, d_params[6 * nbn + 1], nprob * sizeof(float), hipMemcpyDeviceToDevice, st), "copy prob_head.weight");
    const float* y_last = (const float*)(sv + L.out[nbn - 1]);
    if ((rc = crt_dw(P, nbn, L, B, D, H, W, U, 1, y_last, 0, ws, gcat, st)) != GDB_OK) return rc;
    HIP_OK(hipMemcpyAsync(d_grads[3 * nbn], gcat, nfeat * sizeof(float), hipMemcpyDeviceToDevice, st), "copy feat_head gradient");
    HIP_OK(hipMemcpyAsync(d_grads[3 * nbn + 1], gcat + nfeat, nprob * sizeof(float), hipMemcpyDeviceToDevice, st), "copy prob_head gradient");
    // data gradient: element (row = base channel r, ci = head row q, tap) = wcat[q][r][26 - tap]
    if ((rc = crt_pack(DX[nbn], wcat, 27, (long long)base_channels * 27, 1, pdx, st)) != GDB_OK) return rc;
    A[nbn].in = U; A[nbn].out = G[0]; A[nbn].skip = 0; A[nbn].w = pdx; A[nbn].ep = nullptr;
    if ((rc = crt_conv(DX[nbn], A[nbn], st)) != GDB_OK) return rc;

    // the BN layers in reverse.  The gradient of layer li's output is in G[level_out]: the up layers left the skips' share there
    // and each stride-2 layer's data gradient is added to it in place.
    for (int li = nbn - 1; li >= 0; --li) {
        const CrLayer& l = P.L[li];
        const int lo = l.level_out;
        CrtBn b = {};
        crt_bn_grid(&b, L.nvox[lo], l.cout);
        b.z = (const float*)(sv + L.z[li]); b.dy = G[lo]; b.out = DZ[lo];
        b.mean = (const float*)(sv + L.mean[li]); b.invstd = (const float*)(sv + L.invstd[li]);
        b.gamma = (const float*)d_params[6 * li + 1]; b.beta = (const float*)d_params[6 * li + 2];
        b.part = (double*)(ws + L.bnp); b.coef = (const float*)(ws + L.coef);
        hipLaunchKernelGGL(k_crt_colsum<1>, dim3((unsigned)b.nblk), dim3(256), 0, st, b);
        LAUNCH_CHECK("k_crt_colsum");
        CrtBnbFinal f = {};
        f.part = b.part; f.nblk = b.nblk; f.C = l.cout; f.n = (double)b.N;
        f.g_gamma = d_grads[3 * li + 1]; f.g_beta = d_grads[3 * li + 2]; f.coef = (float*)(ws + L.coef);
        hipLaunchKernelGGL(k_crt_bnb_final, dim3(1), dim3(128), 0, st, f);
        LAUNCH_CHECK("k_crt_bnb_final");
        hipLaunchKernelGGL(k_crt_bn_dz, dim3(crt_elem_blocks(b.N, b.C)), dim3(256), 0, st, b);
        LAUNCH_CHECK("k_crt_bn_dz");
        const float* in = li == 0 ? d_cost : (const float*)(sv + L.out[li - 1]);
        // a convolution: P = dz, Q = its input; a transposed one: P = its input, Q = dz
        if (l.mode == CR_UP) rc = crt_dw(P, li, L, B, D, H, W, in, 0, DZ[lo], 0, ws, d_grads[3 * li], st);
        else rc = crt_dw(P, li, L, B, D, H, W, DZ[lo], 0, in, li == 0, ws, d_grads[3 * li], st);
        if (rc != GDB_OK) return rc;
        if (li == 0) {
            if (!d_g_cost) break;   // the cost volume's gradient is not asked for
            // row = input channel ci, k = output channel co of conv0's (co, ci, tap) weights, flipped; channel-last, then planar
            float* p0 = (float*)d_cost_ws;
            float* gcl = (float*)((char*)d_cost_ws + CW.grad_off);
            if ((rc = crt_pack(DX[0], (const float*)d_params[0], 27, (long long)l.cin * 27, 1, p0, st)) != GDB_OK) return rc;
            A[0].in = DZ[0]; A[0].out = gcl; A[0].skip = 0; A[0].w = p0; A[0].ep = nullptr;
            if ((rc = crt_conv(DX[0], A[0], st)) != GDB_OK) return rc;
            const size_t total = L.nvox[0] * (size_t)cin;
            hipLaunchKernelGGL(k_crt_to_planar, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, gcl, d_g_cost, L.nvox[0] / B, cin, total);
            LAUNCH_CHECK("k_crt_to_planar");
            break;
        }
        const float* w = (const float*)d_params[6 * li];
        int skip = 0;
        if (l.mode == CR_S1) rc = crt_pack(DX[li], w, 27, (long long)l.cin * 27, 1, pdx, st);         // row = ci, k = co, flipped
        else if (l.mode == CR_S2) { rc = crt_pack(DX[li], w, 27, (long long)l.cin * 27, 0, pdx, st); skip = 1; }   // CR_UP over (co, ci, tap)
        else rc = crt_pack(DX[li], w, (long long)l.cout * 27, 27, 0, pdx, st);                        // CR_S2 over (ci, co, tap)
        if (rc != GDB_OK) return rc;
        A[li].in = DZ[lo]; A[li].out = G[l.level_in]; A[li].skip = skip; A[li].w = pdx; A[li].ep = nullptr;
        if ((rc = crt_conv(DX[li], A[li], st)) != GDB_OK) return rc;
    }
    return GDB_OK;
}
