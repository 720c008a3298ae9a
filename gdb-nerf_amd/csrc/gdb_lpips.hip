// LPIPS with the VGG-16 backbone (lpips.LPIPS(net='vgg'), eval mode, spatial=False, as of release 0.1.4) as HIP kernels for gfx950,
// from caller-supplied weights, so that the evaluator's third metric leaves one double per frame on the device like the other two.
// The `lpips` package is not available to this project: the definition below is the contract, pinned by tests/test_lpips_referee.py
// with random weights; agreement with the package's published weights and values is unverified.
//
// Definition.  For two images a, b with values in [0, 1], shape (3, h, w):
//   1. scaling layer: x = ((2 img - 1) - shift_c) / scale_c per channel (defaults shift [-.030, -.088, -.188], scale [.458, .448, .450]);
//   2. thirteen 3 x 3 convolutions, stride 1, bias, ReLU, zero padding 1 applied to the SCALED input; channels 3->64, 64->64 |
//      64->128, 128->128 | 128->256, 256->256 x 2 | 256->512, 512->512 x 2 | 512->512 x 3; a 2 x 2 stride-2 max-pool between the groups
//      (floor: an odd last row or column is dropped);
//   3. taps: the five group outputs after ReLU and before the pool (relu1_2, 2_2, 3_3, 4_3, 5_3);
//   4. per tap l and pixel: n = sqrt(sum_c f_c^2) + 1e-10 (eps outside the root), d = sum_c w_lc (fa_c / na - fb_c / nb)^2 with the
//      tap's 1 x 1 weights w_l (no bias); t_l = mean of d over the tap's pixels;   5. LPIPS = sum_l t_l.
// Evaluator wiring on load: the crop, clamp(pred, 0, 1), both images zeroed except where mask >= 1
// (the evaluator's rule: a NaN mask value counts as masked; image value 0, i.e. -1 before the scaling).
//
// * Layout: activations channel-last fp32 (N, h, w, C) in the caller's workspace, N = 2 B: image n < B is pred of item n, image B + n
//   is gt of item n; every layer runs once over all N, so a and b share a launch and the weight stream.
// * k_lpips_conv0: reads pred (B,3,H,W) / gt (B,H,W,3) / mask in place and applies crop, clamp, mask, 2x - 1 and the scaling layer on
//   load; K = 27 (padded to 28) = 7 steps of v_mfma_f32_16x16x4_f32; one wave owns 64 pixels x all 64 output channels.
// * k_lpips_conv (the other twelve): implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate: k-ordered fmaf
//   chains), output channels on the MFMA rows, pixels of the flattened (n, y, x) index on the columns, K = (tap, input channel).  One
//   wave owns 32 output channels x 64 pixels (2 x 4 tiles); a lane loads 4 consecutive channels per tile and k-chunk, and element e
//   keeps a chain of its own (9 cin / 16 MFMAs long at most); the four are added pairwise at the end, then the bias, then ReLU.
//   Operands come straight from global memory (L1 / L2: neighbouring taps and the waves of a workgroup re-read the same lines; the
//   four waves of a workgroup share the pixel tile where cout / 32 is a multiple of 4, at cout = 64 a workgroup covers two tiles);
//   weights are packed on the host in operand order.  Per 16-channel k-chunk a wave issues 2 weight and 4 activation 16-byte loads
//   for 32 MFMAs (1024 matrix cycles): 6 KB per 1024 cycles and SIMD, 24 B / cycle / CU.
//   Measured per layer class: every class from 64 to 512 channels runs at 0.41 - 0.49 of the fp32 matrix
//   peak, the ceiling of one wave per SIMD at this register tile; the 512-channel layers lose 0.07 of it to the weight stream (every
//   64-pixel tile re-reads the layer's 9.4 MB from L2), and the last group runs at 0.28: 640 waves for 1024 SIMDs.
// * k_lpips_pool: 2 x 2 max, floor.  k_lpips_tap: one wave per pixel at a time, lane l holds channels l, l + 64, ...; the channel sums
//   are butterfly reductions (the same order in every lane, on every call); per-pixel d in fp32, added over a wave's pixels in fp64
//   in a fixed order, one slot per wave.  k_lpips_finish: one workgroup per item adds the slots of each tap in a fixed order, divides by
//   the tap's pixel count, writes the five t_l and their sum.  No atomics; every slot read was written in the same call: the record
//   is bit-identical from run to run whatever the workspace held, and whatever position of whatever batch the image has.
// * No scratch, no host sync, no allocation: the caller owns the workspace.
#include "gdb_internal.h"
#include <cstdio>
#include <cstring>

typedef float F4 __attribute__((ext_vector_type(4)));

#define LP_NCONV 13
#define LP_NTAP 5
#define LP_NA 4         // 16-pixel tiles per wave
#define LP_PX (16 * LP_NA)
#define LP_SLOTS 2048   // at most this many waves (partial sums) per item and tap
#define LP_MIN 16       // smallest cropped extent: the fifth tap is 1 x 1

static const int lp_cin[LP_NCONV] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
static const int lp_cout[LP_NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
static const int lp_group[LP_NCONV] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
static const int lp_tapconv[LP_NTAP] = {1, 3, 6, 9, 12};   // the convolution whose output tap l reads

// ---- packed weights ---------------------------------------------------------------------------------------------------------
struct LpPack {
    size_t head;                 // shift[3], scale[3]
    size_t w[LP_NCONV], b[LP_NCONV], lin[LP_NTAP];
    size_t total;
};
static LpPack lp_pack_plan() {
    LpPack P;
    size_t o = 0;
    auto take = [&](size_t n) { size_t at = o; o += (n + 63) / 64 * 64; return at; };
    P.head = take(6);
    P.w[0] = take(4 * 7 * 64);
    P.b[0] = take(64);
    for (int i = 1; i < LP_NCONV; ++i) {
        P.w[i] = take((size_t)lp_cout[i] * lp_cin[i] * 9);
        P.b[i] = take(lp_cout[i]);
    }
    for (int l = 0; l < LP_NTAP; ++l) P.lin[l] = take(lp_cout[lp_tapconv[l]]);
    P.total = o;
    return P;
}

// ---- workspace --------------------------------------------------------------------------------------------------------------
// Stored activations in the order they are written: conv.0, conv.1, pool.0, conv.2, conv.3, pool.1, ... conv.12 (17 of them).
#define LP_NACT 17
struct LpAct { int conv, group, ch; };   // conv: 0 .. 12, or -1 for a pooled map (of `group`, the group it feeds)
static void lp_acts(LpAct a[LP_NACT]) {
    int k = 0;
    for (int i = 0; i < LP_NCONV; ++i) {
        if (i > 0 && lp_group[i] != lp_group[i - 1]) a[k++] = LpAct{-1, lp_group[i], lp_cout[i - 1]};
        a[k++] = LpAct{i, lp_group[i], lp_cout[i]};
    }
}
struct LpLayout {
    int N, gh[LP_NTAP], gw[LP_NTAP];
    int nslots[LP_NTAP];
    size_t scaled, scaled_bytes;      // KEEP only
    size_t act[LP_NACT], act_bytes[LP_NACT];
    size_t taps, partials, partials_bytes, total;
};
static LpLayout lp_layout(int B, int h, int w, int flags) {
    LpLayout L;
    L.N = 2 * B;
    for (int g = 0; g < LP_NTAP; ++g) { L.gh[g] = h >> g; L.gw[g] = w >> g; }
    LpAct a[LP_NACT];
    lp_acts(a);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    const bool keep = (flags & GDB_LPIPS_KEEP) != 0;
    L.scaled = 0; L.scaled_bytes = 0;
    if (keep) { L.scaled_bytes = sizeof(float) * (size_t)L.N * h * w * 3; L.scaled = take(L.scaled_bytes); }
    size_t ping = 0, pong = 0;
    if (!keep) {   // two alternating buffers of the largest map: the first group's (a later group's is at most half of it)
        const size_t big = sizeof(float) * (size_t)L.N * h * w * 64;
        ping = take(big); pong = take(big);
    }
    for (int k = 0; k < LP_NACT; ++k) {
        L.act_bytes[k] = sizeof(float) * (size_t)L.N * L.gh[a[k].group] * L.gw[a[k].group] * a[k].ch;
        L.act[k] = keep ? take(L.act_bytes[k]) : (k % 2 ? pong : ping);
    }
    L.taps = take(sizeof(double) * (size_t)B * LP_NTAP);
    size_t slots = 0;
    for (int l = 0; l < LP_NTAP; ++l) {
        const long long px = (long long)L.gh[l] * L.gw[l];
        L.nslots[l] = (int)(px < LP_SLOTS ? px : LP_SLOTS);
        slots += (size_t)L.nslots[l];
    }
    L.partials_bytes = sizeof(double) * (size_t)B * slots;
    L.partials = take(L.partials_bytes);
    L.total = o;
    return L;
}

static int lp_shape(const char* what, int B, int h, int w, int flags) {
    if (flags & ~GDB_LPIPS_KEEP) return gdb_fail(GDB_E_BADARG, "%s: unknown flags 0x%x", what, flags);
    if (B < 1 || h < 1 || w < 1) return gdb_fail(GDB_E_SHAPE, "%s: bad shape B=%d h=%d w=%d", what, B, h, w);
    if (h < LP_MIN || w < LP_MIN)
        return gdb_fail(GDB_E_SHAPE, "%s: %d x %d pixels; the fifth tap needs at least %d x %d (four 2 x 2 pools)", what, h, w, LP_MIN, LP_MIN);
    if ((double)B * h * w >= 268435456.0) return gdb_fail(GDB_E_SHAPE, "%s: B=%d h=%d w=%d is too large for the launch grid", what, B, h, w);
    return GDB_OK;
}

// ---- device -----------------------------------------------------------------------------------------------------------------
struct LpIn {
    const float *pred, *gt, *mask, *head;   // head: shift[3], scale[3]
    int B, H, W, y0, x0, h, w;
};

// The scaled input of image n (n < B: pred of item n, else gt of item n - B) at pixel (y, x) of the crop, channel c.
__device__ __forceinline__ float lp_input(const LpIn& a, int n, int y, int x, int c) {
    const int item = n < a.B ? n : n - a.B;
    const size_t plane = (size_t)a.H * a.W;
    const size_t px = (size_t)item * plane + (size_t)(a.y0 + y) * a.W + (a.x0 + x);
    float v = 0.f;
    if (a.mask[px] >= 1.f) {
        if (n < a.B) {
            const float p = a.pred[((size_t)item * 3 + c) * plane + (size_t)(a.y0 + y) * a.W + (a.x0 + x)];
            v = p < 0.f ? 0.f : (p > 1.f ? 1.f : p);   // torch.clamp: NaN stays NaN
        } else {
            v = a.gt[px * 3 + c];
        }
    }
    return ((2.f * v - 1.f) - a.head[c]) / a.head[3 + c];
}

// GDB_LPIPS_KEEP: the scaled input as conv.0 forms it, (N, h, w, 3).
__global__ __launch_bounds__(256) void k_lpips_scaled(LpIn a, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)2 * a.B * a.h * a.w * 3;
    if (i >= total) return;
    const int c = (int)(i % 3);
    size_t p = i / 3;
    const int x = (int)(p % a.w); p /= a.w;
    const int y = (int)(p % a.h);
    const int n = (int)(p / a.h);
    out[i] = lp_input(a, n, y, x, c);
}

// conv.0: wave = 64 pixels x 64 output channels.  Packed weights [mt 4][step 7][lane 64]: W[16 mt + (lane & 15)][k = 4 step + (lane >> 4)],
// k = (ci 3 + ky) 3 + kx, zero at k = 27.
__global__ __launch_bounds__(256) void k_lpips_conv0(LpIn a, const float* __restrict__ wp, const float* __restrict__ bias,
                                                      float* __restrict__ out, int P, int nwaves) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (wave >= nwaves) return;
    const int j = lane & 15, kq = lane >> 4;
    int pn[LP_NA], py[LP_NA], px[LP_NA];
    bool pok[LP_NA];
#pragma unroll
    for (int i = 0; i < LP_NA; ++i) {
        const int p = wave * LP_PX + 16 * i + j;
        pok[i] = p < P;
        const int q = pok[i] ? p : 0;
        px[i] = q % a.w;
        py[i] = (q / a.w) % a.h;
        pn[i] = q / (a.w * a.h);
    }
    F4 acc[4][LP_NA];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int i = 0; i < LP_NA; ++i) acc[m][i] = F4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < 7; ++s) {
        const int k = 4 * s + kq;
        const int ci = k / 9, ky = (k / 3) % 3, kx = k % 3;
        float bv[LP_NA];
#pragma unroll
        for (int i = 0; i < LP_NA; ++i) {
            const int iy = py[i] + ky - 1, ix = px[i] + kx - 1;
            const bool ok = pok[i] && k < 27 && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w;
            bv[i] = ok ? lp_input(a, pn[i], iy, ix, ci) : 0.f;   // zero padding of the scaled input
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float wv = wp[((size_t)m * 7 + s) * 64 + lane];
#pragma unroll
            for (int i = 0; i < LP_NA; ++i) acc[m][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, bv[i], acc[m][i], 0, 0, 0);
        }
    }
    // register r of lane (j, kq) = output channel 16 m + 4 kq + r of pixel j of tile i
#pragma unroll
    for (int i = 0; i < LP_NA; ++i) {
        const int p = wave * LP_PX + 16 * i + j;
        if (p >= P) continue;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int co = 16 * m + 4 * kq;
            const F4 bb = *(const F4*)(bias + co);
            F4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc[m][i][r] + bb[r], 0.f);
            *(F4*)(out + (size_t)p * 64 + co) = v;
        }
    }
}

// conv.1 .. conv.12: wave = 32 output channels (mp) x 64 pixels (pt) of the flattened (n, y, x) index.  Packed weights
// [mp][tap 9][cc cin / 16][m 2][lane 64][e 4] = W[32 mp + 16 m + (lane & 15)][16 cc + 4 (lane >> 4) + e][tap = ky 3 + kx].
__global__ __launch_bounds__(256) void k_lpips_conv(const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ bias,
                                                     float* __restrict__ out, int h, int w, int cin, int cout, int P, int nmp, int nwaves) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (wave >= nwaves) return;
    const int j = lane & 15, kq = lane >> 4;
    const int mp = wave % nmp, pt = wave / nmp;
    const int ncc = cin >> 4;
    int py[LP_NA], px[LP_NA];
    size_t pbase[LP_NA];   // float offset of row 0, column 0 of the pixel's image
    bool pok[LP_NA];
#pragma unroll
    for (int i = 0; i < LP_NA; ++i) {
        const int p = pt * LP_PX + 16 * i + j;
        pok[i] = p < P;
        const int q = pok[i] ? p : 0;
        px[i] = q % w;
        py[i] = (q / w) % h;
        pbase[i] = (size_t)(q / (w * h)) * h * w * cin;
    }
    F4 part[2][LP_NA][4];   // one accumulation chain per element of the lane's load
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < LP_NA; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) part[m][i][e] = F4{0.f, 0.f, 0.f, 0.f};
    const float* wl = wp + (size_t)mp * 9 * ncc * 512 + (size_t)lane * 4;
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - 3 * ky;
        const float* src[LP_NA];
        bool ok[LP_NA];
#pragma unroll
        for (int i = 0; i < LP_NA; ++i) {
            const int iy = py[i] + ky - 1, ix = px[i] + kx - 1;
            ok[i] = pok[i] && iy >= 0 && iy < h && ix >= 0 && ix < w;
            src[i] = in + pbase[i] + (ok[i] ? ((size_t)iy * w + ix) * cin : 0) + 4 * kq;
        }
        const float* wt = wl + (size_t)tap * ncc * 512;
        for (int cc = 0; cc < ncc; ++cc) {
            const F4 w0 = *(const F4*)(wt + (size_t)cc * 512), w1 = *(const F4*)(wt + (size_t)cc * 512 + 256);
            F4 bv[LP_NA];
#pragma unroll
            for (int i = 0; i < LP_NA; ++i) bv[i] = ok[i] ? *(const F4*)(src[i] + 16 * cc) : F4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < LP_NA; ++i) {
                    part[0][i][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[e], bv[i][e], part[0][i][e], 0, 0, 0);
                    part[1][i][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[e], bv[i][e], part[1][i][e], 0, 0, 0);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < LP_NA; ++i) {
        const int p = pt * LP_PX + 16 * i + j;
        if (p >= P) continue;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int co = 32 * mp + 16 * m + 4 * kq;
            const F4 s = (part[m][i][0] + part[m][i][1]) + (part[m][i][2] + part[m][i][3]);
            const F4 bb = *(const F4*)(bias + co);
            F4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(s[r] + bb[r], 0.f);   // the bias last
            *(F4*)(out + (size_t)p * cout + co) = v;
        }
    }
}

// 2 x 2 stride-2 max-pool, floor: (N, h, w, C) -> (N, h / 2, w / 2, C); a thread per four channels of an output pixel.
__global__ __launch_bounds__(256) void k_lpips_pool(const float* __restrict__ in, float* __restrict__ out, int h, int w, int C, size_t total4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int c4 = C >> 2, ho = h >> 1, wo = w >> 1;
    const int c = (int)(i % c4) * 4;
    size_t p = i / c4;
    const int x = (int)(p % wo); p /= wo;
    const int y = (int)(p % ho);
    const size_t n = p / ho;
    const float* s = in + ((n * h + 2 * y) * w + 2 * x) * C + c;
    const F4 a = *(const F4*)s, b = *(const F4*)(s + C), d = *(const F4*)(s + (size_t)w * C), e = *(const F4*)(s + (size_t)w * C + C);
    F4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(fmaxf(a[r], b[r]), fmaxf(d[r], e[r]));
    *(F4*)(out + i * 4) = v;
}

__device__ __forceinline__ float lp_wave_sum(float v) {   // butterfly: every lane ends with the same sum, formed in the same order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Tap l: act (N, h, w, C).  Wave s of item b takes pixels s, s + nslots, ... of the tap in that order and writes its fp64 sum of the
// per-pixel fp32 d to partials[b * nslots + s].
template <int KC>   // C / 64
__global__ __launch_bounds__(256) void k_lpips_tap(const float* __restrict__ act, const float* __restrict__ lin, int B, int npx, int nslots,
                                                    double* __restrict__ partials) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (wave >= B * nslots) return;
    const int b = wave / nslots, s = wave - b * nslots;
    constexpr int C = 64 * KC;
    float wl[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) wl[k] = lin[lane + 64 * k];
    const float* pa = act + (size_t)b * npx * C + lane;
    const float* pb = act + ((size_t)B + b) * npx * C + lane;
    double sum = 0.0;
    for (int p = s; p < npx; p += nslots) {
        float fa[KC], fb[KC], sa = 0.f, sb = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            fa[k] = pa[(size_t)p * C + 64 * k];
            fb[k] = pb[(size_t)p * C + 64 * k];
            sa += fa[k] * fa[k];
            sb += fb[k] * fb[k];
        }
        const float na = sqrtf(lp_wave_sum(sa)) + 1e-10f, nb = sqrtf(lp_wave_sum(sb)) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const float df = fa[k] / na - fb[k] / nb;
            d += wl[k] * (df * df);
        }
        sum += (double)lp_wave_sum(d);
    }
    if (lane == 0) partials[(size_t)b * nslots + s] = sum;
}

struct LpFinish {
    const double* partials[LP_NTAP];   // (B, nslots[l])
    int nslots[LP_NTAP];
    double npx[LP_NTAP];
};

// One workgroup per item: lane t adds slots t, t + 256, ... of each tap, then the workgroup's fixed-order sum; t_l = sum / pixels.
__global__ __launch_bounds__(256) void k_lpips_finish(LpFinish f, double* __restrict__ taps, double* __restrict__ records, long long stride) {
    __shared__ double red[4][LP_NTAP];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[LP_NTAP];
#pragma unroll
    for (int l = 0; l < LP_NTAP; ++l) {
        acc[l] = 0.0;
        const double* p = f.partials[l] + (size_t)b * f.nslots[l];
        for (int i = threadIdx.x; i < f.nslots[l]; i += 256) acc[l] += p[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[l] += __shfl_down(acc[l], off, 64);
        if (lane == 0) red[wave][l] = acc[l];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
#pragma unroll
        for (int l = 0; l < LP_NTAP; ++l) {
            const double t = (((red[0][l] + red[1][l]) + red[2][l]) + red[3][l]) / f.npx[l];
            taps[(size_t)b * LP_NTAP + l] = t;
            total += t;
        }
        records[(size_t)b * stride] = total;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
extern "C" int gdb_lpips_packed_floats(size_t* out_floats) {
    if (!out_floats) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    *out_floats = lp_pack_plan().total;
    return GDB_OK;
}

// h_tensors: 0 .. 12 the convolutions' weights (cout, cin, 3, 3), 13 .. 25 their biases, 26 .. 30 the taps' 1 x 1 weights (C_l floats),
// 31 shift (3), 32 scale (3).
extern "C" int gdb_pack_lpips_weights(const float* const* t, float* out) {
    if (!t || !out) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    for (int i = 0; i < GDB_LPIPS_TENSORS; ++i)
        if (!t[i]) return gdb_fail(GDB_E_BADARG, "NULL tensor %d of the LPIPS weights", i);
    const LpPack P = lp_pack_plan();
    memset(out, 0, P.total * sizeof(float));
    for (int c = 0; c < 3; ++c) { out[P.head + c] = t[31][c]; out[P.head + 3 + c] = t[32][c]; }
    for (int m = 0; m < 4; ++m)
        for (int s = 0; s < 7; ++s)
            for (int ln = 0; ln < 64; ++ln) {
                const int k = 4 * s + (ln >> 4);
                out[P.w[0] + ((size_t)m * 7 + s) * 64 + ln] = k < 27 ? t[0][(size_t)(16 * m + (ln & 15)) * 27 + k] : 0.f;
            }
    for (int i = 0; i < LP_NCONV; ++i) memcpy(out + P.b[i], t[13 + i], sizeof(float) * lp_cout[i]);
    for (int i = 1; i < LP_NCONV; ++i) {
        const int cin = lp_cin[i], ncc = cin / 16, nmp = lp_cout[i] / 32;
        const float* w = t[i];
        float* o = out + P.w[i];
        for (int mp = 0; mp < nmp; ++mp)
            for (int tap = 0; tap < 9; ++tap)
                for (int cc = 0; cc < ncc; ++cc)
                    for (int m = 0; m < 2; ++m)
                        for (int ln = 0; ln < 64; ++ln)
                            for (int e = 0; e < 4; ++e) {
                                const int co = 32 * mp + 16 * m + (ln & 15), ci = 16 * cc + 4 * (ln >> 4) + e;
                                o[(((((size_t)mp * 9 + tap) * ncc + cc) * 2 + m) * 64 + ln) * 4 + e] = w[((size_t)co * cin + ci) * 9 + tap];
                            }
    }
    for (int l = 0; l < LP_NTAP; ++l) memcpy(out + P.lin[l], t[26 + l], sizeof(float) * lp_cout[lp_tapconv[l]]);
    return GDB_OK;
}

extern "C" int gdb_lpips_workspace_bytes(int32_t B, int32_t h, int32_t w, int32_t flags, size_t* out_bytes) {
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    int rc = lp_shape("lpips", B, h, w, flags);
    if (rc != GDB_OK) return rc;
    *out_bytes = lp_layout(B, h, w, flags).total;
    return GDB_OK;
}

static void lp_region(GdbDecRegion* r, const char* name, size_t off, size_t bytes, int s0, int s1, int s2, int s3) {
    memset(r, 0, sizeof *r);
    strncpy(r->name, name, sizeof r->name - 1);
    r->offset = off; r->bytes = bytes;
    r->shape[0] = s0; r->shape[1] = s1; r->shape[2] = s2; r->shape[3] = s3;
}

extern "C" int gdb_lpips_layout(int32_t B, int32_t h, int32_t w, int32_t flags, GdbDecRegion* out, int32_t capacity, int32_t* out_count) {
    if (!out_count) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    int rc = lp_shape("lpips_layout", B, h, w, flags);
    if (rc != GDB_OK) return rc;
    const LpLayout L = lp_layout(B, h, w, flags);
    const bool keep = (flags & GDB_LPIPS_KEEP) != 0;
    const int count = (keep ? 1 + LP_NACT : 2) + 2;
    *out_count = count;
    if (!out) return GDB_OK;
    if (capacity < count) return gdb_fail(GDB_E_BADARG, "lpips_layout: room for %d regions, %d needed", capacity, count);
    int k = 0;
    if (keep) {
        LpAct a[LP_NACT];
        lp_acts(a);
        lp_region(&out[k++], "scaled", L.scaled, L.scaled_bytes, L.N, h, w, 3);
        for (int i = 0; i < LP_NACT; ++i) {
            char name[16];
            if (a[i].conv >= 0) snprintf(name, sizeof name, "conv.%d", a[i].conv);
            else snprintf(name, sizeof name, "pool.%d", a[i].group - 1);
            lp_region(&out[k++], name, L.act[i], L.act_bytes[i], L.N, L.gh[a[i].group], L.gw[a[i].group], a[i].ch);
        }
    } else {
        lp_region(&out[k++], "ping", L.act[0], L.act_bytes[0], L.N, h, w, 64);
        lp_region(&out[k++], "pong", L.act[1], L.act_bytes[1], L.N, h, w, 64);
    }
    lp_region(&out[k++], "taps", L.taps, sizeof(double) * (size_t)B * LP_NTAP, B, LP_NTAP, 0, 0);   // doubles
    lp_region(&out[k++], "partials", L.partials, L.partials_bytes, 0, 0, 0, 0);                     // doubles
    return GDB_OK;
}

template <int KC>
static int lp_tap_launch(const float* act, const float* lin, int B, int npx, int nslots, double* part, hipStream_t st) {
    const long long waves = (long long)B * nslots;
    hipLaunchKernelGGL(k_lpips_tap<KC>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, act, lin, B, npx, nslots, part);
    LAUNCH_CHECK("k_lpips_tap");
    return GDB_OK;
}

extern "C" int gdb_eval_lpips(const float* d_pred, const float* d_gt, const float* d_mask, int32_t B, int32_t H, int32_t W, int32_t crop_y0,
                              int32_t crop_x0, int32_t crop_h, int32_t crop_w, const float* d_packed, int32_t flags, void* d_ws,
                              size_t ws_bytes, double* d_records, int64_t record_stride, void* stream_) {
    if (!d_pred || !d_gt || !d_mask || !d_packed || !d_ws || !d_records) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (flags & ~GDB_LPIPS_KEEP) return gdb_fail(GDB_E_BADARG, "eval_lpips: unknown flags 0x%x", flags);
    if (B < 1 || H < 1 || W < 1) return gdb_fail(GDB_E_SHAPE, "eval_lpips: bad shape B=%d H=%d W=%d", B, H, W);
    if ((double)B * H * W >= 2147483648.0) return gdb_fail(GDB_E_SHAPE, "eval_lpips: B=%d H=%d W=%d is too large", B, H, W);
    if (record_stride < 1) return gdb_fail(GDB_E_BADARG, "eval_lpips: record stride %lld (at least 1 double)", (long long)record_stride);
    if (crop_y0 < 0 || crop_x0 < 0 || crop_h < 0 || crop_w < 0 || (long long)crop_y0 + crop_h > H || (long long)crop_x0 + crop_w > W)
        return gdb_fail(GDB_E_SHAPE, "eval_lpips: crop rows [%d, %d + %d) columns [%d, %d + %d) outside the %d x %d image", crop_y0, crop_y0,
                        crop_h, crop_x0, crop_x0, crop_w, H, W);
    int rc = lp_shape("eval_lpips", B, crop_h, crop_w, flags);
    if (rc != GDB_OK) return rc;
    const int h = crop_h, w = crop_w;
    const LpLayout L = lp_layout(B, h, w, flags);
    if (ws_bytes < L.total) return gdb_fail(GDB_E_WORKSPACE, "eval_lpips: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    const LpPack P = lp_pack_plan();
    hipStream_t st = (hipStream_t)stream_;
    char* ws = (char*)d_ws;
    LpAct acts[LP_NACT];
    lp_acts(acts);
    LpIn in{d_pred, d_gt, d_mask, d_packed + P.head, B, H, W, crop_y0, crop_x0, h, w};
    if (flags & GDB_LPIPS_KEEP) {
        const size_t total = (size_t)L.N * h * w * 3;
        hipLaunchKernelGGL(k_lpips_scaled, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, (float*)(ws + L.scaled));
        LAUNCH_CHECK("k_lpips_scaled");
    }
    LpFinish fin;
    double* part = (double*)(ws + L.partials);
    int tap = 0;
    for (int k = 0; k < LP_NACT; ++k) {
        const LpAct& a = acts[k];
        const int gh = L.gh[a.group], gw = L.gw[a.group];
        const int Ppx = L.N * gh * gw;   // < 2^30 (lp_shape)
        float* out = (float*)(ws + L.act[k]);
        const float* src = k ? (const float*)(ws + L.act[k - 1]) : nullptr;
        if (a.conv == 0) {
            const int nwaves = (Ppx + LP_PX - 1) / LP_PX;
            hipLaunchKernelGGL(k_lpips_conv0, dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, st, in, d_packed + P.w[0], d_packed + P.b[0], out,
                               Ppx, nwaves);
            LAUNCH_CHECK("k_lpips_conv0");
        } else if (a.conv > 0) {
            const int nmp = a.ch / 32;
            const long long nw = (long long)((Ppx + LP_PX - 1) / LP_PX) * nmp;   // <= 2^24 x 16
            hipLaunchKernelGGL(k_lpips_conv, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, st, src, d_packed + P.w[a.conv], d_packed + P.b[a.conv],
                               out, gh, gw, lp_cin[a.conv], a.ch, Ppx, nmp, (int)nw);
            LAUNCH_CHECK("k_lpips_conv");
        } else {
            const size_t total4 = (size_t)Ppx * (a.ch / 4);
            hipLaunchKernelGGL(k_lpips_pool, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, src, out, L.gh[a.group - 1],
                               L.gw[a.group - 1], a.ch, total4);
            LAUNCH_CHECK("k_lpips_pool");
        }
        if (a.conv >= 0 && tap < LP_NTAP && a.conv == lp_tapconv[tap]) {
            const int npx = gh * gw, ns = L.nslots[tap];
            const float* lin = d_packed + P.lin[tap];
            fin.partials[tap] = part; fin.nslots[tap] = ns; fin.npx[tap] = (double)npx;
            switch (a.ch / 64) {
                case 1: rc = lp_tap_launch<1>(out, lin, B, npx, ns, part, st); break;
                case 2: rc = lp_tap_launch<2>(out, lin, B, npx, ns, part, st); break;
                case 4: rc = lp_tap_launch<4>(out, lin, B, npx, ns, part, st); break;
                default: rc = lp_tap_launch<8>(out, lin, B, npx, ns, part, st); break;
            }
            if (rc != GDB_OK) return rc;
            part += (size_t)B * ns;
            ++tap;
        }
    }
    hipLaunchKernelGGL(k_lpips_finish, dim3((unsigned)B), dim3(256), 0, st, fin, (double*)(ws + L.taps), d_records, (long long)record_stride);
    LAUNCH_CHECK("k_lpips_finish");
    return GDB_OK;
}
