// The training loss's MSE + SSIM part (train/losses/gdb_nerf.py: PhotometricLoss without its perceptual term) as ONE call that
// returns the value and the gradient with respect to the estimate, and the masked smooth-L1 depth monitor, for gfx950.  The
// definition is the header's (include/gdb_nerf_hip.h, "the training loss"); this file is how it is computed.
//
// * Arithmetic: fp32 per pixel, as torch computes the loss; the 7-tap sums are fmaf chains in tap order (the translation unit is
//   built with -ffp-contract=off, so nothing else contracts); sums over pixels in fp64.
// * Photometric kernel: one workgroup of 256 lanes per (image, channel, LS_T x LS_T output tile).  With a gradient it stages both
//   images for the tile plus a 6-pixel halo (3 for the statistics, 3 for the adjoint; zero outside the image, which IS the zero
//   padding) and runs, all in LDS:
//     1. rows:    the five 7-tap moment sums over (T + 12) rows x (T + 6) columns;
//     2. columns: the same five over (T + 6)^2 positions; there S and the three adjoint maps Am, Bm, Cm, zero outside the image
//                 (kept in registers until every lane has read the row sums, then written over them);
//     3. rows, then columns of the three maps over T^2; G is written from the staged images.
//   LDS: 2 x 44 x 44 + 5 x 44 x 38 floats = 48,928 bytes (the maps, 3 x 38 x 38, and their row sums, 3 x 38 x 32, fit into the row
//   sums' 5 x 44 x 38): three workgroups per CU.  Without a gradient (template flag, not a branch around the passes) the halo is 3,
//   steps 1 and 2 run over the tile alone and nothing else does: 35,872 bytes.
// * Sums: workgroup w writes [sum (x1 - x2)^2, sum S] over the in-image pixels of its tile to slot w of the caller's workspace
//   (lanes by __shfl_down, waves in wave order); a one-workgroup launch adds the slots - lane t takes slots t, t + 256, ... in
//   index order, then the same fixed lane / wave order - and writes the fp32 scalars.  No atomics: every slot that is read was
//   written in the same call, so the workspace's previous contents never matter and two calls give the same bits.
// * Monitor: LS_CHUNK consecutive elements per workgroup, [sum of smooth-L1 over mask > 0.5, their count], the same finish.
#include "gdb_internal.h"

#include <math.h>

#define LS_THREADS 256
#define LS_T 32        // output tile edge
#define LS_WIN 7
#define LS_CHUNK 2048  // elements per workgroup of the monitor kernel
#define LS_MAX_GROUPS ((1LL << 32) / LS_THREADS - 1)   // a launch holds fewer than 2^32 work-items: more is refused as a shape, before the launch

struct LsWindow { float g[LS_WIN]; };   // the 1-D Gaussian; the 2-D window is g (x) g

// Sum of two values per lane over the workgroup: lanes by shuffle, then the four waves in wave order.  Lane 0 ends with the sums.
__device__ __forceinline__ void ls_block_sum(double (&a)[2]) {
    __shared__ double red[LS_THREADS / 64][2];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_down(a[k], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = a[0]; red[wave][1] = a[1]; }
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            double s = red[0][k];
            for (int w = 1; w < LS_THREADS / 64; ++w) s += red[w][k];
            a[k] = s;
        }
}

// est (B,3,H,W) contiguous = x2; gt = x1 at element strides (gsb, gsc, gsy, gsx).  ca = 2 alpha / n, cb = beta / n.
template <bool GRAD>
__global__ __launch_bounds__(LS_THREADS) void k_photometric(const float* __restrict__ est, const float* __restrict__ gt, long long gsb,
                                                            long long gsc, long long gsy, long long gsx, int H, int W, int tilesX,
                                                            int tiles, LsWindow win, float ca, float cb, float* __restrict__ grad,
                                                            double* __restrict__ partials) {
    constexpr int HALO = GRAD ? 6 : 3;       // staged pixels around the tile
    constexpr int IN = LS_T + 2 * HALO;      // staged edge: 44 / 38
    constexpr int ST = IN - (LS_WIN - 1);    // edge of the region that has statistics: 38 / 32
    constexpr int SO = HALO - 3;             // the tile's origin inside that region: 3 / 0
    constexpr int NP = (ST * ST + LS_THREADS - 1) / LS_THREADS;
    static_assert(!GRAD || 3 * ST * ST + 3 * ST * LS_T <= 5 * IN * ST,"the maps and their row sums reuse the moments' row sums");
    __shared__ float s1[IN * IN], s2[IN * IN], su[5 * IN * ST];
    const int tile = blockIdx.x % tiles, bc = blockIdx.x / tiles;   // bc = image * 3 + channel
    const int ty = tile / tilesX, tx = tile - ty * tilesX;
    const int oy = ty * LS_T, ox = tx * LS_T;
    const float* __restrict__ e = est + (size_t)bc * H * W;
    const float* __restrict__ g = gt + (long long)(bc / 3) * gsb + (long long)(bc % 3) * gsc;
    double acc[2] = {0.0, 0.0};

    for (int i = threadIdx.x; i < IN * IN; i += LS_THREADS) {
        const int ly = i / IN, lx = i - ly * IN;
        const int y = oy - HALO + ly, x = ox - HALO + lx;
        float a = 0.f, p = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            a = g[(long long)y * gsy + (long long)x * gsx];
            p = e[(size_t)y * W + x];
            if (ly >= HALO && ly < HALO + LS_T && lx >= HALO && lx < HALO + LS_T) {
                const float d = a - p;
                acc[0] += (double)(d * d);
            }
        }
        s1[i] = a; s2[i] = p;
    }
    __syncthreads();

    // 1. rows: position (ly, lx) of the IN x ST row sums is centred on staged column lx + 3
    for (int i = threadIdx.x; i < IN * ST; i += LS_THREADS) {
        const int ly = i / ST, lx = i - ly * ST;
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < LS_WIN; ++k) {
            const float a = s1[ly * IN + lx + k], p = s2[ly * IN + lx + k], w = win.g[k];
            m1 = fmaf(w, a, m1); m2 = fmaf(w, p, m2);
            e11 = fmaf(w, a * a, e11); e22 = fmaf(w, p * p, e22); e12 = fmaf(w, a * p, e12);
        }
        su[i] = m1; su[IN * ST + i] = m2; su[2 * IN * ST + i] = e11; su[3 * IN * ST + i] = e22; su[4 * IN * ST + i] = e12;
    }
    __syncthreads();

    // 2. columns, S and the adjoint maps
    float mA[NP], mB[NP], mC[NP];
    const float C1 = 1e-4f, C2 = 9e-4f;
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        const int i = threadIdx.x + r * LS_THREADS;
        mA[r] = mB[r] = mC[r] = 0.f;
        if (i >= ST * ST) continue;
        const int sy = i / ST, sx = i - sy * ST;
        const int y = oy - SO + sy, x = ox - SO + sx;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;   // S is defined on the image only: the maps are zero outside it
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < LS_WIN; ++k) {
            const int j = (sy + k) * ST + sx;
            const float w = win.g[k];
            m1 = fmaf(w, su[j], m1); m2 = fmaf(w, su[IN * ST + j], m2);
            e11 = fmaf(w, su[2 * IN * ST + j], e11); e22 = fmaf(w, su[3 * IN * ST + j], e22); e12 = fmaf(w, su[4 * IN * ST + j], e12);
        }
        const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        const float v1 = e11 - m11, v2 = e22 - m22, v12 = e12 - m12;
        const float N1 = 2.f * m12 + C1, N2 = 2.f * v12 + C2, D1 = m11 + m22 + C1, D2 = v1 + v2 + C2;
        const float S = (N1 * N2) / (D1 * D2);
        if (sy >= SO && sy < SO + LS_T && sx >= SO && sx < SO + LS_T) acc[1] += (double)S;
        if constexpr (GRAD) {
            const float Bm = -S / D2, Cm = 2.f * N1 / (D1 * D2);
            mA[r] = 2.f * m1 * N2 / (D1 * D2) - 2.f * m2 * S / D1 - 2.f * m2 * Bm - m1 * Cm;
            mB[r] = Bm; mC[r] = Cm;
        }
    }

    if constexpr (GRAD) {
        float* __restrict__ map = su;                  // [3][ST][ST]
        float* __restrict__ row = su + 3 * ST * ST;    // [3][ST][LS_T]
        __syncthreads();   // every lane has read the moments' row sums
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int i = threadIdx.x + r * LS_THREADS;
            if (i < ST * ST) { map[i] = mA[r]; map[ST * ST + i] = mB[r]; map[2 * ST * ST + i] = mC[r]; }
        }
        __syncthreads();
        // 3. the window is symmetric and the maps are zero outside the image: the adjoint is the same two passes
        for (int i = threadIdx.x; i < ST * LS_T; i += LS_THREADS) {
            const int ly = i / LS_T, lx = i - ly * LS_T;
            float fa = 0.f, fb = 0.f, fc = 0.f;
#pragma unroll
            for (int k = 0; k < LS_WIN; ++k) {
                const int j = ly * ST + lx + k;
                const float w = win.g[k];
                fa = fmaf(w, map[j], fa); fb = fmaf(w, map[ST * ST + j], fb); fc = fmaf(w, map[2 * ST * ST + j], fc);
            }
            row[i] = fa; row[ST * LS_T + i] = fb; row[2 * ST * LS_T + i] = fc;
        }
        __syncthreads();
        float* __restrict__ out = grad + (size_t)bc * H * W;
#pragma unroll
        for (int r = 0; r < LS_T * LS_T / LS_THREADS; ++r) {
            const int i = threadIdx.x + r * LS_THREADS;
            const int ly = i / LS_T, lx = i - ly * LS_T;
            const int y = oy + ly, x = ox + lx;
            if (y >= H || x >= W) continue;
            float fa = 0.f, fb = 0.f, fc = 0.f;
#pragma unroll
            for (int k = 0; k < LS_WIN; ++k) {
                const int j = (ly + k) * LS_T + lx;
                const float w = win.g[k];
                fa = fmaf(w, row[j], fa); fb = fmaf(w, row[ST * LS_T + j], fb); fc = fmaf(w, row[2 * ST * LS_T + j], fc);
            }
            const float a = s1[(ly + HALO) * IN + lx + HALO], p = s2[(ly + HALO) * IN + lx + HALO];
            const float dS = fa + 2.f * p * fb + a * fc;
            out[(size_t)y * W + x] = ca * (p - a) - cb * dS;
        }
    }

    ls_block_sum(acc);
    if (threadIdx.x == 0) { partials[(size_t)blockIdx.x * 2] = acc[0]; partials[(size_t)blockIdx.x * 2 + 1] = acc[1]; }
}

// [sum of smooth-L1 (beta 1) over mask > 0.5, the number of such elements] of LS_CHUNK consecutive elements per workgroup.
__global__ __launch_bounds__(LS_THREADS) void k_smooth_l1(const float* __restrict__ est, const float* __restrict__ gt,
                                                          const float* __restrict__ mask, long long n, double* __restrict__ partials) {
    double acc[2] = {0.0, 0.0};
    const long long base = (long long)blockIdx.x * LS_CHUNK;
    for (int i = threadIdx.x; i < LS_CHUNK; i += LS_THREADS) {
        const long long j = base + i;
        if (j >= n) break;
        if (!(mask[j] > 0.5f)) continue;
        const float d = fabsf(est[j] - gt[j]);
        acc[0] += (double)(d < 1.f ? 0.5f * d * d : d - 0.5f);
        acc[1] += 1.0;
    }
    ls_block_sum(acc);
    if (threadIdx.x == 0) { partials[(size_t)blockIdx.x * 2] = acc[0]; partials[(size_t)blockIdx.x * 2 + 1] = acc[1]; }
}

// One workgroup: lane t adds slots t, t + 256, ... in index order, then the workgroup's fixed-order sum.
// PHOTO: out = [sum0 / n, sum1 / n, alpha sum0 / n + beta (1 - sum1 / n)]; else out = [sum0 / sum1] (0 / 0 = NaN: an empty mask).
template <bool PHOTO>
__global__ __launch_bounds__(LS_THREADS) void k_loss_finish(const double* __restrict__ partials, long long slots, double n, double alpha,
                                                            double beta, float* __restrict__ out) {
    double acc[2] = {0.0, 0.0};
    for (long long i = threadIdx.x; i < slots; i += LS_THREADS) { acc[0] += partials[i * 2]; acc[1] += partials[i * 2 + 1]; }
    ls_block_sum(acc);
    if (threadIdx.x == 0) {
        if constexpr (PHOTO) {
            const double mse = acc[0] / n, ssim = acc[1] / n;
            out[0] = (float)mse; out[1] = (float)ssim; out[2] = (float)(alpha * mse + beta * (1.0 - ssim));
        } else {
            out[0] = (float)(acc[0] / acc[1]);
        }
    }
}

static inline long long ls_tiles(int H, int W) { return (long long)((H + LS_T - 1) / LS_T) * ((W + LS_T - 1) / LS_T); }
static inline long long ls_chunks(long long n) { return (n + LS_CHUNK - 1) / LS_CHUNK; }

static int ls_shape(const char* what, int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return gdb_fail(GDB_E_SHAPE, "%s: bad shape B=%d H=%d W=%d", what, B, H, W);
    if ((double)B * 3.0 * (double)ls_tiles(H, W) > (double)LS_MAX_GROUPS)
        return gdb_fail(GDB_E_SHAPE, "%s: B=%d H=%d W=%d is too large for the launch grid", what, B, H, W);
    return GDB_OK;
}

extern "C" int gdb_loss_workspace_bytes(int32_t B, int32_t H, int32_t W, size_t* out_bytes) {
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    int rc = ls_shape("loss", B, H, W);
    if (rc != GDB_OK) return rc;
    const size_t img = (size_t)B * 3 * (size_t)ls_tiles(H, W), mon = (size_t)ls_chunks((long long)B * H * W);
    *out_bytes = 2 * sizeof(double) * (img > mon ? img : mon);
    return GDB_OK;
}

extern "C" int gdb_photometric_loss(const float* d_est, const float* d_gt, int64_t gt_sb, int64_t gt_sc, int64_t gt_sy, int64_t gt_sx,
                                    int32_t B, int32_t H, int32_t W, float alpha, float beta, float* d_grad, void* d_ws, size_t ws_bytes,
                                    float* d_out3, void* stream_) {
    if (!d_est || !d_gt || !d_ws || !d_out3) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    int rc = ls_shape("photometric_loss", B, H, W);
    if (rc != GDB_OK) return rc;
    if (gt_sb < 0 || gt_sc < 0 || gt_sy < 0 || gt_sx < 0) return gdb_fail(GDB_E_BADARG, "photometric_loss: negative ground-truth stride");
    const long long tiles = ls_tiles(H, W), slots = (long long)B * 3 * tiles;
    const size_t need = 2 * sizeof(double) * (size_t)slots;
    if (ws_bytes < need) return gdb_fail(GDB_E_BADARG, "photometric_loss: workspace of %zu bytes, %zu needed", ws_bytes, need);
    LsWindow win;
    // g in fp32, term by term as torch forms it (ssim_loss.py:9-11): the taps then sum to what the trained module's window sums to.
    // (s = e - m^2 carries the window's sum minus one times x^2; with g rounded from fp64 that term, 7e-8 x^2, showed in SSIM.)
    float ge[LS_WIN], sum = 0.f;
    for (int i = 0; i < LS_WIN; ++i) { ge[i] = expf(-(float)((i - 3) * (i - 3)) / 4.5f); sum += ge[i]; }
    for (int i = 0; i < LS_WIN; ++i) win.g[i] = ge[i] / sum;
    const double n = 3.0 * (double)B * (double)H * (double)W;
    const float ca = (float)(2.0 * (double)alpha / n), cb = (float)((double)beta / n);
    hipStream_t stream = (hipStream_t)stream_;
    double* part = (double*)d_ws;
    const int tilesX = (W + LS_T - 1) / LS_T;
    if (d_grad)
        hipLaunchKernelGGL(k_photometric<true>, dim3((unsigned)slots), dim3(LS_THREADS), 0, stream, d_est, d_gt, (long long)gt_sb,
                           (long long)gt_sc, (long long)gt_sy, (long long)gt_sx, H, W, tilesX, (int)tiles, win, ca, cb, d_grad, part);
    else
        hipLaunchKernelGGL(k_photometric<false>, dim3((unsigned)slots), dim3(LS_THREADS), 0, stream, d_est, d_gt, (long long)gt_sb,
                           (long long)gt_sc, (long long)gt_sy, (long long)gt_sx, H, W, tilesX, (int)tiles, win, ca, cb, (float*)nullptr, part);
    LAUNCH_CHECK("k_photometric");
    hipLaunchKernelGGL(k_loss_finish<true>, dim3(1), dim3(LS_THREADS), 0, stream, (const double*)part, slots, n, (double)alpha,
                       (double)beta, d_out3);
    LAUNCH_CHECK("k_loss_finish");
    return GDB_OK;
}

extern "C" int gdb_smooth_l1_masked(const float* d_est, const float* d_gt, const float* d_mask, int64_t n, void* d_ws, size_t ws_bytes,
                                    float* d_out1, void* stream_) {
    if (!d_est || !d_gt || !d_mask || !d_ws || !d_out1) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (n < 1) return gdb_fail(GDB_E_SHAPE, "smooth_l1_masked: %lld elements", (long long)n);
    const long long chunks = ls_chunks((long long)n);
    if (chunks > LS_MAX_GROUPS) return gdb_fail(GDB_E_SHAPE, "smooth_l1_masked: %lld elements are too many for the launch grid", (long long)n);
    const size_t need = 2 * sizeof(double) * (size_t)chunks;
    if (ws_bytes < need) return gdb_fail(GDB_E_BADARG, "smooth_l1_masked: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t stream = (hipStream_t)stream_;
    double* part = (double*)d_ws;
    hipLaunchKernelGGL(k_smooth_l1, dim3((unsigned)chunks), dim3(LS_THREADS), 0, stream, d_est, d_gt, d_mask, (long long)n, part);
    LAUNCH_CHECK("k_smooth_l1");
    hipLaunchKernelGGL(k_loss_finish<false>, dim3(1), dim3(LS_THREADS), 0, stream, (const double*)part, chunks, 0.0, 0.0, 0.0, d_out1);
    LAUNCH_CHECK("k_loss_finish");
    return GDB_OK;
}
