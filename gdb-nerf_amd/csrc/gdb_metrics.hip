// The evaluator's metrics (evaluators/gdb_nerf.py: masked PSNR, 7x7 SSIM, the MVSNeRF depth errors) as HIP kernels for gfx950, so
// that an evaluation loop never copies a frame to the host: every call leaves one small record of doubles per batch item on the
// device, and the host reads all of them once, in summarize().
//
// * Arithmetic: fp64 from the fp32 inputs, as the numpy evaluator (and skimage, which it restates) computes; SSIM's variances are
//   differences of nearly equal moments.  The translation unit is built with -ffp-contract=off: with gt == pred the two factors of
//   the numerator and of the denominator are then the same bits (2 a a == a a + a a) and every window is exactly 1.
// * Image kernel: one workgroup of 256 lanes owns a tile of EV_TW x EV_TH positions of the cropped image.  It stages the tile plus a
//   6-pixel apron to the right and below of both images in LDS as fp32 (prediction clamped to [0, 1], both zeroed outside the mask:
//   2 x 3 x 22 x 38 floats = 20 KB), sums (gt - pred)^2 and the mask over the tile's own pixels, and evaluates the windows whose
//   top-left corner lies in the tile (two per lane and channel, 49 taps each, five moments).  Only windows that lie wholly inside
//   the crop are evaluated - the interior (h - 6) x (w - 6) the numpy path averages over - so no border mode exists here.
// * Depth kernel: one workgroup owns EV_DPX consecutive pixels of the ground-truth map; the rendered depth is resized to it with
//   _resize_bilinear's formula in fp64 (or read in place when `resize` is 0).
// * Reduction: every workgroup writes its partial sums to its own slot of the caller's workspace (lanes by __shfl_down, waves in
//   wave order); a second launch, one workgroup per batch item, adds the slots in a fixed order.  No atomics; every slot that is
//   read has been written in the same call, so the workspace's previous contents never matter.
#include "gdb_internal.h"

#define EV_THREADS 256
#define EV_TW 32
#define EV_TH 16
#define EV_WIN 7
#define EV_LW (EV_TW + EV_WIN - 1)
#define EV_LH (EV_TH + EV_WIN - 1)
#define EV_DPX 2048   // ground-truth pixels per workgroup of the depth kernel

// Sum of NV values per lane over the workgroup, lanes by shuffle, then the four waves in wave order: the same order on every call.
template <int NV>
__device__ __forceinline__ void block_sum(double (&a)[NV], double* __restrict__ out) {
    __shared__ double red[EV_THREADS / 64][NV];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_down(a[k], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wave][k] = a[k];
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < EV_THREADS / 64; ++w) s += red[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// pred (B,3,H,W), gt (B,H,W,3), mask (B,H,W); the crop is rows [y0, y0 + h), columns [x0, x0 + w).  Workgroup (item, tile) writes
// [sum (gt - pred)^2, masked pixels, sum of SSIM of channel 0, 1, 2] to partials[(item * tiles + tile) * 5 ..].
__global__ __launch_bounds__(EV_THREADS) void k_eval_image(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           const float* __restrict__ mask, int H, int W, int y0, int x0, int h, int w,
                                                           int tilesX, int tiles, double* __restrict__ partials) {
    __shared__ float sg[3][EV_LH][EV_LW], sp[3][EV_LH][EV_LW];
    const int item = blockIdx.x / tiles, tile = blockIdx.x - item * tiles;
    const int ty = tile / tilesX, tx = tile - ty * tilesX;
    const int oy = ty * EV_TH, ox = tx * EV_TW;
    const size_t plane = (size_t)H * W;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < EV_LH * EV_LW; i += EV_THREADS) {
        const int ly = i / EV_LW, lx = i - ly * EV_LW;
        const int y = oy + ly, x = ox + lx;
        float g[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
        if (y < h && x < w) {
            const size_t px = (size_t)item * plane + (size_t)(y0 + y) * W + (x0 + x);
            if (mask[px] >= 1.f) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    g[c] = gt[px * 3 + c];
                    const float v = pred[((size_t)item * 3 + c) * plane + (size_t)(y0 + y) * W + (x0 + x)];
                    p[c] = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);   // torch.clamp: NaN stays NaN
                }
                if (ly < EV_TH && lx < EV_TW) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) { const double d = (double)g[c] - (double)p[c]; acc[0] += d * d; }
                    acc[1] += 1.0;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { sg[c][ly][lx] = g[c]; sp[c][ly][lx] = p[c]; }
    }
    __syncthreads();
    const double c1 = (0.01 * 2.0) * (0.01 * 2.0), c2 = (0.03 * 2.0) * (0.03 * 2.0), norm = 49.0 / 48.0;
    const int wx = threadIdx.x & (EV_TW - 1);
#pragma unroll
    for (int r = 0; r < EV_TH * EV_TW / EV_THREADS; ++r) {
        const int wy = (threadIdx.x >> 5) + r * (EV_THREADS / EV_TW);
        if (oy + wy + EV_WIN > h || ox + wx + EV_WIN > w) continue;   // the window leaves the crop: not an interior one
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
            for (int dy = 0; dy < EV_WIN; ++dy)
#pragma unroll
                for (int dx = 0; dx < EV_WIN; ++dx) {
                    const double a = (double)sg[c][wy + dy][wx + dx], b = (double)sp[c][wy + dy][wx + dx];
                    sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
                }
            const double ux = sx / 49.0, uy = sy / 49.0;
            const double vx = norm * (sxx / 49.0 - ux * ux), vy = norm * (syy / 49.0 - uy * uy), vxy = norm * (sxy / 49.0 - ux * uy);
            acc[2 + c] += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
        }
    }
    block_sum<5>(acc, partials + (size_t)blockIdx.x * 5);
}

// depth (B,Hd,Wd) resized to gt (B,H,W) when `resize`, else read at the same pixel (Hd == H, Wd == W).  Workgroup (item, chunk)
// writes [sum |err|, count(|err| < 2), count(|err| < 10), count(gt != 0)] to partials[(item * chunks + chunk) * 4 ..].
__global__ __launch_bounds__(EV_THREADS) void k_eval_depth(const float* __restrict__ depth, const float* __restrict__ gt, int Hd, int Wd,
                                                           int H, int W, int resize, int chunks, double* __restrict__ partials) {
    const int item = blockIdx.x / chunks, chunk = blockIdx.x - item * chunks;
    const size_t n = (size_t)H * W;
    const float* __restrict__ d = depth + (size_t)item * Hd * Wd;
    const float* __restrict__ g = gt + (size_t)item * n;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < EV_DPX; i += EV_THREADS) {
        const size_t px = (size_t)chunk * EV_DPX + i;
        if (px >= n) break;
        const float gv = g[px];
        if (!(gv != 0.f)) continue;
        double v;
        if (resize) {   // evaluators/gdb_nerf.py::_resize_bilinear, term by term
            const int y = (int)(px / W), x = (int)(px - (size_t)y * W);
            const double ys = fmin(fmax(((double)y + 0.5) * (double)Hd / (double)H - 0.5, 0.0), (double)(Hd - 1));
            const double xs = fmin(fmax(((double)x + 0.5) * (double)Wd / (double)W - 0.5, 0.0), (double)(Wd - 1));
            const int ya = (int)floor(ys), xa = (int)floor(xs);
            const int yb = min(ya + 1, Hd - 1), xb = min(xa + 1, Wd - 1);
            const double fy = ys - (double)ya, fx = xs - (double)xa;
            const double top = (double)d[(size_t)ya * Wd + xa] * (1.0 - fx) + (double)d[(size_t)ya * Wd + xb] * fx;
            const double bot = (double)d[(size_t)yb * Wd + xa] * (1.0 - fx) + (double)d[(size_t)yb * Wd + xb] * fx;
            v = top * (1.0 - fy) + bot * fy;
        } else {
            v = (double)d[px];
        }
        const double err = fabs(v - (double)gv);
        acc[0] += err;
        acc[1] += err < 2.0 ? 1.0 : 0.0;
        acc[2] += err < 10.0 ? 1.0 : 0.0;
        acc[3] += 1.0;
    }
    block_sum<4>(acc, partials + (size_t)blockIdx.x * 4);
}

// One workgroup per batch item: lane t adds slots t, t + 256, ... in that order, then the workgroup's fixed-order sum.
template <int NV>
__global__ __launch_bounds__(EV_THREADS) void k_eval_finish(const double* __restrict__ partials, int slots, double* __restrict__ records,
                                                            long long stride) {
    const double* __restrict__ p = partials + (size_t)blockIdx.x * slots * NV;
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < slots; i += EV_THREADS)
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] += p[(size_t)i * NV + k];
    block_sum<NV>(acc, records + (size_t)blockIdx.x * stride);
}

static inline long long ev_tiles(int h, int w) { return (long long)((h + EV_TH - 1) / EV_TH) * ((w + EV_TW - 1) / EV_TW); }
static inline long long ev_chunks(int H, int W) { return ((long long)H * W + EV_DPX - 1) / EV_DPX; }

static int ev_shape(const char* what, int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return gdb_fail(GDB_E_SHAPE, "%s: bad shape B=%d H=%d W=%d", what, B, H, W);
    if ((double)B * H * W >= 2147483648.0) return gdb_fail(GDB_E_SHAPE, "%s: B=%d H=%d W=%d is too large for the launch grid", what, B, H, W);
    return GDB_OK;
}

static size_t ev_ws_bytes(int B, int H, int W) {
    const size_t img = (size_t)B * (size_t)ev_tiles(H, W) * GDB_EVAL_IMAGE_REC, dep = (size_t)B * (size_t)ev_chunks(H, W) * GDB_EVAL_DEPTH_REC;
    return sizeof(double) * (img > dep ? img : dep);
}

extern "C" int gdb_eval_workspace_bytes(int32_t B, int32_t H, int32_t W, size_t* out_bytes) {
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    int rc = ev_shape("eval", B, H, W);
    if (rc != GDB_OK) return rc;
    *out_bytes = ev_ws_bytes(B, H, W);
    return GDB_OK;
}

extern "C" int gdb_eval_image(const float* d_pred, const float* d_gt, const float* d_mask, int32_t B, int32_t H, int32_t W,
                              int32_t crop_y0, int32_t crop_x0, int32_t crop_h, int32_t crop_w, void* d_ws, size_t ws_bytes,
                              double* d_records, int64_t record_stride, void* stream_) {
    if (!d_pred || !d_gt || !d_mask || !d_ws || !d_records) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    int rc = ev_shape("eval_image", B, H, W);
    if (rc != GDB_OK) return rc;
    if (record_stride < GDB_EVAL_IMAGE_REC) return gdb_fail(GDB_E_BADARG, "eval_image: record stride %lld (at least %d doubles)", (long long)record_stride, GDB_EVAL_IMAGE_REC);
    if (crop_y0 < 0 || crop_x0 < 0 || crop_h < 0 || crop_w < 0 || (long long)crop_y0 + crop_h > H || (long long)crop_x0 + crop_w > W)
        return gdb_fail(GDB_E_SHAPE, "eval_image: crop rows [%d, %d + %d) columns [%d, %d + %d) outside the %d x %d image", crop_y0, crop_y0,
                        crop_h, crop_x0, crop_x0, crop_w, H, W);
    if (crop_h < EV_WIN || crop_w < EV_WIN)
        return gdb_fail(GDB_E_SHAPE, "eval_image: %d x %d pixels after the crop; SSIM needs one %d x %d window", crop_h, crop_w, EV_WIN, EV_WIN);
    const long long tiles = ev_tiles(crop_h, crop_w);
    const size_t need = sizeof(double) * (size_t)B * (size_t)tiles * GDB_EVAL_IMAGE_REC;
    if (ws_bytes < need) return gdb_fail(GDB_E_WORKSPACE, "eval_image: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t stream = (hipStream_t)stream_;
    double* part = (double*)d_ws;
    hipLaunchKernelGGL(k_eval_image, dim3((unsigned)(B * tiles)), dim3(EV_THREADS), 0, stream, d_pred, d_gt, d_mask, H, W, crop_y0, crop_x0,
                       crop_h, crop_w, (crop_w + EV_TW - 1) / EV_TW, (int)tiles, part);
    LAUNCH_CHECK("k_eval_image");
    hipLaunchKernelGGL(k_eval_finish<GDB_EVAL_IMAGE_REC>, dim3((unsigned)B), dim3(EV_THREADS), 0, stream, (const double*)part, (int)tiles,
                       d_records, (long long)record_stride);
    LAUNCH_CHECK("k_eval_finish");
    return GDB_OK;
}

extern "C" int gdb_eval_depth(const float* d_depth, int32_t Hd, int32_t Wd, const float* d_gt, int32_t B, int32_t H, int32_t W,
                              int32_t resize, void* d_ws, size_t ws_bytes, double* d_records, int64_t record_stride, void* stream_) {
    if (!d_depth || !d_gt || !d_ws || !d_records) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    int rc = ev_shape("eval_depth", B, H, W);
    if (rc == GDB_OK) rc = ev_shape("eval_depth (rendered map)", B, Hd, Wd);
    if (rc != GDB_OK) return rc;
    if (record_stride < GDB_EVAL_DEPTH_REC) return gdb_fail(GDB_E_BADARG, "eval_depth: record stride %lld (at least %d doubles)", (long long)record_stride, GDB_EVAL_DEPTH_REC);
    if (!resize && (Hd != H || Wd != W))
        return gdb_fail(GDB_E_SHAPE, "eval_depth: a %d x %d map against a %d x %d ground truth needs the resize", Hd, Wd, H, W);
    const long long chunks = ev_chunks(H, W);
    const size_t need = sizeof(double) * (size_t)B * (size_t)chunks * GDB_EVAL_DEPTH_REC;
    if (ws_bytes < need) return gdb_fail(GDB_E_WORKSPACE, "eval_depth: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t stream = (hipStream_t)stream_;
    double* part = (double*)d_ws;
    hipLaunchKernelGGL(k_eval_depth, dim3((unsigned)(B * chunks)), dim3(EV_THREADS), 0, stream, d_depth, d_gt, Hd, Wd, H, W, resize ? 1 : 0,
                       (int)chunks, part);
    LAUNCH_CHECK("k_eval_depth");
    hipLaunchKernelGGL(k_eval_finish<GDB_EVAL_DEPTH_REC>, dim3((unsigned)B), dim3(EV_THREADS), 0, stream, (const double*)part, (int)chunks,
                       d_records, (long long)record_stride);
    LAUNCH_CHECK("k_eval_finish");
    return GDB_OK;
}
