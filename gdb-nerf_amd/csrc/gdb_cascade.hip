// One cascade MVS stage of DepthNet.forward (networks/gdb_nerf/depth_net.py) as one library call: camera set-up, plane sweep, the
// cost-regularisation U-Net, softmax over D and depth regression, with nothing materialised in between that only this stage reads.
//
// * Hypotheses are computed where they are used (HypRange) from the stage's search range (B, 2, hr, wr): stage 0's near / far
//   (hr = wr = 1, broadcast) or the previous stage's confidence interval, upsampled bilinearly by `ratio` under
//   F.interpolate(scale_factor = ratio, mode = "bilinear", align_corners = False)'s index and weight rule; then get_depth_values:
//   lo + (hi - lo) * step_d with step_d = torch.linspace(0, 1, D)[d], reciprocals of lo and hi first under inv_depth.  Exact fp32
//   (-ffp-contract=off): every multiply-add below is two roundings, as separate torch ops are.
// * k_cascade_proj: k_costvol_proj on the unscaled intrinsics; rows 0-1 are multiplied by feat_scale / vol_scale in fp32 first, as
//   `K[..., :2, :] *= s` does.
// * k_costvol_range<V, PAIR>: the sweep of gdb_costvol.hip (same body, gdb_costvol_body.h) with HypRange as its hypothesis source.
// * The U-Net runs through gdb_costreg.hip and stops at the prob head's logits.
// * k_softmax_regress: softmax over D and depth_regression (depth_net.py:73-83) in one pass over the logits; the probabilities are
//   never written.  One wave owns 16 consecutive pixels, D is split over the 4 lanes of a pixel (plane d belongs to lane group
//   d & 3): the max over D, the exps, the divisions and the products run 4-wide, and the three sums over D (of the exps, of
//   prob * hyp, of prob * (hyp - mean)^2) are taken in plane order from LDS, so the result has the bits of k_costreg_softmax followed
//   by k_depth_regression on the same hypotheses.  No atomics: deterministic.
#include "gdb_internal.h"
#include <cmath>

// gdb_costvol.hip / gdb_costreg.hip
int gdb_costvol_pairs_(const float* d_src, float* d_pair_ws, size_t plane, size_t npairs, hipStream_t st);
enum { CR_RUN_LOGITS = 0, CR_RUN_SOFTMAX = 1, CR_RUN_CHECK = 2 };
int gdb_cost_reg_run_(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B, int32_t D,
                      int32_t H, int32_t W, const float* d_packed, void* d_ws, size_t ws_bytes, float* d_volume, float* d_prob,
                      int mode, void* stream_);

#include "gdb_costvol_body.h"

// ---- hypotheses from the search range -------------------------------------------------------------------------------------------
struct HypRange {
    const float* range;   // (B, 2, hr, wr)
    int hr, wr, D, inv_depth;
    float rscale;         // 1 / ratio, rounded to fp32 as torch's area_pixel_compute_scale does with a given scale_factor

    // source index and weights of one axis: src = max((dst + 0.5) / ratio - 0.5, 0), i0 = (int)src, i1 = i0 + (i0 < n - 1)
    __device__ __forceinline__ void axis(int dst, int n, int& i0, int& i1, float& l0, float& l1) const {
        const float s = fmaxf(((float)dst + 0.5f) * rscale - 0.5f, 0.f);
        const int i = (int)s;
        l1 = s - (float)i; l0 = 1.f - l1;
        i0 = min(i, n - 1);   // (a target beyond ratio * n is outside F.interpolate's output: the last sample, never out of bounds)
        i1 = i0 + (i0 < n - 1 ? 1 : 0);
    }
    // the ends of pixel (y, x)'s hypothesis line: the (upsampled) range, as reciprocals under inv_depth     depth_net.py:43-45
    __device__ __forceinline__ void ends(int b, int y, int x, float& lo, float& hi) const {
        const size_t pl = (size_t)hr * wr;
        const float* r = range + (size_t)b * 2 * pl;
        if (pl == 1) { lo = r[0]; hi = r[1]; }
        else {
            int y0, y1, x0, x1;
            float ly0, ly1, lx0, lx1;
            axis(y, hr, y0, y1, ly0, ly1); axis(x, wr, x0, x1, lx0, lx1);
            const size_t a0 = (size_t)y0 * wr, a1 = (size_t)y1 * wr;
            lo = ly0 * (lx0 * r[a0 + x0] + lx1 * r[a0 + x1]) + ly1 * (lx0 * r[a1 + x0] + lx1 * r[a1 + x1]);
            r += pl;
            hi = ly0 * (lx0 * r[a0 + x0] + lx1 * r[a0 + x1]) + ly1 * (lx0 * r[a1 + x0] + lx1 * r[a1 + x1]);
        }
        if (inv_depth) { lo = 1.f / lo; hi = 1.f / hi; }
    }
    // torch.linspace(0, 1, D)[d]: step = 1 / (D - 1); the first half counts up from 0, the second half down from 1
    __device__ __forceinline__ float step(int d) const {
        if (D == 1) return 0.f;
        const float st = 1.f / (float)(D - 1);
        return d < D / 2 ? st * (float)d : 1.f - st * (float)(D - d - 1);
    }
    __device__ __forceinline__ float at(float lo, float hi, int d) const { return lo + (hi - lo) * step(d); }          // :46-47
    __device__ __forceinline__ float operator()(const CostVolArgs&, int b, int d, int y, int x, size_t) const {
        float lo, hi;
        ends(b, y, x, lo, hi);
        return at(lo, hi, d);
    }
};

__global__ void __launch_bounds__(256) k_mvs_hypotheses(HypRange h, int B, int Ht, int Wt, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, HW = (size_t)Ht * Wt;
    if (t >= (size_t)B * h.D * HW) return;
    const size_t bd = t / HW, p = t - bd * HW;
    const int b = (int)(bd / h.D), d = (int)(bd - (size_t)b * h.D), y = (int)(p / Wt), x = (int)(p - (size_t)y * Wt);
    float lo, hi;
    h.ends(b, y, x, lo, hi);
    out[t] = h.at(lo, hi, d);
}

__global__ void k_cascade_proj(int B, int V, const float* __restrict__ src_exts, const float* __restrict__ src_ints,
                               const float* __restrict__ tar_exts, const float* __restrict__ tar_ints, float feat_scale, float vol_scale,
                               float* __restrict__ proj) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * V) return;
    costvol_proj_one<true>(t, V, src_exts, src_ints, tar_exts, tar_ints, feat_scale, vol_scale, proj);
}

template <int VT, bool PAIR>
__global__ void __launch_bounds__(256) k_costvol_range(CostVolArgs a, HypRange h) { costvol_body<VT, PAIR>(a, h); }

// ---- softmax over D + depth regression ------------------------------------------------------------------------------------------
#define SR_PIX 16   // pixels per wave: one 64-byte segment of a logit plane per lane group
#define SR_SL 4     // lanes per pixel

__global__ void __launch_bounds__(64) k_softmax_regress(HypRange h, const float* __restrict__ logits, int B, int Ht, int Wt, float ci_scale,
                                                        float* __restrict__ depth, float* __restrict__ ci, float* __restrict__ vol_range) {
    extern __shared__ float sm[];                 // pr[D][16] | tm[D][16]
    const int D = h.D, pix = threadIdx.x & (SR_PIX - 1), sl = threadIdx.x / SR_PIX;
    float* pr = sm + pix;
    float* tm = sm + (size_t)D * SR_PIX + pix;
    const size_t HW = (size_t)Ht * Wt, n = (size_t)B * HW;
    size_t t = (size_t)blockIdx.x * SR_PIX + pix;
    const bool live = t < n;
    if (!live) t = n - 1;                         // the tail lanes recompute the last pixel and write nothing: the barriers stay uniform
    const size_t b = t / HW, p = t - b * HW;
    const int y = (int)(p / Wt), x = (int)(p - (size_t)y * Wt);
    float lo, hi;
    h.ends((int)b, y, x, lo, hi);
    const float* lg = logits + b * D * HW + p;
    float m = lg[0];                                                                              // softmax over D (cost_reg_net.py:54)
    for (int d = sl; d < D; d += SR_SL) m = fmaxf(m, lg[d * HW]);
    m = fmaxf(m, __shfl_xor(m, SR_PIX)); m = fmaxf(m, __shfl_xor(m, 2 * SR_PIX));
    for (int d = sl; d < D; d += SR_SL) pr[d * SR_PIX] = expf(lg[d * HW] - m);
    __syncthreads();
    float s = 0.f;
    for (int d = 0; d < D; ++d) s += pr[d * SR_PIX];
    __syncthreads();
    for (int d = sl; d < D; d += SR_SL) {
        const float q = pr[d * SR_PIX] / s;
        pr[d * SR_PIX] = q;
        tm[d * SR_PIX] = q * h.at(lo, hi, d);
    }
    __syncthreads();
    float mean = 0.f;
    for (int d = 0; d < D; ++d) mean += tm[d * SR_PIX];                                           // depth_net.py:76
    __syncthreads();
    for (int d = sl; d < D; d += SR_SL) { const float e = h.at(lo, hi, d) - mean; tm[d * SR_PIX] = pr[d * SR_PIX] * (e * e); }
    __syncthreads();
    float var = 0.f;
    for (int d = 0; d < D; ++d) var += tm[d * SR_PIX];                                            // :77
    if (!live || sl) return;
    const float half = ci_scale * sqrtf(fmaxf(var, 1e-12f));                                      // :77-78
    const float first = h.at(lo, hi, 0), last = h.at(lo, hi, D - 1);
    vol_range[(b * 2) * HW + p] = first; vol_range[(b * 2 + 1) * HW + p] = last;
    if (h.inv_depth) {                                                                            // :80-82
        ci[(b * 2) * HW + p] = 1.f / fminf(mean + half, first);
        ci[(b * 2 + 1) * HW + p] = 1.f / fmaxf(mean - half, last);
        depth[t] = 1.f / mean;
    } else {                                                                                      // :83
        ci[(b * 2) * HW + p] = fmaxf(mean - half, first);
        ci[(b * 2 + 1) * HW + p] = fminf(mean + half, last);
        depth[t] = mean;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
#define MVS_MAX_D 512   // k_softmax_regress keeps 2 x D x 16 floats in LDS: 64 KB at D = 512

static int range_check(const float* d_range, int hr, int wr, double ratio, int B, int D, int Ht, int Wt, HypRange* h, int inv_depth) {
    if (!d_range) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (B < 1 || D < 1 || Ht < 1 || Wt < 1 || hr < 1 || wr < 1) return gdb_fail(GDB_E_SHAPE, "bad search-range shape");
    float rscale = 1.f;
    if ((size_t)hr * wr > 1) {
        if (!(ratio > 0.0) || !std::isfinite(ratio)) return gdb_fail(GDB_E_BADARG, "search range: upsampling ratio %g", ratio);
        rscale = (float)(1.0 / ratio);
        // the source index of the last row / column stays far inside an int
        if (((double)(Ht > Wt ? Ht : Wt) + 0.5) * rscale >= 1e9) return gdb_fail(GDB_E_SHAPE, "search range: ratio %g is too small for the target", ratio);
    }
    *h = HypRange{d_range, hr, wr, D, inv_depth ? 1 : 0, rscale};
    return GDB_OK;
}

extern "C" int gdb_mvs_hypotheses(const float* d_range, int32_t hr, int32_t wr, double ratio, int32_t B, int32_t D, int32_t Ht, int32_t Wt,
                                  int32_t inv_depth, float* d_out, void* stream_) {
    if (!d_out) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    HypRange h;
    int rc = range_check(d_range, hr, wr, ratio, B, D, Ht, Wt, &h, inv_depth);
    if (rc != GDB_OK) return rc;
    const size_t n = (size_t)B * D * Ht * Wt;
    if ((size_t)Ht * Wt >= ((size_t)1 << 31) || (n + 255) / 256 >= ((size_t)1 << 31)) return gdb_fail(GDB_E_SHAPE, "hypotheses too large for the launch grid");
    hipLaunchKernelGGL(k_mvs_hypotheses, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, h, B, Ht, Wt, d_out);
    LAUNCH_CHECK("k_mvs_hypotheses");
    return GDB_OK;
}

static size_t al64(size_t n) { return (n + 63) / 64 * 64; }

struct StagePlan {
    bool pair;
    int tiles, nblk;
    size_t proj, pairs, cost, logits, cr_bytes, bytes;   // floats, except the byte counts
};

// shapes and the workspace split; every refusal of the stage that needs no pointer
static int stage_plan(int B, int V, int C, int Hs, int Ws, int D, int Ht, int Wt, int depth, int cin, int c, int cout, StagePlan* P) {
    if (B < 1 || V < 1 || C < 1 || Hs < 1 || Ws < 2 || D < 1 || Ht < 1 || Wt < 1) return gdb_fail(GDB_E_SHAPE, "bad cost-volume shape");
    if (V > GDB_MAX_VIEWS) return gdb_fail(GDB_E_SHAPE, "V=%d exceeds %d views", V, GDB_MAX_VIEWS);
    if (D > MVS_MAX_D) return gdb_fail(GDB_E_SHAPE, "D=%d exceeds the %d planes the fused softmax holds in LDS", D, MVS_MAX_D);
    if (cin != C) return gdb_fail(GDB_E_BADARG, "the U-Net takes %d channels, the source maps have %d", cin, C);
    if ((size_t)C * Hs * Ws >= ((size_t)1 << 32)) return gdb_fail(GDB_E_SHAPE, "source feature map too large for 32-bit offsets");
    const size_t plane_t = (size_t)Ht * Wt, tiles = (plane_t + 255) / 256, lim = ((size_t)1 << 31) - 8;
    if (plane_t >= lim || (size_t)B * tiles >= lim || (size_t)B * tiles * D >= lim) return gdb_fail(GDB_E_SHAPE, "cost volume too large for the launch grid");
    int rc = gdb_cost_reg_workspace_bytes(depth, cin, c, cout, B, D, Ht, Wt, &P->cr_bytes);
    if (rc != GDB_OK) return rc;
    P->pair = (C % 2) == 0 && V <= 4;   // as gdb_build_feature_volume_ws: the channel-pair form of the sweep
    P->tiles = (int)tiles; P->nblk = (int)((size_t)B * tiles * D);
    P->proj = al64((size_t)B * V * 12);
    P->pairs = P->pair ? al64((size_t)B * V * C * Hs * Ws) : 0;
    P->cost = al64((size_t)B * C * D * plane_t);
    P->logits = al64((size_t)B * D * plane_t);
    P->bytes = (P->proj + P->pairs + P->cost + P->logits) * sizeof(float) + P->cr_bytes;
    return GDB_OK;
}

extern "C" int gdb_mvs_stage_workspace_bytes(int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                                             int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, size_t* out_bytes) {
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    StagePlan P;
    int rc = stage_plan(B, V, C, Hs, Ws, D, Ht, Wt, depth, cin, base_channels, cout, &P);
    if (rc != GDB_OK) return rc;
    *out_bytes = P.bytes;
    return GDB_OK;
}

template <bool PAIR>
static void launch_sweep(int V, dim3 grid, hipStream_t st, const CostVolArgs& a, const HypRange& h) {
    const dim3 blk(256);
    switch (V) {
        case 1: hipLaunchKernelGGL((k_costvol_range<1, PAIR>), grid, blk, 0, st, a, h); break;
        case 2: hipLaunchKernelGGL((k_costvol_range<2, PAIR>), grid, blk, 0, st, a, h); break;
        case 3: hipLaunchKernelGGL((k_costvol_range<3, PAIR>), grid, blk, 0, st, a, h); break;
        case 4: hipLaunchKernelGGL((k_costvol_range<4, PAIR>), grid, blk, 0, st, a, h); break;
        default:
            if constexpr (!PAIR) {
                switch (V) {
                    case 5: hipLaunchKernelGGL((k_costvol_range<5, false>), grid, blk, 0, st, a, h); break;
                    case 6: hipLaunchKernelGGL((k_costvol_range<6, false>), grid, blk, 0, st, a, h); break;
                    case 7: hipLaunchKernelGGL((k_costvol_range<7, false>), grid, blk, 0, st, a, h); break;
                    default: hipLaunchKernelGGL((k_costvol_range<8, false>), grid, blk, 0, st, a, h); break;
                }
            }
    }
}

extern "C" int gdb_mvs_stage(const float* d_src_feat, const float* d_src_exts, const float* d_src_ints, const float* d_tar_exts,
                             const float* d_tar_ints, float feat_scale, float vol_scale, const float* d_range, int32_t hr, int32_t wr,
                             double ratio, int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                             int32_t inv_depth, float ci_scale, int32_t depth, int32_t cin, int32_t base_channels, int32_t cout,
                             const float* d_packed, void* d_ws, size_t ws_bytes, float* d_volume, float* d_depth, float* d_ci,
                             float* d_vol_range, void* stream_) {
    if (!d_src_feat || !d_src_exts || !d_src_ints || !d_tar_exts || !d_tar_ints || !d_range || !d_packed || !d_ws || !d_volume || !d_depth ||
        !d_ci || !d_vol_range)
        return gdb_fail(GDB_E_BADARG, "NULL pointer");
    StagePlan P;
    int rc = stage_plan(B, V, C, Hs, Ws, D, Ht, Wt, depth, cin, base_channels, cout, &P);
    if (rc != GDB_OK) return rc;
    HypRange h;
    if ((rc = range_check(d_range, hr, wr, ratio, B, D, Ht, Wt, &h, inv_depth)) != GDB_OK) return rc;
    if (ws_bytes < P.bytes) return gdb_fail(GDB_E_WORKSPACE, "mvs stage: workspace of %zu bytes, %zu needed", ws_bytes, P.bytes);
    float* proj = (float*)d_ws;
    float* pairs = proj + P.proj;
    float* cost = pairs + P.pairs;
    float* logits = cost + P.cost;
    void* cr_ws = logits + P.logits;
    // the U-Net's own refusals (its launch grids) before anything is launched
    if ((rc = gdb_cost_reg_run_(depth, cin, base_channels, cout, cost, B, D, Ht, Wt, d_packed, cr_ws, P.cr_bytes, d_volume, logits, CR_RUN_CHECK,
                                stream_)) != GDB_OK)
        return rc;
    hipStream_t st = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_cascade_proj, dim3((B * V + 63) / 64), dim3(64), 0, st, B, V, d_src_exts, d_src_ints, d_tar_exts, d_tar_ints, feat_scale,
                       vol_scale, proj);
    LAUNCH_CHECK("k_cascade_proj");
    if (P.pair && (rc = gdb_costvol_pairs_(d_src_feat, pairs, (size_t)Hs * Ws, (size_t)B * V * (C / 2), st)) != GDB_OK) return rc;
    CostVolArgs a{B, V, C, Hs, Ws, D, Ht, Wt, inv_depth ? 1 : 0, C, P.tiles, P.nblk, P.pair ? pairs : d_src_feat, proj, nullptr, cost};
    const dim3 grid((P.nblk + 7) / 8 * 8);
    if (P.pair) launch_sweep<true>(V, grid, st, a, h); else launch_sweep<false>(V, grid, st, a, h);
    LAUNCH_CHECK("k_costvol_range");
    if ((rc = gdb_cost_reg_run_(depth, cin, base_channels, cout, cost, B, D, Ht, Wt, d_packed, cr_ws, P.cr_bytes, d_volume, logits, CR_RUN_LOGITS,
                                stream_)) != GDB_OK)
        return rc;
    const size_t n = (size_t)B * Ht * Wt;
    hipLaunchKernelGGL(k_softmax_regress, dim3((unsigned)((n + SR_PIX - 1) / SR_PIX)), dim3(64), (size_t)2 * D * SR_PIX * sizeof(float), st, h,
                       logits, B, Ht, Wt, ci_scale, d_depth, d_ci, d_vol_range);
    LAUNCH_CHECK("k_softmax_regress");
    return GDB_OK;
}
