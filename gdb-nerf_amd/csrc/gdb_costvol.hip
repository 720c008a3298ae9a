// "Next" rows of SURVEY.md §8(f) on the same bar as the hot path:
//   N2  build_feature_volume  (reference networks/gdb_nerf/depth_net.py:424-476): plane-sweep homography
//       warp of the source feature maps onto the target frustum + biased variance over views;
//   N4  depth_regression      (depth_net.py:479-514): soft-argmax depth and confidence interval.
// Exact fp32 (-ffp-contract=off), gather-bound: one lane per voxel column x, so the NCHW source maps are
// read along x (8-byte x-pair loads) and the NCDHW volume is written in 256-B row segments.
#include "gdb_internal.h"
#include <cstdlib>

#include "gdb_costvol_body.h"

__global__ void k_costvol_proj(int B, int V, const float* __restrict__ src_exts, const float* __restrict__ src_ints,
                               const float* __restrict__ tar_exts, const float* __restrict__ tar_ints, float* __restrict__ proj) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * V) return;
    costvol_proj_one<false>(t, V, src_exts, src_ints, tar_exts, tar_ints, 1.f, 1.f, proj);
}

// Channel-pair re-layout of the source maps for the PAIR form of k_costvol: (B*V, C, Hs, Ws) -> (B*V, C / 2, Hs, Ws, 2), so that one
// 16-byte load at (y, x) holds the x pair of TWO channels.  One thread per (map, channel pair, y, x): two coalesced 4-byte loads, one
// 8-byte store.  15.7 MB at the 256x320 stage: ~5 us, a third of what it saves the sweep (profiles/r04/costvol_pair_layout.txt).
__global__ void __launch_bounds__(256) k_costvol_pairs(const float* __restrict__ src, float2* __restrict__ dst, size_t plane, size_t npairs) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npairs * plane) return;
    const size_t pc = t / plane, p = t - pc * plane;   // pc = map * (C / 2) + channel pair
    dst[t] = make_float2(src[(2 * pc) * plane + p], src[(2 * pc + 1) * plane + p]);
}

template <int VT, bool PAIR>
__global__ void __launch_bounds__(256) k_costvol(CostVolArgs a) { costvol_body<VT, PAIR>(a, HypTensor{}); }

// the re-layout alone, for the cascade stage (gdb_cascade.hip) which runs its own form of the sweep on the copy
int gdb_costvol_pairs_(const float* d_src, float* d_pair_ws, size_t plane, size_t npairs, hipStream_t st) {
    hipLaunchKernelGGL(k_costvol_pairs, dim3((unsigned)((npairs * plane + 255) / 256)), dim3(256), 0, st, d_src, (float2*)d_pair_ws, plane, npairs);
    LAUNCH_CHECK("k_costvol_pairs");
    return GDB_OK;
}

static int build_feature_volume(const float* d_src_feat, const float* d_src_exts, const float* d_src_ints,
                                const float* d_tar_exts, const float* d_tar_ints, const float* d_depth_values,
                                int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                                int32_t inv_depth, float* d_proj_ws, float* d_pair_ws, float* d_out, void* stream_);

extern "C" int gdb_build_feature_volume(const float* d_src_feat, const float* d_src_exts, const float* d_src_ints,
                                        const float* d_tar_exts, const float* d_tar_ints, const float* d_depth_values,
                                        int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                                        int32_t inv_depth, float* d_proj_ws, float* d_out, void* stream_) {
    return build_feature_volume(d_src_feat, d_src_exts, d_src_ints, d_tar_exts, d_tar_ints, d_depth_values, B, V, C, Hs, Ws, D, Ht, Wt, inv_depth,
                                d_proj_ws, nullptr, d_out, stream_);
}

extern "C" int gdb_build_feature_volume_ws(const float* d_src_feat, const float* d_src_exts, const float* d_src_ints,
                                           const float* d_tar_exts, const float* d_tar_ints, const float* d_depth_values,
                                           int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                                           int32_t inv_depth, float* d_proj_ws, float* d_pair_ws, float* d_out, void* stream_) {
    return build_feature_volume(d_src_feat, d_src_exts, d_src_ints, d_tar_exts, d_tar_ints, d_depth_values, B, V, C, Hs, Ws, D, Ht, Wt, inv_depth,
                                d_proj_ws, d_pair_ws, d_out, stream_);
}

static int build_feature_volume(const float* d_src_feat, const float* d_src_exts, const float* d_src_ints,
                                const float* d_tar_exts, const float* d_tar_ints, const float* d_depth_values,
                                int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                                int32_t inv_depth, float* d_proj_ws, float* d_pair_ws, float* d_out, void* stream_) {
    if (!d_src_feat || !d_src_exts || !d_src_ints || !d_tar_exts || !d_tar_ints || !d_depth_values || !d_proj_ws || !d_out)
        return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (B < 1 || V < 1 || C < 1 || Hs < 1 || Ws < 2 || D < 1 || Ht < 1 || Wt < 1) return gdb_fail(GDB_E_SHAPE, "bad cost-volume shape");
    if (V > GDB_MAX_VIEWS) return gdb_fail(GDB_E_SHAPE, "V=%d exceeds %d views", V, GDB_MAX_VIEWS);
    if ((size_t)C * Hs * Ws >= ((size_t)1 << 32)) return gdb_fail(GDB_E_SHAPE, "source feature map too large for 32-bit offsets");
    // channels per thread: all of them (splitting channels over more threads measured no faster on MI355X:
    // 44 / 118 us at the two DTU stage shapes for cpt = 32, 8, 4); GDB_COSTVOL_CPT overrides in the diagnostic build
    int cpt = C;
#ifdef GDB_DIAG  // diagnostic build only: the product entry reads no environment
    if (getenv("GDB_COSTVOL_CPT")) cpt = atoi(getenv("GDB_COSTVOL_CPT")) > 0 ? atoi(getenv("GDB_COSTVOL_CPT")) : C;
#endif
    // every refusal comes before the first launch; the plane and the block count in 64 bits (Ht * Wt may not fit an int, and the grid
    // is the block count rounded up to a multiple of 8)
    const size_t plane_t = (size_t)Ht * Wt, tiles_ = (plane_t + 255) / 256;
    const int groups = (C + cpt - 1) / cpt;
    const size_t lim = ((size_t)1 << 31) - 8;   // each partial product stays below 2^62
    if (plane_t >= lim || (size_t)B * tiles_ >= lim || (size_t)B * tiles_ * D >= lim || (size_t)B * tiles_ * D * groups >= lim)
        return gdb_fail(GDB_E_SHAPE, "cost volume too large for the launch grid");
    const int tiles = (int)tiles_, nblk = B * tiles * D * groups;
    hipStream_t st = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_costvol_proj, dim3((B * V + 63) / 64), dim3(64), 0, st, B, V, d_src_exts, d_src_ints, d_tar_exts, d_tar_ints, d_proj_ws);
    LAUNCH_CHECK("k_costvol_proj");
    // The channel-pair form: given C * Hs * Ws * V * B floats of scratch (gdb_build_feature_volume_ws) and an even channel count, the
    // source maps are re-laid once ([c / 2][y][x][2], k_costvol_pairs) and the sweep loads 16 bytes per (channel PAIR, row, view)
    // instead of 8 per (channel, row, view): half the load instructions of a kernel the texture addresser bounds.  Bit-identical.
    const bool pair = d_pair_ws != nullptr && (C % 2) == 0 && (cpt % 2) == 0 && V <= 4;   // (5..8 views: the doubled tap state leaves the registers)
    if (pair) {
        const size_t plane = (size_t)Hs * Ws, npairs = (size_t)B * V * (C / 2);
        const int rc = gdb_costvol_pairs_(d_src_feat, d_pair_ws, plane, npairs, st);
        if (rc != GDB_OK) return rc;
    }
    CostVolArgs a{B, V, C, Hs, Ws, D, Ht, Wt, inv_depth, cpt, tiles, nblk, pair ? d_pair_ws : d_src_feat, d_proj_ws, d_depth_values, d_out};
    const dim3 grid((nblk + 7) / 8 * 8), blk(256);
    if (pair) {
        switch (V) {
            case 1: hipLaunchKernelGGL((k_costvol<1, true>), grid, blk, 0, st, a); break;
            case 2: hipLaunchKernelGGL((k_costvol<2, true>), grid, blk, 0, st, a); break;
            case 3: hipLaunchKernelGGL((k_costvol<3, true>), grid, blk, 0, st, a); break;
            default: hipLaunchKernelGGL((k_costvol<4, true>), grid, blk, 0, st, a); break;
        }
    } else {
        switch (V) {
            case 1: hipLaunchKernelGGL((k_costvol<1, false>), grid, blk, 0, st, a); break;
            case 2: hipLaunchKernelGGL((k_costvol<2, false>), grid, blk, 0, st, a); break;
            case 3: hipLaunchKernelGGL((k_costvol<3, false>), grid, blk, 0, st, a); break;
            case 4: hipLaunchKernelGGL((k_costvol<4, false>), grid, blk, 0, st, a); break;
            case 5: hipLaunchKernelGGL((k_costvol<5, false>), grid, blk, 0, st, a); break;
            case 6: hipLaunchKernelGGL((k_costvol<6, false>), grid, blk, 0, st, a); break;
            case 7: hipLaunchKernelGGL((k_costvol<7, false>), grid, blk, 0, st, a); break;
            default: hipLaunchKernelGGL((k_costvol<8, false>), grid, blk, 0, st, a); break;
        }
    }
    LAUNCH_CHECK("k_costvol");
    return GDB_OK;
}

// ---- N4  depth_regression ---------------------------------------------------------------------
__global__ void k_depth_regression(int B, int D, size_t HW, float ci_scale, int inv_depth, const float* __restrict__ dv,
                                   const float* __restrict__ prob, float* __restrict__ depth, float* __restrict__ ci) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)B * HW) return;
    size_t b = t / HW, p = t - b * HW;
    const float* dvb = dv + b * D * HW + p; const float* pb = prob + b * D * HW + p;
    float mean = 0.f;
    for (int d = 0; d < D; ++d) mean += pb[d * HW] * dvb[d * HW];                          // :495
    float var = 0.f;
    for (int d = 0; d < D; ++d) { float e = dvb[d * HW] - mean; var += pb[d * HW] * (e * e); }  // :496
    float half = ci_scale * sqrtf(fmaxf(var, 1e-12f));                                       // :497-500
    float first = dvb[0], last = dvb[(size_t)(D - 1) * HW];
    if (inv_depth) {                                                                          // :502-507
        ci[(b * 2) * HW + p] = 1.f / fminf(mean + half, first);
        ci[(b * 2 + 1) * HW + p] = 1.f / fmaxf(mean - half, last);
        depth[t] = 1.f / mean;
    } else {                                                                                  // :508-512
        ci[(b * 2) * HW + p] = fmaxf(mean - half, first);
        ci[(b * 2 + 1) * HW + p] = fminf(mean + half, last);
        depth[t] = mean;
    }
}

extern "C" int gdb_depth_regression(const float* d_depth_values, const float* d_depth_prob, int32_t B, int32_t D, int32_t H, int32_t W,
                                    float ci_scale, int32_t inv_depth, float* d_depth, float* d_ci, void* stream_) {
    if (!d_depth_values || !d_depth_prob || !d_depth || !d_ci) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (B < 1 || D < 1 || H < 1 || W < 1) return gdb_fail(GDB_E_SHAPE, "bad shape");
    size_t HW = (size_t)H * W, n = (size_t)B * HW;
    hipLaunchKernelGGL(k_depth_regression, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, B, D, HW, ci_scale,
                       inv_depth, d_depth_values, d_depth_prob, d_depth, d_ci);
    LAUNCH_CHECK("k_depth_regression");
    return GDB_OK;
}
