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
#include "gdb_costreg_body.h"

template <int MODE, int E, bool NC, int ZS, int EPI>
__global__ void __launch_bounds__(256) k_costreg_conv(CrArgs a) { costreg_conv_body<MODE, E, NC, ZS, EPI>(a); }

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
