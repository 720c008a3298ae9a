// The depth net's train-time stage render (reference networks/gdb_nerf/depth_net.py:97-114, 248-298): the auxiliary MVSNeRF-style
// NeRF of one cascade stage and its un-normalised alpha composite, forward and backward, fp32 throughout.
//
//   forward   rgb_map[ray] = sum_i alpha_i T_i c_i,  alpha = 1 - e^-sigma,  T_i = prod_{j<i} (1 - alpha_j + 1e-10)
//             (sigma_i, c_i) = NeRF(vox_feat[i], img_feat_rgb_dir[i]) per sample; c_i blends the source colours x[..., -7:-4] by a softmax
//             over the views.  No rgbs prefix, no feat_head, nothing normalised; inputs are sample-major, (N, V, C_f+3+4).
//   backward  nothing is saved by the forward: the tile's activations are recomputed, the chain of activation gradients runs per
//             tile, dW = dY^T [X | 1] accumulates in registers across a workgroup's tiles (persistent grid), every workgroup writes ONE
//             partial in packed layout, and k_stage_reduce adds the partials in workgroup order in double.  No atomics.
//
// A tile is a whole number of rays (the composite never crosses a tile): up to 16 samples and up to 64 (view, sample) rows.  Every
// linear layer with more than one output runs on v_mfma_f32_16x16x4_f32 from the tile's LDS image - the forward products Y = X W^T,
// the backward products dX = dY W and dW = dY^T X alike; the one-output layers (agg_w_fc, sigma, color.2) and view_fc (K = 4) are
// dot products on the vector ALUs.  The weights are read from the packed buffer in global memory (55 KiB at feat_dim 32: they stay
// in the caches); the tile's LDS image leaves no room for them beside it.
//
// Derivative conventions (shared with k_mlp_bwd): ReLU'(0) = 0; softplus has threshold 20; the variance divisor is
// V - 1; both view softmaxes are over relu(score); the colour channels feed the blend AND the layers, their gradient is the sum.
#include "gdb_dw_tiles.h"
#include <cstring>
#include <type_traits>

#define SN_THREADS 256
#define SN_MAX_WG 256
#define SN_RM 64     // (view, sample) rows of a tile at most
#define SN_SM 16     // samples of a tile at most
#define SN_XW (GDB_HID + GDB_HD)   // 88: [x | vox | im], the shared columns of color.0

// ---- packed weights (float offsets; every block 4-float aligned), C = feat_dim + 3 ----
template <int C> struct SnW {
    static constexpr int W0IN = SN_XW + C + 4;
    static constexpr int VIEW_W = 0;                                  // (C,4)
    static constexpr int VIEW_B = pw_al(VIEW_W + C * 4);
    static constexpr int GLOB_W = pw_al(VIEW_B + C);                  // (32,3C)
    static constexpr int GLOB_B = pw_al(GLOB_W + GDB_GF * 3 * C);
    static constexpr int AGG_W = pw_al(GLOB_B + GDB_GF);              // (1,32)
    static constexpr int AGG_B = pw_al(AGG_W + GDB_GF);
    static constexpr int FC_W = pw_al(AGG_B + 1);                     // (16,32)
    static constexpr int FC_B = pw_al(FC_W + GDB_IM * GDB_GF);
    static constexpr int LR0_W = pw_al(FC_B + GDB_IM);                // (64,24)
    static constexpr int LR0_B = pw_al(LR0_W + GDB_HID * GDB_HD);
    static constexpr int SIG_W = pw_al(LR0_B + GDB_HID);              // (1,64)
    static constexpr int SIG_B = pw_al(SIG_W + GDB_HID);
    static constexpr int C0_W = pw_al(SIG_B + 1);                     // (64,88+C+4)
    static constexpr int C0_B = pw_al(C0_W + GDB_HID * W0IN);
    static constexpr int C2_W = pw_al(C0_B + GDB_HID);                // (1,64)
    static constexpr int C2_B = pw_al(C2_W + GDB_HID);
    static constexpr int FLOATS = (C2_B + 1 + 63) / 64 * 64;
};

// ---- LDS image of a tile (float offsets).  Row r of a per-view array = view r / TSP, sample r % TSP. ----
template <int C> struct SnL {
    static constexpr int XT = 0;                        // [RM][C+5]  [feat C | dir 4 | 1]: the view's input row; X of color.0's tail, view_fc
    static constexpr int GV = XT + SN_RM * (C + 5);     // [RM][C+1]  [g_v | 1]: X of global_fc's per-view columns
    static constexpr int VP = GV + SN_RM * (C + 1);     // [RM][C]    view_fc pre-activation, then its gradient
    static constexpr int TG = VP + SN_RM * C;           // [RM][C]    global_fc^T dY, per view
    static constexpr int G = TG + SN_RM * C;            // [RM][33]   [relu(global_fc) | 1]
    static constexpr int DA = G + SN_RM * 33;           // [RM][32]   dY of global_fc
    static constexpr int HID = DA + SN_RM * 32;         // [RM][65]   [relu(color.0) | 1]
    static constexpr int DHID = HID + SN_RM * 65;       // [RM][64]   dY of color.0
    static constexpr int ROW = DHID + SN_RM * 64;       // [RM][8]    per (view, sample) scalars
    static constexpr int DT = ROW + SN_RM * 8;          // [RM][C+4]  gradient of the view's row through the layers
    static constexpr int VM = DT + SN_RM * (C + 4);     // [SM][2C]   [var | mean]
    static constexpr int DVM = VM + SN_SM * 2 * C;      // [SM][2C]
    static constexpr int SDA = DVM + SN_SM * 2 * C;     // [SM][32]   sum over views of dY(global_fc)
    static constexpr int AGG = SDA + SN_SM * 32;        // [SM][33]   [agg | 1]
    static constexpr int DAGG = AGG + SN_SM * 33;       // [SM][32]
    static constexpr int DFC = DAGG + SN_SM * 32;       // [SM][16]   dY of fc
    static constexpr int XH = DFC + SN_SM * 16;         // [SM][89]   [x64 | vox8 | im16 | 1]
    static constexpr int DX = XH + SN_SM * 89;          // [SM][88]   gradient of [x | vox | im]; columns 0..63 become dY of lr0
    static constexpr int SG = DX + SN_SM * SN_XW;       // [SM]       dY of sigma
    static constexpr int SDH = SG + SN_SM;              // [SM][64]   sum over views of dY(color.0)
    static constexpr int P0 = SDH + SN_SM * 64;         // [SM][64]   the shared columns' part of a pre-activation (global_fc, color.0)
    static constexpr int SMP = P0 + SN_SM * 64;         // [SM][16]   per-sample scalars
    static constexpr int END = SMP + SN_SM * 16;
};
static_assert(SnL<35>::END * sizeof(float) <= 160 * 1024, "the tile does not fit the LDS of a CU");
enum { ROW_SPRE = 0, ROW_A = 1, ROW_DS = 2, ROW_UPRE = 3, ROW_WV = 4, ROW_DU = 5, ROW_TMP = 6 };
enum { SMP_SIGMA = 0, SMP_SPRE = 1, SMP_RGB = 2 /* 3 */, SMP_W = 5, SMP_T = 6, SMP_E = 7, SMP_GRGB = 8 /* 3 */ };

// ---- the products dW = dY^T [X | 1] ----
#define SN_MAX_TILES 80
typedef DwTable<SN_MAX_TILES> SnTable;

template <int C> constexpr SnTable sn_make_table() {
    using L = SnL<C>; using W = SnW<C>;
    const DwProduct prods[10] = {
        // dy               ldy M        x           ldx    Nw      xone          pv w                 ldw      b
        {L::VP,             C,  C,       L::XT + C,  C + 5, 4,      L::XT + C + 4, 1, W::VIEW_W,        4,       W::VIEW_B},   // view_fc
        {L::DA,             32, GDB_GF,  L::GV,      C + 1, C,      L::GV + C,    1, W::GLOB_W,        3 * C,   W::GLOB_B},   // global_fc, per-view columns
        {L::SDA,            32, GDB_GF,  L::VM,      2 * C, 2 * C,  -1,           0, W::GLOB_W + C,    3 * C,   -1},          // global_fc, [var | mean]
        {L::ROW + ROW_DS,   8,  1,       L::G,       33,    GDB_GF, L::G + 32,    1, W::AGG_W,         GDB_GF,  W::AGG_B},    // agg_w_fc
        {L::DFC,            16, GDB_IM,  L::AGG,     33,    GDB_GF, L::AGG + 32,  0, W::FC_W,          GDB_GF,  W::FC_B},     // fc
        {L::DX,             SN_XW, GDB_HID, L::XH + 64, 89, GDB_HD, L::XH + 88,   0, W::LR0_W,         GDB_HD,  W::LR0_B},    // lr0
        {L::SG,             1,  1,       L::XH,      89,    GDB_HID, L::XH + 88,  0, W::SIG_W,         GDB_HID, W::SIG_B},    // sigma
        {L::SDH,            64, GDB_HID, L::XH,      89,    SN_XW,  -1,           0, W::C0_W,          W::W0IN, -1},          // color.0, [x | vox | im]
        {L::DHID,           64, GDB_HID, L::XT,      C + 5, C + 4,  L::XT + C + 4, 1, W::C0_W + SN_XW, W::W0IN, W::C0_B},     // color.0, per-view tail
        {L::ROW + ROW_DU,   8,  1,       L::HID,     65,    GDB_HID, L::HID + 64, 1, W::C2_W,          GDB_HID, W::C2_B},     // color.2
    };
    return dw_make_table<SN_MAX_TILES>(prods);
}
template <int C> struct SnTab { static constexpr SnTable host = sn_make_table<C>(); static constexpr int per_wave = (host.n + 3) / 4; };
static_assert(SnTab<35>::host.n <= SN_MAX_TILES && SnTab<19>::host.n <= SN_MAX_TILES && SnTab<11>::host.n <= SN_MAX_TILES, "more output tiles than table slots");
template <int C> __constant__ SnTable c_sn_table = SnTab<C>::host;

#define SN_DOT _Pragma("unroll 4")
#define SN_VIEWS _Pragma("nounroll")
#define SN_FOR(i, count) for (int i = tid; i < (count); i += SN_THREADS)

// Y[row][m] = op(init + sum_k X[row][k] Wm[m * sm + k * sk]) for row < rows16 (a multiple of 16), m < M, on the matrix cores: X and Y in
// LDS, the weights in global memory.  init = lds[init + (row % imod) * ldi + m] when init >= 0 (may be Y itself: every element is read
// and written by the same lane), else bias[m] (or 0).  Forward layers: sm = row stride of W, sk = 1.  dX = dY W: sm = 1, sk = row stride.
// Output tiles go round the four waves; A row i feeds D row i only, so rows past the tile's last hold whatever they hold.
// (k_mlp_bwd has the same layers as fp32 dot products on the vector ALUs: another summation order, its own bits - not shared.)
__device__ __forceinline__ void sn_gemm(float* __restrict__ lds, int y, int ldy, int x, int ldx, int K, int M, int rows16,
                                        const float* __restrict__ wm, int sm, int sk, const float* __restrict__ bias,
                                        int init, int ldi, int imod, bool relu, int wave, int lane) {
    const int li = lane & 15, kq = lane >> 4;
    const int mt = (M + 15) >> 4, tiles = (rows16 >> 4) * mt;
    for (int t = wave; t < tiles; t += 4) {
        const int r0 = (t / mt) << 4, m0 = (t % mt) << 4;
        const int m = m0 + li;
        const bool mok = m < M;
        f32x4 acc;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = r0 + 4 * kq + e;
            float v = 0.f;
            if (mok) v = init >= 0 ? lds[init + (row % imod) * ldi + m] : (bias ? bias[m] : 0.f);
            acc[e] = v;
        }
        const float* wp = wm + (mok ? m : 0) * sm;
        const int xo = x + (r0 + li) * ldx;
        SN_VIEWS
        for (int k = 0; k < K; k += 4) {
            const int kk = k + kq;
            const bool kok = kk < K;
            float a = lds[xo + (kok ? kk : 0)];
            float b = wp[(kok ? kk : 0) * sk];
            a = kok ? a : 0.f;
            b = (kok && mok) ? b : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
        if (mok) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = r0 + 4 * kq + e;
                lds[y + row * ldy + m] = relu ? relu_f(acc[e]) : acc[e];
            }
        }
    }
}

// One workgroup of 4 waves walks tiles of `rpt` rays (tile t belongs to workgroup t mod grid).  TS = rpt * S samples, TSP = TS rounded up
// to 4 (the dW products step over rows by 4), R = V * TSP <= 64 (view, sample) rows.
template <int C, bool BWD>
__global__ void __launch_bounds__(SN_THREADS)
k_stage_nerf(const float* __restrict__ pw, int V, int S, int viewdir, int rpt, const float* __restrict__ vox, const float* __restrict__ xin,
             int64_t n_rays, float* __restrict__ rgb_map, float* __restrict__ sigma_out, float* __restrict__ rgb_out,
             const float* __restrict__ g_map, float* __restrict__ g_vox, float* __restrict__ g_xin, float* __restrict__ partials) {
    using L = SnL<C>; using W = SnW<C>;
    __shared__ float lds[L::END];
    constexpr int P = C + 4;                 // floats of a view's input row
    constexpr int PER_WAVE = BWD ? SnTab<C>::per_wave : 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int TS = rpt * S, TSP = (TS + 3) & ~3;
    const int R = V * TSP, R16 = (R + 15) & ~15;
    const float Vf = (float)V;
    const int64_t n = n_rays * S;
    const int64_t ntiles = (n_rays + rpt - 1) / rpt;

    f32x4 acc[PER_WAVE];
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t ray0 = t * rpt, base = ray0 * S;
        // ---- 0. inputs.  Rows past the last ray, the pad rows of a view's block and the rows past R read as zeros
        SN_FOR(k, R16 * (C + 5)) {
            int r = k / (C + 5), c = k % (C + 5), v = r / TSP, s = r % TSP; int64_t i = base + s;
            float val = 1.f;
            if (c < P) val = (r < R && s < TS && i < n) ? xin[((size_t)i * V + v) * P + c] : 0.f;
            lds[L::XT + r * (C + 5) + c] = val;
        }
        SN_FOR(k, SN_SM * 9) {
            int s = k / 9, c = k % 9; int64_t i = base + s;
            lds[L::XH + s * 89 + (c < 8 ? GDB_HID + c : 88)] = c < 8 ? ((s < TS && i < n) ? vox[i * GDB_CV + c] : 0.f) : 1.f;
        }
        __syncthreads();
        // ---- 1. g_v = feat + relu(view_fc dir)      depth_net.py:258-261
        SN_FOR(k, R * (C + 1)) {
            int r = k / (C + 1), c = k % (C + 1);
            float a = 0.f, g = 1.f;
            if (c < C) {
                const float* tl = lds + L::XT + r * (C + 5);
                if (viewdir) {
                    a = pw[W::VIEW_B + c];
                    a = fmaf(pw[W::VIEW_W + 4 * c + 0], tl[C + 0], a);
                    a = fmaf(pw[W::VIEW_W + 4 * c + 1], tl[C + 1], a);
                    a = fmaf(pw[W::VIEW_W + 4 * c + 2], tl[C + 2], a);
                    a = fmaf(pw[W::VIEW_W + 4 * c + 3], tl[C + 3], a);
                }
                g = tl[c] + relu_f(a);
                lds[L::VP + r * C + c] = a;
            }
            lds[L::GV + r * (C + 1) + c] = g;
        }
        __syncthreads();
        // ---- 2. mean / unbiased variance over views      :263
        SN_FOR(k, SN_SM * C) {
            int s = k / C, c = k % C;
            float m = 0.f, vr = 0.f;
            if (s < TSP) {
                SN_VIEWS
                for (int v = 0; v < V; ++v) m += lds[L::GV + (v * TSP + s) * (C + 1) + c];
                m = m / Vf;
                SN_VIEWS
                for (int v = 0; v < V; ++v) { float d = lds[L::GV + (v * TSP + s) * (C + 1) + c] - m; vr += d * d; }
                vr = vr / (Vf - 1.f);
            }
            lds[L::VM + s * 2 * C + c] = vr;
            lds[L::VM + s * 2 * C + C + c] = m;
        }
        __syncthreads();
        // ---- 3. G_v = relu(global_fc [g_v | var | mean]): the shared columns once per sample, then the view's own      :267-268
        sn_gemm(lds, L::P0, 64, L::VM, 2 * C, 2 * C, GDB_GF, 16, pw + W::GLOB_W + C, 3 * C, 1, pw + W::GLOB_B, -1, 0, 1, false, wave, lane);
        __syncthreads();
        sn_gemm(lds, L::G, 33, L::GV, C + 1, C, GDB_GF, R16, pw + W::GLOB_W, 3 * C, 1, nullptr, L::P0, 64, TSP, true, wave, lane);
        SN_FOR(r, R16) lds[L::G + r * 33 + 32] = 1.f;
        __syncthreads();
        // ---- 4. view scores and their softmax over relu(score)      :269
        SN_FOR(r, R) {
            float sv = pw[W::AGG_B];
            SN_DOT
            for (int j = 0; j < GDB_GF; ++j) sv = fmaf(pw[W::AGG_W + j], lds[L::G + r * 33 + j], sv);
            lds[L::ROW + r * 8 + ROW_SPRE] = sv;
        }
        __syncthreads();
        SN_FOR(s, TSP) {
            float m = relu_f(lds[L::ROW + s * 8 + ROW_SPRE]);
            SN_VIEWS
            for (int v = 1; v < V; ++v) m = fmaxf(m, relu_f(lds[L::ROW + (v * TSP + s) * 8 + ROW_SPRE]));
            float sum = 0.f;
            SN_VIEWS
            for (int v = 0; v < V; ++v) { float e = expf(relu_f(lds[L::ROW + (v * TSP + s) * 8 + ROW_SPRE]) - m); lds[L::ROW + (v * TSP + s) * 8 + ROW_A] = e; sum += e; }
            SN_VIEWS
            for (int v = 0; v < V; ++v) lds[L::ROW + (v * TSP + s) * 8 + ROW_A] /= sum;
        }
        __syncthreads();
        // ---- 5. agg = sum_v G_v a_v      :270
        SN_FOR(k, SN_SM * 33) {
            int s = k / 33, j = k % 33;
            float a = 1.f;
            if (j < GDB_GF) {
                a = 0.f;
                if (s < TSP) {
                    SN_VIEWS
                    for (int v = 0; v < V; ++v) a += lds[L::G + (v * TSP + s) * 33 + j] * lds[L::ROW + (v * TSP + s) * 8 + ROW_A];
                }
            }
            lds[L::AGG + s * 33 + j] = a;
        }
        __syncthreads();
        // ---- 6. im = relu(fc agg)      :272
        sn_gemm(lds, L::XH + GDB_HID + GDB_CV, 89, L::AGG, 33, GDB_GF, GDB_IM, 16, pw + W::FC_W, GDB_GF, 1, pw + W::FC_B, -1, 0, 1, true, wave, lane);
        __syncthreads();
        // ---- 7. x = relu(lr0 [vox | im])      :288-289
        sn_gemm(lds, L::XH, 89, L::XH + GDB_HID, 89, GDB_HD, GDB_HID, 16, pw + W::LR0_W, GDB_HD, 1, pw + W::LR0_B, -1, 0, 1, true, wave, lane);
        __syncthreads();
        // ---- 8. sigma = softplus(sigma.0 x); hidden rows of color.0: the shared columns once per sample, then the view's tail     :290-295
        SN_FOR(s, SN_SM) {
            float sg = pw[W::SIG_B];
            SN_DOT
            for (int j = 0; j < GDB_HID; ++j) sg = fmaf(pw[W::SIG_W + j], lds[L::XH + s * 89 + j], sg);
            lds[L::SMP + s * 16 + SMP_SPRE] = sg;
            lds[L::SMP + s * 16 + SMP_SIGMA] = softplus_t20(sg);
        }
        sn_gemm(lds, L::P0, 64, L::XH, 89, SN_XW, GDB_HID, 16, pw + W::C0_W, W::W0IN, 1, pw + W::C0_B, -1, 0, 1, false, wave, lane);
        __syncthreads();
        sn_gemm(lds, L::HID, 65, L::XT, C + 5, P, GDB_HID, R16, pw + W::C0_W + SN_XW, W::W0IN, 1, nullptr, L::P0, 64, TSP, true, wave, lane);
        SN_FOR(r, R16) lds[L::HID + r * 65 + 64] = 1.f;
        __syncthreads();
        // ---- 9. blend scores, their softmax over relu(score), the sample's colour      :295-296
        SN_FOR(r, R) {
            float u = pw[W::C2_B];
            SN_DOT
            for (int j = 0; j < GDB_HID; ++j) u = fmaf(pw[W::C2_W + j], lds[L::HID + r * 65 + j], u);
            lds[L::ROW + r * 8 + ROW_UPRE] = u;
        }
        __syncthreads();
        SN_FOR(s, TSP) {
            float m = relu_f(lds[L::ROW + s * 8 + ROW_UPRE]);
            SN_VIEWS
            for (int v = 1; v < V; ++v) m = fmaxf(m, relu_f(lds[L::ROW + (v * TSP + s) * 8 + ROW_UPRE]));
            float sum = 0.f;
            SN_VIEWS
            for (int v = 0; v < V; ++v) { float e = expf(relu_f(lds[L::ROW + (v * TSP + s) * 8 + ROW_UPRE]) - m); lds[L::ROW + (v * TSP + s) * 8 + ROW_WV] = e; sum += e; }
            float c0 = 0.f, c1 = 0.f, c2 = 0.f;
            SN_VIEWS
            for (int v = 0; v < V; ++v) {
                const int r = v * TSP + s;
                float w = lds[L::ROW + r * 8 + ROW_WV] / sum;
                lds[L::ROW + r * 8 + ROW_WV] = w;
                c0 += lds[L::XT + r * (C + 5) + C - 3] * w;
                c1 += lds[L::XT + r * (C + 5) + C - 2] * w;
                c2 += lds[L::XT + r * (C + 5) + C - 1] * w;
            }
            lds[L::SMP + s * 16 + SMP_RGB + 0] = c0; lds[L::SMP + s * 16 + SMP_RGB + 1] = c1; lds[L::SMP + s * 16 + SMP_RGB + 2] = c2;
            const int64_t i = base + s;
            if (!BWD && s < TS && i < n) {
                if (sigma_out) sigma_out[i] = lds[L::SMP + s * 16 + SMP_SIGMA];
                if (rgb_out) { rgb_out[i * 3 + 0] = c0; rgb_out[i * 3 + 1] = c1; rgb_out[i * 3 + 2] = c2; }
            }
        }
        __syncthreads();
        // ---- 10. the composite, one lane per ray      :109-114
        if (tid < rpt) {
            const int64_t ray = ray0 + tid;
            float T = 1.f, m0 = 0.f, m1 = 0.f, m2 = 0.f;
            for (int q = 0; q < S; ++q) {
                float* sp = lds + L::SMP + (tid * S + q) * 16;
                const float e = expf(-sp[SMP_SIGMA]);
                const float alpha = 1.f - e;
                const float w = alpha * T;
                sp[SMP_E] = e; sp[SMP_T] = T; sp[SMP_W] = w;
                m0 += w * sp[SMP_RGB + 0]; m1 += w * sp[SMP_RGB + 1]; m2 += w * sp[SMP_RGB + 2];
                T = T * ((1.f - alpha) + 1e-10f);
            }
            if (!BWD && ray < n_rays) { rgb_map[ray * 3 + 0] = m0; rgb_map[ray * 3 + 1] = m1; rgb_map[ray * 3 + 2] = m2; }
            if (BWD) {
                // g_c,i = w_i g_C;  g_w,i = g_C . c_i;  g_sigma,i = e^-sigma_i T_i (g_w,i - Q_i),  Q_i = sum_{k>i} g_w,k alpha_k prod_{i<j<k} a_j
                // = g_w,i+1 alpha_i+1 + a_i+1 Q_i+1: no division by a_i = 1 - alpha_i + 1e-10.  alpha, T are the forward's fp32 values; the
                // sums run in double, as k_render_weights_bwd's do (g_w,i - Q_i cancels when a ray's samples look alike)
                float gc0 = 0.f, gc1 = 0.f, gc2 = 0.f;
                if (ray < n_rays) { gc0 = g_map[ray * 3 + 0]; gc1 = g_map[ray * 3 + 1]; gc2 = g_map[ray * 3 + 2]; }
                double Q = 0.0;
                for (int q = S - 1; q >= 0; --q) {
                    float* sp = lds + L::SMP + (tid * S + q) * 16;
                    const double gw = (double)gc0 * (double)sp[SMP_RGB + 0] + (double)gc1 * (double)sp[SMP_RGB + 1] + (double)gc2 * (double)sp[SMP_RGB + 2];
                    const float e = sp[SMP_E], alpha = 1.f - e;
                    const float gs = (float)((double)e * (double)sp[SMP_T] * (gw - Q));
                    Q = gw * (double)alpha + (double)((1.f - alpha) + 1e-10f) * Q;
                    const float w = sp[SMP_W], pre = sp[SMP_SPRE];
                    sp[SMP_GRGB + 0] = w * gc0; sp[SMP_GRGB + 1] = w * gc1; sp[SMP_GRGB + 2] = w * gc2;
                    lds[L::SG + tid * S + q] = gs * (pre > 20.f ? 1.f : 1.f / (1.f + expf(-pre)));
                }
            }
        }
        if constexpr (BWD) {
            // the samples of the tile past its rays carry no gradient
            SN_FOR(s, SN_SM) if (s >= TS) { lds[L::SG + s] = 0.f; lds[L::SMP + s * 16 + SMP_GRGB + 0] = 0.f; lds[L::SMP + s * 16 + SMP_GRGB + 1] = 0.f; lds[L::SMP + s * 16 + SMP_GRGB + 2] = 0.f; }
            __syncthreads();
            // ---- 11. d wv = g_c . colour_v, the softmax's backward and the ReLU of the score.  With every view's score positive the
            //          du_v of a sample sum to zero, and color.2's bias gradient is what the rounding leaves of that: the products and the
            //          weighted mean run in double, and the mean is taken over the fp32 weights as they are (sum_v w_v (d_v - mean) = 0
            //          whatever they sum to), as k_render_weights_bwd keeps its cancelling sums in double
            SN_FOR(s, TSP) {
                const float* gp = lds + L::SMP + s * 16 + SMP_GRGB;
                double num = 0.0, den = 0.0;
                SN_VIEWS
                for (int v = 0; v < V; ++v) {
                    const int r = v * TSP + s;
                    const float* xr = lds + L::XT + r * (C + 5) + C - 3;
                    const double d = (double)gp[0] * (double)xr[0] + (double)gp[1] * (double)xr[1] + (double)gp[2] * (double)xr[2];
                    const double w = (double)lds[L::ROW + r * 8 + ROW_WV];
                    num += w * d; den += w;
                }
                const double mean = num / den;
                SN_VIEWS
                for (int v = 0; v < V; ++v) {
                    const int r = v * TSP + s;
                    const float* xr = lds + L::XT + r * (C + 5) + C - 3;
                    const double d = (double)gp[0] * (double)xr[0] + (double)gp[1] * (double)xr[1] + (double)gp[2] * (double)xr[2];
                    const float du = (float)((double)lds[L::ROW + r * 8 + ROW_WV] * (d - mean));
                    lds[L::ROW + r * 8 + ROW_DU] = lds[L::ROW + r * 8 + ROW_UPRE] > 0.f ? du : 0.f;
                }
            }
            __syncthreads();
            // ---- 12. d hidden of color.0, per view and summed over views
            SN_FOR(k, R16 * GDB_HID) {
                int r = k / GDB_HID, j = k % GDB_HID;
                lds[L::DHID + r * 64 + j] = (r < R && lds[L::HID + r * 65 + j] > 0.f) ? pw[W::C2_W + j] * lds[L::ROW + r * 8 + ROW_DU] : 0.f;
            }
            __syncthreads();
            SN_FOR(k, SN_SM * GDB_HID) {
                int s = k / GDB_HID, j = k % GDB_HID;
                float a = 0.f;
                if (s < TSP) {
                    SN_VIEWS
                    for (int v = 0; v < V; ++v) a += lds[L::DHID + (v * TSP + s) * 64 + j];
                }
                lds[L::SDH + s * 64 + j] = a;
            }
            __syncthreads();
            // ---- 13. color.0^T dY: d [x | vox | im] from the summed rows, d tail per view
            sn_gemm(lds, L::DX, SN_XW, L::SDH, 64, GDB_HID, SN_XW, 16, pw + W::C0_W, 1, W::W0IN, nullptr, -1, 0, 1, false, wave, lane);
            sn_gemm(lds, L::DT, P, L::DHID, 64, GDB_HID, P, R16, pw + W::C0_W + SN_XW, 1, W::W0IN, nullptr, -1, 0, 1, false, wave, lane);
            __syncthreads();
            // ---- 14. d x += sigma.0^T d sigma-pre; through lr0's ReLU: dY of lr0
            SN_FOR(k, SN_SM * GDB_HID) {
                int s = k / GDB_HID, c = k % GDB_HID;
                float a = lds[L::DX + s * SN_XW + c] + pw[W::SIG_W + c] * lds[L::SG + s];
                lds[L::DX + s * SN_XW + c] = lds[L::XH + s * 89 + c] > 0.f ? a : 0.f;
            }
            __syncthreads();
            // ---- 15. d [vox | im] += lr0^T dY; g_vox; through fc's ReLU: dY of fc
            sn_gemm(lds, L::DX + GDB_HID, SN_XW, L::DX, SN_XW, GDB_HID, GDB_HD, 16, pw + W::LR0_W, 1, GDB_HD, nullptr, L::DX + GDB_HID, SN_XW, 16, false, wave, lane);
            __syncthreads();
            SN_FOR(k, SN_SM * GDB_HD) {
                int s = k / GDB_HD, c = k % GDB_HD; int64_t i = base + s;
                float a = lds[L::DX + s * SN_XW + GDB_HID + c];
                if (c < GDB_CV) {
                    if (g_vox && s < TS && i < n) g_vox[i * GDB_CV + c] = a;
                } else {
                    lds[L::DFC + s * 16 + c - GDB_CV] = lds[L::XH + s * 89 + GDB_HID + c] > 0.f ? a : 0.f;
                }
            }
            __syncthreads();
            // ---- 16. d agg = fc^T dY
            sn_gemm(lds, L::DAGG, 32, L::DFC, 16, GDB_IM, GDB_GF, 16, pw + W::FC_W, 1, GDB_GF, nullptr, -1, 0, 1, false, wave, lane);
            __syncthreads();
            // ---- 17. d a_v = d agg . G_v, the softmax's backward and the ReLU of the score (in double as step 11, where k_mlp_bwd's
            //          is fp32: not shared, either change moves bits)
            SN_FOR(r, R) {
                int s = r % TSP;
                float a = 0.f;
                SN_DOT
                for (int j = 0; j < GDB_GF; ++j) a = fmaf(lds[L::DAGG + s * 32 + j], lds[L::G + r * 33 + j], a);
                lds[L::ROW + r * 8 + ROW_TMP] = a;
            }
            __syncthreads();
            SN_FOR(s, TSP) {
                double num = 0.0, den = 0.0;   // (as step 11)
                SN_VIEWS
                for (int v = 0; v < V; ++v) {
                    const double w = (double)lds[L::ROW + (v * TSP + s) * 8 + ROW_A];
                    num += w * (double)lds[L::ROW + (v * TSP + s) * 8 + ROW_TMP]; den += w;
                }
                const double mean = num / den;
                SN_VIEWS
                for (int v = 0; v < V; ++v) {
                    int r = v * TSP + s;
                    float ds = (float)((double)lds[L::ROW + r * 8 + ROW_A] * ((double)lds[L::ROW + r * 8 + ROW_TMP] - mean));
                    lds[L::ROW + r * 8 + ROW_DS] = lds[L::ROW + r * 8 + ROW_SPRE] > 0.f ? ds : 0.f;
                }
            }
            __syncthreads();
            // ---- 18. dY of global_fc, per view and summed over views
            SN_FOR(k, R16 * GDB_GF) {
                int r = k / GDB_GF, j = k % GDB_GF, s = r % TSP;
                float dG = 0.f;
                if (r < R && lds[L::G + r * 33 + j] > 0.f)
                    dG = lds[L::DAGG + s * 32 + j] * lds[L::ROW + r * 8 + ROW_A] + pw[W::AGG_W + j] * lds[L::ROW + r * 8 + ROW_DS];
                lds[L::DA + r * 32 + j] = dG;
            }
            __syncthreads();
            SN_FOR(k, SN_SM * GDB_GF) {
                int s = k / GDB_GF, j = k % GDB_GF;
                float a = 0.f;
                if (s < TSP) {
                    SN_VIEWS
                    for (int v = 0; v < V; ++v) a += lds[L::DA + (v * TSP + s) * 32 + j];
                }
                lds[L::SDA + s * 32 + j] = a;
            }
            __syncthreads();
            // ---- 19. global_fc^T dY: d [var | mean] from the sum over views (they feed every view's row), d g_v per view
            sn_gemm(lds, L::DVM, 2 * C, L::SDA, 32, GDB_GF, 2 * C, 16, pw + W::GLOB_W + C, 1, 3 * C, nullptr, -1, 0, 1, false, wave, lane);
            sn_gemm(lds, L::TG, C, L::DA, 32, GDB_GF, C, R16, pw + W::GLOB_W, 1, 3 * C, nullptr, -1, 0, 1, false, wave, lane);
            __syncthreads();
            // ---- 20. d g_v += mean (1 / V) and var (2 (g_v - mean) / (V - 1)); d feat joins the tail's gradient; dY of view_fc
            SN_FOR(k, R * C) {
                int r = k / C, c = k % C, s = r % TSP;
                float a = lds[L::TG + r * C + c];
                float dev = lds[L::GV + r * (C + 1) + c] - lds[L::VM + s * 2 * C + C + c];
                a += lds[L::DVM + s * 2 * C + C + c] / Vf;
                a += lds[L::DVM + s * 2 * C + c] * (2.f * dev / (Vf - 1.f));
                lds[L::DT + r * P + c] += a;
                lds[L::VP + r * C + c] = (viewdir && lds[L::VP + r * C + c] > 0.f) ? a : 0.f;
            }
            __syncthreads();
            // ---- 21. d dir from view_fc
            if (viewdir) SN_FOR(k, R * 4) {
                int r = k / 4, d = k % 4;
                float a = 0.f;
                SN_DOT
                for (int c = 0; c < C; ++c) a = fmaf(pw[W::VIEW_W + 4 * c + d], lds[L::VP + r * C + c], a);
                lds[L::DT + r * P + C + d] += a;
            }
            __syncthreads();
            // ---- 22. g_img_feat_rgb_dir: the colour channels C-3 .. C-1 are blended AND fed to the layers: the sum of both paths
            if (g_xin) SN_FOR(k, R * P) {
                int r = k / P, c = k % P, v = r / TSP, s = r % TSP; int64_t i = base + s;
                if (s < TS && i < n) {
                    float a = lds[L::DT + r * P + c];
                    if (c >= C - 3 && c < C) a += lds[L::SMP + s * 16 + SMP_GRGB + c - (C - 3)] * lds[L::ROW + r * 8 + ROW_WV];
                    g_xin[((size_t)i * V + v) * P + c] = a;
                }
            }
            // ---- 23. dW += dY^T [X | 1] on the matrix cores
            dw_accumulate<PER_WAVE>(c_sn_table<C>, lds, R, TSP, acc, wave, lane);
        }
        __syncthreads();   // the next tile overwrites the LDS image
    }

    if constexpr (BWD) {
        // ---- this workgroup's ONE partial: zeros (pad slots, view_fc without viewdir_agg), then every wave's tiles
        float* part = partials + (size_t)blockIdx.x * W::FLOATS;
        SN_FOR(k, W::FLOATS) part[k] = 0.f;
        __syncthreads();
        dw_store_partial<PER_WAVE>(c_sn_table<C>, part, acc, wave, lane);
    }
}

__global__ void k_stage_reduce(const float* __restrict__ partials, int nparts, int floats, float* __restrict__ out) {
    dw_reduce(partials, nparts, floats, out);
}

// ---- host ----
// f(std::integral_constant<int, C>) for the C = feat_dim + 3 of the three networks sn_check_net lets through
template <class F> static auto sn_dispatch(int C, F&& f) {
    if (C == 11) return f(std::integral_constant<int, 11>{});
    if (C == 19) return f(std::integral_constant<int, 19>{});
    return f(std::integral_constant<int, 35>{});
}
static int sn_floats(int C) { return sn_dispatch(C, [](auto c) { return SnW<decltype(c)::value>::FLOATS; }); }

static int sn_check_net(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg) {
    if (feat_dim != 8 && feat_dim != 16 && feat_dim != 32) return gdb_fail(GDB_E_BADARG, "stage NeRF: feat_dim %d is not 8, 16 or 32", feat_dim);
    if (voxel_dim != GDB_CV || hid_dim != GDB_HID) return gdb_fail(GDB_E_BADARG, "stage NeRF: built for voxel_dim %d, hid_dim %d (got %d, %d)", GDB_CV, GDB_HID, voxel_dim, hid_dim);
    if (viewdir_agg != 0 && viewdir_agg != 1) return gdb_fail(GDB_E_BADARG, "stage NeRF: viewdir_agg must be 0 or 1");
    return GDB_OK;
}

// rays per tile: whole rays, at most 16 samples, at most 64 (view, sample) rows with a view's block padded to a multiple of 4 samples
static int sn_rays_per_tile(int V, int S) {
    int rpt = SN_SM / S;
    while (rpt > 1 && V * ((rpt * S + 3) & ~3) > SN_RM) --rpt;
    return rpt < 1 ? 1 : rpt;
}

static int sn_check_shape(int32_t V, int32_t S, int64_t n_rays) {
    if (V < 2 || V > GDB_MAX_VIEWS) return gdb_fail(GDB_E_SHAPE, "stage NeRF: V=%d outside 2..%d (the unbiased variance has no derivative at V = 1)", V, GDB_MAX_VIEWS);
    if (S < 1 || S > GDB_MAX_SAMPLES) return gdb_fail(GDB_E_SHAPE, "stage NeRF: S=%d outside 1..%d", S, GDB_MAX_SAMPLES);
    if (V * ((S + 3) & ~3) > SN_RM) return gdb_fail(GDB_E_SHAPE, "stage NeRF: one ray of V=%d views x S=%d samples exceeds the tile's %d (view, sample) rows", V, S, SN_RM);
    if (n_rays < 1 || n_rays >= ((int64_t)1 << 31) / S) return gdb_fail(GDB_E_SHAPE, "stage NeRF: n_rays=%lld outside the supported range", (long long)n_rays);
    return GDB_OK;
}

static int sn_grid(int V, int S, int64_t n_rays) {
    int rpt = sn_rays_per_tile(V, S);
    int64_t tiles = (n_rays + rpt - 1) / rpt;
    return (int)(tiles < SN_MAX_WG ? tiles : SN_MAX_WG);
}

extern "C" int gdb_stage_nerf_packed_floats(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg, size_t* out_floats) {
    int rc = sn_check_net(feat_dim, voxel_dim, hid_dim, viewdir_agg); if (rc) return rc;
    if (!out_floats) return gdb_fail(GDB_E_BADARG, "out_floats is NULL");
    *out_floats = (size_t)sn_floats(feat_dim + 3);
    return GDB_OK;
}

static void sn_offsets_of(int C_, int offs[16], int sizes[16]) {
    sn_dispatch(C_, [&](auto c) {
        constexpr int C = decltype(c)::value;
        using W = SnW<C>;
        const int o[16] = {W::VIEW_W, W::VIEW_B, W::GLOB_W, W::GLOB_B, W::AGG_W, W::AGG_B, W::FC_W, W::FC_B, W::LR0_W, W::LR0_B, W::SIG_W, W::SIG_B,
                           W::C0_W, W::C0_B, W::C2_W, W::C2_B};
        const int s[16] = {C * 4, C, GDB_GF * 3 * C, GDB_GF, GDB_GF, 1, GDB_IM * GDB_GF, GDB_IM, GDB_HID * GDB_HD, GDB_HID, GDB_HID, 1,
                           GDB_HID * W::W0IN, GDB_HID, GDB_HID, 1};
        for (int i = 0; i < 16; ++i) { offs[i] = o[i]; sizes[i] = s[i]; }
    });
}

extern "C" int gdb_pack_stage_nerf_weights(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg,
                                           const float* const h_tensors[16], float* h_out) {
    int rc = sn_check_net(feat_dim, voxel_dim, hid_dim, viewdir_agg); if (rc) return rc;
    if (!h_tensors || !h_out) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    int offs[16], sizes[16];
    sn_offsets_of(feat_dim + 3, offs, sizes);
    memset(h_out, 0, sizeof(float) * (size_t)sn_floats(feat_dim + 3));
    for (int i = 0; i < 16; ++i) {
        if (i < 2 && !viewdir_agg) continue;   // view_fc does not exist without viewdir_agg: its slots stay zero
        if (!h_tensors[i]) return gdb_fail(GDB_E_BADARG, "tensor %d is NULL", i);
        memcpy(h_out + offs[i], h_tensors[i], sizeof(float) * sizes[i]);
    }
    return GDB_OK;
}

extern "C" int gdb_unpack_stage_nerf_grads(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg,
                                           const float* h_packed, float* const h_tensors[16]) {
    int rc = sn_check_net(feat_dim, voxel_dim, hid_dim, viewdir_agg); if (rc) return rc;
    if (!h_packed || !h_tensors) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    int offs[16], sizes[16];
    sn_offsets_of(feat_dim + 3, offs, sizes);
    for (int i = 0; i < 16; ++i) {
        if (i < 2 && !viewdir_agg) continue;
        if (!h_tensors[i]) return gdb_fail(GDB_E_BADARG, "gradient tensor %d is NULL", i);
        memcpy(h_tensors[i], h_packed + offs[i], sizeof(float) * sizes[i]);
    }
    return GDB_OK;
}

extern "C" int gdb_stage_nerf_layout(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg, int32_t V, int32_t S,
                                     int64_t n_rays, size_t out[3]) {
    int rc = sn_check_net(feat_dim, voxel_dim, hid_dim, viewdir_agg); if (rc) return rc;
    if (!out) return gdb_fail(GDB_E_BADARG, "out is NULL");
    rc = sn_check_shape(V, S, n_rays); if (rc) return rc;
    int g = sn_grid(V, S, n_rays);
    out[0] = sizeof(float) * (size_t)g * sn_floats(feat_dim + 3); out[1] = (size_t)g; out[2] = (size_t)sn_rays_per_tile(V, S);
    return GDB_OK;
}

extern "C" int gdb_stage_nerf(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg, const float* d_packed, int32_t V, int32_t S,
                              const float* d_vox, const float* d_img, int64_t n_rays, float* d_rgb_map, float* d_sigma, float* d_rgb, void* stream_) {
    size_t lay[3];
    int rc = gdb_stage_nerf_layout(feat_dim, voxel_dim, hid_dim, viewdir_agg, V, S, n_rays, lay); if (rc) return rc;
    if (!d_packed || !d_vox || !d_img || !d_rgb_map) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    hipStream_t st = (hipStream_t)stream_;
    const int g = (int)lay[1], rpt = (int)lay[2], C = feat_dim + 3;
    sn_dispatch(C, [&](auto c) {
        hipLaunchKernelGGL((k_stage_nerf<decltype(c)::value, false>), dim3((unsigned)g), dim3(SN_THREADS), 0, st, d_packed, V, S, viewdir_agg, rpt, d_vox, d_img,
                           n_rays, d_rgb_map, d_sigma, d_rgb, (const float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
    });
    LAUNCH_CHECK("k_stage_nerf");
    return GDB_OK;
}

extern "C" int gdb_stage_nerf_backward(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg, const float* d_packed, int32_t V,
                                       int32_t S, const float* d_vox, const float* d_img, int64_t n_rays, const float* d_g_rgb_map, float* d_g_packed,
                                       float* d_g_vox, float* d_g_img, void* d_workspace, size_t workspace_bytes, void* stream_) {
    size_t lay[3];
    int rc = gdb_stage_nerf_layout(feat_dim, voxel_dim, hid_dim, viewdir_agg, V, S, n_rays, lay); if (rc) return rc;
    if (!d_packed || !d_vox || !d_img || !d_g_rgb_map || !d_g_packed || !d_workspace) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (workspace_bytes < lay[0]) return gdb_fail(GDB_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, lay[0]);
    hipStream_t st = (hipStream_t)stream_;
    const int g = (int)lay[1], rpt = (int)lay[2], C = feat_dim + 3;
    float* parts = (float*)d_workspace;
    sn_dispatch(C, [&](auto c) {
        hipLaunchKernelGGL((k_stage_nerf<decltype(c)::value, true>), dim3((unsigned)g), dim3(SN_THREADS), 0, st, d_packed, V, S, viewdir_agg, rpt, d_vox, d_img,
                           n_rays, (float*)nullptr, (float*)nullptr, (float*)nullptr, d_g_rgb_map, d_g_vox, d_g_img, parts);
    });
    LAUNCH_CHECK("k_stage_nerf (backward)");
    const int floats = sn_floats(C);
    hipLaunchKernelGGL(k_stage_reduce, dim3((floats + 255) / 256), dim3(256), 0, st, (const float*)parts, g, floats, d_g_packed);
    LAUNCH_CHECK("k_stage_reduce");
    return GDB_OK;
}
