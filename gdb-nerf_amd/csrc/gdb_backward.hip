// Backward of NeRF.forward (networks/gdb_nerf/nerf.py:58-115) and of the normalised alpha composite
// (networks/gdb_nerf/utils.py:19-43,88-121), fp32 throughout.  The operator mirrors of gdb_mlp.hip are the forward;
// nothing is saved between forward and backward: every kernel here recomputes what it needs from the inputs.
//
// Derivative conventions: ReLU'(0) = 0 as torch; softplus with threshold 20 has derivative 1 above it;
// var / mean are torch.var_mean with the unbiased divisor V - 1; both view softmaxes are over relu(score);
// clamp_min(1e-6) on the weight sum has derivative 0 below 1e-6.
#include "gdb_dw_tiles.h"
#include <cstring>

// ============================================================================================
// MLP backward
// ============================================================================================
// One workgroup of 4 waves walks tiles of BWD_TS samples (persistent grid: tile t belongs to workgroup t mod grid).  Per tile:
//   1. the vector ALUs recompute the forward activations of the tile into LDS and run the per-sample chain of activation
//      gradients, leaving for every linear layer its input X (rows = samples, or (view, sample) pairs) and the gradient dY of
//      its pre-activation in LDS;
//   2. the matrix cores add dW += dY^T [X | 1] into accumulator registers that live across all tiles of the workgroup, which writes
//      ONE partial (the packed fp32 section's layout) to the workspace after its last tile; k_mlp_bwd_reduce adds the partials in
//      workgroup order (gdb_dw_tiles.h).
// The depth net's stage render (k_stage_nerf) walks the same chain with its linear layers on the matrix cores and its softmax backwards
// in double; here both are fp32 on the vector ALUs - DESIGN.md 4.14 names the step not taken, and taking it changes this kernel's bits.
#define BWD_TS 8
#define BWD_THREADS 256
#define BWD_MAX_WG 256
#define BWD_R (GDB_MAX_VIEWS * BWD_TS)   // (view, sample) rows of a tile at most

// ---- LDS image of a tile (float offsets).  Row r of a per-view array = view r / BWD_TS, sample r % BWD_TS. ----
constexpr int L_FV = 0;                          // [R][24]  [feat19 | dir4 | 1]: X of weight.0's per-view columns; dir4 | 1 = X of view_fc
constexpr int L_GV = L_FV + BWD_R * 24;          // [R][20]  [g_v | 1]: X of global_fc's per-view columns
constexpr int L_VP = L_GV + BWD_R * 20;          // [R][20]  view_fc pre-activation, then its gradient (dY of view_fc)
constexpr int L_G = L_VP + BWD_R * 20;           // [R][33]  [relu(global_fc) | 1]: X of agg_w_fc
constexpr int L_DA = L_G + BWD_R * 33;           // [R][32]  dY of global_fc
constexpr int L_HID = L_DA + BWD_R * 32;         // [R][65]  [relu(weight.0) | 1]: X of weight.2
constexpr int L_DHID = L_HID + BWD_R * 65;       // [R][64]  dY of weight.0
constexpr int L_ROW = L_DHID + BWD_R * 64;       // [R][8]   per (view, sample) scalars, ROW_* below
constexpr int L_DT = L_ROW + BWD_R * 8;          // [R][24]  gradient of the view's tail [feat19 | dir4]
constexpr int L_VM = L_DT + BWD_R * 24;          // [TS][38] [var | mean]: X of global_fc's shared columns
constexpr int L_DVM = L_VM + BWD_TS * 38;        // [TS][38] gradient of [var | mean]
constexpr int L_SDA = L_DVM + BWD_TS * 38;       // [TS][32] sum over views of dY(global_fc): dY of the shared columns
constexpr int L_AGG = L_SDA + BWD_TS * 32;       // [TS][33] [agg | 1]: X of fc
constexpr int L_DAGG = L_AGG + BWD_TS * 33;      // [TS][32]
constexpr int L_DFC = L_DAGG + BWD_TS * 32;      // [TS][16] dY of fc
constexpr int L_XH = L_DFC + BWD_TS * 16;        // [TS][89] [x64 | vox8 | im16 | 1]: X of sigma, feat_head, weight.0 (shared columns), lr0
constexpr int L_DL = L_XH + BWD_TS * 89;         // [TS][64] dY of lr0
constexpr int L_DH = L_DL + BWD_TS * 64;         // [TS][24]
constexpr int L_SG = L_DH + BWD_TS * 24;         // [TS]     dY of sigma
constexpr int L_FH = L_SG + BWD_TS;              // [TS][8]  dY of feat_head
constexpr int L_SDH = L_FH + BWD_TS * 8;         // [TS][64] sum over views of dY(weight.0): dY of the shared columns
constexpr int L_END = L_SDH + BWD_TS * 64;
static_assert(L_END * sizeof(float) <= 160 * 1024, "the tile does not fit the LDS of a CU");
enum { ROW_SPRE = 0, ROW_A = 1, ROW_DS = 2, ROW_UPRE = 3, ROW_WV = 4, ROW_DU = 5, ROW_TMP = 6 };

// ---- the products dW = dY^T [X | 1] ----
#define BWD_TILES_PER_WAVE 19
typedef DwTable<4 * BWD_TILES_PER_WAVE> BwdTable;

constexpr BwdTable bwd_make_table() {
    const DwProduct prods[11] = {
        // dy      ldy M   x            ldx Nw  xone         pv w                    ldw       b
        {L_VP,   20, GDB_CFR, L_FV + GDB_CFR, 24, 4,  L_FV + 23, 1, PW_VIEW_W,           4,        PW_VIEW_B},   // view_fc
        {L_DA,   32, GDB_GF,  L_GV,     20, GDB_CFR,  L_GV + 19, 1, PW_GLOB_W,           3 * GDB_CFR, PW_GLOB_B},   // global_fc, per-view columns
        {L_SDA,  32, GDB_GF,  L_VM,     38, 2 * GDB_CFR, -1,     0, PW_GLOB_W + GDB_CFR, 3 * GDB_CFR, -1},          // global_fc, [var | mean]
        {L_ROW + ROW_DS, 8, 1, L_G,     33, GDB_GF,   L_G + 32,  1, PW_AGG_W,            GDB_GF,   PW_AGG_B},    // agg_w_fc
        {L_DFC,  16, GDB_IM,  L_AGG,    33, GDB_GF,   L_AGG + 32, 0, PW_FC_W,            GDB_GF,   PW_FC_B},     // fc
        {L_DL,   64, GDB_HID, L_XH + 64, 89, GDB_HD,  L_XH + 88, 0, PW_LR0_W,            GDB_HD,   PW_LR0_B},    // lr0
        {L_SG,   1,  1,       L_XH,     89, GDB_HID,  L_XH + 88, 0, PW_SIG_W,            GDB_HID,  PW_SIG_B},    // sigma
        {L_SDH,  64, GDB_HID, L_XH,     89, GDB_HID + GDB_HD, -1, 0, PW_W0_W,            GDB_W0IN, -1},          // weight.0, [x | h]
        {L_DHID, 64, GDB_HID, L_FV,     24, GDB_FV,   L_FV + 23, 1, PW_W0_W + GDB_HID + GDB_HD, GDB_W0IN, PW_W0_B},   // weight.0, per-view tail
        {L_ROW + ROW_DU, 8, 1, L_HID,   65, GDB_HID,  L_HID + 64, 1, PW_W2_W,            GDB_HID,  PW_W2_B},     // weight.2
        {L_FH,   8,  GDB_CV,  L_XH,     89, GDB_HID,  L_XH + 88, 0, PW_FH_W,             GDB_HID,  PW_FH_B},     // feat_head
    };
    return dw_make_table<4 * BWD_TILES_PER_WAVE>(prods);
}
constexpr BwdTable k_bwd_table = bwd_make_table();
static_assert(k_bwd_table.n <= 4 * BWD_TILES_PER_WAVE, "more output tiles than accumulators");
__constant__ BwdTable c_bwd_table = k_bwd_table;

// inner loops stay rolled: unrolled, their weight loads pile up in registers until the accumulators spill
#define BWD_DOT _Pragma("unroll 4")
#define BWD_VIEWS _Pragma("nounroll")
#define BWD_FOR(i, count) for (int i = tid; i < (count); i += BWD_THREADS)

__global__ void __launch_bounds__(BWD_THREADS)
k_mlp_bwd(const float* __restrict__ pw, int V, int viewdir, int P, const float* __restrict__ vox, const float* __restrict__ xin,
          const int64_t* __restrict__ total, int64_t n_alloc, const float* __restrict__ g_sigma, const float* __restrict__ g_feat,
          float* __restrict__ g_vox, float* __restrict__ g_xin, float* __restrict__ partials) {
    __shared__ float lds[L_END];
    constexpr int TS = BWD_TS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t n = total ? *total : n_alloc;
    n = n < 0 ? 0 : (n > n_alloc ? n_alloc : n);
    const int T = P - GDB_FV;        // first channel of [feat | rgb | dir]
    const int Q = P - 4;             // blended channels
    const int F = Q + GDB_CV;        // columns of g_feat
    const int R = V * TS;
    const float Vf = (float)V;
    const int64_t ntiles = (n_alloc + TS - 1) / TS;

    f32x4 acc[BWD_TILES_PER_WAVE];
#pragma unroll
    for (int i = 0; i < BWD_TILES_PER_WAVE; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t base = t * TS;
        if (base >= n) {
            // rows [*d_total, n_alloc): nothing for dW, zero rows of g_vox / g_rgbs_feat_dir
            if (g_vox) BWD_FOR(k, TS * GDB_CV) { int64_t i = base + k / GDB_CV; if (i < n_alloc) g_vox[i * GDB_CV + k % GDB_CV] = 0.f; }
            if (g_xin) BWD_FOR(k, R * P) {
                int r = k / P, c = k % P; int64_t i = base + r % TS;
                if (i < n_alloc) g_xin[((size_t)(r / TS) * n_alloc + i) * P + c] = 0.f;
            }
            continue;
        }
        // ---- 0. inputs: the views' tails, vox; rows past *d_total read as zeros (finite activations, zero gradients)
        BWD_FOR(k, R * 24) {
            int r = k / 24, c = k % 24; int64_t i = base + r % TS;
            float val = 1.f;
            if (c < GDB_FV) val = i < n ? xin[((size_t)(r / TS) * n_alloc + i) * P + T + c] : 0.f;
            lds[L_FV + r * 24 + c] = val;
            lds[L_DT + r * 24 + c] = 0.f;
        }
        BWD_FOR(k, TS * 9) {
            int s = k / 9, c = k % 9; int64_t i = base + s;
            lds[L_XH + s * 89 + (c < 8 ? GDB_HID + c : 88)] = c < 8 ? (i < n ? vox[i * GDB_CV + c] : 0.f) : 1.f;
        }
        __syncthreads();
        // ---- 1. g_v = feat19 + relu(W_view dir + b)      nerf.py:69-71
        BWD_FOR(k, R * 20) {
            int r = k / 20, c = k % 20;
            float a = 0.f, g = 1.f;
            if (c < GDB_CFR) {
                const float* tl = lds + L_FV + r * 24;
                if (viewdir) {
                    a = pw[PW_VIEW_B + c];
                    a = fmaf(pw[PW_VIEW_W + 4 * c + 0], tl[GDB_CFR + 0], a);
                    a = fmaf(pw[PW_VIEW_W + 4 * c + 1], tl[GDB_CFR + 1], a);
                    a = fmaf(pw[PW_VIEW_W + 4 * c + 2], tl[GDB_CFR + 2], a);
                    a = fmaf(pw[PW_VIEW_W + 4 * c + 3], tl[GDB_CFR + 3], a);
                }
                g = tl[c] + relu_f(a);
            }
            lds[L_VP + r * 20 + c] = a;
            lds[L_GV + r * 20 + c] = g;
        }
        __syncthreads();
        // ---- 2. mean / unbiased variance over views      :73
        BWD_FOR(k, TS * GDB_CFR) {
            int s = k / GDB_CFR, c = k % GDB_CFR;
            float m = 0.f, vr = 0.f;
            BWD_VIEWS
            for (int v = 0; v < V; ++v) m += lds[L_GV + (v * TS + s) * 20 + c];
            m = m / Vf;
            BWD_VIEWS
            for (int v = 0; v < V; ++v) { float d = lds[L_GV + (v * TS + s) * 20 + c] - m; vr += d * d; }
            lds[L_VM + s * 38 + c] = vr / (Vf - 1.f);
            lds[L_VM + s * 38 + GDB_CFR + c] = m;
        }
        __syncthreads();
        // ---- 3. G_v = relu(global_fc [g_v | var | mean])      :77-78
        BWD_FOR(k, R * 33) {
            int r = k / 33, j = k % 33, s = r % TS;
            float val = 1.f;
            if (j < GDB_GF) {
                const float* wr = pw + PW_GLOB_W + j * 3 * GDB_CFR;
                float a = pw[PW_GLOB_B + j];
                BWD_DOT
                for (int c = 0; c < 2 * GDB_CFR; ++c) a = fmaf(wr[GDB_CFR + c], lds[L_VM + s * 38 + c], a);
                BWD_DOT
                for (int c = 0; c < GDB_CFR; ++c) a = fmaf(wr[c], lds[L_GV + r * 20 + c], a);
                val = relu_f(a);
            }
            lds[L_G + r * 33 + j] = val;
        }
        __syncthreads();
        // ---- 4. view scores      :79
        BWD_FOR(r, R) {
            float sv = pw[PW_AGG_B];
            BWD_DOT
            for (int j = 0; j < GDB_GF; ++j) sv = fmaf(pw[PW_AGG_W + j], lds[L_G + r * 33 + j], sv);
            lds[L_ROW + r * 8 + ROW_SPRE] = sv;
        }
        __syncthreads();
        BWD_FOR(s, TS) {
            float m = relu_f(lds[L_ROW + s * 8 + ROW_SPRE]);
            BWD_VIEWS
            for (int v = 1; v < V; ++v) m = fmaxf(m, relu_f(lds[L_ROW + (v * TS + s) * 8 + ROW_SPRE]));
            float sum = 0.f;
            BWD_VIEWS
            for (int v = 0; v < V; ++v) { float e = expf(relu_f(lds[L_ROW + (v * TS + s) * 8 + ROW_SPRE]) - m); lds[L_ROW + (v * TS + s) * 8 + ROW_A] = e; sum += e; }
            BWD_VIEWS
            for (int v = 0; v < V; ++v) lds[L_ROW + (v * TS + s) * 8 + ROW_A] /= sum;
        }
        __syncthreads();
        // ---- 5. agg = sum_v G_v a_v      :80
        BWD_FOR(k, TS * 33) {
            int s = k / 33, j = k % 33;
            float a = 1.f;
            if (j < GDB_GF) {
                a = 0.f;
                BWD_VIEWS
                for (int v = 0; v < V; ++v) a += lds[L_G + (v * TS + s) * 33 + j] * lds[L_ROW + (v * TS + s) * 8 + ROW_A];
            }
            lds[L_AGG + s * 33 + j] = a;
        }
        __syncthreads();
        // ---- 6. im = relu(fc agg); h = [vox | im]      :82
        BWD_FOR(k, TS * GDB_IM) {
            int s = k / GDB_IM, j = k % GDB_IM;
            float a = pw[PW_FC_B + j];
            BWD_DOT
            for (int c = 0; c < GDB_GF; ++c) a = fmaf(pw[PW_FC_W + j * GDB_GF + c], lds[L_AGG + s * 33 + c], a);
            lds[L_XH + s * 89 + GDB_HID + GDB_CV + j] = relu_f(a);
        }
        __syncthreads();
        // ---- 7. x = relu(lr0 h)      :100-101
        BWD_FOR(k, TS * GDB_HID) {
            int s = k / GDB_HID, j = k % GDB_HID;
            float a = pw[PW_LR0_B + j];
            BWD_DOT
            for (int c = 0; c < GDB_HD; ++c) a = fmaf(pw[PW_LR0_W + j * GDB_HD + c], lds[L_XH + s * 89 + GDB_HID + c], a);
            lds[L_XH + s * 89 + j] = relu_f(a);
        }
        __syncthreads();
        // ---- 8. heads on x: d sigma-pre (softplus, threshold 20), d feat_head-pre; the views' hidden rows of `weight`
        BWD_FOR(s, TS) {
            int64_t i = base + s;
            float sg = pw[PW_SIG_B];
            BWD_DOT
            for (int j = 0; j < GDB_HID; ++j) sg = fmaf(pw[PW_SIG_W + j], lds[L_XH + s * 89 + j], sg);
            float d = sg > 20.f ? 1.f : 1.f / (1.f + expf(-sg));
            lds[L_SG + s] = i < n ? g_sigma[i] * d : 0.f;
        }
        BWD_FOR(k, TS * GDB_CV) {
            int s = k / GDB_CV, j = k % GDB_CV; int64_t i = base + s;
            float a = pw[PW_FH_B + j];
            BWD_DOT
            for (int c = 0; c < GDB_HID; ++c) a = fmaf(pw[PW_FH_W + j * GDB_HID + c], lds[L_XH + s * 89 + c], a);
            lds[L_FH + s * 8 + j] = (i < n && a > 0.f) ? g_feat[i * F + Q + j] : 0.f;
        }
        BWD_FOR(k, R * 65) {
            int r = k / 65, j = k % 65, s = r % TS;
            float val = 1.f;
            if (j < GDB_HID) {
                const float* wr = pw + PW_W0_W + j * GDB_W0IN;
                float a = pw[PW_W0_B + j];
                BWD_DOT
                for (int c = 0; c < GDB_HID + GDB_HD; ++c) a = fmaf(wr[c], lds[L_XH + s * 89 + c], a);
                BWD_DOT
                for (int c = 0; c < GDB_FV; ++c) a = fmaf(wr[GDB_HID + GDB_HD + c], lds[L_FV + r * 24 + c], a);
                val = relu_f(a);
            }
            lds[L_HID + r * 65 + j] = val;
        }
        __syncthreads();
        // ---- 9. blend scores, and d wv = g_feat[:Q] . x_v[:Q]      :106-110
        BWD_FOR(r, R) {
            int64_t i = base + r % TS;
            float u = pw[PW_W2_B];
            BWD_DOT
            for (int j = 0; j < GDB_HID; ++j) u = fmaf(pw[PW_W2_W + j], lds[L_HID + r * 65 + j], u);
            lds[L_ROW + r * 8 + ROW_UPRE] = u;
            float d = 0.f;
            if (i < n) {
                const float* xr = xin + ((size_t)(r / TS) * n_alloc + i) * P;
                const float* gr = g_feat + (size_t)i * F;
                BWD_DOT
                for (int c = 0; c < Q; ++c) d = fmaf(gr[c], xr[c], d);
            }
            lds[L_ROW + r * 8 + ROW_TMP] = d;
        }
        __syncthreads();
        BWD_FOR(s, TS) {   // softmax over relu(u), its backward, and the ReLU of the score
            float m = relu_f(lds[L_ROW + s * 8 + ROW_UPRE]);
            BWD_VIEWS
            for (int v = 1; v < V; ++v) m = fmaxf(m, relu_f(lds[L_ROW + (v * TS + s) * 8 + ROW_UPRE]));
            float sum = 0.f;
            BWD_VIEWS
            for (int v = 0; v < V; ++v) { float e = expf(relu_f(lds[L_ROW + (v * TS + s) * 8 + ROW_UPRE]) - m); lds[L_ROW + (v * TS + s) * 8 + ROW_WV] = e; sum += e; }
            float dot = 0.f;
            BWD_VIEWS
            for (int v = 0; v < V; ++v) {
                float w = lds[L_ROW + (v * TS + s) * 8 + ROW_WV] / sum;
                lds[L_ROW + (v * TS + s) * 8 + ROW_WV] = w;
                dot = fmaf(w, lds[L_ROW + (v * TS + s) * 8 + ROW_TMP], dot);
            }
            BWD_VIEWS
            for (int v = 0; v < V; ++v) {
                int r = v * TS + s;
                float du = lds[L_ROW + r * 8 + ROW_WV] * (lds[L_ROW + r * 8 + ROW_TMP] - dot);
                lds[L_ROW + r * 8 + ROW_DU] = lds[L_ROW + r * 8 + ROW_UPRE] > 0.f ? du : 0.f;
            }
        }
        __syncthreads();
        // ---- 10. d hidden of `weight`, per view and summed over views
        BWD_FOR(k, R * GDB_HID) {
            int r = k / GDB_HID, j = k % GDB_HID;
            lds[L_DHID + r * 64 + j] = lds[L_HID + r * 65 + j] > 0.f ? pw[PW_W2_W + j] * lds[L_ROW + r * 8 + ROW_DU] : 0.f;
        }
        __syncthreads();
        BWD_FOR(k, TS * GDB_HID) {
            int s = k / GDB_HID, j = k % GDB_HID;
            float a = 0.f;
            BWD_VIEWS
            for (int v = 0; v < V; ++v) a += lds[L_DHID + (v * TS + s) * 64 + j];
            lds[L_SDH + s * 64 + j] = a;
        }
        __syncthreads();
        // ---- 11. d x (from weight.0, sigma, feat_head) -> d lr0-pre; d h from weight.0; d tail from weight.0
        BWD_FOR(k, TS * GDB_HID) {
            int s = k / GDB_HID, c = k % GDB_HID;
            float a = pw[PW_SIG_W + c] * lds[L_SG + s];
            BWD_DOT
            for (int j = 0; j < GDB_CV; ++j) a = fmaf(pw[PW_FH_W + j * GDB_HID + c], lds[L_FH + s * 8 + j], a);
            BWD_DOT
            for (int j = 0; j < GDB_HID; ++j) a = fmaf(pw[PW_W0_W + j * GDB_W0IN + c], lds[L_SDH + s * 64 + j], a);
            lds[L_DL + s * 64 + c] = lds[L_XH + s * 89 + c] > 0.f ? a : 0.f;
        }
        BWD_FOR(k, TS * GDB_HD) {
            int s = k / GDB_HD, c = k % GDB_HD;
            float a = 0.f;
            BWD_DOT
            for (int j = 0; j < GDB_HID; ++j) a = fmaf(pw[PW_W0_W + j * GDB_W0IN + GDB_HID + c], lds[L_SDH + s * 64 + j], a);
            lds[L_DH + s * 24 + c] = a;
        }
        BWD_FOR(k, R * GDB_FV) {
            int r = k / GDB_FV, c = k % GDB_FV;
            float a = 0.f;
            BWD_DOT
            for (int j = 0; j < GDB_HID; ++j) a = fmaf(pw[PW_W0_W + j * GDB_W0IN + GDB_HID + GDB_HD + c], lds[L_DHID + r * 64 + j], a);
            lds[L_DT + r * 24 + c] = a;
        }
        __syncthreads();
        // ---- 12. d h += lr0^T d lr0-pre; g_vox; d fc-pre
        BWD_FOR(k, TS * GDB_HD) {
            int s = k / GDB_HD, c = k % GDB_HD; int64_t i = base + s;
            float a = lds[L_DH + s * 24 + c];
            BWD_DOT
            for (int j = 0; j < GDB_HID; ++j) a = fmaf(pw[PW_LR0_W + j * GDB_HD + c], lds[L_DL + s * 64 + j], a);
            if (c < GDB_CV) {
                if (g_vox && i < n_alloc) g_vox[i * GDB_CV + c] = i < n ? a : 0.f;
            } else {
                lds[L_DFC + s * 16 + c - GDB_CV] = lds[L_XH + s * 89 + GDB_HID + c] > 0.f ? a : 0.f;
            }
        }
        __syncthreads();
        // ---- 13. d agg
        BWD_FOR(k, TS * GDB_GF) {
            int s = k / GDB_GF, c = k % GDB_GF;
            float a = 0.f;
            BWD_DOT
            for (int j = 0; j < GDB_IM; ++j) a = fmaf(pw[PW_FC_W + j * GDB_GF + c], lds[L_DFC + s * 16 + j], a);
            lds[L_DAGG + s * 32 + c] = a;
        }
        __syncthreads();
        // ---- 14. d a_v = d agg . G_v, the softmax's backward and the ReLU of the score
        BWD_FOR(r, R) {
            int s = r % TS;
            float a = 0.f;
            BWD_DOT
            for (int j = 0; j < GDB_GF; ++j) a = fmaf(lds[L_DAGG + s * 32 + j], lds[L_G + r * 33 + j], a);
            lds[L_ROW + r * 8 + ROW_TMP] = a;
        }
        __syncthreads();
        BWD_FOR(s, TS) {
            float dot = 0.f;
            BWD_VIEWS
            for (int v = 0; v < V; ++v) dot = fmaf(lds[L_ROW + (v * TS + s) * 8 + ROW_A], lds[L_ROW + (v * TS + s) * 8 + ROW_TMP], dot);
            BWD_VIEWS
            for (int v = 0; v < V; ++v) {
                int r = v * TS + s;
                float ds = lds[L_ROW + r * 8 + ROW_A] * (lds[L_ROW + r * 8 + ROW_TMP] - dot);
                lds[L_ROW + r * 8 + ROW_DS] = lds[L_ROW + r * 8 + ROW_SPRE] > 0.f ? ds : 0.f;
            }
        }
        __syncthreads();
        // ---- 15. d global_fc-pre, per view and summed over views
        BWD_FOR(k, R * GDB_GF) {
            int r = k / GDB_GF, j = k % GDB_GF, s = r % TS;
            float dG = lds[L_DAGG + s * 32 + j] * lds[L_ROW + r * 8 + ROW_A] + pw[PW_AGG_W + j] * lds[L_ROW + r * 8 + ROW_DS];
            lds[L_DA + r * 32 + j] = lds[L_G + r * 33 + j] > 0.f ? dG : 0.f;
        }
        __syncthreads();
        BWD_FOR(k, TS * GDB_GF) {
            int s = k / GDB_GF, j = k % GDB_GF;
            float a = 0.f;
            BWD_VIEWS
            for (int v = 0; v < V; ++v) a += lds[L_DA + (v * TS + s) * 32 + j];
            lds[L_SDA + s * 32 + j] = a;
        }
        __syncthreads();
        // ---- 16. d [var | mean]: they feed global_fc of EVERY view, so their gradient takes the sum over views of d global_fc-pre
        BWD_FOR(k, TS * 2 * GDB_CFR) {
            int s = k / (2 * GDB_CFR), c = k % (2 * GDB_CFR);
            float a = 0.f;
            BWD_DOT
            for (int j = 0; j < GDB_GF; ++j) a = fmaf(pw[PW_GLOB_W + j * 3 * GDB_CFR + GDB_CFR + c], lds[L_SDA + s * 32 + j], a);
            lds[L_DVM + s * 38 + c] = a;
        }
        __syncthreads();
        // ---- 17. d g_v: its own columns of global_fc, plus mean (1 / V) and var (2 (g_v - mean) / (V - 1)); d view_fc-pre;
        //          d feat19 joins the tail's gradient from weight.0
        BWD_FOR(k, R * 20) {
            int r = k / 20, c = k % 20, s = r % TS;
            float dv = 0.f;
            if (c < GDB_CFR) {
                float a = 0.f;
                BWD_DOT
                for (int j = 0; j < GDB_GF; ++j) a = fmaf(pw[PW_GLOB_W + j * 3 * GDB_CFR + c], lds[L_DA + r * 32 + j], a);
                float dev = lds[L_GV + r * 20 + c] - lds[L_VM + s * 38 + GDB_CFR + c];
                a += lds[L_DVM + s * 38 + GDB_CFR + c] / Vf;
                a += lds[L_DVM + s * 38 + c] * (2.f * dev / (Vf - 1.f));
                lds[L_DT + r * 24 + c] += a;
                dv = lds[L_VP + r * 20 + c] > 0.f ? a : 0.f;
            }
            lds[L_VP + r * 20 + c] = dv;
        }
        __syncthreads();
        // ---- 18. d dir from view_fc
        if (viewdir) BWD_FOR(k, R * 4) {
            int r = k / 4, d = k % 4;
            float a = 0.f;
            BWD_DOT
            for (int c = 0; c < GDB_CFR; ++c) a = fmaf(pw[PW_VIEW_W + 4 * c + d], lds[L_VP + r * 20 + c], a);
            lds[L_DT + r * 24 + GDB_CFR + d] += a;
        }
        __syncthreads();
        // ---- 19. g_rgbs_feat_dir.  Channels Q-19 .. Q-1 of a view's row are BOTH blended (x[..., :-4] * wv) and fed to view_fc /
        //          global_fc / weight.0 as the tail's feat19: their gradient is the sum of both paths.
        if (g_xin) BWD_FOR(k, R * P) {
            int r = k / P, c = k % P; int64_t i = base + r % TS;
            if (i < n_alloc) {
                float a = 0.f;
                if (i < n) {
                    if (c < Q) a = g_feat[(size_t)i * F + c] * lds[L_ROW + r * 8 + ROW_WV];
                    if (c >= T) a += lds[L_DT + r * 24 + c - T];
                }
                g_xin[((size_t)(r / TS) * n_alloc + i) * P + c] = a;
            }
        }
        // ---- 20. dW += dY^T [X | 1] on the matrix cores
        dw_accumulate<BWD_TILES_PER_WAVE>(c_bwd_table, lds, R, TS, acc, wave, lane);
        __syncthreads();   // the next tile overwrites the LDS image
    }

    // ---- this workgroup's ONE partial: zeros (pad slots, view_fc without viewdir_agg), then every wave's tiles
    float* part = partials + (size_t)blockIdx.x * PW_FP32_FLOATS;
    BWD_FOR(k, PW_FP32_FLOATS) part[k] = 0.f;
    __syncthreads();
    dw_store_partial<BWD_TILES_PER_WAVE>(c_bwd_table, part, acc, wave, lane);
}

__global__ void k_mlp_bwd_reduce(const float* __restrict__ partials, int nparts, float* __restrict__ out) {
    dw_reduce(partials, nparts, PW_FP32_FLOATS, out);
}

static int bwd_grid(int64_t n_alloc) {
    int64_t tiles = (n_alloc + BWD_TS - 1) / BWD_TS;
    return (int)(tiles < BWD_MAX_WG ? tiles : BWD_MAX_WG);
}

extern "C" int gdb_mlp_backward_layout(const GdbConfig* cfg, int32_t V, int64_t n_alloc, size_t out[3]) {
    int rc = gdb_check_cfg(cfg); if (rc) return rc;
    if (!out) return gdb_fail(GDB_E_BADARG, "out is NULL");
    if (V < 2 || V > GDB_MAX_VIEWS) return gdb_fail(GDB_E_SHAPE, "V=%d outside 2..%d (the unbiased variance has no derivative at V = 1)", V, GDB_MAX_VIEWS);
    if (n_alloc < 1) return gdb_fail(GDB_E_SHAPE, "n_alloc must be positive");
    int g = bwd_grid(n_alloc);
    out[0] = sizeof(float) * (size_t)g * PW_FP32_FLOATS; out[1] = (size_t)g; out[2] = BWD_TS;
    return GDB_OK;
}

extern "C" int gdb_mlp_backward(const GdbConfig* cfg, const float* pw, int32_t V, const float* vox, const float* xin,
                                const int64_t* total, int64_t n_alloc, const float* g_sigma, const float* g_feat, float* g_packed,
                                float* g_vox, float* g_xin, void* workspace, size_t workspace_bytes, void* stream_) {
    size_t lay[3];
    int rc = gdb_mlp_backward_layout(cfg, V, n_alloc, lay); if (rc) return rc;
    if (!pw || !vox || !xin || !g_sigma || !g_feat || !g_packed || !workspace) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (workspace_bytes < lay[0]) return gdb_fail(GDB_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, lay[0]);
    hipStream_t st = (hipStream_t)stream_;
    int P = 3 * cfg->bundle_size * cfg->bundle_size + GDB_FV;
    int g = (int)lay[1];
    hipLaunchKernelGGL(k_mlp_bwd, dim3((unsigned)g), dim3(BWD_THREADS), 0, st, pw, V, cfg->viewdir_agg, P, vox, xin, total, n_alloc,
                       g_sigma, g_feat, g_vox, g_xin, (float*)workspace);
    LAUNCH_CHECK("k_mlp_bwd");
    hipLaunchKernelGGL(k_mlp_bwd_reduce, dim3((PW_FP32_FLOATS + 255) / 256), dim3(256), 0, st, (const float*)workspace, g, g_packed);
    LAUNCH_CHECK("k_mlp_bwd_reduce");
    return GDB_OK;
}

extern "C" int gdb_unpack_weight_grads(const GdbConfig* cfg, const float* h_packed, float* const t[18]) {
    int rc = gdb_check_cfg(cfg); if (rc) return rc;
    if (!h_packed || !t) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    static const int offs[18] = {PW_VIEW_W, PW_VIEW_B, PW_GLOB_W, PW_GLOB_B, PW_AGG_W, PW_AGG_B, PW_FC_W, PW_FC_B, PW_LR0_W,
                                 PW_LR0_B, PW_SIG_W, PW_SIG_B, PW_W0_W, PW_W0_B, PW_W2_W, PW_W2_B, PW_FH_W, PW_FH_B};
    static const int sizes[18] = {GDB_CFR * 4, GDB_CFR, GDB_GF * 3 * GDB_CFR, GDB_GF, GDB_GF, 1, GDB_IM * GDB_GF, GDB_IM,
                                  GDB_HID * GDB_HD, GDB_HID, GDB_HID, 1, GDB_HID * GDB_W0IN, GDB_HID, GDB_HID, 1,
                                  GDB_CV * GDB_HID, GDB_CV};
    for (int i = 0; i < 18; ++i) {
        if (i < 2 && !cfg->viewdir_agg) continue;   // view_fc does not exist without viewdir_agg: its slots are zero, nothing to hand out
        if (!t[i]) return gdb_fail(GDB_E_BADARG, "gradient tensor %d is NULL", i);
        memcpy(t[i], h_packed + offs[i], sizeof(float) * sizes[i]);
    }
    return GDB_OK;
}

// ============================================================================================
// composite backward
// ============================================================================================
// One lane per bundle.  alpha = 1 - e^-sigma, T_i = prod_{j<i}(1 - alpha_j), u_i = alpha_i T_i, D = max(sum u, 1e-6), w = u / D:
//   g_u,i = (g_w,i - [sum u > 1e-6] sum_k g_w,k w_k) / D          g_sigma,i = g_u,i T_i (1 - alpha_i) - sum_{k>i} g_u,k u_k
// Division-free in (1 - alpha), which underflows to 0 at sigma ~ 100.  The forward sweep parks T_{i+1} in g_sigma[i] (this lane's
// own rows), the backward sweep reads it back and overwrites it with the result.
__global__ void k_render_weights_bwd(int64_t n_bundles, const int32_t* __restrict__ seg, const float* __restrict__ sigma,
                                     const float* __restrict__ g_w, float* __restrict__ g_sigma) {
    int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bundles) return;
    int s = seg[2 * b], e = seg[2 * b + 1];
    // alpha, T and u are the forward's fp32 values; the sums around them run in double: g_w,i - sum_k g_w,k w_k cancels to a small
    // fraction of g_w when a bundle's samples look alike (a freshly initialised network), and fp32 sums left the gradient of
    // sigma.0 outside the referee's bound there
    float T = 1.f;
    double sum = 0.0, dot = 0.0;
    for (int i = s; i < e; ++i) {
        float alpha = 1.f - expf(-sigma[i]);
        float u = alpha * T;
        T = T * (1.f - alpha);
        g_sigma[i] = T;
        sum += (double)u;
        dot += (double)g_w[i] * (double)u;
    }
    const bool clamped = !((float)sum > 1e-6f);
    const double den = clamped ? (double)1e-6f : sum;
    const double c = clamped ? 0.0 : dot / den;   // sum_k g_w,k w_k; clamp_min has derivative 0 below the clamp
    double suffix = 0.0;
    for (int i = e - 1; i >= s; --i) {
        float Tn = g_sigma[i], Ti = i == s ? 1.f : g_sigma[i - 1];
        float alpha = 1.f - expf(-sigma[i]);
        float u = alpha * Ti;
        double gu = ((double)g_w[i] - c) / den;
        g_sigma[i] = (float)(gu * (double)Tn - suffix);
        suffix += gu * (double)u;
    }
}

extern "C" int gdb_render_weights_backward(const GdbConfig* cfg, const float* sigma, const int64_t* idx, const int64_t* total,
                                           int64_t n_alloc, int64_t n_bundles, const float* g_weights, float* g_sigma,
                                           void* scratch, void* stream_) {
    int rc = gdb_check_cfg(cfg); if (rc) return rc;
    if (!sigma || !idx || !g_weights || !g_sigma || !scratch) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (n_alloc < 1 || n_bundles < 1 || n_alloc >= ((int64_t)1 << 31)) return gdb_fail(GDB_E_SHAPE, "bad sizes");
    hipStream_t st = (hipStream_t)stream_;
    int32_t* seg = (int32_t*)scratch;
    hipError_t e = hipMemsetAsync(g_sigma, 0, sizeof(float) * (size_t)n_alloc, st);   // samples of no bundle, rows past *d_total
    if (e != hipSuccess) return gdb_fail(GDB_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    rc = gdb_seg_bounds_launch(idx, total, n_alloc, n_bundles, seg, st); if (rc) return rc;
    hipLaunchKernelGGL(k_render_weights_bwd, dim3((unsigned)((n_bundles + 255) / 256)), dim3(256), 0, st, n_bundles, (const int32_t*)seg,
                       sigma, g_weights, g_sigma);
    LAUNCH_CHECK("k_render_weights_bwd");
    return GDB_OK;
}

// One lane per sample: g_w,i = g_F[b] . f_i + g_Z[b] z_i + g_O[b];  g_f,i = w_i g_F[b].  z_vals gets no gradient (it comes from the
// sampler).  Rows past *d_total and samples of no bundle get zeros.
__global__ void k_accumulate_bwd(int64_t n_alloc, const int64_t* __restrict__ total, int64_t n_bundles, int C,
                                 const int64_t* __restrict__ idx, const float* __restrict__ weights, const float* __restrict__ feat,
                                 const float* __restrict__ z, const float* __restrict__ gF, const float* __restrict__ gZ,
                                 const float* __restrict__ gO, float* __restrict__ g_w, float* __restrict__ g_f) {
    int64_t n = total ? *total : n_alloc;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_alloc) return;
    int64_t b = i < n ? idx[i] : -1;
    if (b < 0 || b >= n_bundles) {
        g_w[i] = 0.f;
        for (int c = 0; c < C; ++c) g_f[(size_t)i * C + c] = 0.f;
        return;
    }
    const float w = weights[i];
    double a = 0.0;   // (double: the three terms may cancel)
    for (int c = 0; c < C; ++c) {
        float g = gF[(size_t)b * C + c];
        a += (double)g * (double)feat[(size_t)i * C + c];
        g_f[(size_t)i * C + c] = w * g;
    }
    g_w[i] = (float)(a + (double)gZ[b] * (double)z[i] + (double)gO[b]);
}

extern "C" int gdb_accumulate_backward(const GdbConfig* cfg, const float* weights, const float* feat, const float* z, const int64_t* idx,
                                       const int64_t* total, int64_t n_alloc, int64_t n_bundles, int32_t channels, const float* gF,
                                       const float* gZ, const float* gO, float* g_weights, float* g_feat, void* scratch, void* stream_) {
    int rc = gdb_check_cfg(cfg); if (rc) return rc;
    (void)scratch;   // the per-sample form needs no segment bounds
    if (!weights || !feat || !z || !idx || !gF || !gZ || !gO || !g_weights || !g_feat) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (n_alloc < 1 || n_bundles < 1 || channels < 1 || n_alloc >= ((int64_t)1 << 31)) return gdb_fail(GDB_E_SHAPE, "bad sizes");
    hipLaunchKernelGGL(k_accumulate_bwd, dim3((unsigned)((n_alloc + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, n_alloc, total,
                       n_bundles, (int)channels, idx, weights, feat, z, gF, gZ, gO, g_weights, g_feat);
    LAUNCH_CHECK("k_accumulate_bwd");
    return GDB_OK;
}
