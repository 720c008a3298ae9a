// Backward of the plane-sweep cost volume (gdb_build_feature_volume, gdb_costvol.hip; networks/gdb_nerf/depth_net.py
// build_feature_volume is the specification): given the forward's inputs and the upstream g_cost (B, C, D, Ht, Wt),
//   g_src_feat     (B, V, C, Hs, Ws)  d val_v = g (2 / V)(val_v - mean) (biased variance) scattered through the four bilinear tap
//                                     weights of view v; zeros padding: an out-of-range tap, a non-finite projection and a view behind
//                                     the clamp contribute what the forward's weights say (nothing where the weight is 0);
//   g_depth_values (B, D, Ht, Wt)     per voxel sum over views and channels of d val_v (dval_v/dix dix/ddepth + dval_v/diy diy/ddepth),
//                                     d/ddepth of p = q depth + t through the perspective divide with clamp_min(1e-6)'s derivative
//                                     (1 where p_z >= 1e-6), times -1 / h^2 under inv_depth.  A view whose dix/ddepth or diy/ddepth
//                                     is not finite (a non-finite hypothesis) adds nothing.
// The cameras get no gradient.  Coordinates, floor, tap indices and weights are the forward's own bits: costvol_view of
// gdb_costvol_body.h under -ffp-contract=off, the code k_costvol runs.
//
// g_src_feat is a scatter-add into arbitrary texels, made reproducible as gdb_encode_backward.hip does by
// accumulating in FIXED POINT:
//   1. k_cvb_max   G = max |g_cost| and S = max |src_feat| as unsigned integer maxima of the float bit patterns (order-independent).
//   2. k_cvb       one lane per voxel regathers val_v (the forward's products and sums), forms mean and d val_v in double and leaves
//                  d val_v in LDS; then all lanes walk the (view, row, voxel, x tap, channel) slots, channel fastest and the x tap next,
//                  form w d val_v in double, scale by 2^(F - e), round to int64 (llrint) and add with ONE 64-bit integer atomic:
//                  integer addition is associative, so the sum does not depend on arrival order.  The scale is a power of two.
//   3. k_cvb_fold  integer -> double -> float, one lane per destination, channel-last -> planar.
// Fixed-point rule: |val_v| <= S (the four weights are non-negative and sum to at most 1), |val_v - mean| <= 2 S, 2 / V <= 2, so
// |w d val_v| <= 4 G S <= 2^e with e = ceil(log2 G) + ceil(log2 S) + 2.  One texel of one (batch, view, channel) receives at most
// four contributions from each of the D Ht Wt voxels of its batch, so F = min(40, 62 - ceil(log2(4 D Ht Wt))) keeps every sum
// inside int64.  The absolute resolution of a contribution is 2^(e - F).
// G == 0 or S == 0: nothing is scattered and both outputs are exact zeros.  G or S not finite: the values cannot be scaled; both
// outputs are filled with NaN.
//
// Accumulator (caller's workspace, zeroed by the entry), channel-last so that the lanes of a wave-instruction run along the channels
// of a tap and its x neighbour:  int64 [B * V][Hs][Ws][C].  A pass walks CVB_CC = 8 channels, so the slots of one (voxel, view, row)
// are two runs of 64 contiguous bytes, C * 8 bytes apart: one 128-byte run only at C == 8, runs 128 / 256 bytes apart at C = 16 / 32.
// Four voxels to a wave-instruction.  That is short of the 128 .. 256 contiguous bytes per atomic wave-instruction the guides ask
// for; walking 16 channels per pass would reach it at the cost of twice the LDS, and was not tried.
// g_depth_values has one owner per element (the voxel's lane): a gather, fixed order.
#include "gdb_internal.h"
#include "gdb_costvol_body.h"

#define CVB_HDR_BYTES 256   // [0] max |g_cost| bits, [1] max |src_feat| bits
#define CVB_TV 128          // voxels (= threads) per workgroup
#define CVB_CC 8            // channels per pass through LDS

static int cvb_ceil_log2(uint64_t x) { int r = 0; while (((uint64_t)1 << r) < x) ++r; return r; }
static int cvb_frac_bits(int D, int Ht, int Wt) { int f = 62 - cvb_ceil_log2((uint64_t)4 * D * (uint64_t)Ht * Wt); return f < 40 ? f : 40; }

struct CvbLayout { size_t projOff, accOff, accBytes, small, total; };
static CvbLayout cvb_layout(int B, int V, int C, int Hs, int Ws) {
    CvbLayout l{};
    l.projOff = CVB_HDR_BYTES;
    l.accOff = align_up(l.projOff + sizeof(float) * 12 * (size_t)B * V, 256);
    l.small = l.accOff;   // what a call without g_src_feat needs
    l.accBytes = sizeof(int64_t) * (size_t)B * V * C * Hs * Ws;
    l.total = align_up(l.accOff + l.accBytes, 256);
    return l;
}

// e = ceil(log2 x) of a finite positive float given by its bits (denormals included)
__device__ __forceinline__ int cvb_exp(unsigned gb) {
    int ex;
    float m = frexpf(__uint_as_float(gb), &ex);   // x = m 2^ex, m in [0.5, 1)
    return m == 0.5f ? ex - 1 : ex;
}
__device__ __forceinline__ double cvb_pow2(int k) { return __longlong_as_double((long long)(1023 + k) << 52); }   // -1022 <= k <= 1023

__global__ void k_cvb_proj(int B, int V, const float* __restrict__ src_exts, const float* __restrict__ src_ints,
                           const float* __restrict__ tar_exts, const float* __restrict__ tar_ints, float* __restrict__ proj) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * V) return;
    costvol_proj_one<false>(t, V, src_exts, src_ints, tar_exts, tar_ints, 1.f, 1.f, proj);
}

// ---- 1. scale: blockIdx.y = 0 the upstream, 1 the source maps ----------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cvb_max(const float* __restrict__ g, size_t ng, const float* __restrict__ f, size_t nf,
                                                 unsigned* __restrict__ hdr) {
    const float* p = blockIdx.y ? f : g;
    const size_t n = blockIdx.y ? nf : ng, step = (size_t)gridDim.x * blockDim.x;
    unsigned m = 0;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += step) m = max(m, __float_as_uint(p[t]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    __shared__ unsigned s_m[4];
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {   // one atomic per workgroup of a bounded grid, and only if it can still raise the word
#pragma unroll
        for (int w = 1; w < 4; ++w) m = max(m, s_m[w]);
        if (m > __hip_atomic_load(hdr + blockIdx.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(hdr + blockIdx.y, m);
    }
}

// ---- 2. regather, depth gradient, scatter ----------------------------------------------------------------------------------------
struct CvbArgs {
    int B, V, C, Hs, Ws, D, Ht, Wt, inv_depth, tiles, F;
    const float* feat; const float* proj; const float* depth_values; const float* g_cost; const unsigned* hdr;
    long long* acc; float* g_depth;
};
struct CvbTap { unsigned off0, off1; float w[4]; };   // the row offsets of the x pair and (w00, w01, w10, w11) of one (voxel, view)

template <int VT, bool SRC, bool DEPTH>
__global__ void __launch_bounds__(CVB_TV) k_cvb(CvbArgs a) {
    extern __shared__ __align__(16) unsigned char cvb_lds[];
    CvbTap* s_tap = (CvbTap*)cvb_lds;                                       // [CVB_TV][VT]
    float* s_dv = (float*)(cvb_lds + sizeof(CvbTap) * CVB_TV * VT);         // [CVB_TV][VT][CVB_CC]
    // 1-D grid over (batch, depth plane, tile of CVB_TV voxels of the flattened (y, x) plane), tile innermost
    unsigned lb = blockIdx.x;
    const int tile = lb % a.tiles; lb /= a.tiles;
    const int d = lb % a.D, b = lb / a.D;
    const int tid = threadIdx.x;
    const int t = tile * CVB_TV + tid;
    const bool live = t < a.Ht * a.Wt;
    const int y = live ? t / a.Wt : 0, x = live ? t - y * a.Wt : 0;
    const size_t vox = ((size_t)d * a.Ht + y) * a.Wt + x;
    const size_t ovol = (size_t)a.D * a.Ht * a.Wt;
    const unsigned gb = a.hdr[0], sb = a.hdr[1];
    if (gb == 0 || sb == 0 || gb >= 0x7f800000u || sb >= 0x7f800000u) {   // uniform: the whole workgroup leaves
        if (DEPTH && live) a.g_depth[(size_t)b * ovol + vox] = (gb >= 0x7f800000u || sb >= 0x7f800000u) ? __uint_as_float(0x7fc00000u) : 0.f;
        return;
    }
    const float h = live ? a.depth_values[(size_t)b * ovol + vox] : 1.f;
    float depth = h;
    if (a.inv_depth) depth = 1.f / depth;                                                     // :445-446
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    unsigned off0[VT], off1[VT];
    float w00[VT], w01[VT], w10[VT], w11[VT];
    float q00[VT], q01[VT], q10[VT], q11[VT];   // d val_v / d depth = a0 q00 + a1 q01 + b0 q10 + b1 q11 over the four texels
#pragma unroll
    for (int v = 0; v < VT; ++v) {
        CostVolView g;
        costvol_view(a.proj + ((size_t)b * a.V + v) * 12, px, py, depth, a.Hs, a.Ws, g);
        off0[v] = (unsigned)(g.ya * a.Ws + g.xs); off1[v] = (unsigned)(g.yb * a.Ws + g.xs);
        w00[v] = g.e0 * g.ra; w01[v] = g.e1 * g.ra; w10[v] = g.e0 * g.rb; w11[v] = g.e1 * g.rb;
        if (!live) { w00[v] = w01[v] = w10[v] = w11[v] = 0.f; }
        if (SRC) {
            CvbTap tp;
            tp.off0 = off0[v]; tp.off1 = off1[v]; tp.w[0] = w00[v]; tp.w[1] = w01[v]; tp.w[2] = w10[v]; tp.w[3] = w11[v];
            s_tap[tid * VT + v] = tp;
        }
        if (DEPTH) {
            // ix = p0 / z - 1/2, z = max(p2, 1e-6): d ix / d depth = q0 / z - p0 dz / z^2, dz = q2 where the clamp passes
            const double z = (double)fmaxf(g.p[2], 1e-6f), dz = g.p[2] >= 1e-6f ? (double)g.q[2] : 0.0;
            const double kx = (double)g.q[0] / z - (double)g.p[0] * dz / (z * z), ky = (double)g.q[1] / z - (double)g.p[1] * dz / (z * z);
            // the derivatives of the forward's weights: the in-range x taps are 1 - fx at x0 and fx at x0 + 1, the rows likewise
            const float da = (g.x0 >= 0 && g.x0 <= a.Ws - 1) ? -1.f : 0.f, db = (g.x0 + 1 >= 0 && g.x0 + 1 <= a.Ws - 1) ? 1.f : 0.f;
            float d0 = (g.x0 == g.xs ? da : 0.f) + (g.x0 + 1 == g.xs ? db : 0.f);
            float d1 = (g.x0 == g.xs + 1 ? da : 0.f) + (g.x0 + 1 == g.xs + 1 ? db : 0.f);
            if (!g.finite) { d0 = d1 = 0.f; }
            const float sa = (g.y0 >= 0 && g.y0 <= a.Hs - 1) ? -1.f : 0.f, sb2 = (g.y0 + 1 >= 0 && g.y0 + 1 <= a.Hs - 1) ? 1.f : 0.f;
            const bool ok = live && kx - kx == 0.0 && ky - ky == 0.0;   // finite
            q00[v] = ok ? (float)((double)(d0 * g.ra) * kx + (double)(g.e0 * sa) * ky) : 0.f;
            q01[v] = ok ? (float)((double)(d1 * g.ra) * kx + (double)(g.e1 * sa) * ky) : 0.f;
            q10[v] = ok ? (float)((double)(d0 * g.rb) * kx + (double)(g.e0 * sb2) * ky) : 0.f;
            q11[v] = ok ? (float)((double)(d1 * g.rb) * kx + (double)(g.e1 * sb2) * ky) : 0.f;
        }
    }
    const size_t plane = (size_t)a.Hs * a.Ws;
    const double two_over_v = 2.0 / (double)a.V, inv_v = 1.0 / (double)a.V;
    const double scale = cvb_pow2(a.F - (cvb_exp(gb) + cvb_exp(sb) + 2));
    double gd = 0.0;
    for (int c0 = 0; c0 < a.C; c0 += CVB_CC) {
        const int cn = min(CVB_CC, a.C - c0);
        for (int cc = 0; cc < cn; ++cc) {
            const int c = c0 + cc;
            const float g = live ? a.g_cost[((size_t)b * a.C + c) * ovol + vox] : 0.f;
            float val[VT], ta[VT], tb[VT], tc[VT], td[VT];
            double mean = 0.0;
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const float* pl = a.feat + (((size_t)b * a.V + v) * a.C + c) * plane;
                const F2c t0 = *(const F2c*)(pl + off0[v]), t1 = *(const F2c*)(pl + off1[v]);
                ta[v] = t0.x; tb[v] = t0.y; tc[v] = t1.x; td[v] = t1.y;
                val[v] = t0.x * w00[v] + t0.y * w01[v] + t1.x * w10[v] + t1.y * w11[v];      // :472, the forward's sequence
                mean += (double)val[v];
            }
            mean *= inv_v;
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const double dv = (double)g * two_over_v * ((double)val[v] - mean);
                if (SRC) s_dv[(tid * VT + v) * CVB_CC + cc] = (float)dv;
                if (DEPTH) gd += dv * ((double)ta[v] * (double)q00[v] + (double)tb[v] * (double)q01[v] + (double)tc[v] * (double)q10[v] + (double)td[v] * (double)q11[v]);
            }
        }
        if (SRC) {
            __syncthreads();
            // slot = (((v 2 + dy) CVB_TV + voxel) 2 + dx) CVB_CC + channel
            for (int s = tid; s < VT * 4 * CVB_TV * CVB_CC; s += CVB_TV) {
                const int cc = s % CVB_CC, dx = (s / CVB_CC) & 1, vx = (s / (2 * CVB_CC)) % CVB_TV, r = s / (2 * CVB_CC * CVB_TV);
                const int dy = r & 1, v = r >> 1;
                if (cc >= cn) continue;
                const CvbTap& tp = s_tap[vx * VT + v];
                const float w = tp.w[dy * 2 + dx];
                if (w == 0.f) continue;   // the forward's zero weight: nothing to add
                const float dv = s_dv[(vx * VT + v) * CVB_CC + cc];
                const size_t texel = ((size_t)b * a.V + v) * plane + (dy ? tp.off1 : tp.off0) + dx;
                __hip_atomic_fetch_add(a.acc + texel * a.C + c0 + cc, llrint((double)w * (double)dv * scale), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);   // result unused: a no-return vector atomic
            }
            __syncthreads();
        }
    }
    if (DEPTH && live) {
        if (a.inv_depth && gd != 0.0) gd *= -1.0 / ((double)h * (double)h);   // (a zero sum stays zero at h = 0)
        a.g_depth[(size_t)b * ovol + vox] = (float)gd;
    }
}

// ---- 3. fold: one lane per element of g_src_feat ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cvb_fold(size_t n, int C, size_t plane, const unsigned* __restrict__ hdr, int F,
                                                  const long long* __restrict__ acc, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const unsigned gb = hdr[0], sb = hdr[1];
    if (gb >= 0x7f800000u || sb >= 0x7f800000u) { out[t] = __uint_as_float(0x7fc00000u); return; }
    const double unit = (gb && sb) ? cvb_pow2(cvb_exp(gb) + cvb_exp(sb) + 2 - F) : 0.0;
    const size_t bvc = t / plane, p = t - bvc * plane, bv = bvc / C, c = bvc - bv * C;
    out[t] = (float)((double)acc[(bv * plane + p) * C + c] * unit);
}

// ---- entries -----------------------------------------------------------------------------------------------------------------------
static int cvb_check(int B, int V, int C, int Hs, int Ws, int D, int Ht, int Wt) {
    if (B < 1 || V < 1 || C < 1 || Hs < 1 || Ws < 2 || D < 1 || Ht < 1 || Wt < 1) return gdb_fail(GDB_E_SHAPE, "bad cost-volume shape");
    if (V > GDB_MAX_VIEWS) return gdb_fail(GDB_E_SHAPE, "V=%d exceeds %d views", V, GDB_MAX_VIEWS);
    if ((size_t)C * Hs * Ws >= ((size_t)1 << 32)) return gdb_fail(GDB_E_SHAPE, "source feature map too large for 32-bit offsets");
    const size_t lim = ((size_t)1 << 31) - 8;
    const size_t plane_t = (size_t)Ht * Wt, tiles = (plane_t + CVB_TV - 1) / CVB_TV;
    if (plane_t >= lim || (size_t)B * D >= lim || (size_t)B * D * tiles >= lim)
        return gdb_fail(GDB_E_SHAPE, "cost volume too large for the launch grid");
    if ((size_t)D * plane_t >= ((size_t)1 << 40)) return gdb_fail(GDB_E_SHAPE, "cost volume too large for the fixed-point accumulators");
    if ((size_t)B * V * C * Hs * Ws >= ((size_t)1 << 40) || ((size_t)B * V * C * Hs * Ws + 255) / 256 >= lim)
        return gdb_fail(GDB_E_SHAPE, "source feature maps too large for the accumulators");
    return GDB_OK;
}

extern "C" int gdb_feature_volume_backward_workspace_bytes(int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht,
                                                           int32_t Wt, size_t* out_bytes, int32_t* out_frac_bits) {
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "out_bytes is NULL");
    int rc = cvb_check(B, V, C, Hs, Ws, D, Ht, Wt); if (rc) return rc;
    *out_bytes = cvb_layout(B, V, C, Hs, Ws).total;
    if (out_frac_bits) *out_frac_bits = cvb_frac_bits(D, Ht, Wt);
    return GDB_OK;
}

template <int VT>
static void cvb_launch(const CvbArgs& a, dim3 grid, hipStream_t st) {
    const size_t tap = sizeof(CvbTap) * CVB_TV * VT, lds = tap + sizeof(float) * CVB_TV * VT * CVB_CC;
    if (a.acc && a.g_depth) hipLaunchKernelGGL((k_cvb<VT, true, true>), grid, dim3(CVB_TV), lds, st, a);
    else if (a.acc) hipLaunchKernelGGL((k_cvb<VT, true, false>), grid, dim3(CVB_TV), lds, st, a);
    else hipLaunchKernelGGL((k_cvb<VT, false, true>), grid, dim3(CVB_TV), 0, st, a);
}

extern "C" int gdb_feature_volume_backward(const float* d_src_feat, const float* d_src_exts, const float* d_src_ints,
                                           const float* d_tar_exts, const float* d_tar_ints, const float* d_depth_values,
                                           const float* d_g_cost, int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D,
                                           int32_t Ht, int32_t Wt, int32_t inv_depth, void* d_ws, size_t ws_bytes, float* d_g_src_feat,
                                           float* d_g_depth_values, void* stream_) {
    if (!d_src_feat || !d_src_exts || !d_src_ints || !d_tar_exts || !d_tar_ints || !d_depth_values || !d_g_cost || !d_ws)
        return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (!d_g_src_feat && !d_g_depth_values) return gdb_fail(GDB_E_BADARG, "both outputs are NULL");
    int rc = cvb_check(B, V, C, Hs, Ws, D, Ht, Wt); if (rc) return rc;
    const CvbLayout l = cvb_layout(B, V, C, Hs, Ws);
    const size_t need = d_g_src_feat ? l.total : l.small;
    if (ws_bytes < need) return gdb_fail(GDB_E_WORKSPACE, "workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream_;
    unsigned* hdr = (unsigned*)d_ws;
    float* proj = (float*)((char*)d_ws + l.projOff);
    long long* acc = d_g_src_feat ? (long long*)((char*)d_ws + l.accOff) : nullptr;
    hipError_t err = hipMemsetAsync(d_ws, 0, CVB_HDR_BYTES, st);
    if (err == hipSuccess && acc) err = hipMemsetAsync(acc, 0, l.accBytes, st);
    if (err != hipSuccess) return gdb_fail(GDB_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(err));
    hipLaunchKernelGGL(k_cvb_proj, dim3((B * V + 63) / 64), dim3(64), 0, st, B, V, d_src_exts, d_src_ints, d_tar_exts, d_tar_ints, proj);
    LAUNCH_CHECK("k_cvb_proj");
    // the scale is taken over the whole upstream and all source maps whichever outputs are asked for
    const size_t ng = (size_t)B * C * D * Ht * Wt, nf = (size_t)B * V * C * Hs * Ws;
    const size_t mblk = ((ng > nf ? ng : nf) + 255) / 256;
    hipLaunchKernelGGL(k_cvb_max, dim3((unsigned)(mblk < 256 ? mblk : 256), 2), dim3(256), 0, st, d_g_cost, ng, d_src_feat, nf, hdr);
    LAUNCH_CHECK("k_cvb_max");
    const int tiles = (int)(((size_t)Ht * Wt + CVB_TV - 1) / CVB_TV), F = cvb_frac_bits(D, Ht, Wt);
    CvbArgs a{B, V, C, Hs, Ws, D, Ht, Wt, inv_depth, tiles, F, d_src_feat, proj, d_depth_values, d_g_cost, hdr, acc, d_g_depth_values};
    const dim3 grid((unsigned)((size_t)B * D * tiles));
    switch (V) {
        case 1: cvb_launch<1>(a, grid, st); break;
        case 2: cvb_launch<2>(a, grid, st); break;
        case 3: cvb_launch<3>(a, grid, st); break;
        case 4: cvb_launch<4>(a, grid, st); break;
        case 5: cvb_launch<5>(a, grid, st); break;
        case 6: cvb_launch<6>(a, grid, st); break;
        case 7: cvb_launch<7>(a, grid, st); break;
        default: cvb_launch<8>(a, grid, st); break;
    }
    LAUNCH_CHECK("k_cvb");
    if (acc) {
        hipLaunchKernelGGL(k_cvb_fold, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, nf, C, (size_t)Hs * Ws, hdr, F, acc, d_g_src_feat);
        LAUNCH_CHECK("k_cvb_fold");
    }
    return GDB_OK;
}
