// Backward of BundleSampler.encode (gdb_encode, gdb_ops.hip) with respect to the VALUES it gathers: the feature map img_feat
// (through the 2x2 box-filter mip chain and the linear-mipmap-linear fetch) and the feature volume (trilinear, border).
// The sample positions are held constant: rays_xyz, uvd, ball_radii, the cameras and src_images get no gradient.
//
// With the positions fixed the forward is linear in both tensors, so the backward is the transpose of the gather: a scatter-add
// into arbitrary texels.  It is made reproducible by accumulating in FIXED POINT:
//   1. k_encbwd_max    G = max |upstream| over the valid rows (i < *d_total) of g_vox and of the C_f + 3 feature columns of g_rfd
//                      (an unsigned integer max of the float bit patterns: order-independent).
//   2. k_encbwd_vol /  every contribution w * g is formed in double, scaled by 2^(F - e), e = ceil(log2 G), rounded to a 64-bit
//      k_encbwd_tex    integer (llrint) and added with ONE 64-bit integer atomic: integer addition is associative, so the sum does
//                      not depend on arrival order.  The scale is a power of two: the conversion is exact scaling.
//   3. k_encbwd_fold_* integer -> double -> float, one lane per destination; the pyramid levels are folded down through the
//                      transpose of the box chain in double, in the fixed order l = 0 .. L, and rounded to float once.
// Fixed-point rule: |w g| <= 2^e, and one destination receives at most 8 n_alloc contributions (8 volume taps, or the 4 texture
// taps of one level when both axes clamp), so F = min(40, 62 - ceil(log2(8 n_alloc))) keeps every sum inside int64.  The
// absolute resolution of a contribution is 2^(e - F): at F = 40 that is 2^-40 of the largest upstream value.
// G == 0: the accumulators stay zero, the scatters return at once and the outputs are exact zeros.  G not finite: a non-finite
// upstream cannot be scaled; the scatters return at once and the requested outputs are filled with NaN.
//
// Accumulators (caller's workspace, zeroed by the entry), channel-last so that the lanes of a wave-instruction run along the
// channels and the two x taps of a row:
//   pyramid  int64 [B * V][level][y][x][GDB_CP]   (GDB_CP = 20: the C_f + 3 = 19 channels + one pad that is never touched;
//                                                  a tap row is 160 B, x0 | x1 are adjacent: 320 B per wave-instruction segment)
//   volume   int64 [B][z][y][x][C_v]              (a tap row is 64 B, x0 | x1 128 B; one wave-instruction = the 8 taps of a sample)
// Compiled with -ffp-contract=off like gdb_ops.hip: the coordinates, levels and tap indices are the forward's own bits because they are
// the forward's own code, the gdb_encode_geom.h helpers k_encode_vox / k_encode_views call (vox_coords; subray_cam, centre_tex, tex_taps).
#include "gdb_encode_geom.h"

#define EB_HDR_BYTES 256   // [0] uint32: max over the upstream of (float bits & 0x7fffffff)
#define EB_ITEMS 64        // (view, sample) items per workgroup of k_encbwd_tex
#define EB_THREADS 256
#define EB_SLOTS (8 * GDB_CP)   // lanes of work per item: 2 levels x 2 y x 2 x x 20 channels

static int eb_ceil_log2(uint64_t x) { int r = 0; while (((uint64_t)1 << r) < x) ++r; return r; }
static int eb_frac_bits(int64_t n_alloc) { int f = 62 - eb_ceil_log2((uint64_t)8 * (uint64_t)n_alloc); return f < 40 ? f : 40; }

struct EbLayout { size_t pyrOff, pyrBytes, volOff, volBytes, total; };
static EbLayout eb_layout(const GdbFrame& f, const WsLayout& L) {
    EbLayout e{};
    e.pyrOff = EB_HDR_BYTES;
    e.pyrBytes = sizeof(int64_t) * L.pyrStride * f.B * f.V;
    e.volOff = align_up(e.pyrOff + e.pyrBytes, 256);
    e.volBytes = sizeof(int64_t) * (size_t)f.B * f.D * f.H * f.W * GDB_CV;
    e.total = align_up(e.volOff + e.volBytes, 256);
    return e;
}

// e = ceil(log2 G) of a finite positive float given by its bits (denormals included)
__device__ __forceinline__ int eb_exp(unsigned gb) {
    int ex;
    float m = frexpf(__uint_as_float(gb), &ex);   // G = m 2^ex, m in [0.5, 1)
    return m == 0.5f ? ex - 1 : ex;
}
__device__ __forceinline__ double eb_pow2(int k) { return __longlong_as_double((long long)(1023 + k) << 52); }   // -1022 <= k <= 1023

__device__ __forceinline__ void eb_add(long long* p, double c) {
    __hip_atomic_fetch_add(p, llrint(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // result unused: a no-return vector atomic
}

// ---- 1. scale ----------------------------------------------------------------------------------------------------------------
// blockIdx.y = view: 32 lanes per sample row, lanes 0 .. 18 read the row's 76 contiguous bytes of feature columns (no index division);
// blockIdx.y = V: the flat g_vox
__global__ void k_encbwd_max(int V, int P, int col0, const float* __restrict__ g_rfd, const float* __restrict__ g_vox,
                             const int64_t* __restrict__ total, int64_t n_alloc, unsigned* __restrict__ hdr) {
    const int64_t n = total_clamped(total, n_alloc);
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    unsigned m = 0;
    if ((int)blockIdx.y == V) {
        for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * GDB_CV; t += step) m = max(m, __float_as_uint(g_vox[t]) & 0x7fffffffu);
    } else {
        const float* g = g_rfd + (int64_t)blockIdx.y * n_alloc * P + col0;
        for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * 32; t += step) {
            const int c = (int)(t & 31);
            if (c < GDB_CFR) m = max(m, __float_as_uint(g[(t >> 5) * P + c]) & 0x7fffffffu);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    // ONE atomic per workgroup of a bounded grid, and only if it can still raise the word: atomics on a single address serialise
    // (one per wave of 4,096 workgroups took 196 us here, the reads themselves a fraction of that)
    __shared__ unsigned s_m[EB_THREADS / 64];
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < EB_THREADS / 64; ++w) m = max(m, s_m[w]);
        if (m > __hip_atomic_load(hdr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(hdr, m);
    }
}

// ---- 2a. volume scatter: one wave per sample, lane = (dz, dy, dx, channel) -----------------------------------------------------
__global__ void k_encbwd_vol(DevFrame f, const float* __restrict__ uvd, const int64_t* __restrict__ per_batch,
                             const int64_t* __restrict__ total, int64_t n_alloc, const float* __restrict__ g_vox,
                             const unsigned* __restrict__ hdr, int F, long long* __restrict__ acc) {
    const unsigned gb = hdr[0];
    if (gb == 0 || gb >= 0x7f800000u) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = t >> 6;
    if (i >= total_clamped(total, n_alloc)) return;
    const int r = (int)(t & 63), c = r & 7, dx = (r >> 3) & 1, dy = (r >> 4) & 1, dz = (r >> 5) & 1;
    const int bi = batch_of(f.B, per_batch, i);
    VoxCoords t3;
    vox_coords(f, uvd, i, t3);
    int xx = t3.x0 + dx, yy = t3.y0 + dy, zz = t3.z0 + dz;
    if (xx > f.W - 1 || yy > f.H - 1 || zz > f.D - 1 || xx < 0 || yy < 0 || zz < 0) return;   // the forward's out-of-range tap: weight 0
    double w = (double)(dx ? t3.wx : 1.f - t3.wx) * (double)(dy ? t3.wy : 1.f - t3.wy) * (double)(dz ? t3.wz : 1.f - t3.wz);
    double scale = eb_pow2(F - eb_exp(gb));
    size_t vox = (((size_t)bi * f.D + zz) * f.H + yy) * f.W + xx;
    eb_add(acc + vox * GDB_CV + c, w * (double)g_vox[i * GDB_CV + c] * scale);
}

// ---- 2b. pyramid scatter ---------------------------------------------------------------------------------------------------------
// A workgroup takes EB_ITEMS samples of one view.  Its first wave recomputes each sample's texture coordinate and level with
// k_encode_views' helpers (centre_tex, tex_taps) and leaves the 8 taps (2 levels x 2 y x 2 x: texel index inside the (batch, view) pyramid, weight) in LDS;
// then all lanes walk the (sample, tap, channel) slots, channel fastest, x tap next: 40 consecutive lanes = one 320-byte segment.
template <int BB>
__global__ void __launch_bounds__(EB_THREADS)
k_encbwd_tex(DevFrame f, const float* __restrict__ rays_xyz, const float* __restrict__ ball_radii,
             const int64_t* __restrict__ per_batch, const int64_t* __restrict__ total, int64_t n_alloc,
             const float* __restrict__ g_rfd, const unsigned* __restrict__ hdr, int F, long long* __restrict__ acc) {
    constexpr int P = 3 * BB + GDB_CFR + 4;
    __shared__ int s_idx[EB_ITEMS * 8];      // texel index of the tap inside one (batch, view) pyramid; -1: no contribution
    __shared__ double s_w[EB_ITEMS * 8];
    __shared__ int s_bi[EB_ITEMS];
    const unsigned gb = hdr[0];
    if (gb == 0 || gb >= 0x7f800000u) return;   // uniform: the whole workgroup leaves
    const int64_t n = total_clamped(total, n_alloc);
    const int64_t i0 = (int64_t)blockIdx.x * EB_ITEMS;
    if (i0 >= n) return;
    const int v = blockIdx.y, tid = threadIdx.x;
    if (tid < EB_ITEMS) {
        const int64_t i = i0 + tid;
        if (i < n) {
            const int bi = batch_of(f.B, per_batch, i);
            const float* sc = src_cam(f, bi, v);
            float cc[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < BB; ++s) {
                float p[3], cam[3];
                subray_point<BB>(rays_xyz, i, s, p);
                subray_cam(sc, p, cam);
#pragma unroll
                for (int c = 0; c < 3; ++c) cc[c] += cam[c];
            }
            subray_mean<BB>(cc);
            CentreTex ct;
            centre_tex(f, sc, cc, ball_radii[i], ct);
            s_bi[tid] = bi;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double wl = k ? (double)ct.frac : 1.0 - (double)ct.frac;
                const bool on = k == 0 || ct.frac > 0.f;   // the forward skips level l1 when frac == 0
                TexTaps t;
                tex_taps(f, k ? ct.l1 : ct.l0, ct.tu, ct.tv, t);
                const int base = (int)(t.off / GDB_CP);
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int tap = k * 4 + dy * 2 + dx;
                        s_idx[tid * 8 + tap] = on ? base + (dy ? t.y1 : t.y0) * t.W + (dx ? t.x1 : t.x0) : -1;
                        s_w[tid * 8 + tap] = wl * (double)(dx ? t.fx : 1.f - t.fx) * (double)(dy ? t.fy : 1.f - t.fy);
                    }
            }
        } else {
            s_bi[tid] = 0;
#pragma unroll
            for (int tap = 0; tap < 8; ++tap) { s_idx[tid * 8 + tap] = -1; s_w[tid * 8 + tap] = 0.0; }
        }
    }
    __syncthreads();
    const double scale = eb_pow2(F - eb_exp(gb));
    const size_t texels = f.pyrStride / GDB_CP;
    for (int s = tid; s < EB_ITEMS * EB_SLOTS; s += EB_THREADS) {
        const int item = s / EB_SLOTS, r = s - item * EB_SLOTS;
        const int tap = r / GDB_CP, c = r - tap * GDB_CP;
        const int idx = s_idx[item * 8 + tap];
        if (idx < 0 || c >= GDB_CFR) continue;
        const int64_t i = i0 + item;
        const float g = g_rfd[((size_t)v * n_alloc + i) * P + 3 * BB + c];
        const size_t texel = ((size_t)s_bi[item] * f.V + v) * texels + (size_t)idx;
        eb_add(acc + texel * GDB_CP + c, s_w[item * 8 + tap] * (double)g * scale);
    }
}

// ---- 3. fold and convert -----------------------------------------------------------------------------------------------------------
// value of the outputs when nothing was scattered: 0 scales the (zero) accumulators, NaN marks a non-finite upstream
__device__ __forceinline__ bool eb_unit(unsigned gb, int F, double& unit) {
    if (gb >= 0x7f800000u) return false;
    unit = gb ? eb_pow2(eb_exp(gb) - F) : 0.0;
    return true;
}

__global__ void k_encbwd_fold_vol(int B, int D, int H, int W, const unsigned* __restrict__ hdr, int F,
                                  const long long* __restrict__ acc, float* __restrict__ out) {
    const size_t plane = (size_t)D * H * W, nvox = (size_t)B * plane;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nvox) return;
    double unit;
    const bool finite = eb_unit(hdr[0], F, unit);
    const size_t bi = t / plane, p = t - bi * plane;
#pragma unroll
    for (int c = 0; c < GDB_CV; ++c)
        out[(bi * GDB_CV + c) * plane + p] = finite ? (float)((double)acc[t * GDB_CV + c] * unit) : __uint_as_float(0x7fc00000u);
}

__global__ void k_encbwd_fold_img(DevFrame f, const unsigned* __restrict__ hdr, int F, const long long* __restrict__ acc,
                                  float* __restrict__ out) {
    const size_t plane = (size_t)f.H * f.W, ntex = (size_t)f.B * f.V * plane;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntex) return;
    double unit;
    const bool finite = eb_unit(hdr[0], F, unit);
    const size_t bv = t / plane, p = t - bv * plane;
    const int y = (int)(p / f.W), x = (int)(p - (size_t)y * f.W);
    const long long* a = acc + bv * f.pyrStride;
    // transpose of the 2x2 box chain: texel (y, x) of level 0 holds 4^-l of texel (y >> l, x >> l) of level l
    const long long* row[GDB_MAX_MIP + 1];
#pragma unroll
    for (int l = 0; l <= GDB_MAX_MIP; ++l)
        row[l] = l <= f.levels ? a + f.lvlOff[l] + ((size_t)(y >> l) * f.lvlW[l] + (x >> l)) * GDB_CP : a;
    for (int c = 0; c < GDB_CFR; ++c) {
        double s = 0.0;
#pragma unroll
        for (int l = 0; l <= GDB_MAX_MIP; ++l)
            if (l <= f.levels) s += (double)row[l][c] * (1.0 / (double)(1 << (2 * l)));
        out[(bv * GDB_CFR + c) * plane + p] = finite ? (float)(s * unit) : __uint_as_float(0x7fc00000u);
    }
}

// ---- entries -----------------------------------------------------------------------------------------------------------------------
static int eb_check(const GdbConfig* cfg, const GdbFrame* f, int64_t n_alloc) {
    int rc = gdb_check_cfg(cfg); if (rc) return rc;
    rc = gdb_check_frame(cfg, f, false); if (rc) return rc;
    return gdb_check_n_alloc(cfg, f, n_alloc);
}

extern "C" int gdb_encode_backward_layout(const GdbConfig* cfg, const GdbFrame* shape, int64_t n_alloc, size_t out[4]) {
    if (!out) return gdb_fail(GDB_E_BADARG, "out is NULL");
    int rc = eb_check(cfg, shape, n_alloc); if (rc) return rc;
    EbLayout e = eb_layout(*shape, ws_layout(*cfg, *shape));
    out[0] = e.total; out[1] = (size_t)eb_frac_bits(n_alloc); out[2] = e.pyrOff; out[3] = e.volOff;
    return GDB_OK;
}

extern "C" int gdb_encode_backward(const GdbConfig* cfg, const GdbFrame* f, const void* ws, const float* rays_xyz, const float* uvd,
                                   const float* ball, const int64_t* per_batch, const int64_t* total, int64_t n_alloc,
                                   const float* g_rfd, const float* g_vox, float* g_img_feat, float* g_feat_volume,
                                   void* bwd_ws, size_t bwd_bytes, void* stream_) {
    int rc = eb_check(cfg, f, n_alloc); if (rc) return rc;
    if (!ws || !rays_xyz || !uvd || !ball || !per_batch || !total || !g_rfd || !g_vox || !bwd_ws) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (!g_img_feat && !g_feat_volume) return gdb_fail(GDB_E_BADARG, "both outputs are NULL");
    WsLayout L = ws_layout(*cfg, *f);
    EbLayout e = eb_layout(*f, L);
    if (bwd_bytes < e.total) return gdb_fail(GDB_E_WORKSPACE, "workspace of %zu bytes, %zu needed", bwd_bytes, e.total);
    if ((size_t)f->B * f->V * L.pyrStride >= ((size_t)1 << 40) || L.pyrStride / GDB_CP >= ((size_t)1 << 31))
        return gdb_fail(GDB_E_SHAPE, "feature map too large for the pyramid accumulators");
    DevFrame d = dev_frame(*cfg, *f, L, ws);
    hipStream_t st = (hipStream_t)stream_;
    const int F = eb_frac_bits(n_alloc), bb = cfg->bundle_size * cfg->bundle_size, P = 3 * bb + GDB_CFR + 4;
    unsigned* hdr = (unsigned*)bwd_ws;
    long long* accP = (long long*)((char*)bwd_ws + e.pyrOff);
    long long* accV = (long long*)((char*)bwd_ws + e.volOff);
    hipError_t err = hipMemsetAsync(bwd_ws, 0, g_img_feat ? e.pyrOff + e.pyrBytes : EB_HDR_BYTES, st);
    if (err == hipSuccess && g_feat_volume) err = hipMemsetAsync(accV, 0, e.volBytes, st);
    if (err != hipSuccess) return gdb_fail(GDB_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(err));
    // the scale is taken over BOTH upstreams whichever outputs are asked for: an output alone is bit-identical to the pair's
    const size_t mblk = ((size_t)n_alloc * 32 + 255) / 256;
    hipLaunchKernelGGL(k_encbwd_max, dim3((unsigned)(mblk < 256 ? mblk : 256), f->V + 1), dim3(EB_THREADS), 0, st,
                       f->V, P, 3 * bb, g_rfd, g_vox, total, n_alloc, hdr);
    LAUNCH_CHECK("k_encbwd_max");
    if (g_feat_volume) {
        hipLaunchKernelGGL(k_encbwd_vol, dim3((unsigned)(((size_t)n_alloc * 64 + 255) / 256)), dim3(256), 0, st, d, uvd, per_batch, total,
                           n_alloc, g_vox, hdr, F, accV);
        LAUNCH_CHECK("k_encbwd_vol");
        const size_t nvox = (size_t)f->B * f->D * f->H * f->W;
        hipLaunchKernelGGL(k_encbwd_fold_vol, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, st, f->B, f->D, f->H, f->W, hdr, F,
                           accV, g_feat_volume);
        LAUNCH_CHECK("k_encbwd_fold_vol");
    }
    if (g_img_feat) {
        dim3 g((unsigned)((n_alloc + EB_ITEMS - 1) / EB_ITEMS), f->V);
        bb_dispatch(cfg->bundle_size, [&](auto bb) {
            hipLaunchKernelGGL(k_encbwd_tex<decltype(bb)::value>, g, dim3(EB_THREADS), 0, st, d, rays_xyz, ball, per_batch, total, n_alloc, g_rfd, hdr, F, accP);
        });
        LAUNCH_CHECK("k_encbwd_tex");
        const size_t ntex = (size_t)f->B * f->V * f->H * f->W;
        hipLaunchKernelGGL(k_encbwd_fold_img, dim3((unsigned)((ntex + 255) / 256)), dim3(256), 0, st, d, hdr, F, accP, g_img_feat);
        LAUNCH_CHECK("k_encbwd_fold_img");
    }
    return GDB_OK;
}
