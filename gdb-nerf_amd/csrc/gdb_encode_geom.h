// The geometry of BundleSampler.encode, stated ONCE for gdb_ops.hip and its backwards gdb_encode_backward.hip, gdb_position_backward.hip
// (the only units that include this).  The backwards must reproduce the forward's decisions - tap indices, fractions, the mip level
// and its blend, every clamp - bit for bit, so all three call the SAME helpers in the same order under -ffp-contract=off.
#pragma once
#include "gdb_internal.h"
#include <type_traits>

// bundle_size -> BB = b * b as a compile-time constant: f(std::integral_constant<int, BB>{})
template <class F> static auto bb_dispatch(int bundle_size, F&& f) {
    if (bundle_size == 1) return f(std::integral_constant<int, 1>{});
    if (bundle_size == 2) return f(std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 16>{});
}
// n_alloc, the rows the caller's sample buffers hold: gdb_encode's refusal, shared by its backwards
static inline int gdb_check_n_alloc(const GdbConfig* cfg, const GdbFrame* f, int64_t n_alloc) {
    if (n_alloc >= 1 && n_alloc <= (int64_t)f->B * f->H * f->W * cfg->max_num_samples) return GDB_OK;
    return gdb_fail(GDB_E_SHAPE, "n_alloc %lld outside 1..B*H*W*S_max", (long long)n_alloc);
}

#ifdef __HIPCC__
// ---- sub-ray point -> source camera -> source image ---------------------------------------------------------------------------
template <int BB>   // point s of sample i in rays_xyz (N, 3, b^2)
__device__ __forceinline__ void subray_point(const float* __restrict__ rays_xyz, int64_t i, int s, float p[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = rays_xyz[((size_t)i * 3 + c) * BB + s];
}
// cam = E [p; 1], E = sc[S_E..], the 3x4 world-to-camera rows.  :330
__device__ __forceinline__ void subray_cam(const float* __restrict__ sc, const float p[3], float cam[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = sc[S_E + 4 * r] * p[0] + sc[S_E + 4 * r + 1] * p[1] + sc[S_E + 4 * r + 2] * p[2] + sc[S_E + 4 * r + 3];
}
// im = K cam, zc = max(im_z, 1e-6), (gx, gy) = the grid_sample coordinate of im / zc in the Ho x Wo source image.  :331-335
__device__ __forceinline__ void cam_to_grid(const float* __restrict__ sc, const float cam[3], int Wo, int Ho, float im[3], float& zc,
                                            float& gx, float& gy) {
#pragma unroll
    for (int r = 0; r < 3; ++r) im[r] = sc[S_K + 3 * r] * cam[0] + sc[S_K + 3 * r + 1] * cam[1] + sc[S_K + 3 * r + 2] * cam[2];
    zc = fmaxf(im[2], 1e-6f);
    gx = 2.f * (im[0] / zc) / (float)Wo - 1.f; gy = 2.f * (im[1] / zc) / (float)Ho - 1.f;
}
// The four colour taps at (gx, gy), for k_posbwd_colour: the SECOND statement of what rgb_fetch (gdb_internal.h) does inside itself.
// rgb_fetch is also gdb_fused.hip's, whose kernels compile to other instructions once it is written through this helper, so it stays
// as it is and the forward keeps calling it.  A tap past the far edge (inx / iny false) is worth 0 and its index is clamped.  :336
struct ImgTaps { int x0, x1, y0, y1; bool inx, iny; float wx, wy; };
__device__ __forceinline__ void img_taps(float gx, float gy, int Ho, int Wo, ImgTaps& t) {
    float x = gs_coord(gx, Wo), y = gs_coord(gy, Ho);
    float xf = floorf(x), yf = floorf(y);
    t.wx = x - xf; t.wy = y - yf;
    t.x0 = (int)xf; t.y0 = (int)yf;
    t.inx = t.x0 + 1 <= Wo - 1; t.iny = t.y0 + 1 <= Ho - 1;
    t.x1 = min(t.x0 + 1, Wo - 1); t.y1 = min(t.y0 + 1, Ho - 1);
}

// ---- bundle centre -> mip level and texture coordinate ----------------------------------------------------------------------
template <int BB>   // the mean over the b^2 sub-rays of a sum formed in sub-ray order
__device__ __forceinline__ void subray_mean(float sum[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) sum[c] = sum[c] / (float)BB;
}

// Footprint -> mip level, with its intermediates (the position backward differentiates through them).  bundle_sampler.py:343-348
struct MipParts { float dist, q, sec2, r, A, C, a, c; };   // A, C: the arguments of the two floored square roots a, c
__device__ __forceinline__ void mip_level_parts(const float cc[3], float ball, MipParts& m) {
    m.dist = sqrtf(cc[0] * cc[0] + cc[1] * cc[1] + cc[2] * cc[2]);
    m.q = m.dist / cc[2];
    m.sec2 = m.q * m.q;
    m.r = m.dist / ball;
    m.A = m.r * m.r - 1.f; m.C = m.sec2 - 1.f;
    m.a = sqrtf(fmaxf(m.A, 1e-12f));
    m.c = sqrtf(fmaxf(m.C, 1e-12f));
}
__device__ __forceinline__ float mip_level(const MipParts& m, float src_pixr) { return log2f((m.sec2 / (m.a + m.c)) / src_pixr); }

// The centre cc (source camera frame) of a sample of radius ball: level and its clamp / blend, ci = KS cc, zc = max(ci_z, 1e-6),
// (tu, tv) = the texture coordinate in [0, 1]^2.  :340-354
struct CentreTex { MipParts mip; float level, ci[3], zc, tu, tv, frac; int l0, l1; };
__device__ __forceinline__ void centre_tex(const DevFrame& f, const float* __restrict__ sc, const float cc[3], float ball, CentreTex& t) {
    mip_level_parts(cc, ball, t.mip);
    t.level = mip_level(t.mip, sc[S_PIXR]);
#pragma unroll
    for (int r = 0; r < 3; ++r) t.ci[r] = sc[S_KS + 3 * r] * cc[0] + sc[S_KS + 3 * r + 1] * cc[1] + sc[S_KS + 3 * r + 2] * cc[2];
    t.zc = fmaxf(t.ci[2], 1e-6f);
    t.tu = t.ci[0] / t.zc / (float)f.W; t.tv = t.ci[1] / t.zc / (float)f.H;
    mip_select(t.level, f.levels, t.l0, t.l1, t.frac);
}

// The 2 x 2 texels of mip level l around (u, v), clamp-to-edge: level size and float offset inside a (batch, view) pyramid, tap
// indices, fractions.  (Level geometry by selects, level_geom: a per-lane index into the kernel-argument arrays can park them in
// private memory.)
struct TexTaps { int W, H; unsigned off; int x0, x1, y0, y1; float fx, fy; };
__device__ __forceinline__ void tex_taps(const DevFrame& f, int l, float u, float v, TexTaps& t) {
    level_geom(f, l, t.W, t.H, t.off);
    tex_coord(u, t.W, t.x0, t.x1, t.fx);
    tex_coord(v, t.H, t.y0, t.y1, t.fy);
}

// Forward half of the direction code at the world-space centre cw: at = cw - o, as = cw - C_v, td / sd their normalisations,
// dif = td - sd (the code is normalize(dif) and td . sd).  :361-368
__device__ __forceinline__ void dir_code_fwd(const float cw[3], const float* __restrict__ tc, const float* __restrict__ sc, float at[3],
                                             float as[3], float td[3], float sd[3], float dif[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) at[c] = cw[c] - tc[T_O + c];
    normalize3(at, td);
#pragma unroll
    for (int c = 0; c < 3; ++c) as[c] = cw[c] - sc[S_C + c];
    normalize3(as, sd);
#pragma unroll
    for (int c = 0; c < 3; ++c) dif[c] = td[c] - sd[c];
}

// ---- feature volume ---------------------------------------------------------------------------------------------------------
// Trilinear coordinates of sample i: 5-D grid_sample, border, align_corners=False.  Tap (dx, dy, dz) sits at (x0 + dx, ..) with
// weight (dx ? wx : 1 - wx) ..; a tap past the far edge is worth 0.  :322-324
struct VoxCoords { int x0, y0, z0; float wx, wy, wz; };
__device__ __forceinline__ void vox_coords(const DevFrame& f, const float* __restrict__ uvd, int64_t i, VoxCoords& t) {
    float x = gs_coord(uvd[i * 3 + 0], f.W), y = gs_coord(uvd[i * 3 + 1], f.H), z = gs_coord(uvd[i * 3 + 2], f.D);
    float xf = floorf(x), yf = floorf(y), zf = floorf(z);
    t.wx = x - xf; t.wy = y - yf; t.wz = z - zf;
    t.x0 = (int)xf; t.y0 = (int)yf; t.z0 = (int)zf;
}
#endif
