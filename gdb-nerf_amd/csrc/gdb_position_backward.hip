// Backward of BundleSampler.encode (gdb_encode) with respect to the sample POSITIONS - rays_xyz, the normalised depth uvd[:, 2] and
// ball_radii - and of BundleSampler.sample (gdb_sample) with respect to depth_range / vol_range.  Together with
// gdb_encode_backward (the gathered values, 4.15) this is every path the colour loss takes through the hot path to a trainable tensor.
//
// Conventions (what torch autograd of the restatement does):
//   * tap indices, fractions, the mip level and every clamp decision are the forward's own bits: no forward formula is restated here,
//     they come from the gdb_encode_geom.h helpers that k_encode_vox / k_encode_views call (vox_coords; subray_cam, cam_to_grid;
//     centre_tex with mip_level_parts, tex_taps; dir_code_fwd; img_taps states rgb_fetch's taps) under -ffp-contract=off; derivatives in double.
//   * d/dx of a bilinear fetch = (1 - f_y)(t01 - t00) + f_y (t11 - t10), times the coordinate scale (W_o / 2 for the sub-ray colours,
//     W_l per mip level, D / 2 for the volume's depth axis); a coordinate clamped by border / clamp-to-edge has derivative 0, equality
//     included (torch's grid_sample rule).
//   * the level clamped to [0, L] passes its derivative strictly inside and 0 outside (NaN: 0); d out / d level = tex(l1) - tex(l0)
//     where frac was used; both blended levels contribute to d / d(u, v) with their blend weights.
//   * clamp_min floors (1e-6 on the projected depths, 1e-12 under the square roots of mip_level): derivative 0 below the floor.
//   * u, v (columns 0, 1 of uvd) are not differentiated: they sit on voxel centres, where the trilinear derivative is one-sided, and
//     depend on no trainable tensor.  The columns are written as zeros.
//
// Kernels - gathers, no atomics, every sum in a fixed order (bit-identical from run to run):
//   k_posbwd_vol     lane = sample: the 8 volume taps x C_v channels -> g_uvd
//   k_posbwd_centre  lane = sample, views v = 0 .. V-1 in order: centre -> (u, v, level) -> the C_f + 3 feature columns (float4 rows of
//                    the chunk-planar pyramid, consecutive lanes on consecutive texels) and centre -> the four direction columns;
//                    writes g_ball_radii and the centre's share of g_rays_xyz (the same for every sub-ray: both means are 1 / b^2)
//   k_posbwd_colour  lane = (sample, sub-ray), views in order: sub-ray point -> camera -> image -> the 4 colour taps; adds to the
//                    centre's share
//   k_smpbwd         lane = bundle: its <= S_max samples in sample order -> the four range scalars (a segmented sum with a fixed
//                    order; the sample offsets come from gdb_sample's own exclusive scan of the counts, gdb_scan_launch)
#include "gdb_encode_geom.h"

#define PB_THREADS 128

// the unclamped coordinate of gs_coord (same expression, same bits): strictly inside (0, size - 1) the clamp passes the derivative
__device__ __forceinline__ bool gs_inside(float g, int size) {
    float x = ((g + 1.f) * (float)size - 1.f) / 2.f;
    return x > 0.f && x < (float)(size - 1);
}
// ... and of tex_coord
__device__ __forceinline__ bool tex_inside(float u, int size) {
    float x = u * (float)size - 0.5f;
    return x > 0.f && x < (float)(size - 1);
}
// backward of F.normalize (eps 1e-12) at a: y = a / max(|a|, eps); g <- gradient with respect to a
__device__ __forceinline__ void normalize3_bwd(const float a[3], const double gy[3], double g[3]) {
    const float nf = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double n = (double)fmaxf(nf, 1e-12f);
    const double dot = gy[0] * (double)a[0] + gy[1] * (double)a[1] + gy[2] * (double)a[2];
    const double k = (nf >= 1e-12f && nf > 0.f) ? dot / (n * n * (double)nf) : 0.0;   // the norm's own path: 0 below the floor
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = gy[c] / n - k * (double)a[c];
}

// ---- volume: d vox / d (normalised depth) ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PB_THREADS)
k_posbwd_vol(DevFrame f, const float* __restrict__ uvd, const int64_t* __restrict__ per_batch, const int64_t* __restrict__ total,
             int64_t n_alloc, const float* __restrict__ g_vox, float* __restrict__ g_uvd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_alloc) return;
    float gd = 0.f;
    if (i < total_clamped(total, n_alloc)) {
        const int bi = batch_of(f.B, per_batch, i);
        VoxCoords t3;
        vox_coords(f, uvd, i, t3);
        const int z0 = t3.z0, z1 = min(z0 + 1, f.D - 1);
        const bool inz = z0 + 1 <= f.D - 1;
        double w[4]; size_t o0[4], o1[4];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int xx = t3.x0 + dx, yy = t3.y0 + dy, t = dy * 2 + dx;
                const bool in = xx <= f.W - 1 && yy <= f.H - 1;   // the forward's out-of-range tap: weight 0
                w[t] = in ? (double)(dx ? t3.wx : 1.f - t3.wx) * (double)(dy ? t3.wy : 1.f - t3.wy) : 0.0;
                const size_t yx = (size_t)min(yy, f.H - 1) * f.W + min(xx, f.W - 1);
                o0[t] = (size_t)z0 * f.H * f.W + yx; o1[t] = (size_t)z1 * f.H * f.W + yx;
            }
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < GDB_CV; ++c) {
            const float* vol = f.feat_volume + ((size_t)bi * GDB_CV + c) * f.D * f.H * f.W;
            double a = 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) a += w[t] * ((inz ? (double)vol[o1[t]] : 0.0) - (double)vol[o0[t]]);
            s += (double)g_vox[i * GDB_CV + c] * a;
        }
        gd = gs_inside(uvd[i * 3 + 2], f.D) ? (float)(s * (0.5 * (double)f.D)) : 0.f;
    }
    g_uvd[i * 3 + 0] = 0.f; g_uvd[i * 3 + 1] = 0.f; g_uvd[i * 3 + 2] = gd;
}

// ---- centre paths -------------------------------------------------------------------------------------------------------------
// One mip level: val = sum_c g_c tex_c, dx / dy = its derivative with respect to the texture coordinate (u, v) of this level.
// The four taps are contracted with the upstream first (S_t = sum_c g_c t_c, in double), then combined with the forward's fractions.
__device__ __forceinline__ void pb_tex_level(const DevFrame& f, const float* __restrict__ pyr, int l, float u, float v,
                                             const float g[GDB_CP], double& val, double& du, double& dv) {
    TexTaps t;
    tex_taps(f, l, u, v, t);
    const int W = t.W, H = t.H, x0 = t.x0, x1 = t.x1, y0 = t.y0, y1 = t.y1; const float fx = t.fx, fy = t.fy;
    const float4* base = (const float4*)(pyr + t.off);   // chunk-planar: [chunk][y][x]
    double s00 = 0.0, s01 = 0.0, s10 = 0.0, s11 = 0.0;
#pragma unroll
    for (int c = 0; c < GDB_CP / 4; ++c) {
        const float4* pl = base + (size_t)c * H * W;
        const float4 a = pl[(size_t)y0 * W + x0], b = pl[(size_t)y0 * W + x1], d = pl[(size_t)y1 * W + x0], e = pl[(size_t)y1 * W + x1];
        const double g0 = g[4 * c], g1 = g[4 * c + 1], g2 = g[4 * c + 2];
        s00 += g0 * (double)a.x + g1 * (double)a.y + g2 * (double)a.z;
        s01 += g0 * (double)b.x + g1 * (double)b.y + g2 * (double)b.z;
        s10 += g0 * (double)d.x + g1 * (double)d.y + g2 * (double)d.z;
        s11 += g0 * (double)e.x + g1 * (double)e.y + g2 * (double)e.z;
        if (4 * c + 3 < GDB_CFR) {   // (channel 19 is the pad)
            const double g3 = g[4 * c + 3];
            s00 += g3 * (double)a.w; s01 += g3 * (double)b.w; s10 += g3 * (double)d.w; s11 += g3 * (double)e.w;
        }
    }
    const double dfx = fx, dfy = fy;
    val = (1.0 - dfy) * ((1.0 - dfx) * s00 + dfx * s01) + dfy * ((1.0 - dfx) * s10 + dfx * s11);
    du = tex_inside(u, W) ? ((1.0 - dfy) * (s01 - s00) + dfy * (s11 - s10)) * (double)W : 0.0;
    dv = tex_inside(v, H) ? ((1.0 - dfx) * (s10 - s00) + dfx * (s11 - s01)) * (double)H : 0.0;
}

template <int BB>
__global__ void __launch_bounds__(PB_THREADS)
k_posbwd_centre(DevFrame f, const float* __restrict__ rays_xyz, const float* __restrict__ ball_radii,
                const int64_t* __restrict__ per_batch, const int64_t* __restrict__ total, int64_t n_alloc,
                const float* __restrict__ g_rfd, float* __restrict__ g_rays, float* __restrict__ g_ball) {
    constexpr int P = 3 * BB + GDB_CFR + 4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_alloc) return;
    double gw[3] = {0.0, 0.0, 0.0};   // gradient with respect to every sub-ray point, summed over the centre paths and the views
    double gb = 0.0;
    if (i < total_clamped(total, n_alloc)) {
        const int bi = batch_of(f.B, per_batch, i);
        const float* tc = tar_cam(f, bi);
        const float ball = ball_radii[i];
        for (int v = 0; v < f.V; ++v) {
            const float* sc = src_cam(f, bi, v);
            float cw[3] = {0.f, 0.f, 0.f}, cc[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < BB; ++s) {
                float p[3], cam[3];
                subray_point<BB>(rays_xyz, i, s, p);
                subray_cam(sc, p, cam);
#pragma unroll
                for (int c = 0; c < 3; ++c) { cw[c] += p[c]; cc[c] += cam[c]; }
            }
            subray_mean<BB>(cw);
            subray_mean<BB>(cc);
            CentreTex ct;
            centre_tex(f, sc, cc, ball, ct);
            const float *ci = ct.ci, zc = ct.zc, frac = ct.frac;

            const float* gr = g_rfd + ((size_t)v * n_alloc + i) * P + 3 * BB;
            float g[GDB_CP];
#pragma unroll
            for (int c = 0; c < GDB_CFR; ++c) g[c] = gr[c];
            g[GDB_CFR] = 0.f;
            const float* pyr = f.pyr + ((size_t)bi * f.V + v) * f.pyrStride;
            double val0, du0, dv0, val1 = 0.0, du1 = 0.0, dv1 = 0.0;
            pb_tex_level(f, pyr, ct.l0, ct.tu, ct.tv, g, val0, du0, dv0);
            const bool blend = frac > 0.f;   // the forward skips level l1 when frac == 0; frac > 0 is also "level strictly inside (0, L)"
            if (blend) pb_tex_level(f, pyr, ct.l1, ct.tu, ct.tv, g, val1, du1, dv1);
            const double dfr = frac;
            const double g_tu = (1.0 - dfr) * du0 + dfr * du1, g_tv = (1.0 - dfr) * dv0 + dfr * dv1;
            const double g_level = blend ? val1 - val0 : 0.0;

            double gcc[3];   // gradient with respect to the centre in the source camera's frame
            // (u, v) <- ci / zc / (W, H), zc = max(ci_z, 1e-6)
            {
                const double dz = zc;
                const double gci0 = g_tu / (dz * (double)f.W), gci1 = g_tv / (dz * (double)f.H);
                const double gzc = -(g_tu * (double)ci[0] / (double)f.W + g_tv * (double)ci[1] / (double)f.H) / (dz * dz);
                const double gci2 = ci[2] >= 1e-6f ? gzc : 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) gcc[c] = (double)sc[S_KS + c] * gci0 + (double)sc[S_KS + 3 + c] * gci1 + (double)sc[S_KS + 6 + c] * gci2;
            }
            // level <- mip_level(cc, ball, pixr), through the forward's own intermediates (mip_level_parts)
            {
                const float dist = ct.mip.dist, q = ct.mip.q, sec2 = ct.mip.sec2, r = ct.mip.r, A = ct.mip.A, Cc = ct.mip.C, a = ct.mip.a, c = ct.mip.c;
                const double apc = (double)(a + c);
                const double m = (double)(sec2 / (a + c));
                const double g_m = g_level / (m * 0.69314718055994530942);
                double g_sec2 = g_m / apc;
                const double g_apc = -g_m * (double)sec2 / (apc * apc);
                const double g_A = A >= 1e-12f ? g_apc / (2.0 * (double)a) : 0.0;
                const double g_C = Cc >= 1e-12f ? g_apc / (2.0 * (double)c) : 0.0;
                g_sec2 += g_C;
                const double g_r = g_A * 2.0 * (double)r;
                const double g_q = g_sec2 * 2.0 * (double)q;
                const double g_dist = g_q / (double)cc[2] + g_r / (double)ball;
                gcc[2] += -g_q * (double)dist / ((double)cc[2] * (double)cc[2]);
                gb += -g_r * (double)dist / ((double)ball * (double)ball);
                if (dist > 0.f) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) gcc[k] += g_dist * (double)cc[k] / (double)dist;
                }
            }
            // centre in the camera's frame <- mean_s (E p_s): E^T, the 1 / b^2 of the mean is applied once at the end
#pragma unroll
            for (int c = 0; c < 3; ++c) gw[c] += (double)sc[S_E + c] * gcc[0] + (double)sc[S_E + 4 + c] * gcc[1] + (double)sc[S_E + 8 + c] * gcc[2];

            // direction code: dn = normalize(td - sd), dot = td . sd, td = normalize(cw - o), sd = normalize(cw - C_v)
            {
                float at[3], as[3], td[3], sd[3], dif[3];
                dir_code_fwd(cw, tc, sc, at, as, td, sd, dif);
                const double gdn[3] = {(double)gr[GDB_CFR], (double)gr[GDB_CFR + 1], (double)gr[GDB_CFR + 2]};
                const double gdot = gr[GDB_CFR + 3];
                double gdif[3], gtd[3], gsd[3], ga[3], gs[3];
                normalize3_bwd(dif, gdn, gdif);
#pragma unroll
                for (int c = 0; c < 3; ++c) { gtd[c] = gdif[c] + gdot * (double)sd[c]; gsd[c] = gdot * (double)td[c] - gdif[c]; }
                normalize3_bwd(at, gtd, ga);
                normalize3_bwd(as, gsd, gs);
#pragma unroll
                for (int c = 0; c < 3; ++c) gw[c] += ga[c] + gs[c];
            }
        }
    }
    if (g_ball) g_ball[i] = (float)gb;
    if (g_rays) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gv = (float)(gw[c] / (double)BB);
#pragma unroll
            for (int s = 0; s < BB; ++s) g_rays[((size_t)i * 3 + c) * BB + s] = gv;
        }
    }
}

// ---- sub-ray colours ------------------------------------------------------------------------------------------------------------
template <int BB>
__global__ void __launch_bounds__(PB_THREADS)
k_posbwd_colour(DevFrame f, const float* __restrict__ rays_xyz, const int64_t* __restrict__ per_batch,
                const int64_t* __restrict__ total, int64_t n_alloc, const float* __restrict__ g_rfd, float* __restrict__ g_rays) {
    constexpr int P = 3 * BB + GDB_CFR + 4;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = t / BB;
    const int s = (int)(t - i * BB);
    if (i >= total_clamped(total, n_alloc)) return;   // (the tail rows were zeroed by k_posbwd_centre)
    const int bi = batch_of(f.B, per_batch, i);
    float p[3];
    subray_point<BB>(rays_xyz, i, s, p);
    const size_t plane = (size_t)f.Ho * f.Wo;
    double gp[3] = {0.0, 0.0, 0.0};
    for (int v = 0; v < f.V; ++v) {
        const float* sc = src_cam(f, bi, v);
        const float* img = f.src_images + ((size_t)bi * f.V + v) * 3 * plane;
        // k_encode_views' projection of one sub-ray point and its colour taps
        float cam[3], im[3], zc, gx, gy;
        subray_cam(sc, p, cam);
        cam_to_grid(sc, cam, f.Wo, f.Ho, im, zc, gx, gy);
        ImgTaps it;
        img_taps(gx, gy, f.Ho, f.Wo, it);
        const float* gr = g_rfd + ((size_t)v * n_alloc + i) * P + s;
        double s00 = 0.0, s01 = 0.0, s10 = 0.0, s11 = 0.0;   // sum_c g_c tap_c; an out-of-range tap is worth 0
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pc = img + c * plane;
            const double g = gr[c * BB];
            s00 += g * (double)pc[(size_t)it.y0 * f.Wo + it.x0];
            s01 += g * (double)pc[(size_t)it.y0 * f.Wo + it.x1];
            s10 += g * (double)pc[(size_t)it.y1 * f.Wo + it.x0];
            s11 += g * (double)pc[(size_t)it.y1 * f.Wo + it.x1];
        }
        if (!it.inx) { s01 = 0.0; s11 = 0.0; }
        if (!it.iny) { s10 = 0.0; s11 = 0.0; }
        const double dwx = it.wx, dwy = it.wy;
        // pixel coordinate <- grid coordinate: (W_o / 2) (2 / W_o) = 1
        const double g_px = gs_inside(gx, f.Wo) ? (1.0 - dwy) * (s01 - s00) + dwy * (s11 - s10) : 0.0;
        const double g_py = gs_inside(gy, f.Ho) ? (1.0 - dwx) * (s10 - s00) + dwx * (s11 - s01) : 0.0;
        const double dz = zc;
        const double gim0 = g_px / dz, gim1 = g_py / dz;
        const double gzc = -(g_px * (double)im[0] + g_py * (double)im[1]) / (dz * dz);
        const double gim2 = im[2] >= 1e-6f ? gzc : 0.0;
        double gcam[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) gcam[c] = (double)sc[S_K + c] * gim0 + (double)sc[S_K + 3 + c] * gim1 + (double)sc[S_K + 6 + c] * gim2;
#pragma unroll
        for (int c = 0; c < 3; ++c) gp[c] += (double)sc[S_E + c] * gcam[0] + (double)sc[S_E + 4 + c] * gcam[1] + (double)sc[S_E + 8 + c] * gcam[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* o = g_rays + ((size_t)i * 3 + c) * BB + s;
        *o = (float)((double)*o + gp[c]);
    }
}

// ---- sample -----------------------------------------------------------------------------------------------------------------------
template <int BB>
__global__ void __launch_bounds__(PB_THREADS)
k_smpbwd(DevFrame f, const int32_t* __restrict__ spb, const int32_t* __restrict__ offs, const int32_t* __restrict__ bsum,
         const int64_t* __restrict__ total, int64_t n_alloc, const float* __restrict__ g_rays, const float* __restrict__ g_uvd,
         const float* __restrict__ g_z, const float* __restrict__ g_ball, float* __restrict__ g_dr, float* __restrict__ g_vr) {
    const size_t nb = (size_t)f.B * f.H * f.W;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nb) return;
    const int w = (int)(t % f.W); const size_t r = t / f.W; const int h = (int)(r % f.H); const int bi = (int)(r / f.H);
    float raw[4];
    load_ranges(f, bi, h, w, raw);
    Bundle<BB> q;
    load_bundle<BB, false, false>(f, tar_cam(f, bi), bi, h, w, q, raw);
    const int cnt = min(max(spb[t], 0), f.S_max);   // the counts are data: ceil / clamp have derivative 0
    q.count = cnt;
    const int64_t off = (int64_t)offs[t] + bsum[t / SCAN_BLOCK];
    const int64_t n = total_clamped(total, n_alloc);
    double md[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < BB; ++s)
#pragma unroll
        for (int c = 0; c < 3; ++c) md[c] += (double)q.d[s][c];
#pragma unroll
    for (int c = 0; c < 3; ++c) md[c] /= (double)BB;
    // the continuous chain in double from the float ranges (the counts, the only decisions of the forward, are given)
    double rg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) rg[j] = f.inv_depth ? 1.0 / (double)raw[j] : (double)raw[j];
    const double span = rg[3] - rg[2];
    const double mdn = sqrt(md[0] * md[0] + md[1] * md[1] + md[2] * md[2]);
    double G[4] = {0.0, 0.0, 0.0, 0.0};   // near, far, vol_near, vol_far in sampling space
    for (int k = 0; k < cnt; ++k) {
        const int64_t i = off + k;
        if (i < 0 || i >= n) break;
        const double wk = ((double)k + 0.5) / (double)cnt;
        const double tm = rg[0] + (rg[1] - rg[0]) * wk;   // t_k = n + (f - n)(k + 1/2) / c, the sample's depth in sampling space
        const double z = f.inv_depth ? 1.0 / tm : tm;
        // z_vals, rays_xyz = o + dir z, ball = unit |mean dir| |z|
        double gz = g_z ? (double)g_z[i] : 0.0;
        if (g_rays) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int s = 0; s < BB; ++s) gz += (double)g_rays[((size_t)i * 3 + c) * BB + s] * (double)q.d[s][c];
        }
        if (g_ball && z != 0.0) gz += (double)g_ball[i] * (double)q.unit * mdn * (z > 0.0 ? 1.0 : -1.0);
        double gt = f.inv_depth ? -gz / (tm * tm) : gz;   // z = 1 / t under inv_depth
        // d = 2 (t - v_n) / (v_f - v_n) - 1
        if (g_uvd) {
            const double gd = g_uvd[i * 3 + 2];
            const double num = tm - rg[2];
            gt += gd * 2.0 / span;
            G[2] += gd * (2.0 * num / (span * span) - 2.0 / span);
            G[3] += -gd * 2.0 * num / (span * span);
        }
        G[0] += gt * (1.0 - wk);
        G[1] += gt * wk;
    }
    if (f.inv_depth) {   // the four ranges are inverted first: x -> 1 / x
#pragma unroll
        for (int j = 0; j < 4; ++j) G[j] = -G[j] / ((double)raw[j] * (double)raw[j]);
    }
    const size_t hw = (size_t)f.H * f.W, p = (size_t)h * f.W + w;
    if (g_dr) { g_dr[((size_t)bi * 2) * hw + p] = (float)G[0]; g_dr[((size_t)bi * 2 + 1) * hw + p] = (float)G[1]; }
    if (g_vr) { g_vr[((size_t)bi * 2) * hw + p] = (float)G[2]; g_vr[((size_t)bi * 2 + 1) * hw + p] = (float)G[3]; }
}

// ---- entries -----------------------------------------------------------------------------------------------------------------------
extern "C" int gdb_encode_position_backward(const GdbConfig* cfg, const GdbFrame* f, const void* ws, const float* rays_xyz,
                                            const float* uvd, const float* ball, const int64_t* per_batch, const int64_t* total,
                                            int64_t n_alloc, const float* g_rfd, const float* g_vox, float* g_rays_xyz, float* g_uvd,
                                            float* g_ball, void* stream_) {
    int rc = gdb_check_cfg(cfg); if (rc) return rc;
    rc = gdb_check_frame(cfg, f, true); if (rc) return rc;
    if (!ws || !rays_xyz || !uvd || !ball || !per_batch || !total || !g_rfd || !g_vox) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (!g_rays_xyz && !g_uvd && !g_ball) return gdb_fail(GDB_E_BADARG, "all three outputs are NULL");
    rc = gdb_check_n_alloc(cfg, f, n_alloc); if (rc) return rc;
    WsLayout L = ws_layout(*cfg, *f);
    DevFrame d = dev_frame(*cfg, *f, L, ws);
    hipStream_t st = (hipStream_t)stream_;
    const unsigned gn = (unsigned)((n_alloc + PB_THREADS - 1) / PB_THREADS);
    if (g_uvd) {
        hipLaunchKernelGGL(k_posbwd_vol, dim3(gn), dim3(PB_THREADS), 0, st, d, uvd, per_batch, total, n_alloc, g_vox, g_uvd);
        LAUNCH_CHECK("k_posbwd_vol");
    }
    if (g_rays_xyz || g_ball) {
        bb_dispatch(cfg->bundle_size, [&](auto bb) {
            hipLaunchKernelGGL(k_posbwd_centre<decltype(bb)::value>, dim3(gn), dim3(PB_THREADS), 0, st, d, rays_xyz, ball, per_batch, total, n_alloc, g_rfd,
                               g_rays_xyz, g_ball);
        });
        LAUNCH_CHECK("k_posbwd_centre");
    }
    if (g_rays_xyz) {
        const int bb = cfg->bundle_size * cfg->bundle_size;
        const unsigned gc = (unsigned)((n_alloc * bb + PB_THREADS - 1) / PB_THREADS);
        bb_dispatch(cfg->bundle_size, [&](auto bb) {
            hipLaunchKernelGGL(k_posbwd_colour<decltype(bb)::value>, dim3(gc), dim3(PB_THREADS), 0, st, d, rays_xyz, per_batch, total, n_alloc, g_rfd, g_rays_xyz);
        });
        LAUNCH_CHECK("k_posbwd_colour");
    }
    return GDB_OK;
}

extern "C" int gdb_sample_backward(const GdbConfig* cfg, const GdbFrame* f, const void* ws, const int32_t* spb, const int64_t* total,
                                   int64_t n_alloc, const float* g_rays_xyz, const float* g_uvd, const float* g_z_vals,
                                   const float* g_ball, float* g_depth_range, float* g_vol_range, void* scratch, void* stream_) {
    int rc = gdb_check_cfg(cfg); if (rc) return rc;
    rc = gdb_check_frame(cfg, f, false); if (rc) return rc;
    if (!f->d_depth_range || !f->d_vol_range) return gdb_fail(GDB_E_BADARG, "frame has a NULL depth_range / vol_range pointer");
    if (!ws || !spb || !total || !scratch) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (!g_rays_xyz && !g_uvd && !g_z_vals && !g_ball) return gdb_fail(GDB_E_BADARG, "all four upstream gradients are NULL");
    if (!g_depth_range && !g_vol_range) return gdb_fail(GDB_E_BADARG, "both outputs are NULL");
    rc = gdb_check_n_alloc(cfg, f, n_alloc); if (rc) return rc;
    WsLayout L = ws_layout(*cfg, *f);
    DevFrame d = dev_frame(*cfg, *f, L, ws);
    hipStream_t st = (hipStream_t)stream_;
    const size_t nb = (size_t)f->B * f->H * f->W;
    int32_t* offs = (int32_t*)scratch;   // [nb] offsets inside a scan block, then [nBlocksScan] block offsets
    int32_t* bsum = offs + nb;
    // gdb_sample's scan, without the grand total: the scratch has exactly nBlocksScan block slots
    rc = gdb_scan_launch(nb, L.nBlocksScan, spb, offs, bsum, false, st); if (rc) return rc;
    const unsigned g = (unsigned)((nb + PB_THREADS - 1) / PB_THREADS);
    bb_dispatch(cfg->bundle_size, [&](auto bb) {
        hipLaunchKernelGGL(k_smpbwd<decltype(bb)::value>, dim3(g), dim3(PB_THREADS), 0, st, d, spb, offs, bsum, total, n_alloc, g_rays_xyz, g_uvd,
                           g_z_vals, g_ball, g_depth_range, g_vol_range);
    });
    LAUNCH_CHECK("k_smpbwd");
    return GDB_OK;
}
