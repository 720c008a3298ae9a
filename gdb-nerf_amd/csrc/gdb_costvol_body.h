// The plane-sweep cost volume's device code, shared by gdb_costvol.hip (hypotheses read from a (B, D, Ht, Wt) tensor) and
// gdb_cascade.hip (hypotheses recomputed from the stage's search range): the camera set-up of one (batch, view) and the body of the
// sweep.  Both translation units are built with -ffp-contract=off; the arithmetic below is the reference's sequence of roundings.
#pragma once
#include "gdb_internal.h"

// pixel(target) -> pixel(source) map of every (batch, view): P_src * inverse([P_tar; 0 0 0 1])   :449-453
__device__ __forceinline__ void inv4_rowmajor_f64(const double* m, double* o) {
    double s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[6] - m[4] * m[2], s2 = m[0] * m[7] - m[4] * m[3];
    double s3 = m[1] * m[6] - m[5] * m[2], s4 = m[1] * m[7] - m[5] * m[3], s5 = m[2] * m[7] - m[6] * m[3];
    double c5 = m[10] * m[15] - m[14] * m[11], c4 = m[9] * m[15] - m[13] * m[11], c3 = m[9] * m[14] - m[13] * m[10];
    double c2 = m[8] * m[15] - m[12] * m[11], c1 = m[8] * m[14] - m[12] * m[10], c0 = m[8] * m[13] - m[12] * m[9];
    double inv = 1.0 / (s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0);
    o[0] = (m[5] * c5 - m[6] * c4 + m[7] * c3) * inv;   o[1] = (-m[1] * c5 + m[2] * c4 - m[3] * c3) * inv;
    o[2] = (m[13] * s5 - m[14] * s4 + m[15] * s3) * inv; o[3] = (-m[9] * s5 + m[10] * s4 - m[11] * s3) * inv;
    o[4] = (-m[4] * c5 + m[6] * c2 - m[7] * c1) * inv;  o[5] = (m[0] * c5 - m[2] * c2 + m[3] * c1) * inv;
    o[6] = (-m[12] * s5 + m[14] * s2 - m[15] * s1) * inv; o[7] = (m[8] * s5 - m[10] * s2 + m[11] * s1) * inv;
    o[8] = (m[4] * c4 - m[5] * c2 + m[7] * c0) * inv;   o[9] = (-m[0] * c4 + m[1] * c2 - m[3] * c0) * inv;
    o[10] = (m[12] * s4 - m[13] * s2 + m[15] * s0) * inv; o[11] = (-m[8] * s4 + m[9] * s2 - m[11] * s0) * inv;
    o[12] = (-m[4] * c3 + m[5] * c1 - m[6] * c0) * inv; o[13] = (m[0] * c3 - m[1] * c1 + m[2] * c0) * inv;
    o[14] = (-m[12] * s3 + m[13] * s1 - m[14] * s0) * inv; o[15] = (m[8] * s3 - m[9] * s1 + m[10] * s0) * inv;
}

// SCALED: the intrinsics are the unscaled ones and rows 0-1 are multiplied by the stage's scales in fp32 first, which is what
// DepthNet.forward's `K[..., :2, :] *= s` does before the products (gdb_cascade.hip); otherwise they are used as given.
template <bool SCALED>
__device__ __forceinline__ void costvol_proj_one(int t, int V, const float* __restrict__ src_exts, const float* __restrict__ src_ints,
                                                 const float* __restrict__ tar_exts, const float* __restrict__ tar_ints, float feat_scale,
                                                 float vol_scale, float* __restrict__ proj) {
    int b = t / V;
    double Pt[16], Pti[16], Ps[12];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = 0.f, q = 0.f;  // the reference multiplies fp32 tensors: round the 3x4 products to fp32 first
            for (int k = 0; k < 3; ++k) {
                float kt = tar_ints[b * 9 + i * 3 + k], ks = src_ints[(size_t)t * 9 + i * 3 + k];
                if (SCALED && i < 2) { kt = kt * vol_scale; ks = ks * feat_scale; }
                s += kt * tar_exts[b * 16 + k * 4 + j];
                q += ks * src_exts[(size_t)t * 16 + k * 4 + j];
            }
            Pt[i * 4 + j] = s; Ps[i * 4 + j] = q;
        }
    Pt[12] = 0; Pt[13] = 0; Pt[14] = 0; Pt[15] = 1;
    inv4_rowmajor_f64(Pt, Pti);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += Ps[i * 4 + k] * (double)(float)Pti[k * 4 + j];
            proj[(size_t)t * 12 + i * 4 + j] = (float)s;
        }
}

struct F2c { float x, y; } __attribute__((packed, aligned(4)));

struct CostVolArgs {
    int B, V, C, Hs, Ws, D, Ht, Wt, inv_depth, cpt, tiles, nblk;  // cpt: channels per thread
    const float* feat; const float* proj; const float* depth_values; float* out;
};

// HYP: where a voxel's hypothesis comes from, `float operator()(a, b, d, y, x, vox)`: HypTensor reads the materialised
// (B, D, Ht, Wt) tensor; gdb_cascade.hip's HypRange recomputes it from the stage's search range.
struct HypTensor {
    __device__ __forceinline__ float operator()(const CostVolArgs& a, int b, int d, int y, int x, size_t vox) const {
        return a.depth_values[(size_t)b * a.D * a.Ht * a.Wt + vox];
    }
};

// One view's warp of the voxel at pixel centre (px, py) and plane depth `depth`, stated ONCE for the sweep below and for its backward
// (gdb_costvol_backward.hip), which must reproduce the coordinates, the floor, the tap indices and the weights bit for bit:
//   q[r] = P[r][:3] . (px, py, 1),  p[r] = q[r] * depth + P[r][3]  (:466),  ix / iy the grid_sample pixel coordinates (:467-468),
//   the x pair (xs, xs + 1) with weights (e0, e1) and the rows (ya, yb) with weights (ra, rb); zeros padding = weight 0, the
//   indices are clamped into the map so every tap address exists.
struct CostVolView { float q[3], p[3]; int x0, y0, xs, ya, yb; float fx, fy, e0, e1, ra, rb; bool finite; };
__device__ __forceinline__ void costvol_view(const float* __restrict__ P, float px, float py, float depth, int Hs, int Ws, CostVolView& t) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        t.q[r] = P[4 * r] * px + P[4 * r + 1] * py + P[4 * r + 2];
        t.p[r] = t.q[r] * depth + P[4 * r + 3];  // :466
    }
    float z = fmaxf(t.p[2], 1e-6f);
    float gx = 2.f * (t.p[0] / z) / (float)Ws - 1.f, gy = 2.f * (t.p[1] / z) / (float)Hs - 1.f;   // :467-468
    float ix = ((gx + 1.f) * (float)Ws - 1.f) / 2.f, iy = ((gy + 1.f) * (float)Hs - 1.f) / 2.f;
    // keep far-away coordinates representable as int (they are outside anyway)
    ix = fminf(fmaxf(ix, -4.f), (float)Ws + 4.f); iy = fminf(fmaxf(iy, -4.f), (float)Hs + 4.f);
    t.finite = (t.p[0] == t.p[0]) && (t.p[1] == t.p[1]) && (t.p[2] == t.p[2]);
    float xf = floorf(ix), yf = floorf(iy);
    t.fx = ix - xf; t.fy = iy - yf;
    t.x0 = (int)xf; t.y0 = (int)yf;
    // x pair (xs, xs+1) covers columns x0, x0+1 where they exist
    t.xs = min(max(t.x0, 0), Ws - 2);
    float ea = (t.x0 >= 0 && t.x0 <= Ws - 1) ? 1.f - t.fx : 0.f, eb = (t.x0 + 1 >= 0 && t.x0 + 1 <= Ws - 1) ? t.fx : 0.f;
    t.e0 = (t.x0 == t.xs ? ea : 0.f) + (t.x0 + 1 == t.xs ? eb : 0.f);
    t.e1 = (t.x0 == t.xs + 1 ? ea : 0.f) + (t.x0 + 1 == t.xs + 1 ? eb : 0.f);
    t.ra = (t.y0 >= 0 && t.y0 <= Hs - 1) ? 1.f - t.fy : 0.f; t.rb = (t.y0 + 1 >= 0 && t.y0 + 1 <= Hs - 1) ? t.fy : 0.f;
    if (!t.finite) { t.e0 = t.e1 = 0.f; }
    t.ya = min(max(t.y0, 0), Hs - 1); t.yb = min(max(t.y0 + 1, 0), Hs - 1);
}

// PAIR: a.feat is the channel-pair-interleaved copy (k_costvol_pairs; C even): per (row, view) ONE 16-byte load serves two channels.
template <int VT, bool PAIR, class HYP>  // VT = number of source views: the per-view tap state lives in registers
__device__ __forceinline__ void costvol_body(const CostVolArgs& a, const HYP& hyp) {
    // 1-D grid over (batch, tile of 256 voxels of the flattened (y,x) plane, depth plane, channel group), depth
    // innermost, remapped so that each XCD (blocks b, b+8, ...) walks one contiguous band: the D planes of a tile
    // and the neighbouring tiles re-read the same source rows out of that XCD's L2.  (With depth as a grid
    // dimension the 16 MB of source maps were fetched from HBM ~16x: 383 MB FETCH_SIZE at the 256x320 stage.)
    const int groups = (a.C + a.cpt - 1) / a.cpt;
    const int chunk = (a.nblk + 7) >> 3;
    int lb = (blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    if (lb >= a.nblk) return;
    const int g = lb % groups; lb /= groups;
    const int d = lb % a.D; lb /= a.D;
    const int tile = lb % a.tiles, b = lb / a.tiles;
    const int c_begin = g * a.cpt, c_end = min(c_begin + a.cpt, a.C);
    const int t = tile * blockDim.x + threadIdx.x;  // the (y,x) plane flattened: no ragged-row waste
    if (t >= a.Ht * a.Wt) return;
    const int y = t / a.Wt, x = t - y * a.Wt;
    const size_t vox = ((size_t)d * a.Ht + y) * a.Wt + x;
    float depth = hyp(a, b, d, y, x, vox);
    if (a.inv_depth) depth = 1.f / depth;                                                     // :445-446
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    // per view: two clamped row offsets and the four tap weights of the x pair (zeros padding = weight 0)
    unsigned off0[VT], off1[VT];
    float w00[VT], w01[VT], w10[VT], w11[VT];
#pragma unroll
    for (int v = 0; v < VT; ++v) {
        CostVolView t;
        costvol_view(a.proj + ((size_t)b * a.V + v) * 12, px, py, depth, a.Hs, a.Ws, t);
        off0[v] = (unsigned)(t.ya * a.Ws + t.xs); off1[v] = (unsigned)(t.yb * a.Ws + t.xs);
        w00[v] = t.e0 * t.ra; w01[v] = t.e1 * t.ra; w10[v] = t.e0 * t.rb; w11[v] = t.e1 * t.rb;
    }
    const size_t plane = (size_t)a.Hs * a.Ws, ovol = (size_t)a.D * a.Ht * a.Wt;
    const float invV = 1.f / (float)a.V;
    if constexpr (PAIR) {
        // [c / 2][y][x][2]: the 16 bytes at (y, xs) are (c @ xs, c + 1 @ xs, c @ xs + 1, c + 1 @ xs + 1); same products, same order of
        // sums as the planar form below: bit-identical results
        struct F4c { float x, y, z, w; } __attribute__((packed, aligned(8)));
        for (int c = c_begin; c < c_end; c += 2) {
            float val[2][VT], mean[2] = {0.f, 0.f};
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const float* pl = a.feat + (((size_t)b * a.V + v) * a.C + c) * plane;   // start of the pair's interleaved plane (2 plane floats)
                const F4c t0 = *(const F4c*)(pl + 2 * (size_t)off0[v]), t1 = *(const F4c*)(pl + 2 * (size_t)off1[v]);
                val[0][v] = t0.x * w00[v] + t0.z * w01[v] + t1.x * w10[v] + t1.z * w11[v];
                val[1][v] = t0.y * w00[v] + t0.w * w01[v] + t1.y * w10[v] + t1.w * w11[v];
                mean[0] += val[0][v]; mean[1] += val[1][v];
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float m = mean[e] * invV;
                float var = 0.f;
#pragma unroll
                for (int v = 0; v < VT; ++v) { float d = val[e][v] - m; var += d * d; }
                a.out[((size_t)b * a.C + c + e) * ovol + vox] = var * invV;
            }
        }
        return;
    }
    for (int c = c_begin; c < c_end; ++c) {
        float val[VT], mean = 0.f;
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            {
                const float* pl = a.feat + (((size_t)b * a.V + v) * a.C + c) * plane;
#ifndef GDB_XP_CV_SCALAR   // one 8-byte load per x pair (any 4-byte alignment costs the same 16 TA cycles per wave instruction:
                           // tools/ubench/ta_rate.hip); two dword loads per pair measured slower: 115 vs 72 us at the 256x320 stage
                F2c t0 = *(const F2c*)(pl + off0[v]), t1 = *(const F2c*)(pl + off1[v]);
                val[v] = t0.x * w00[v] + t0.y * w01[v] + t1.x * w10[v] + t1.y * w11[v];      // :472
#else
                const float a0 = pl[off0[v]], a1 = pl[off0[v] + 1], b0 = pl[off1[v]], b1 = pl[off1[v] + 1];
                val[v] = a0 * w00[v] + a1 * w01[v] + b0 * w10[v] + b1 * w11[v];              // :472
#endif
                mean += val[v];
            }
        }
        mean *= invV;
        float var = 0.f;
#pragma unroll
        for (int v = 0; v < VT; ++v) { float e = val[v] - mean; var += e * e; }
        a.out[((size_t)b * a.C + c) * ovol + vox] = var * invV;                               // :474 (unbiased=False)
    }
}

