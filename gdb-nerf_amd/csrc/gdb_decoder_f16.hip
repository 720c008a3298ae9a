// The residual-dense decoder (gdb_decoder.hip has the network and its fp32 / split-f16 forms) on plain f16 MFMA with half-precision
// activations: the opt-in form behind `nerf.decoder_precision: f16` (gdb_decode_f16).  bundle_size 2, 1 .. 16 dense blocks.
//
// Numerical contract (tests/test_decoder_f16.py referees every line of it):
// * weights are f16(w); the up stage is folded with out_conv in fp64 as in gdb_pack_decoder_weights and rounded once to f16; biases fp32;
// * the input is the 27 channels read in place from the fp32 bundle rows, rounded to f16 (nearest even) when staged;
// * every convolution: f16 operands, fp32 accumulate (v_mfma_f32_16x16x32_f16), bias + ReLU in fp32, ONE rounding to f16, stored
//   channel-last (64 B per pixel for the 32-channel layers, 128 B for the 64-channel ones);
// * torch.cat([x, x1, x2]) = "channels from three buffers": no copies;
// * squeeze-excitation sums come from conv3's unrounded fp32 accumulators (per (row, 32-pixel segment), the layout k_se_gate reads);
//   the reduction, the two linears and the sigmoid are gdb_decoder.hip's k_se_gate, fp32, fixed order;
// * trunk update x <- f16(fmaf(c, gate, x)) from the stored f16 x and c, fused into the next convolution's staging and materialised;
// * global residual u = f16(shallow + trunk) in fp32, rounded once, materialised;
// * the folded 64 -> 12 convolution writes fp32 rgb_c (B, 3, 2H, 2W) pixel-shuffled, no f16 rounding.
//
// Kernel: one template, k_conv_h.  A workgroup = 4 waves = 4 image rows x 32 pixels.  Per 64-channel chunk of the input (one source
// buffer: the trunk, or [x1 | x2]) it stages rows + halo in LDS as f16, channel-last, pixel stride 160 B: the B operand of the MFMA is 8
// consecutive channels of one pixel = ONE ds_read_b128 per lane, and with a stride of 10 sixteen-byte slots the 16 lanes of every
// ds_read_b128 lane group fall on 16 distinct slots of the 256-byte bank row (pixels p and p + 8 never share a group with the same k
// quarter).  A chunk is staged once and then read by 9 taps x 2 K-steps of 32 channels with no barrier in between: 2 barriers per 64
// channels instead of the split-f16 kernel's 2 per 16.  The A operand (16 output channels x 32 input channels of one tap, packed on the
// host in lane order) streams from L2 as one 16-byte load per lane and MFMA group, a tap ahead of its use; a wave owns one 16-channel
// output tile and 2 NCT 16-pixel groups (NCT = the layer's tile count), so a weight fragment feeds 8 / 4 / 2 MFMAs.
// The accumulation order of an output element is (chunk, tap, K-step): it does not depend on the grid or the tile.
#include "gdb_internal.h"
#include <cstdio>
#include <cstring>
#include <vector>

// gdb_decoder.hip: k_se_gate on the per-segment channel sums (its own launch geometry)
int gdb_dec_se_groups(int nseg);
hipError_t gdb_dec_se_gate_launch(const float* part, int B, int nseg, float inv_hw, const float* w1, const float* w2, float* part2,
                                  unsigned* count, float* gate, hipStream_t st);

typedef float F4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

#define H16_NF 64          // num_feats
#define H16_G 32           // growth rate
#define H16_TR 4           // image rows per workgroup
#define H16_PX 34          // staged pixels per row: 32 + halo
#define H16_PSTR 160       // bytes per staged pixel: 64 halves + 32 (bank spread, see above)
#define H16_MAX_LAYERS 16
#define H16_SE_R 4

// ---- packed weights ---------------------------------------------------------------------------------------------------
// A convolution of nct 16-channel output tiles and nks 32-channel K-steps: [tile][K-step][tap 9][lane 64][8 halves]; element j of lane l
// = f16(W[16 tile + (l & 15)][32 kstep + 8 (l >> 4) + j][tap]) - the A fragment of v_mfma_f32_16x16x32_f16 - zero beyond the layer's
// channels.  Sections (bytes, each a multiple of 256): in_conv (4 tiles, 1 step), in_conv.bias (64 floats), per block conv1 (2, 2),
// conv2 (2, 3), conv3 (4, 4), se.fc.0 (4 x 64 floats), se.fc.2 (64 x 4 floats), then the folded up stage (1, 2) and its bias (64 floats,
// 12 used).
static size_t h_conv_bytes(int nct, int nks) { return (size_t)nct * nks * 9 * 64 * 16; }
struct H16Layout { size_t in_w, in_b, blk[H16_MAX_LAYERS][5], up_w, up_b, total; };
static H16Layout h_layout(int nlayers) {
    H16Layout L{};
    size_t o = 0;
    L.in_w = o; o += h_conv_bytes(4, 1);
    L.in_b = o; o += 256;
    for (int b = 0; b < nlayers; ++b) {
        L.blk[b][0] = o; o += h_conv_bytes(2, 2);
        L.blk[b][1] = o; o += h_conv_bytes(2, 3);
        L.blk[b][2] = o; o += h_conv_bytes(4, 4);
        L.blk[b][3] = o; o += sizeof(float) * H16_SE_R * H16_NF;
        L.blk[b][4] = o; o += sizeof(float) * H16_NF * H16_SE_R;
    }
    L.up_w = o; o += h_conv_bytes(1, 2);
    L.up_b = o; o += 256;
    L.total = o;
    return L;
}
template <typename T>
static void h_pack_conv(const T* w, int cout, int cin, int nct, int nks, _Float16* o) {
    for (int t = 0; t < nct; ++t)
        for (int ks = 0; ks < nks; ++ks)
            for (int tap = 0; tap < 9; ++tap)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const int co = 16 * t + (l & 15), ci = 32 * ks + 8 * (l >> 4) + j;
                        const T v = (co < cout && ci < cin) ? w[((size_t)co * cin + ci) * 9 + tap] : (T)0;
                        o[((((size_t)t * nks + ks) * 9 + tap) * 64 + l) * 8 + j] = (_Float16)v;   // one rounding, to nearest even
                    }
}

static int h_check(const GdbConfig* cfg, int nlayers) {
    int rc = gdb_check_cfg(cfg); if (rc) return rc;
    if (cfg->bundle_size != 2) return gdb_fail(GDB_E_BADARG, "the f16 decoder is built for bundle_size 2; got %d", cfg->bundle_size);
    if (cfg->feat_dim != GDB_CF || cfg->voxel_dim != GDB_CV)
        return gdb_fail(GDB_E_BADARG, "the f16 decoder is built for feat_dim %d and voxel_dim %d; got %d and %d", GDB_CF, GDB_CV, cfg->feat_dim, cfg->voxel_dim);
    if (nlayers < 1 || nlayers > H16_MAX_LAYERS) return gdb_fail(GDB_E_BADARG, "decoder layers %d outside 1..%d", nlayers, H16_MAX_LAYERS);
    return GDB_OK;
}

extern "C" int gdb_decoder_f16_packed_bytes(const GdbConfig* cfg, int32_t num_layers, size_t* out_bytes) {
    int rc = h_check(cfg, num_layers); if (rc) return rc;
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "out_bytes is NULL");
    *out_bytes = h_layout(num_layers).total;
    return GDB_OK;
}

// h_tensors: as gdb_pack_decoder_weights at bundle_size 2 (2 + 5 num_layers + 4 host pointers, state-dict order).
extern "C" int gdb_pack_decoder_weights_f16(const GdbConfig* cfg, int32_t num_layers, const float* const* t, void* out_) {
    int rc = h_check(cfg, num_layers); if (rc) return rc;
    if (!t || !out_) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    const int n = 2 + 5 * num_layers + 4;
    for (int i = 0; i < n; ++i)
        if (!t[i]) return gdb_fail(GDB_E_BADARG, "decoder tensor %d is NULL", i);
    const H16Layout L = h_layout(num_layers);
    char* out = (char*)out_;
    memset(out, 0, L.total);
    h_pack_conv(t[0], H16_NF, GDB_CFR + GDB_CV, 4, 1, (_Float16*)(out + L.in_w));
    memcpy(out + L.in_b, t[1], sizeof(float) * H16_NF);
    for (int b = 0; b < num_layers; ++b) {
        const float* const* q = t + 2 + 5 * b;
        h_pack_conv(q[0], H16_G, H16_NF, 2, 2, (_Float16*)(out + L.blk[b][0]));
        h_pack_conv(q[1], H16_G, H16_NF + H16_G, 2, 3, (_Float16*)(out + L.blk[b][1]));
        h_pack_conv(q[2], H16_NF, H16_NF + 2 * H16_G, 4, 4, (_Float16*)(out + L.blk[b][2]));
        memcpy(out + L.blk[b][3], q[3], sizeof(float) * H16_SE_R * H16_NF);
        memcpy(out + L.blk[b][4], q[4], sizeof(float) * H16_NF * H16_SE_R);
    }
    // out_conv o PixelShuffle(2) o up as ONE 64 -> 12 convolution, channel c = 3 s + o of sub-pixel s = dy * 2 + dx: summed in fp64 as
    // gdb_pack_decoder_weights does and rounded ONCE, from the fp64 sum to f16 (the bias to fp32)
    const float* wup = t[n - 4]; const float* bup = t[n - 3]; const float* wout = t[n - 2]; const float* bout = t[n - 1];
    std::vector<double> wf((size_t)12 * H16_NF * 9);
    float* bf = (float*)(out + L.up_b);
    for (int s = 0; s < 4; ++s)
        for (int o = 0; o < 3; ++o) {
            for (int ci = 0; ci < H16_NF; ++ci)
                for (int tap = 0; tap < 9; ++tap) {
                    double acc = 0;
                    for (int k = 0; k < H16_NF; ++k) acc += (double)wout[o * H16_NF + k] * (double)wup[((size_t)(4 * k + s) * H16_NF + ci) * 9 + tap];
                    wf[((size_t)(3 * s + o) * H16_NF + ci) * 9 + tap] = acc;
                }
            double acc = bout[o];
            for (int k = 0; k < H16_NF; ++k) acc += (double)wout[o * H16_NF + k] * (double)bup[4 * k + s];
            bf[3 * s + o] = (float)acc;
        }
    h_pack_conv(wf.data(), 12, H16_NF, 1, 2, (_Float16*)(out + L.up_w));
    return GDB_OK;
}

// ---- workspace ----------------------------------------------------------------------------------------------------------
// trunk[b] = the input x of dense block b (trunk[0] = in_conv's output = the global residual's `shallow`; trunk[L] = the blocks' output),
// a1 / a2 = conv1 / conv2 of the block in flight (32 channels each), c = conv3, u = f16(shallow + trunk[L]), the up stage's input.
// Without GDB_DECF16_KEEP_LAYERS trunk[b >= 1] alternates between two buffers and a1, a2, c and the gate are shared by the blocks; with it
// every one of them has a region of its own.  part / part2 / count: k_se_gate's (gdb_decoder.hip).
struct H16Ws { size_t trunk[H16_MAX_LAYERS + 1], a1[H16_MAX_LAYERS], a2[H16_MAX_LAYERS], c[H16_MAX_LAYERS], gate[H16_MAX_LAYERS], u, part, part2, count, total; int nseg, ngrp; };
static H16Ws h_ws(int B, int H, int W, int nlayers, bool keep) {
    H16Ws w{};
    const size_t n = (size_t)B * H * W;
    w.nseg = H * ((W + 31) / 32);
    w.ngrp = gdb_dec_se_groups(w.nseg);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
    w.trunk[0] = take(n * 128);
    size_t alt[2] = {0, 0};
    if (!keep) { alt[0] = take(n * 128); alt[1] = take(n * 128); }
    for (int b = 1; b <= nlayers; ++b) w.trunk[b] = keep ? take(n * 128) : alt[(b - 1) & 1];
    for (int b = 0; b < nlayers; ++b) {
        const bool own = keep || b == 0;
        w.a1[b] = own ? take(n * 64) : w.a1[0];
        w.a2[b] = own ? take(n * 64) : w.a2[0];
        w.c[b] = own ? take(n * 128) : w.c[0];
        w.gate[b] = own ? take(sizeof(float) * (size_t)B * H16_NF) : w.gate[0];
    }
    w.u = take(n * 128);
    w.part = take(sizeof(float) * (size_t)B * w.nseg * H16_NF);
    w.part2 = take(sizeof(float) * (size_t)B * w.ngrp * H16_NF);
    w.count = take(sizeof(unsigned) * (size_t)B);
    w.total = o;
    return w;
}
static int h_check_shape(const GdbFrame* shape) {
    if (!shape) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (shape->B < 1 || shape->H < 1 || shape->W < 1) return gdb_fail(GDB_E_SHAPE, "non-positive bundle map");
    if (shape->B > 256) return gdb_fail(GDB_E_SHAPE, "decoder batch %d > 256", shape->B);
    if ((size_t)shape->B * shape->H * shape->W >= ((size_t)1 << 31) / 64) return gdb_fail(GDB_E_SHAPE, "bundle map too large for the f16 decoder");
    return GDB_OK;
}
static int h_check_flags(int32_t flags) {
    if (flags & ~GDB_DECF16_KEEP_LAYERS) return gdb_fail(GDB_E_BADARG, "unknown f16 decoder flags 0x%x", flags);
    return GDB_OK;
}

extern "C" int gdb_decoder_f16_workspace_bytes(const GdbConfig* cfg, const GdbFrame* shape, int32_t num_layers, int32_t flags, size_t* out_bytes) {
    int rc = h_check(cfg, num_layers); if (rc) return rc;
    if ((rc = h_check_shape(shape)) || (rc = h_check_flags(flags))) return rc;
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    *out_bytes = h_ws(shape->B, shape->H, shape->W, num_layers, flags & GDB_DECF16_KEEP_LAYERS).total;
    return GDB_OK;
}

extern "C" int gdb_decoder_f16_layout(const GdbConfig* cfg, const GdbFrame* shape, int32_t num_layers, int32_t flags, GdbDecF16Region* out,
                                      int32_t capacity, int32_t* out_count) {
    int rc = h_check(cfg, num_layers); if (rc) return rc;
    if ((rc = h_check_shape(shape)) || (rc = h_check_flags(flags))) return rc;
    if (!out_count) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    const int count = (num_layers + 1) + 4 * num_layers + 1;
    *out_count = count;
    if (!out) return GDB_OK;   // a size query
    if (capacity < count) return gdb_fail(GDB_E_BADARG, "room for %d regions, %d needed", capacity, count);
    const H16Ws ws = h_ws(shape->B, shape->H, shape->W, num_layers, flags & GDB_DECF16_KEEP_LAYERS);
    int k = 0;
    auto put = [&](const char* name, size_t off, int ch, int type, int per_pixel) {
        GdbDecF16Region& r = out[k++];
        memset(&r, 0, sizeof(r));
        snprintf(r.name, sizeof(r.name), "%s", name);
        r.offset = off; r.channels = ch; r.dtype = type; r.per_pixel = per_pixel;
    };
    char nm[32];
    for (int b = 0; b <= num_layers; ++b) { snprintf(nm, sizeof(nm), "trunk.%d", b); put(nm, ws.trunk[b], H16_NF, GDB_DECF16_T_F16, 1); }
    for (int b = 0; b < num_layers; ++b) {
        snprintf(nm, sizeof(nm), "blocks.%d.conv1", b); put(nm, ws.a1[b], H16_G, GDB_DECF16_T_F16, 1);
        snprintf(nm, sizeof(nm), "blocks.%d.conv2", b); put(nm, ws.a2[b], H16_G, GDB_DECF16_T_F16, 1);
        snprintf(nm, sizeof(nm), "blocks.%d.conv3", b); put(nm, ws.c[b], H16_NF, GDB_DECF16_T_F16, 1);
        snprintf(nm, sizeof(nm), "blocks.%d.gate", b); put(nm, ws.gate[b], H16_NF, GDB_DECF16_T_F32, 0);
    }
    put("residual", ws.u, H16_NF, GDB_DECF16_T_F16, 1);
    return GDB_OK;
}

// ---- the convolution ------------------------------------------------------------------------------------------------------
struct HArgs {
    const float* in32; int ld32, off32, cin32;     // in_conv: the fp32 bundle rows, read in place
    const _Float16* src[2][2]; int spx[2][2];      // [chunk][32-channel half]: source and its halves per pixel
    // FUSE (chunk 0 only; src[0] = the previous trunk x): the staged input is t = f16(fmaf(c, gate, x)) - written to fX on the workgroup's
    // own pixels - or, with fS, u = f16(t + shallow), written to fU
    const _Float16* fT; const float* fgate; const _Float16* fS; _Float16* fX; _Float16* fU;
    const _Float16* w; const float* bias;
    _Float16* out; int cout, relu;
    float* rgb;                                     // folded up stage: (B, 3, 2H, 2W), channel c = 3 s + o of sub-pixel s = dy * 2 + dx
    float* se_part; unsigned* zero;
    int B, H, W, tilesX, tilesY;
};

// Sum of v over the 16 lanes of the caller's row group (fixed tree), valid in every lane.
__device__ __forceinline__ float h_row16_sum(float v) {
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xf, 0xf, true));
    };
    v += dpp(v, std::integral_constant<int, 0xB1>{});    // quad_perm [1,0,3,2]
    v += dpp(v, std::integral_constant<int, 0x4E>{});    // quad_perm [2,3,0,1]
    v += dpp(v, std::integral_constant<int, 0x141>{});   // row_half_mirror
    v += dpp(v, std::integral_constant<int, 0x140>{});   // row_mirror
    return v;
}

enum { H_PLAIN = 0, H_IN32 = 1, H_FUSE = 2 };

// NCT: 16-channel output tiles of the layer (4: in_conv, conv3; 2: conv1, conv2; 1: the folded up stage).  A wave owns tile wid % NCT
// and the NCT rows from (wid / NCT) NCT of the workgroup's four, both 16-pixel halves: 2 NCT accumulators.
// NKS0 / NKS1: 32-channel K-steps of the first / second chunk (NKS1 = 0: one chunk).  SEP: conv3's channel sums.  RGB: the up stage.
template <int NCT, int NKS0, int NKS1, int MODE, bool SEP, bool RGB>
__global__ void __launch_bounds__(256, (NCT == 4 && NKS1 > 0) ? 3 : 4) k_conv_h(HArgs a) {   // (conv3 spills 14 registers at four waves per SIMD)
    constexpr int NPW = 2 * NCT, NKST = NKS0 + NKS1;
    __shared__ __attribute__((aligned(16))) char lds[(H16_TR + 2) * H16_PX * H16_PSTR];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pl = lane & 15, kq = lane >> 4;
    const int ct = wid % NCT, rbase = (wid / NCT) * NCT;
    const int bx = blockIdx.x % a.tilesX, by = (blockIdx.x / a.tilesX) % a.tilesY, b = blockIdx.x / (a.tilesX * a.tilesY);
    const int x0 = bx * 32, y0 = by * H16_TR;
    if (a.zero && blockIdx.x == 0 && tid < a.B) a.zero[tid] = 0u;
    const int co = 16 * ct + 4 * kq;
    F4 acc[NPW];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float bv = a.bias ? a.bias[co + r] : 0.f;   // (the bias sections hold 64 floats)
#pragma unroll
        for (int g = 0; g < NPW; ++g) acc[g][r] = bv;
    }
    const size_t img = (size_t)b * a.H * a.W;
    const half8* wtile = (const half8*)a.w + (size_t)ct * NKST * 9 * 64 + lane;
    const char* bl = lds + (rbase * H16_PX + pl) * H16_PSTR + kq * 16;

    auto chunk = [&](auto cidx, auto nks_) {
        constexpr int c = decltype(cidx)::value, NKS = decltype(nks_)::value, NQ = 4 * NKS;
        const half8* wch = wtile + (size_t)(c == 0 ? 0 : NKS0) * 9 * 64;
        half8 wn[NKS];   // the next tap's A fragments, requested before this chunk is staged / under the current tap's MFMAs
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) wn[ks] = wch[(size_t)ks * 9 * 64];
        if (c > 0) __syncthreads();   // the previous chunk's reads are done
        // staging: every load of the chunk is issued before the first is used (branch-free: a slot outside the image or beyond the
        // tile loads a valid address and is zeroed in value), then converted / updated and stored
        constexpr int NSLOT = (H16_TR + 2) * H16_PX * NQ, NR = (NSLOT + 255) / 256;
        constexpr bool FU = MODE == H_FUSE && c == 0, FS = FU && RGB;   // (the up stage alone adds the global residual)
        half8 v[NR], ft[FU ? NR : 1], fs[FS ? NR : 1];
        float v32[MODE == H_IN32 ? NR : 1][8];
        unsigned inimg = 0;
#pragma unroll
        for (int s = 0; s < NR; ++s) {
            const int idx = min(tid + 256 * s, NSLOT - 1);
            const int p = idx / NQ, q = idx % NQ, rx = p % H16_PX, ry = p / H16_PX;
            const int px = x0 - 1 + rx, py = y0 - 1 + ry;
            const bool in = px >= 0 && px < a.W && py >= 0 && py < a.H;
            inimg |= (in ? 1u : 0u) << s;
            const size_t pix = in ? img + (size_t)py * a.W + px : img;
            const int hf = q >> 2, ch = 8 * (q & 3);
            if (MODE == H_IN32) {
                const float* sp = a.in32 + pix * a.ld32 + a.off32;
#pragma unroll
                for (int k = 0; k < 8; ++k) v32[s][k] = sp[min(ch + k, a.cin32 - 1)];
            } else {
                v[s] = *(const half8*)(a.src[c][hf] + pix * a.spx[c][hf] + ch);
                if (FU) {
                    ft[s] = *(const half8*)(a.fT + pix * H16_NF + 32 * hf + ch);
                    if (FS) fs[s] = *(const half8*)(a.fS + pix * H16_NF + 32 * hf + ch);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < NR; ++s) {
            const int idx = tid + 256 * s;
            if (idx >= NSLOT) continue;
            const int p = idx / NQ, q = idx % NQ, rx = p % H16_PX, ry = p / H16_PX;
            const int hf = q >> 2, ch = 8 * (q & 3);
            const bool in = (inimg >> s) & 1;
            half8 o = v[MODE == H_IN32 ? 0 : s];
            if (MODE == H_IN32) {
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = ch + k < a.cin32 ? (_Float16)v32[s][k] : (_Float16)0;   // nearest even
            }
            if (FU) {
                const int cc = 32 * hf + ch;
                const float* g = a.fgate + (size_t)b * H16_NF + cc;
                const bool inner = in && rx >= 1 && rx <= 32 && ry >= 1 && ry <= H16_TR;
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = (_Float16)fmaf((float)ft[s][k], g[k], (float)o[k]);
                const size_t pix = img + (size_t)(y0 - 1 + ry) * a.W + (x0 - 1 + rx);   // (used for inner pixels only: inside the image)
                if (inner && a.fX) *(half8*)(a.fX + pix * H16_NF + cc) = o;
                if (FS) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[k] = (_Float16)((float)o[k] + (float)fs[s][k]);
                    if (inner && a.fU) *(half8*)(a.fU + pix * H16_NF + cc) = o;
                }
            }
            if (!in) o = half8{0, 0, 0, 0, 0, 0, 0, 0};   // padding = 1: zeros outside the image
            *(half8*)(lds + p * H16_PSTR + q * 16) = o;
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
            half8 w[NKS];
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) w[ks] = wn[ks];
            if (tap < 8) {
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) wn[ks] = wch[((size_t)ks * 9 + tap + 1) * 64];
            }
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                // one K-step's B fragments at a time (left alone the scheduler hoists every tap's reads to the top: 260 registers spilled)
                __builtin_amdgcn_sched_barrier(0);
                half8 bv[NPW];
#pragma unroll
                for (int g = 0; g < NPW; ++g) bv[g] = *(const half8*)(bl + (((g >> 1) + dy) * H16_PX + 16 * (g & 1) + dx) * H16_PSTR + ks * 64);
#pragma unroll
                for (int g = 0; g < NPW; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[ks], bv[g], acc[g], 0, 0, 0);
            }
        }
    };
    chunk(std::integral_constant<int, 0>{}, std::integral_constant<int, NKS0>{});
    if constexpr (NKS1 > 0) chunk(std::integral_constant<int, 1>{}, std::integral_constant<int, NKS1>{});

    // epilogue: lane (pl, kq) holds output channels co .. co + 3 of pixel (y0 + rbase + (g >> 1), x0 + 16 (g & 1) + pl) in acc[g]
    if (SEP) {   // the (row, segment)'s channel sums of the UNROUNDED accumulators: part[b][y tilesX + bx][64]
#pragma unroll
        for (int r = 0; r < NCT; ++r) {
            const int y = y0 + rbase + r;
            if (y >= a.H) continue;   // (wave-uniform)
            F4 sum;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float v = 0.f;
#pragma unroll
                for (int h = 0; h < 2; ++h) v += (x0 + 16 * h + pl < a.W) ? acc[2 * r + h][k] : 0.f;
                sum[k] = h_row16_sum(v);
            }
            if (pl == 0) *(F4*)(a.se_part + (((size_t)b * a.H + y) * a.tilesX + bx) * H16_NF + co) = sum;
        }
    }
#pragma unroll
    for (int g = 0; g < NPW; ++g) {
        const int y = y0 + rbase + (g >> 1), x = x0 + 16 * (g & 1) + pl;
        if (y >= a.H || x >= a.W) continue;
        F4 v = acc[g];
        if (a.relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
        if (RGB) {   // channel c = 3 s + o -> rgb[b][o][2y + (s >> 1)][2x + (s & 1)], fp32
            const int Ho = 2 * a.H, Wo = 2 * a.W;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = co + k;
                if (c < 12) {
                    const int sp = c / 3, o = c - 3 * sp;
                    a.rgb[(((size_t)b * 3 + o) * Ho + 2 * y + (sp >> 1)) * Wo + 2 * x + (sp & 1)] = v[k];
                }
            }
        } else {
            const half4 h = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};   // round to nearest even, once
            *(half4*)(a.out + (img + (size_t)y * a.W + x) * a.cout + co) = h;
        }
    }
}

// ---- entry --------------------------------------------------------------------------------------------------------------
extern "C" int gdb_decode_f16(const GdbConfig* cfg, const GdbFrame* shape, const float* d_bundle_feat, int32_t ld_bundle_feat,
                              const void* d_packed_f16, int32_t num_layers, int32_t flags, void* d_ws, size_t ws_bytes, float* d_rgb_c,
                              void* stream_) {
    int rc = h_check(cfg, num_layers); if (rc) return rc;
    if ((rc = h_check_shape(shape)) || (rc = h_check_flags(flags))) return rc;
    const int B = shape->B, H = shape->H, W = shape->W;
    const int n_rgb = 3 * cfg->bundle_size * cfg->bundle_size, Q = n_rgb + GDB_CFR + GDB_CV;
    if (ld_bundle_feat < Q) return gdb_fail(GDB_E_SHAPE, "bundle_feat row stride %d < %d channels", ld_bundle_feat, Q);
    if (!d_bundle_feat || !d_packed_f16 || !d_ws || !d_rgb_c) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    const H16Ws ws = h_ws(B, H, W, num_layers, flags & GDB_DECF16_KEEP_LAYERS);
    if (ws_bytes < ws.total) return gdb_fail(GDB_E_WORKSPACE, "f16 decoder workspace %zu B < required %zu B", ws_bytes, ws.total);
    const H16Layout L = h_layout(num_layers);
    hipStream_t st = (hipStream_t)stream_;
    const char* pk = (const char*)d_packed_f16;
    auto H16 = [&](size_t off) { return (_Float16*)((char*)d_ws + off); };
    auto F32 = [&](size_t off) { return (float*)((char*)d_ws + off); };
    HArgs base{};
    base.B = B; base.H = H; base.W = W; base.tilesX = (W + 31) / 32; base.tilesY = (H + H16_TR - 1) / H16_TR;
    const dim3 grid((unsigned)(B * base.tilesX * base.tilesY)), block(256);
    auto trunk_src = [&](HArgs& a, int c, const _Float16* x) { a.src[c][0] = x; a.src[c][1] = x + 32; a.spx[c][0] = a.spx[c][1] = H16_NF; };
    hipError_t e;
#define CK(...) do { __VA_ARGS__; e = hipGetLastError(); if (e != hipSuccess) return gdb_fail(GDB_E_HIP, "f16 decoder launch: %s", hipGetErrorString(e)); } while (0)
    {   // shallow = in_conv(bundle channels n_rgb .. Q-1)
        HArgs a = base;
        a.in32 = d_bundle_feat; a.ld32 = ld_bundle_feat; a.off32 = n_rgb; a.cin32 = Q - n_rgb;
        a.w = (const _Float16*)(pk + L.in_w); a.bias = (const float*)(pk + L.in_b);
        a.out = H16(ws.trunk[0]); a.cout = H16_NF; a.zero = (unsigned*)((char*)d_ws + ws.count);
        CK(hipLaunchKernelGGL((k_conv_h<4, 1, 0, H_IN32, false, false>), grid, block, 0, st, a));
    }
    for (int b = 0; b < num_layers; ++b) {
        HArgs a = base;
        a.relu = 1; a.cout = H16_G;
        a.w = (const _Float16*)(pk + L.blk[b][0]); a.out = H16(ws.a1[b]);
        if (b == 0) {
            trunk_src(a, 0, H16(ws.trunk[0]));
            CK(hipLaunchKernelGGL((k_conv_h<2, 2, 0, H_PLAIN, false, false>), grid, block, 0, st, a));
        } else {   // conv1 first forms the block's own input x_b = f16(x_{b-1} + c_{b-1} gate_{b-1}) and leaves it in trunk[b]
            trunk_src(a, 0, H16(ws.trunk[b - 1]));
            a.fT = H16(ws.c[b - 1]); a.fgate = F32(ws.gate[b - 1]); a.fX = H16(ws.trunk[b]);
            CK(hipLaunchKernelGGL((k_conv_h<2, 2, 0, H_FUSE, false, false>), grid, block, 0, st, a));
            a.fT = nullptr; a.fgate = nullptr; a.fX = nullptr;
        }
        trunk_src(a, 0, H16(ws.trunk[b]));
        a.src[1][0] = H16(ws.a1[b]); a.spx[1][0] = H16_G;
        a.w = (const _Float16*)(pk + L.blk[b][1]); a.out = H16(ws.a2[b]);
        CK(hipLaunchKernelGGL((k_conv_h<2, 2, 1, H_PLAIN, false, false>), grid, block, 0, st, a));
        a.src[1][1] = H16(ws.a2[b]); a.spx[1][1] = H16_G;
        a.w = (const _Float16*)(pk + L.blk[b][2]); a.out = H16(ws.c[b]); a.cout = H16_NF; a.relu = 0; a.se_part = F32(ws.part);
        CK(hipLaunchKernelGGL((k_conv_h<4, 2, 2, H_PLAIN, true, false>), grid, block, 0, st, a));
        e = gdb_dec_se_gate_launch(F32(ws.part), B, ws.nseg, 1.f / (float)((size_t)H * W), (const float*)(pk + L.blk[b][3]),
                                   (const float*)(pk + L.blk[b][4]), F32(ws.part2), (unsigned*)((char*)d_ws + ws.count), F32(ws.gate[b]), st);
        if (e != hipSuccess) return gdb_fail(GDB_E_HIP, "f16 decoder launch: %s", hipGetErrorString(e));
    }
    {   // the folded up stage on u = f16(shallow + trunk[L]), trunk[L] = f16(x_{L-1} + c_{L-1} gate_{L-1})
        HArgs a = base;
        trunk_src(a, 0, H16(ws.trunk[num_layers - 1]));
        a.fT = H16(ws.c[num_layers - 1]); a.fgate = F32(ws.gate[num_layers - 1]); a.fX = H16(ws.trunk[num_layers]);
        a.fS = H16(ws.trunk[0]); a.fU = H16(ws.u);
        a.w = (const _Float16*)(pk + L.up_w); a.bias = (const float*)(pk + L.up_b); a.rgb = d_rgb_c;
        CK(hipLaunchKernelGGL((k_conv_h<1, 2, 0, H_FUSE, false, true>), grid, block, 0, st, a));
    }
#undef CK
    return GDB_OK;
}
