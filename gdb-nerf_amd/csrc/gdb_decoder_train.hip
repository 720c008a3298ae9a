// The residual-dense decoder in TRAINING mode: the weight pack on the device, the saved-activation forward
// and - further down, with its own comment - the backward.  fp32 only (v_mfma_f32_16x16x4_f32, the reference's precision), bundle_size 2, whole frames.
//
// * gdb_decoder_train_pack: the parameters stay where the optimiser keeps them.  Two launches read them through device pointers in
//   state-dict order and writes the fp32 operand forms of gdb_pack_decoder_weights (pack_conv16 packets, biases, the two
//   squeeze-excitation matrices, the last up stage folded with out_conv in double, summed in the host's order and rounded once):
//   byte for byte what the host pack writes from the same values.  No host copy of a parameter, no synchronisation.  The buffer is
//   the fp32 prefix of the eval-mode packed buffer (same offsets, dec_layout) plus the tap block the convolution's weight prefetch
//   runs into, then the data-gradient forms of every convolution (dect_packed).
// * gdb_decoder_train_forward: gdb_decode's fp32 launch sequence (dec_phases, gdb_decoder.hip: the same kernels, the same
//   arithmetic, rgb_c bit-identical) with every block's activations in a caller-owned "saved" buffer instead of the rotating
//   workspace: per block b its input x.b (x.0 = shallow), ab.b = [a | b] after ReLU, T.b = conv3's output and gate.b, and xu = the up
//   stage's input x_L + shallow - what a backward needs.  gdb_decoder_train_layout names the regions.
//
// The element <-> (tile, chunk, tap, group, lane, e) arithmetic of the pack is in __host__ __device__ helpers (dect_conv16_elem), so
// that a host program can walk every section and check each address (gdb_decoder_train_index.h, tools/check_decoder_train_index.cpp).
#include "gdb_decoder_layout.h"
#include "gdb_decoder_train_index.h"
#include <cstring>
#include <cstdio>

// dect_conv16_elem, dect_conv16_src, dect_conv16_src_t, dect_dw_wave, dect_dw_part_index: gdb_decoder_train_index.h
enum { DECT_CONV = 0, DECT_COPY = 1, DECT_FOLD_W = 2, DECT_FOLD_B = 3, DECT_ZERO = 4, DECT_CONV_T = 5, DECT_FOLD_WT = 6 };
#define DECT_MAX_SECT (2 + 5 * DEC_MAX_LAYERS + 3)   // in_conv w, b; five per block; the folded stage's w, b; the tail (either launch)
struct DectSect { const float* src; unsigned dst, n; int kind_cout, cin, rs_c0, pad; };   // kind << 16 | cout;  rs << 16 | c0
struct DectPack {
    float* out;
    const float* up_w; const float* up_b; const float* out_w; const float* out_b;   // the fold's four tensors
    int nsect;
    DectSect s[DECT_MAX_SECT];
};
static_assert(sizeof(DectPack) <= 4096, "the pack's section table travels as a kernel argument");

// One thread per packed float; blockIdx.y = section.  The fold: channel c = 3 s + o of the folded stage, s = 2 dy + dx the sub-pixel:
// Wf[c][ci][tap] = sum_k out_w[o][k] up_w[4 k + s][ci][tap], bf[c] = out_b[o] + sum_k out_w[o][k] up_b[4 k + s], in double in k order
// (a product of two floats is exact in double, so whether the compiler fuses the multiply-add cannot change a bit), rounded once.
__global__ void __launch_bounds__(256) k_dect_pack(DectPack p) {
    const DectSect s = p.s[blockIdx.y];
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= s.n) return;
    const int kind = s.kind_cout >> 16, cout = s.kind_cout & 0xffff;
    float v = 0.f;
    if (kind == DECT_CONV) {
        const long long k = dect_conv16_src(i, (s.cin + 31) / 32, cout, s.cin);
        if (k >= 0) v = s.src[k];
    } else if (kind == DECT_COPY) {
        v = s.src[i];
    } else if (kind == DECT_FOLD_W) {
        int c, ci, tap;
        dect_conv16_elem(i, DEC_NF / 32, &c, &ci, &tap);
        if (c < 12) {   // (ci < 64 always: two whole chunks)
            const int sp = c / 3, o = c - 3 * sp;
            double acc = 0;
            for (int k = 0; k < DEC_NF; ++k)
                acc += (double)p.out_w[o * DEC_NF + k] * (double)p.up_w[((size_t)(4 * k + sp) * DEC_NF + ci) * 9 + tap];
            v = (float)acc;
        }
    } else if (kind == DECT_CONV_T) {
        const long long k = dect_conv16_src_t(i, (s.cin + 31) / 32, cout, s.cin, s.rs_c0 >> 16, s.rs_c0 & 0xffff);
        if (k >= 0) v = s.src[k];
    } else if (kind == DECT_FOLD_WT) {   // the folded stage's data gradient: output channel ci of 64, input channel c of 12, tap flipped
        int ci, c, tap;
        dect_conv16_elem(i, 1, &ci, &c, &tap);
        if (c < 12) {
            const int sp = c / 3, o = c - 3 * sp;
            double acc = 0;
            for (int k = 0; k < DEC_NF; ++k)
                acc += (double)p.out_w[o * DEC_NF + k] * (double)p.up_w[((size_t)(4 * k + sp) * DEC_NF + ci) * 9 + (8 - tap)];
            v = (float)acc;
        }
    } else if (kind == DECT_FOLD_B) {
        if (i < 12) {
            const int sp = (int)i / 3, o = (int)i - 3 * sp;
            double acc = p.out_b[o];
            for (int k = 0; k < DEC_NF; ++k) acc += (double)p.out_w[o * DEC_NF + k] * (double)p.up_b[4 * k + sp];
            v = (float)acc;
        }
    }
    p.out[s.dst + i] = v;
}

// ---- checks ---------------------------------------------------------------------------------------------------------------------
static int dect_check(const GdbConfig* cfg, int nlayers, int precision) {
    int rc = gdb_check_cfg(cfg); if (rc) return rc;
    if (cfg->bundle_size != 2)
        return gdb_fail(GDB_E_BADARG, "the HIP decoder's training mode is built for bundle_size 2 (one up stage); got %d", cfg->bundle_size);
    if (nlayers < 1 || nlayers > DEC_MAX_LAYERS) return gdb_fail(GDB_E_BADARG, "decoder layers %d outside 1..%d", nlayers, DEC_MAX_LAYERS);
    if (precision != GDB_PREC_F32)
        return gdb_fail(GDB_E_BADARG, "the HIP decoder's training mode is fp32 only (precision 1 = fp32 MFMA); got %d", precision);
    return GDB_OK;
}
static int dect_check_shape(const GdbConfig* cfg, const GdbFrame* shape) {
    if (!shape) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    if (shape->B < 1 || shape->H < 1 || shape->W < 1) return gdb_fail(GDB_E_SHAPE, "non-positive bundle map");
    if (shape->B > 256) return gdb_fail(GDB_E_SHAPE, "decoder batch %d > 256", shape->B);
    return GDB_OK;
}

// The fp32 sections of dec_layout and the prefetch tail behind them, then the data-gradient forms (pack_conv16 packets of the
// transposed, tap-flipped layers) and a tail of their own:
//   up_t   the folded stage: 12 -> 64;   per block c3x, c3ab (conv3: 64 -> its x and its [a | b] input channels), c2x, c2a (conv2:
//   32 -> x, 32 -> a), c1x (conv1: 32 -> x);   in_t  in_conv: 64 -> 27.
struct DectPacked { size_t fwd_tail, up_t, blk_t[DEC_MAX_LAYERS][5], in_t, bwd_tail, total; };
static DectPacked dect_packed(const DecLayout& L, int nlayers) {
    DectPacked P{};
    P.fwd_tail = L.in_wx;
    size_t o = (L.in_wx + 8 * 128 + 63) / 64 * 64;
    P.up_t = o; o += conv_floats(12, 2);
    for (int b = 0; b < nlayers; ++b) {
        P.blk_t[b][0] = o; o += conv_floats(DEC_NF, 2);
        P.blk_t[b][1] = o; o += conv_floats(DEC_NF, 2);
        P.blk_t[b][2] = o; o += conv_floats(DEC_G, 2);
        P.blk_t[b][3] = o; o += conv_floats(DEC_G, 1);
        P.blk_t[b][4] = o; o += conv_floats(DEC_G, 2);
    }
    P.in_t = o; o += conv_floats(DEC_NF, 1);
    P.bwd_tail = o;
    P.total = (o + 8 * 128 + 63) / 64 * 64;
    return P;
}
static size_t dect_packed_floats(const DecLayout& L, int nlayers) { return dect_packed(L, nlayers).total; }

extern "C" int gdb_decoder_train_packed_floats(const GdbConfig* cfg, int32_t num_layers, size_t* out_floats) {
    int rc = dect_check(cfg, num_layers, GDB_PREC_F32); if (rc) return rc;
    if (!out_floats) return gdb_fail(GDB_E_BADARG, "out_floats is NULL");
    *out_floats = dect_packed_floats(dec_layout(num_layers, 2), num_layers);
    return GDB_OK;
}

extern "C" int gdb_decoder_train_pack(const GdbConfig* cfg, int32_t num_layers, int32_t precision, const float* const* d_tensors,
                                      float* d_packed, size_t packed_floats, void* stream_) {
    int rc = dect_check(cfg, num_layers, precision); if (rc) return rc;
    if (!d_tensors || !d_packed) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    const int n = 2 + 5 * num_layers + 4;
    for (int i = 0; i < n; ++i)
        if (!d_tensors[i]) return gdb_fail(GDB_E_BADARG, "decoder tensor %d is NULL", i);
    const DecLayout L = dec_layout(num_layers, 2);
    const DectPacked P = dect_packed(L, num_layers);
    const size_t total = P.total;
    if (packed_floats < total) return gdb_fail(GDB_E_WORKSPACE, "decoder packed buffer %zu floats < required %zu", packed_floats, total);
    DectPack p{};
    p.out = d_packed;
    p.up_w = d_tensors[n - 4]; p.up_b = d_tensors[n - 3]; p.out_w = d_tensors[n - 2]; p.out_b = d_tensors[n - 1];
    size_t nmax = 0;
    auto add = [&](int kind, const float* src, size_t dst, size_t cnt, int cout, int cin) {
        DectSect& s = p.s[p.nsect++];
        s.src = src; s.dst = (unsigned)dst; s.n = (unsigned)cnt; s.kind_cout = kind << 16 | cout; s.cin = cin;
        if (cnt > nmax) nmax = cnt;
    };
    auto add_t = [&](const float* src, size_t dst, int cout, int cin, int rs, int c0) {   // a data-gradient form: cout <- cin channels
        add(DECT_CONV_T, src, dst, conv_floats(cin, cout > 32 ? 2 : 1), cout, cin);
        p.s[p.nsect - 1].rs_c0 = rs << 16 | c0;
    };
    const int cin0 = GDB_CFR + GDB_CV;  // 27
    add(DECT_CONV, d_tensors[0], L.in_w, conv_floats(cin0, 2), DEC_NF, cin0);
    add(DECT_COPY, d_tensors[1], L.in_b, DEC_NF, 0, 0);
    for (int b = 0; b < num_layers; ++b) {
        const float* const* q = d_tensors + 2 + 5 * b;
        add(DECT_CONV, q[0], L.blk[b][0], conv_floats(DEC_NF, 1), DEC_G, DEC_NF);
        add(DECT_CONV, q[1], L.blk[b][1], conv_floats(DEC_NF + DEC_G, 1), DEC_G, DEC_NF + DEC_G);
        add(DECT_CONV, q[2], L.blk[b][2], conv_floats(DEC_NF + 2 * DEC_G, 2), DEC_NF, DEC_NF + 2 * DEC_G);
        add(DECT_COPY, q[3], L.blk[b][3], DEC_SE_R * DEC_NF, 0, 0);
        add(DECT_COPY, q[4], L.blk[b][4], DEC_NF * DEC_SE_R, 0, 0);
    }
    add(DECT_FOLD_W, nullptr, L.up_w, conv_floats(DEC_NF, 1), 12, DEC_NF);
    add(DECT_FOLD_B, nullptr, L.up_b, 32, 12, 0);
    add(DECT_ZERO, nullptr, P.fwd_tail, P.up_t - P.fwd_tail, 0, 0);
    hipLaunchKernelGGL(k_dect_pack, dim3((unsigned)((nmax + 255) / 256), (unsigned)p.nsect), dim3(256), 0, (hipStream_t)stream_, p);
    LAUNCH_CHECK("k_dect_pack");
    // the data-gradient forms: a second launch (the section table of both would not fit one kernel argument)
    p.nsect = 0; nmax = 0;
    add(DECT_FOLD_WT, nullptr, P.up_t, conv_floats(12, 2), DEC_NF, 12);
    for (int b = 0; b < num_layers; ++b) {
        const float* const* q = d_tensors + 2 + 5 * b;
        add_t(q[2], P.blk_t[b][0], DEC_NF, DEC_NF, DEC_NF + 2 * DEC_G, 0);
        add_t(q[2], P.blk_t[b][1], DEC_NF, DEC_NF, DEC_NF + 2 * DEC_G, DEC_NF);
        add_t(q[1], P.blk_t[b][2], DEC_NF, DEC_G, DEC_NF + DEC_G, 0);
        add_t(q[1], P.blk_t[b][3], DEC_G, DEC_G, DEC_NF + DEC_G, DEC_NF);
        add_t(q[0], P.blk_t[b][4], DEC_NF, DEC_G, DEC_NF, 0);
    }
    add_t(d_tensors[0], P.in_t, cin0, DEC_NF, cin0, 0);
    add(DECT_ZERO, nullptr, P.bwd_tail, total - P.bwd_tail, 0, 0);
    hipLaunchKernelGGL(k_dect_pack, dim3((unsigned)((nmax + 255) / 256), (unsigned)p.nsect), dim3(256), 0, (hipStream_t)stream_, p);
    LAUNCH_CHECK("k_dect_pack");
    return GDB_OK;
}

// ---- the saved buffer -------------------------------------------------------------------------------------------------------------
struct DectSaved { size_t x[DEC_MAX_LAYERS], ab[DEC_MAX_LAYERS], T[DEC_MAX_LAYERS], gate[DEC_MAX_LAYERS], xu, part, part2, count, total; int nseg, ngrp; };
static DectSaved dect_saved(int B, int H, int W, int nlayers) {
    DectSaved s{};
    const size_t act = sizeof(float) * (size_t)B * H * W * DEC_NF;
    s.nseg = H * ((W + 31) / 32);
    s.ngrp = gdb_dec_se_groups(s.nseg);
    size_t o = 0;
    for (int b = 0; b < nlayers; ++b) {
        s.x[b] = o; o = align_up(o + act, 256);
        s.ab[b] = o; o = align_up(o + act, 256);
        s.T[b] = o; o = align_up(o + act, 256);
        s.gate[b] = o; o = align_up(o + sizeof(float) * (size_t)B * DEC_NF, 256);
    }
    s.xu = o; o = align_up(o + act, 256);
    s.part = o; o = align_up(o + sizeof(float) * (size_t)B * s.nseg * DEC_NF, 256);
    s.part2 = o; o = align_up(o + sizeof(float) * (size_t)B * s.ngrp * DEC_NF, 256);
    s.count = o; o = align_up(o + sizeof(unsigned) * (size_t)B, 256);
    s.total = o;
    return s;
}

extern "C" int gdb_decoder_train_saved_bytes(const GdbConfig* cfg, const GdbFrame* shape, int32_t num_layers, size_t* out_bytes) {
    int rc = dect_check(cfg, num_layers, GDB_PREC_F32); if (rc) return rc;
    rc = dect_check_shape(cfg, shape); if (rc) return rc;
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    *out_bytes = dect_saved(shape->B, shape->H, shape->W, num_layers).total;
    return GDB_OK;
}

extern "C" int gdb_decoder_train_layout(const GdbConfig* cfg, const GdbFrame* shape, int32_t num_layers, GdbDecRegion* out, int32_t capacity,
                                        int32_t* out_count) {
    int rc = dect_check(cfg, num_layers, GDB_PREC_F32); if (rc) return rc;
    rc = dect_check_shape(cfg, shape); if (rc) return rc;
    if (!out_count) return gdb_fail(GDB_E_BADARG, "out_count is NULL");
    const int count = 4 * num_layers + 3;
    *out_count = count;
    if (!out) return GDB_OK;
    if (capacity < count) return gdb_fail(GDB_E_BADARG, "region capacity %d < %d", capacity, count);
    const int B = shape->B, H = shape->H, W = shape->W;
    const DectSaved s = dect_saved(B, H, W, num_layers);
    int k = 0;
    auto put = [&](const char* fmt, int b, size_t off, int d0, int d1, int d2, int d3) {
        GdbDecRegion& r = out[k++];
        memset(&r, 0, sizeof r);
        snprintf(r.name, sizeof r.name, fmt, b);
        r.offset = off;
        r.shape[0] = d0; r.shape[1] = d1; r.shape[2] = d2; r.shape[3] = d3;
        r.bytes = sizeof(float) * (size_t)d0 * (size_t)d1 * (size_t)(d2 ? d2 : 1) * (size_t)(d3 ? d3 : 1);
    };
    for (int b = 0; b < num_layers; ++b) {
        put("x.%d", b, s.x[b], B, H, W, DEC_NF); put("ab.%d", b, s.ab[b], B, H, W, DEC_NF);
        put("T.%d", b, s.T[b], B, H, W, DEC_NF); put("gate.%d", b, s.gate[b], B, DEC_NF, 0, 0);
    }
    put("xu", 0, s.xu, B, H, W, DEC_NF);
    put("part", 0, s.part, B, H, (W + 31) / 32, DEC_NF);
    put("part2", 0, s.part2, B, s.ngrp, DEC_NF, 0);
    return GDB_OK;
}

// ---- the training forward ---------------------------------------------------------------------------------------------------------
extern "C" int gdb_decoder_train_forward(const GdbConfig* cfg, const GdbFrame* shape, const float* d_bundle_feat, int32_t ld_bundle_feat,
                                         const float* d_packed, int32_t num_layers, int32_t precision, void* d_saved, size_t saved_bytes,
                                         float* d_rgb_c, void* stream_) {
    int rc = dect_check(cfg, num_layers, precision); if (rc) return rc;
    rc = dect_check_shape(cfg, shape); if (rc) return rc;
    const int B = shape->B, H = shape->H, W = shape->W;
    const int Q = 3 * cfg->bundle_size * cfg->bundle_size + GDB_CFR + GDB_CV;
    if (ld_bundle_feat < Q) return gdb_fail(GDB_E_SHAPE, "bundle_feat row stride %d < %d channels", ld_bundle_feat, Q);
    if ((size_t)H * W * (size_t)(ld_bundle_feat > DEC_NF ? ld_bundle_feat : DEC_NF) >= ((size_t)1 << 30))
        return gdb_fail(GDB_E_SHAPE, "bundle map too large for the decoder's 32-bit staging byte offsets");
    if (!d_bundle_feat || !d_packed || !d_saved || !d_rgb_c) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    const DectSaved s = dect_saved(B, H, W, num_layers);
    if (saved_bytes < s.total) return gdb_fail(GDB_E_WORKSPACE, "decoder saved buffer %zu B < required %zu B", saved_bytes, s.total);
    DecBufs bufs{};
    char* base = (char*)d_saved;
    for (int b = 0; b < num_layers; ++b) {
        bufs.x[b] = (float*)(base + s.x[b]); bufs.ab[b] = (float*)(base + s.ab[b]);
        bufs.T[b] = (float*)(base + s.T[b]); bufs.gate[b] = (float*)(base + s.gate[b]);
    }
    bufs.xu = (float*)(base + s.xu);
    bufs.part = (float*)(base + s.part); bufs.part2 = (float*)(base + s.part2); bufs.count = (unsigned*)(base + s.count);
    return gdb_dec_phases_on(cfg, B, H, W, d_bundle_feat, ld_bundle_feat, d_packed, num_layers, bufs, d_rgb_c, (hipStream_t)stream_);
}

// ==== the backward ===================================================================================================================
// Input g_rgb_c (B, 3, 2H, 2W); output the gradient of every parameter in its own layout and of the bundle rows.  In the order run:
//   un-shuffle g_rgb_c into 12-channel rows G12 (channel 3 s + o, as the folded stage writes them);
//   the folded stage: dWf, dbf like any other layer, mapped back to up.0 / out_conv (k_dect_fold_back); its data gradient GXU = the
//     gradient of xu = x_L + shallow, i.e. of the trunk's end AND of shallow (the global residual);
//   per block, in reverse, with dxn the gradient of x_{b+1}: squeeze-excitation (k_dect_psum: per batch item and group of pixels the
//     channel sums of dxn * T and of T, in double, four strided partial sums and a fixed tree; k_dect_psum2: four groups each, in index
//     order; k_dect_se: those sums the same way as the pixels,
//     the two tiny linears, d fc.0 and d fc.2 summed over the batch in index order), dT = dxn g + dmean / HW, then the data gradients
//     of conv3, conv2, conv1 on the forward convolution kernel with the transposed, tap-flipped weights of the pack, the ReLU masks
//     from the saved post-ReLU values (ReLU'(0) = 0), and dx_b = ((dxn + GX3) + GX2) + GX1 in that order;
//   shallow's gradient = dx_0 + GXU; in_conv's weight and bias gradients; its data gradient into columns 12 .. 38 of the row gradient.
// Weight gradients: k_dect_dw, a GEMM with K = pixels on v_mfma_f32_16x16x4_f32 (k_crt_dw of gdb_costreg_train.hip is the model): a
// wave owns a 16 x 16 (co, ci) tile, TG taps and a slab of image rows and writes one partial; the partials are added in slab order
// in double in two levels (DECT_R1 slabs per first-level group).  Bias gradients: k_dect_psum's column sums through k_dect_psum2, then four strided
// sums over (item, group) and a fixed tree in double (k_dect_bias).  No atomics on data anywhere: two runs are bit-identical.
typedef float F4 __attribute__((ext_vector_type(4)));

struct DectDw {
    const float* dY; int ys, yo, M;              // dY[pixel * ys + yo + m]
    const float* X1; int s1, o1, nsplit;         // X channel n < nsplit: X1[pixel * s1 + o1 + n]
    const float* X2; int s2, o2, N;              //            otherwise: X2[pixel * s2 + o2 + n - nsplit]
    float* part;                                 // [nslab][M][N][9]
    int B, H, W, nmt, nnt, nslab, rps, rows, nwaves;
};
template <int TG>
__global__ void __launch_bounds__(256) k_dect_dw(DectDw a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (wave >= a.nwaves) return;
    const int j = lane & 15, kq = lane >> 4;
    int mt, nt, tg, slab, r0, r1;
    dect_dw_wave(wave, a.nmt, a.nnt, 9 / TG, a.rps, a.rows, &mt, &nt, &tg, &slab, &r0, &r1);
    F4 acc[TG];
#pragma unroll
    for (int q = 0; q < TG; ++q) acc[q] = F4{0.f, 0.f, 0.f, 0.f};
    const int m = 16 * mt + j, n = 16 * nt + j;
    const bool mok = m < a.M, nok = n < a.N;
    const bool first = n < a.nsplit;
    const float* xb = first ? a.X1 + a.o1 + n : a.X2 + a.o2 + (n - a.nsplit);   // (never dereferenced when !nok)
    const int xs = first ? a.s1 : a.s2;
    for (int r = r0; r < r1; ++r) {
        const int y = r % a.H, b = r / a.H;
        const size_t img = (size_t)b * a.H * a.W;
        const float* yrow = a.dY + (img + (size_t)y * a.W) * a.ys + a.yo + m;
        for (int x0 = 0; x0 < a.W; x0 += 4) {
            const int x = x0 + kq;
            const bool xok = x < a.W;
            const float av = (mok && xok) ? yrow[(size_t)x * a.ys] : 0.f;
#pragma unroll
            for (int q = 0; q < TG; ++q) {
                const int tap = tg * TG + q, iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
                float bv = 0.f;
                if (nok && xok && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) bv = xb[(img + (size_t)iy * a.W + ix) * xs];
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[q], 0, 0, 0);
            }
        }
    }
    // register r of lane (j, kq) = row 4 kq + r, column j of the tile
#pragma unroll
    for (int q = 0; q < TG; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long k = dect_dw_part_index(slab, a.M, a.N, 16 * mt + 4 * kq + r, 16 * nt + j, tg * TG + q);
            if (k >= 0) a.part[k] = acc[q][r];
        }
}

#define DECT_R1 16   // slabs per first-level group
__global__ void __launch_bounds__(256) k_dect_reduce1(const float* __restrict__ part, double* __restrict__ p2, size_t wn, int nslab, int ng) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= wn * ng) return;
    const size_t g = i / wn, w = i - g * wn;
    const int s1 = (int)g * DECT_R1 + DECT_R1 < nslab ? (int)g * DECT_R1 + DECT_R1 : nslab;
    double s = 0.0;
    for (int q = (int)g * DECT_R1; q < s1; ++q) s += (double)part[(size_t)q * wn + w];
    p2[i] = s;
}
__global__ void __launch_bounds__(256) k_dect_reduce2(const double* __restrict__ p2, float* __restrict__ out, size_t wn, int ng) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= wn) return;
    double s = 0.0;
    for (int g = 0; g < ng; ++g) s += p2[(size_t)g * wn + w];
    out[w] = (float)s;
}

// (B, 3, 2H, 2W) -> rows of 16 floats: channel c = 3 s + o < 12 of pixel (y, x) = g[b][o][2y + (s >> 1)][2x + (s & 1)], 12 .. 15 zero
__global__ void __launch_bounds__(256) k_dect_unshuffle(const float* __restrict__ g, float* __restrict__ out, int B, int H, int W) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * H * W * 16) return;
    const int c = (int)(i & 15);
    const size_t pix = i >> 4;
    const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((size_t)W * H));
    float v = 0.f;
    if (c < 12) {
        const int sp = c / 3, o = c - 3 * sp;
        v = g[(((size_t)b * 3 + o) * (2 * H) + 2 * y + (sp >> 1)) * (2 * (size_t)W) + 2 * x + (sp & 1)];
    }
    out[i] = v;
}

// Channel sums per (batch item, group of DECT_PG pixels): part[(b ngrp + g) 2 + 0][c] = sum A[p][c] * (Bm ? Bm[p][c] : 1),
// part[..+ 1][c] = sum Bm[p][c] (0 without Bm); c < nc <= 64.  Thread (c, q) adds the group's pixels q, q + 4, .. in order in double;
// the four are then added as (0 + 1) + (2 + 3).
#define DECT_PG 64
__global__ void __launch_bounds__(256) k_dect_psum(const float* __restrict__ A, int sa, int oa, const float* __restrict__ Bm, int nc,
                                                   size_t npix, int ngrp, double* __restrict__ part) {
    __shared__ double red[2][256];
    const int g = blockIdx.x % ngrp, b = blockIdx.x / ngrp;
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const size_t p0 = (size_t)g * DECT_PG, p1 = p0 + DECT_PG < npix ? p0 + DECT_PG : npix;
    double s0 = 0.0, s1 = 0.0;
    if (c < nc)
        for (size_t p = p0 + q; p < p1; p += 4) {
            const size_t pix = (size_t)b * npix + p;
            const double av = (double)A[pix * sa + oa + c];
            if (Bm) { const double t = (double)Bm[pix * DEC_NF + c]; s0 += av * t; s1 += t; }
            else s0 += av;
        }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1;
    __syncthreads();
    if (q < 2) {
        const double* r = red[q];
        part[((size_t)blockIdx.x * 2 + q) * 64 + c] = (r[c] + r[64 + c]) + (r[128 + c] + r[192 + c]);
    }
}
// The second level of those sums: part2[(b ng2 + g2) 2 + which][c] = the groups g2 DECT_R2 .. g2 DECT_R2 + DECT_R2 - 1 of item b, added in
// index order.  One thread per (which, c); grid B ng2.
#define DECT_R2 4
__global__ void __launch_bounds__(128) k_dect_psum2(const double* __restrict__ part, int ngrp, int ng2, double* __restrict__ part2) {
    const int g2 = blockIdx.x % ng2, b = blockIdx.x / ng2;
    const int c = threadIdx.x & 63, which = threadIdx.x >> 6;
    const int g1 = g2 * DECT_R2 + DECT_R2 < ngrp ? g2 * DECT_R2 + DECT_R2 : ngrp;
    double s = 0.0;
    for (int g = g2 * DECT_R2; g < g1; ++g) s += part[(((size_t)b * ngrp + g) * 2 + which) * 64 + c];
    part2[((size_t)blockIdx.x * 2 + which) * 64 + c] = s;
}

// Column sums over every (item, group) -> out[c], c < nc: the bias gradients.  One workgroup; thread (c, q) adds the partials q, q + 4, ..
// in index order, the four are then added as (0 + 1) + (2 + 3).
__global__ void __launch_bounds__(256) k_dect_bias(const double* __restrict__ part, int n, int nc, float* __restrict__ out) {
    __shared__ double red[256];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    double s = 0.0;
    for (int k = q; k < n; k += 4) s += part[((size_t)k * 2) * 64 + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (q == 0 && c < nc) out[c] = (float)((red[c] + red[64 + c]) + (red[128 + c] + red[192 + c]));
}

// The squeeze-excitation's backward, one workgroup, batch items in index order.  With S = sum_p dxn T, mean = sum_p T / HW (both from
// k_dect_psum's groups: thread (c, q) adds the groups q, q + 4, .. in index order, the four are then added as (0 + 1) + (2 + 3)),
// h = fc0 mean, hid = ReLU(h), gate g (the forward's, saved): dz = S g (1 - g), d fc2[c][r] += dz[c] hid[r], dhid = fc2^T dz,
// dh = ReLU'(h) dhid, d fc0[r][k] += dh[r] mean[k], dmean = fc0^T dh; dm[b][k] = dmean[k] / HW (what every pixel of T receives).
__global__ void __launch_bounds__(256) k_dect_se(const double* __restrict__ part, int ngrp, int B, double inv_hw, const float* __restrict__ fc0,
                                                 const float* __restrict__ fc2, const float* __restrict__ gate, float* __restrict__ dm,
                                                 float* __restrict__ dfc0, float* __restrict__ dfc2) {
    __shared__ double red[2][256];
    __shared__ double mean[DEC_NF], dz[DEC_NF], h[DEC_SE_R], dh[DEC_SE_R];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    double a0[DEC_SE_R] = {0, 0, 0, 0}, a2[DEC_SE_R] = {0, 0, 0, 0};   // d fc0[r][c], d fc2[c][r] (threads q == 0)
    for (int b = 0; b < B; ++b) {
        double S = 0.0, M = 0.0;
        for (int g = q; g < ngrp; g += 4) {
            S += part[(((size_t)b * ngrp + g) * 2) * 64 + c];
            M += part[(((size_t)b * ngrp + g) * 2 + 1) * 64 + c];
        }
        __syncthreads();   // the previous item's reads of red / mean / dz / h / dh are done
        red[0][threadIdx.x] = S; red[1][threadIdx.x] = M;
        __syncthreads();
        if (q == 0) {
            S = (red[0][c] + red[0][64 + c]) + (red[0][128 + c] + red[0][192 + c]);
            M = (red[1][c] + red[1][64 + c]) + (red[1][128 + c] + red[1][192 + c]);
            mean[c] = M * inv_hw;
            const double gt = (double)gate[(size_t)b * DEC_NF + c];
            dz[c] = S * gt * (1.0 - gt);
        }
        __syncthreads();
        if (threadIdx.x < DEC_SE_R) {
            const int r = threadIdx.x;
            double acc = 0.0;
            for (int k = 0; k < DEC_NF; ++k) acc += (double)fc0[r * DEC_NF + k] * mean[k];
            h[r] = acc;
            double d = 0.0;
            for (int k = 0; k < DEC_NF; ++k) d += (double)fc2[k * DEC_SE_R + r] * dz[k];
            dh[r] = acc > 0.0 ? d : 0.0;
        }
        __syncthreads();
        if (q == 0) {
            double dmean = 0.0;
#pragma unroll
            for (int r = 0; r < DEC_SE_R; ++r) {
                a2[r] += dz[c] * (h[r] > 0.0 ? h[r] : 0.0);
                a0[r] += dh[r] * mean[c];
                dmean += (double)fc0[r * DEC_NF + c] * dh[r];
            }
            dm[(size_t)b * DEC_NF + c] = (float)(dmean * inv_hw);
        }
    }
    if (q == 0) {
#pragma unroll
        for (int r = 0; r < DEC_SE_R; ++r) {
            if (dfc0) dfc0[r * DEC_NF + c] = (float)a0[r];
            if (dfc2) dfc2[c * DEC_SE_R + r] = (float)a2[r];
        }
    }
}

// dT[p][c] = dxn[p][c] * gate[b][c] + dm[b][c]   (two roundings)
__global__ void __launch_bounds__(256) k_dect_dt(const float* __restrict__ dxn, const float* __restrict__ gate, const float* __restrict__ dm,
                                                 float* __restrict__ out, size_t npix, int B) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // one float4 of a pixel's 64 channels
    if (i >= (size_t)B * npix * 16) return;
    const size_t pix = i >> 4; const int c4 = (int)(i & 15) * 4;
    const int b = (int)(pix / npix);
    const F4 d = *(const F4*)(dxn + pix * DEC_NF + c4), g = *(const F4*)(gate + (size_t)b * DEC_NF + c4), m = *(const F4*)(dm + (size_t)b * DEC_NF + c4);
    F4 v = d * g;
    v = v + m;
    *(F4*)(out + pix * DEC_NF + c4) = v;
}
// 32 channels of (pixels, 64) rows at channel offset `off`: G = (G + (A2 ? A2[.][0 .. 31] : 0)) where the saved post-ReLU value is > 0, else 0
__global__ void __launch_bounds__(256) k_dect_mask(float* __restrict__ G, const float* __restrict__ A2, const float* __restrict__ act, int off, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // one float4 of a pixel's 32 channels
    if (i >= n * 8) return;
    const size_t pix = i >> 3; const int c4 = (int)(i & 7) * 4;
    F4 v = *(const F4*)(G + pix * DEC_NF + off + c4);
    if (A2) v = v + *(const F4*)(A2 + pix * DEC_NF + c4);
    const F4 s = *(const F4*)(act + pix * DEC_NF + off + c4);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = s[k] > 0.f ? v[k] : 0.f;
    *(F4*)(G + pix * DEC_NF + off + c4) = v;
}
// out = ((a + b) + c) + d over n floats (a multiple of 4); c, d may be NULL
__global__ void __launch_bounds__(256) k_dect_add(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                  const float* __restrict__ d, float* __restrict__ out, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    F4 v = ((const F4*)a)[i] + ((const F4*)b)[i];
    if (c) v = v + ((const F4*)c)[i];
    if (d) v = v + ((const F4*)d)[i];
    ((F4*)out)[i] = v;
}
// The row gradient: columns 0 .. 11 zero, 12 .. 38 from the 27 channels of GR (pixels, 32); columns from 39 on are left alone.
__global__ void __launch_bounds__(256) k_dect_rows(const float* __restrict__ GR, float* __restrict__ rows, int ld, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 39) return;
    const size_t pix = i / 39; const int c = (int)(i - pix * 39);
    rows[pix * ld + c] = c < 12 ? 0.f : GR[pix * 32 + (c - 12)];
}

// The fold's backward: from dWf (12, 64, 9) and dbf (12)
//   d up_w[4m+s][ci][tap] = sum_o out_w[o][m] dWf[3s+o][ci][tap],   d up_b[4m+s] = sum_o out_w[o][m] dbf[3s+o],
//   d out_w[o][m] = sum_{s,ci,tap} dWf[3s+o][ci][tap] up_w[4m+s][ci][tap] + sum_s dbf[3s+o] up_b[4m+s],   d out_b[o] = sum_s dbf[3s+o],
// each in double in the order written, rounded once.  One thread per output element: 256*576 + 256 + 192 + 3.
__global__ void __launch_bounds__(256) k_dect_fold_back(const float* __restrict__ dWf, const float* __restrict__ dbf, const float* __restrict__ up_w,
                                                        const float* __restrict__ up_b, const float* __restrict__ out_w, float* __restrict__ d_up_w,
                                                        float* __restrict__ d_up_b, float* __restrict__ d_out_w, float* __restrict__ d_out_b) {
    const int NW = 256 * DEC_NF * 9;
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i < NW) {
        if (!d_up_w) return;
        const int r = i % (DEC_NF * 9), ch = i / (DEC_NF * 9), m = ch >> 2, s = ch & 3;
        double acc = 0.0;
        for (int o = 0; o < 3; ++o) acc += (double)out_w[o * DEC_NF + m] * (double)dWf[(3 * s + o) * DEC_NF * 9 + r];
        d_up_w[i] = (float)acc;
        return;
    }
    i -= NW;
    if (i < 256) {
        if (!d_up_b) return;
        const int m = i >> 2, s = i & 3;
        double acc = 0.0;
        for (int o = 0; o < 3; ++o) acc += (double)out_w[o * DEC_NF + m] * (double)dbf[3 * s + o];
        d_up_b[i] = (float)acc;
        return;
    }
    i -= 256;
    if (i < 3 * DEC_NF) {
        if (!d_out_w) return;
        const int o = i / DEC_NF, m = i % DEC_NF;
        double acc = 0.0;
        for (int s = 0; s < 4; ++s)
            for (int r = 0; r < DEC_NF * 9; ++r) acc += (double)dWf[(3 * s + o) * DEC_NF * 9 + r] * (double)up_w[(size_t)(4 * m + s) * DEC_NF * 9 + r];
        for (int s = 0; s < 4; ++s) acc += (double)dbf[3 * s + o] * (double)up_b[4 * m + s];
        d_out_w[i] = (float)acc;
        return;
    }
    i -= 3 * DEC_NF;
    if (i < 3 && d_out_b) {
        double acc = 0.0;
        for (int s = 0; s < 4; ++s) acc += (double)dbf[3 * s + i];
        d_out_b[i] = (float)acc;
    }
}

// ---- the backward's workspace ---------------------------------------------------------------------------------------------------
struct DectWs { size_t G12, GXU, DX, GT, GX3, GAB, GX2, GA2, GX1, GR, dm, psum, psum2, dWf, dbf, dwp, dwp2, total; int ngrp, ng2; size_t dwp_floats; };
static DectWs dect_ws(int B, int H, int W) {
    DectWs w{};
    const size_t n = (size_t)B * H * W, act = sizeof(float) * n * DEC_NF;
    w.ngrp = (int)(((size_t)H * W + DECT_PG - 1) / DECT_PG);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
    w.G12 = take(sizeof(float) * n * 16);
    w.GXU = take(act); w.DX = take(act); w.GT = take(act); w.GX3 = take(act); w.GAB = take(act);
    w.GX2 = take(act); w.GA2 = take(act); w.GX1 = take(act);
    w.GR = take(sizeof(float) * n * 32);
    w.dm = take(sizeof(float) * (size_t)B * DEC_NF);
    w.psum = take(sizeof(double) * (size_t)B * w.ngrp * 2 * 64);
    w.ng2 = (w.ngrp + DECT_R2 - 1) / DECT_R2;
    w.psum2 = take(sizeof(double) * (size_t)B * w.ng2 * 2 * 64);
    w.dWf = take(sizeof(float) * 12 * DEC_NF * 9);
    w.dbf = take(sizeof(float) * 16);
    // the largest weight gradient's partials: every layer's plan has at most min(256, rows) slabs
    size_t pmax = 0, p2max = 0;
    const int dims[5][2] = {{12, DEC_NF}, {DEC_NF, DEC_NF + 2 * DEC_G}, {DEC_G, DEC_NF + DEC_G}, {DEC_G, DEC_NF}, {DEC_NF, GDB_CFR + GDB_CV}};
    for (const auto& d : dims) {
        int tg, nslab, rps;
        dect_dw_plan(d[0], d[1], B * H, &tg, &nslab, &rps);
        const size_t wn = (size_t)d[0] * d[1] * 9;
        if (wn * nslab > pmax) pmax = wn * nslab;
        const size_t ng = (size_t)(nslab + DECT_R1 - 1) / DECT_R1;
        if (wn * ng > p2max) p2max = wn * ng;
    }
    w.dwp_floats = pmax;
    w.dwp = take(sizeof(float) * pmax);
    w.dwp2 = take(sizeof(double) * p2max);
    w.total = o;
    return w;
}

extern "C" int gdb_decoder_train_backward_bytes(const GdbConfig* cfg, const GdbFrame* shape, int32_t num_layers, size_t* out_bytes) {
    int rc = dect_check(cfg, num_layers, GDB_PREC_F32); if (rc) return rc;
    rc = dect_check_shape(cfg, shape); if (rc) return rc;
    if (!out_bytes) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    *out_bytes = dect_ws(shape->B, shape->H, shape->W).total;
    return GDB_OK;
}

static int dect_dw(const DectWs& ws, char* wsb, DectDw a, int B, int H, int W, float* out, hipStream_t st) {
    int tg, nslab, rps;
    a.B = B; a.H = H; a.W = W; a.rows = B * H;
    dect_dw_plan(a.M, a.N, a.rows, &tg, &nslab, &rps);
    a.nmt = (a.M + 15) / 16; a.nnt = (a.N + 15) / 16; a.nslab = nslab; a.rps = rps;
    a.nwaves = a.nmt * a.nnt * (9 / tg) * nslab;
    a.part = (float*)(wsb + ws.dwp);
    const size_t wn = (size_t)a.M * a.N * 9;
    if (wn * nslab > ws.dwp_floats) return gdb_fail(GDB_E_WORKSPACE, "weight-gradient partials exceed the workspace plan");
    const dim3 grid((unsigned)((a.nwaves + 3) / 4));
    if (tg == 9) hipLaunchKernelGGL(k_dect_dw<9>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_dect_dw<3>, grid, dim3(256), 0, st, a);
    LAUNCH_CHECK("k_dect_dw");
    const int ng = (nslab + DECT_R1 - 1) / DECT_R1;
    double* p2 = (double*)(wsb + ws.dwp2);
    hipLaunchKernelGGL(k_dect_reduce1, dim3((unsigned)((wn * ng + 255) / 256)), dim3(256), 0, st, a.part, p2, wn, nslab, ng);
    LAUNCH_CHECK("k_dect_reduce1");
    hipLaunchKernelGGL(k_dect_reduce2, dim3((unsigned)((wn + 255) / 256)), dim3(256), 0, st, p2, out, wn, ng);
    LAUNCH_CHECK("k_dect_reduce2");
    return GDB_OK;
}

// d_tensors: the parameters (device, state-dict order; the fold's backward reads up.0 and out_conv).  d_grads: 2 + 5 num_layers + 4
// pointers in the same order, any of them NULL, or d_grads itself NULL.  d_g_rows (B H W, ld_g_rows) may be NULL.
extern "C" int gdb_decoder_train_backward(const GdbConfig* cfg, const GdbFrame* shape, const float* d_bundle_feat, int32_t ld_bundle_feat,
                                          const float* d_packed, int32_t num_layers, int32_t precision, const float* const* d_tensors,
                                          const void* d_saved, size_t saved_bytes, const float* d_g_rgb_c, void* d_ws, size_t ws_bytes,
                                          float* const* d_grads, float* d_g_rows, int32_t ld_g_rows, void* stream_) {
    int rc = dect_check(cfg, num_layers, precision); if (rc) return rc;
    rc = dect_check_shape(cfg, shape); if (rc) return rc;
    const int B = shape->B, H = shape->H, W = shape->W, L = num_layers;
    const int Q = 3 * cfg->bundle_size * cfg->bundle_size + GDB_CFR + GDB_CV, cin0 = GDB_CFR + GDB_CV;
    if (ld_bundle_feat < Q) return gdb_fail(GDB_E_SHAPE, "bundle_feat row stride %d < %d channels", ld_bundle_feat, Q);
    if (d_g_rows && ld_g_rows < Q) return gdb_fail(GDB_E_SHAPE, "row-gradient stride %d < %d channels", ld_g_rows, Q);
    if ((size_t)H * W * (size_t)(ld_bundle_feat > DEC_NF ? ld_bundle_feat : DEC_NF) >= ((size_t)1 << 30))
        return gdb_fail(GDB_E_SHAPE, "bundle map too large for the decoder's 32-bit staging byte offsets");
    if (!d_bundle_feat || !d_packed || !d_tensors || !d_saved || !d_g_rgb_c || !d_ws) return gdb_fail(GDB_E_BADARG, "NULL pointer");
    const int nt = 2 + 5 * L + 4;
    for (int i = nt - 4; i < nt - 1; ++i)
        if (!d_tensors[i]) return gdb_fail(GDB_E_BADARG, "decoder tensor %d is NULL", i);
    const DectSaved sv = dect_saved(B, H, W, L);
    if (saved_bytes < sv.total) return gdb_fail(GDB_E_WORKSPACE, "decoder saved buffer %zu B < required %zu B", saved_bytes, sv.total);
    const DectWs ws = dect_ws(B, H, W);
    if (ws_bytes < ws.total) return gdb_fail(GDB_E_WORKSPACE, "decoder backward workspace %zu B < required %zu B", ws_bytes, ws.total);
    const DecLayout LY = dec_layout(L, 2);
    const DectPacked PK = dect_packed(LY, L);
    hipStream_t st = (hipStream_t)stream_;
    char* wsb = (char*)d_ws; const char* svb = (const char*)d_saved;
    auto F = [&](size_t off) { return (float*)(wsb + off); };
    auto S = [&](size_t off) { return (const float*)(svb + off); };
    auto grad = [&](int i) -> float* { return d_grads ? d_grads[i] : nullptr; };
    const size_t n = (size_t)B * H * W, npix = (size_t)H * W;
    const unsigned eb16 = (unsigned)((n * 16 + 255) / 256);
    double* psum = (double*)(wsb + ws.psum); double* psum2 = (double*)(wsb + ws.psum2);
    auto conv = [&](const float* in, int in_stride, int in_off, int cin, const float* w, float* out, int out_stride, int cout) {
        ConvArgs a{};
        a.in = in; a.in_stride = in_stride; a.in_off = in_off; a.cin = cin; a.w = w;
        a.out = out; a.out_stride = out_stride; a.out_off = 0; a.cout = cout;
        return gdb_dec_conv_on(a, B, H, W, st);
    };
#define RC(x) do { rc = (x); if (rc) return rc; } while (0)
    // the folded stage
    hipLaunchKernelGGL(k_dect_unshuffle, dim3(eb16), dim3(256), 0, st, d_g_rgb_c, F(ws.G12), B, H, W);
    LAUNCH_CHECK("k_dect_unshuffle");
    if (grad(nt - 4) || grad(nt - 3) || grad(nt - 2) || grad(nt - 1)) {
        DectDw a{};
        a.dY = F(ws.G12); a.ys = 16; a.yo = 0; a.M = 12;
        a.X1 = S(sv.xu); a.s1 = DEC_NF; a.o1 = 0; a.nsplit = DEC_NF; a.X2 = a.X1; a.s2 = DEC_NF; a.o2 = 0; a.N = DEC_NF;
        RC(dect_dw(ws, wsb, a, B, H, W, F(ws.dWf), st));
        hipLaunchKernelGGL(k_dect_psum, dim3((unsigned)(B * ws.ngrp)), dim3(256), 0, st, F(ws.G12), 16, 0, (const float*)nullptr, 12, npix, ws.ngrp, psum);
        LAUNCH_CHECK("k_dect_psum");
        hipLaunchKernelGGL(k_dect_psum2, dim3((unsigned)(B * ws.ng2)), dim3(128), 0, st, (const double*)psum, ws.ngrp, ws.ng2, psum2);
        LAUNCH_CHECK("k_dect_psum2");
        hipLaunchKernelGGL(k_dect_bias, dim3(1), dim3(256), 0, st, (const double*)psum2, B * ws.ng2, 12, F(ws.dbf));
        LAUNCH_CHECK("k_dect_bias");
        hipLaunchKernelGGL(k_dect_fold_back, dim3((unsigned)((256 * DEC_NF * 9 + 256 + 3 * DEC_NF + 3 + 255) / 256)), dim3(256), 0, st, F(ws.dWf),
                           F(ws.dbf), d_tensors[nt - 4], d_tensors[nt - 3], d_tensors[nt - 2], grad(nt - 4), grad(nt - 3), grad(nt - 2), grad(nt - 1));
        LAUNCH_CHECK("k_dect_fold_back");
    }
    RC(conv(F(ws.G12), 16, 0, 12, d_packed + PK.up_t, F(ws.GXU), DEC_NF, DEC_NF));
    // the blocks, in reverse
    const float* dxn = F(ws.GXU);
    for (int b = L - 1; b >= 0; --b) {
        float* const* g = d_grads ? d_grads + 2 + 5 * b : nullptr;
        const float* x = S(sv.x[b]); const float* ab = S(sv.ab[b]); const float* T = S(sv.T[b]); const float* gate = S(sv.gate[b]);
        hipLaunchKernelGGL(k_dect_psum, dim3((unsigned)(B * ws.ngrp)), dim3(256), 0, st, dxn, DEC_NF, 0, T, DEC_NF, npix, ws.ngrp, psum);
        LAUNCH_CHECK("k_dect_psum");
        hipLaunchKernelGGL(k_dect_psum2, dim3((unsigned)(B * ws.ng2)), dim3(128), 0, st, (const double*)psum, ws.ngrp, ws.ng2, psum2);
        LAUNCH_CHECK("k_dect_psum2");
        hipLaunchKernelGGL(k_dect_se, dim3(1), dim3(256), 0, st, (const double*)psum2, ws.ng2, B, 1.0 / (double)npix, d_packed + LY.blk[b][3], d_packed + LY.blk[b][4],
                           gate, F(ws.dm), g ? g[3] : nullptr, g ? g[4] : nullptr);
        LAUNCH_CHECK("k_dect_se");
        hipLaunchKernelGGL(k_dect_dt, dim3(eb16), dim3(256), 0, st, dxn, gate, F(ws.dm), F(ws.GT), npix, B);
        LAUNCH_CHECK("k_dect_dt");
        // conv3: 64 -> [x | a | b]
        RC(conv(F(ws.GT), DEC_NF, 0, DEC_NF, d_packed + PK.blk_t[b][0], F(ws.GX3), DEC_NF, DEC_NF));
        RC(conv(F(ws.GT), DEC_NF, 0, DEC_NF, d_packed + PK.blk_t[b][1], F(ws.GAB), DEC_NF, DEC_NF));
        if (g && g[2]) {
            DectDw a{};
            a.dY = F(ws.GT); a.ys = DEC_NF; a.yo = 0; a.M = DEC_NF;
            a.X1 = x; a.s1 = DEC_NF; a.o1 = 0; a.nsplit = DEC_NF; a.X2 = ab; a.s2 = DEC_NF; a.o2 = 0; a.N = DEC_NF + 2 * DEC_G;
            RC(dect_dw(ws, wsb, a, B, H, W, g[2], st));
        }
        // conv2: db = ReLU mask of b on GAB[:, 32 .. 63]; 32 -> [x | a]
        hipLaunchKernelGGL(k_dect_mask, dim3((unsigned)((n * 8 + 255) / 256)), dim3(256), 0, st, F(ws.GAB), (const float*)nullptr, ab, DEC_G, n);
        LAUNCH_CHECK("k_dect_mask");
        RC(conv(F(ws.GAB), DEC_NF, DEC_G, DEC_G, d_packed + PK.blk_t[b][2], F(ws.GX2), DEC_NF, DEC_NF));
        RC(conv(F(ws.GAB), DEC_NF, DEC_G, DEC_G, d_packed + PK.blk_t[b][3], F(ws.GA2), DEC_NF, DEC_G));
        if (g && g[1]) {
            DectDw a{};
            a.dY = F(ws.GAB); a.ys = DEC_NF; a.yo = DEC_G; a.M = DEC_G;
            a.X1 = x; a.s1 = DEC_NF; a.o1 = 0; a.nsplit = DEC_NF; a.X2 = ab; a.s2 = DEC_NF; a.o2 = 0; a.N = DEC_NF + DEC_G;
            RC(dect_dw(ws, wsb, a, B, H, W, g[1], st));
        }
        // conv1: da = ReLU mask of a on (conv3's + conv2's gradient of a); 32 -> x
        hipLaunchKernelGGL(k_dect_mask, dim3((unsigned)((n * 8 + 255) / 256)), dim3(256), 0, st, F(ws.GAB), (const float*)F(ws.GA2), ab, 0, n);
        LAUNCH_CHECK("k_dect_mask");
        RC(conv(F(ws.GAB), DEC_NF, 0, DEC_G, d_packed + PK.blk_t[b][4], F(ws.GX1), DEC_NF, DEC_NF));
        if (g && g[0]) {
            DectDw a{};
            a.dY = F(ws.GAB); a.ys = DEC_NF; a.yo = 0; a.M = DEC_G;
            a.X1 = x; a.s1 = DEC_NF; a.o1 = 0; a.nsplit = DEC_NF; a.X2 = x; a.s2 = DEC_NF; a.o2 = 0; a.N = DEC_NF;
            RC(dect_dw(ws, wsb, a, B, H, W, g[0], st));
        }
        // dx_b = ((dxn + GX3) + GX2) + GX1
        hipLaunchKernelGGL(k_dect_add, dim3(eb16), dim3(256), 0, st, dxn, (const float*)F(ws.GX3), (const float*)F(ws.GX2), (const float*)F(ws.GX1),
                           F(ws.DX), n * 16);
        LAUNCH_CHECK("k_dect_add");
        dxn = F(ws.DX);
    }
    // shallow: block 0's gradient + the global residual; in_conv
    float* GS = F(ws.GT);
    hipLaunchKernelGGL(k_dect_add, dim3(eb16), dim3(256), 0, st, dxn, (const float*)F(ws.GXU), (const float*)nullptr, (const float*)nullptr, GS, n * 16);
    LAUNCH_CHECK("k_dect_add");
    if (grad(0)) {
        DectDw a{};
        a.dY = GS; a.ys = DEC_NF; a.yo = 0; a.M = DEC_NF;
        a.X1 = d_bundle_feat; a.s1 = ld_bundle_feat; a.o1 = Q - cin0; a.nsplit = cin0; a.X2 = a.X1; a.s2 = a.s1; a.o2 = a.o1; a.N = cin0;
        RC(dect_dw(ws, wsb, a, B, H, W, grad(0), st));
    }
    if (grad(1)) {
        hipLaunchKernelGGL(k_dect_psum, dim3((unsigned)(B * ws.ngrp)), dim3(256), 0, st, (const float*)GS, DEC_NF, 0, (const float*)nullptr, DEC_NF, npix,
                           ws.ngrp, psum);
        LAUNCH_CHECK("k_dect_psum");
        hipLaunchKernelGGL(k_dect_psum2, dim3((unsigned)(B * ws.ng2)), dim3(128), 0, st, (const double*)psum, ws.ngrp, ws.ng2, psum2);
        LAUNCH_CHECK("k_dect_psum2");
        hipLaunchKernelGGL(k_dect_bias, dim3(1), dim3(256), 0, st, (const double*)psum2, B * ws.ng2, DEC_NF, grad(1));
        LAUNCH_CHECK("k_dect_bias");
    }
    if (d_g_rows) {
        RC(conv(GS, DEC_NF, 0, DEC_NF, d_packed + PK.in_t, F(ws.GR), 32, cin0));
        hipLaunchKernelGGL(k_dect_rows, dim3((unsigned)((n * 39 + 255) / 256)), dim3(256), 0, st, (const float*)F(ws.GR), d_g_rows, ld_g_rows, n);
        LAUNCH_CHECK("k_dect_rows");
    }
#undef RC
    return GDB_OK;
}
