// The residual-dense decoder's sizes and packed-weight layout, shared by gdb_decoder.hip (the eval-mode decode and the host pack) and
// gdb_decoder_train.hip (the device-side pack and the saved-activation forward), and the one launch sequence both run (dec_phases,
// gdb_decoder.hip) on the buffers a DecBufs names.
#pragma once
#include "gdb_internal.h"

#define DEC_NF 64    // num_feats (network.py:51)
#define DEC_G 32     // growth rate (decoder_rdn.py:27)
#define DEC_PX 34    // pixels per staged row: 32 + halo
#define DEC_CHS 34   // floats per staged pixel: 32 channels of the chunk + 2 (bank spread for the 8-byte reads)
#define DECX_PXD 20  // split-f16 staging: dwords per pixel = 8 (hi halves of a chunk's 16 channels) + 8 (lo halves) + 4 (bank spread for the 16-byte reads)
#define DEC_SE_R 4   // SE bottleneck: 64 / 16

// ---- packed weights -------------------------------------------------------------------------------------------------
// conv_floats(cin, nt): floats of a packed layer of 32 nt output channels (fp32 form pack_conv16 and split-f16 form pack_conv_x alike).
static size_t conv_floats(int cin, int nt) { return (size_t)((cin + 31) / 32) * 9 * 8 * 64 * 2 * nt; }
#define DEC_MAX_LAYERS 16   // dense blocks (decoder_rdn.py:57 takes any count; every config of the reference has 3)
struct DecLayout {
    size_t in_w, in_b, blk[DEC_MAX_LAYERS][5] /* conv1, conv2, conv3, fc0, fc2 */, up_w, up_b;
    size_t in_wx, blkx[DEC_MAX_LAYERS][3], up_wx;  // the same convolutions as split-f16 fragments (pack_conv_x), behind the fp32 ones
    // upscale_factor 4 (bundle_size 4: two up stages, decoder_rdn.py:59-62): the FIRST stage's 64 -> 256 convolution as four 64 -> 64
    // convolutions, one per sub-pixel of its PixelShuffle (fp32 and split-f16 forms, biases); up_w / up_b then hold the SECOND stage folded
    // with out_conv.  Zero-sized at upscale_factor 2.
    size_t u1_w[4], u1_wx[4], u1_b[4];
    size_t total;
};
static DecLayout dec_layout(int nlayers, int bundle_size = 2) {
    DecLayout L{};
    size_t o = 0;
    L.in_w = o; o += conv_floats(27, 2);
    L.in_b = o; o += 64;
    for (int b = 0; b < nlayers; ++b) {
        L.blk[b][0] = o; o += conv_floats(64, 1);
        L.blk[b][1] = o; o += conv_floats(96, 1);
        L.blk[b][2] = o; o += conv_floats(128, 2);
        L.blk[b][3] = o; o += DEC_SE_R * DEC_NF;
        L.blk[b][4] = o; o += DEC_NF * DEC_SE_R;
    }
    L.up_w = o; o += conv_floats(64, 1);
    L.up_b = o; o += 32;
    L.in_wx = o; o += conv_floats(27, 2);
    for (int b = 0; b < nlayers; ++b) {
        L.blkx[b][0] = o; o += conv_floats(64, 1);
        L.blkx[b][1] = o; o += conv_floats(96, 1);
        L.blkx[b][2] = o; o += conv_floats(128, 2);
    }
    L.up_wx = o; o += conv_floats(64, 1);
    if (bundle_size == 4)
        for (int sp = 0; sp < 4; ++sp) {
            L.u1_w[sp] = o; o += conv_floats(64, 2);
            L.u1_wx[sp] = o; o += conv_floats(64, 2);
            L.u1_b[sp] = o; o += 64;
        }
    L.total = (o + 8 * 128 + 63) / 64 * 64;  // + one tap block: the fp32 conv kernel's weight prefetch runs one tap ahead
    return L;
}

// ---- 3x3 convolution ----------------------------------------------------------------------------------------------------
struct ConvArgs {
    const float* in; int in_stride, in_off, cin, nchunk, vec;  // vec: the input rows allow 16-byte loads
    const float* in2; int split;    // 32-channel chunks >= split come from in2 (row stride in_stride, channel 32 (chunk - split))
    const float* w; const float* bias;
    float* out; int out_stride, out_off, cout, relu;
    float* rgb;                     // folded up stage: (B,3,2H,2W) NCHW, channel c = 3 s + o of sub-pixel s = dy*2 + dx
    int up2, up_dy, up_dx;          // first up stage of upscale_factor 4: output pixel (y, x) is written at (2y + up_dy, 2x + up_dx) of a (2H, 2W) map
    // squeeze-excitation folded into the consumer (FUSE kernels; decoder_rdn.py:40,78): the staged input is x = in + fT * gate (+ fS),
    // all (pixels, 64); the workgroup's own pixels of x are also written to fX (the next block's P) when fX is set
    const float* fT; const float* fgate; const float* fS; float* fX;
    float* se_part;                 // SEP kernels (conv3): channel sums of the output per (row, 32-pixel segment)
    unsigned* zero;                 // in_conv: the arrival counters of k_se_gate, cleared for this decode
    int B, H, W, tilesX, tilesY;
    // row window (gdb_decode_rows): the map the kernel runs on is rows [wy0, wy0 + H) of a frame of Hf rows.  `in` holds in_H rows per
    // batch item starting at row in_y0 (in_conv reads the frame-sized bundle rows in place; every other input is window-sized); se_part
    // is frame-sized and receives - like rgb - the rows [own0, own1) of the frame only.  The whole-frame decode: 0, H, H, 0, 0, H.
    int wy0, Hf, in_H, in_y0, own0, own1;
};

// ---- where a decode keeps its activations -----------------------------------------------------------------------------------
// Per dense block b: x = its input (x[0] = in_conv's output, the global residual), ab = [x1 | x2] after ReLU, T = conv3's output, gate =
// its 64 gates per batch item; all (pixels, 64) but gate.  The eval-mode decode points them into its rotating workspace (dec_ws: three
// x, one ab, one T, one gate); the training forward gives every block its own.  xu, when set, receives the up stage's staged input
// x_L + shallow (bundle_size 2), which the eval-mode decode never stores.  part / part2 / count: the squeeze-excitation sums' scratch.
struct DecBufs {
    float* x[DEC_MAX_LAYERS]; float* ab[DEC_MAX_LAYERS]; float* T[DEC_MAX_LAYERS]; float* gate[DEC_MAX_LAYERS];
    float* xu;
    float* part; float* part2; unsigned* count;
};
// k_se_gate's first stage sums groups of DEC_SEG segments: the group count of nseg segments (gdb_decoder.hip).
int gdb_dec_se_groups(int nseg);
// gdb_decode's fp32 launch sequence (dec_phases, phases 0 .. num_layers of the whole frame, bundle_size 2) on the buffers of `bufs`.
int gdb_dec_phases_on(const GdbConfig* cfg, int B, int H, int W, const float* d_bundle_feat, int ld_bundle_feat, const float* d_packed,
                      int num_layers, const DecBufs& bufs, float* d_rgb_c, hipStream_t st);
// One fp32 convolution of a whole (B, H, W) frame on k_conv16 (gdb_decoder.hip): operands from `a`, geometry filled in.
int gdb_dec_conv_on(ConvArgs a, int B, int H, int W, hipStream_t st);
