// Index arithmetic of the training-mode decoder's pack and weight-gradient kernels (gdb_decoder_train.hip), in __host__ __device__
// helpers: tools/check_decoder_train_index.cpp includes this header alone, walks every section and every test shape on the CPU
// (built with -fsanitize=address,undefined) and asserts that each address lies inside its buffer.
#pragma once
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

// ---- index arithmetic (host-checkable) --------------------------------------------------------------------------------------------
// Element idx of a pack_conv16 layer of nchunk 32-channel chunks, [tile mt][chunk][tap 9][g4 2][lane 64][e 4]:
// W[16 mt + (l & 15)][32 chunk + 4 (4 g4 + e) + (l >> 4)][tap].
__host__ __device__ inline void dect_conv16_elem(unsigned idx, int nchunk, int* co, int* ci, int* tap) {
    const int e = idx & 3, l = (idx >> 2) & 63, g4 = (idx >> 8) & 1;
    const unsigned r = idx >> 9;             // (mt * nchunk + ch) * 9 + tap
    const int t = (int)(r % 9u), mc = (int)(r / 9u), ch = mc % nchunk, mt = mc / nchunk;
    *co = 16 * mt + (l & 15);
    *ci = 32 * ch + 4 * (4 * g4 + e) + (l >> 4);
    *tap = t;
}
// Source element of W (cout, cin, 3, 3), or -1 where the packet holds padding.
__host__ __device__ inline long long dect_conv16_src(unsigned idx, int nchunk, int cout, int cin) {
    int co, ci, tap;
    dect_conv16_elem(idx, nchunk, &co, &ci, &tap);
    return (co < cout && ci < cin) ? ((long long)co * cin + ci) * 9 + tap : -1;
}

// Source element of the DATA-GRADIENT form of W (rows, rs, 3, 3): the convolution with the channel roles swapped and the taps flipped,
// restricted to W's input channels [c0, c0 + cout): packed output channel j = W's input channel c0 + j, packed input channel i = W's
// output channel i, tap 8 - tap.  -1 where the packet holds padding.
__host__ __device__ inline long long dect_conv16_src_t(unsigned idx, int nchunk, int cout, int cin, int rs, int c0) {
    int j, i, tap;
    dect_conv16_elem(idx, nchunk, &j, &i, &tap);
    return (j < cout && i < cin) ? ((long long)i * rs + c0 + j) * 9 + (8 - tap) : -1;
}

// Which (tile, tap group, slab) a wave owns, and its rows: host-checkable.
__host__ __device__ inline void dect_dw_wave(int wave, int nmt, int nnt, int ntg, int rps, int rows, int* mt, int* nt, int* tg, int* slab,
                                             int* r0, int* r1) {
    int t = wave;
    *mt = t % nmt; t /= nmt;
    *nt = t % nnt; t /= nnt;
    *tg = t % ntg;
    *slab = t / ntg;
    *r0 = *slab * rps;
    *r1 = *r0 + rps < rows ? *r0 + rps : rows;
}
// Element of the partial buffer a lane writes, or -1 (outside M x N).
__host__ __device__ inline long long dect_dw_part_index(int slab, int M, int N, int mm, int nn, int tap) {
    return (mm < M && nn < N) ? (long long)slab * M * N * 9 + ((long long)mm * N + nn) * 9 + tap : -1;
}
// the weight gradient's split: TG taps per wave (nine for a layer of 16 tiles or more - conv3 - else three: a small layer needs the
// waves), slabs of image rows sized for about 8192 waves (eight per SIMD: a wave's loads are 4 bytes per lane and matrix
// instruction and nothing but other waves hides their latency), at most 256 slabs and at most one per row
__host__ __device__ inline void dect_dw_plan(int M, int N, int rows, int* tg, int* nslab, int* rps) {
    const long long tiles = (long long)((M + 15) / 16) * ((N + 15) / 16);
    *tg = tiles >= 16 ? 9 : 3;
    const long long per = tiles * (9 / *tg);
    long long ns = (8192 + per - 1) / per;
    if (ns > 256) ns = 256;
    if (ns > rows) ns = rows;
    if (ns < 1) ns = 1;
    *rps = (int)((rows + ns - 1) / ns);
    *nslab = (rows + *rps - 1) / *rps;
}

