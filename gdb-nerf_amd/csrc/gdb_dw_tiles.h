// The weight-gradient engine of the training kernels (k_mlp_bwd, k_stage_nerf<C, true>): every product dW = dY^T [X | 1] of a
// network is cut into 16 x 16 output tiles that go round the four waves of a persistent workgroup.  Per tile of samples the matrix
// cores add dY^T X (v_mfma_f32_16x16x4_f32, K = the tile's rows) from the kernel's LDS image into accumulator registers that live
// across all tiles of the workgroup; a bias gradient is the column of ones behind X.  After its last tile the workgroup writes ONE
// partial in the packed weights' layout, and dw_reduce adds the partials in workgroup order.  No atomics: the sum order is fixed by
// (grid, tile size) alone.
// A kernel keeps its own product list, LDS map and __constant__ table; the descriptor, the table builder and the loops are here.
#pragma once
#include "gdb_internal.h"

struct DwTile {
    int dy, ldy, M, m0;      // dY in LDS: offset, row stride, columns in use, first column of this tile
    int x, ldx, Nw, n0;      // X in LDS: offset of its first column, row stride, columns in use, first column of this tile
    int xone;                // LDS offset of the ones column (column Nw of the product: the bias), -1 without bias
    int perview;             // rows: one per (view, sample), else one per sample
    int w, ldw, b;           // packed section: offset of dW's element (0, 0) of this product, its row stride, bias offset (-1: none)
};
template <int SLOTS> struct DwTable { DwTile t[SLOTS]; int n; };

// One product, before it is cut into tiles (fields as DwTile's).
struct DwProduct { int dy, ldy, M, x, ldx, Nw, xone, perview, w, ldw, b; };

// n counts every tile, also those past SLOTS: the kernels static_assert on it.
template <int SLOTS, int N> constexpr DwTable<SLOTS> dw_make_table(const DwProduct (&prods)[N]) {
    DwTable<SLOTS> T{};
    for (int i = 0; i < SLOTS; ++i) { T.t[i] = DwTile{}; T.t[i].xone = -1; T.t[i].b = -1; }
    int n = 0;
    for (int p = 0; p < N; ++p) {
        const DwProduct& q = prods[p];
        const int cols = q.Nw + (q.xone >= 0 ? 1 : 0);
        for (int m0 = 0; m0 < q.M; m0 += 16)
            for (int n0 = 0; n0 < cols; n0 += 16) {
                if (n < SLOTS) T.t[n] = DwTile{q.dy, q.ldy, q.M, m0, q.x, q.ldx, q.Nw, n0, q.xone, q.perview, q.w, q.ldw, q.b};
                ++n;
            }
    }
    T.n = n;
    return T;
}

#ifdef __HIPCC__
// dW += dY^T [X | 1] of one tile of samples: wave w owns output tiles w, w + 4, ...  rows_perview / rows_shared = the LDS rows (a
// multiple of 4) of the per-(view, sample) and of the per-sample arrays.
template <int PER_WAVE, int SLOTS>
__device__ __forceinline__ void dw_accumulate(const DwTable<SLOTS>& table, const float* lds, int rows_perview, int rows_shared,
                                              f32x4 (&acc)[PER_WAVE], int wave, int lane) {
    const int li = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int q = 0; q < PER_WAVE; ++q) {
        const DwTile& d = table.t[4 * q + wave];
        const int rows = d.perview ? rows_perview : rows_shared;
        const int m = d.m0 + li, nn = d.n0 + li;
        const bool mok = m < d.M;
        const bool nok = nn < d.Nw || (nn == d.Nw && d.xone >= 0);
        const int ao = d.dy + (mok ? m : 0);
        const int bo = nn < d.Nw ? d.x + nn : (nok ? d.xone : d.x);
#pragma nounroll
        for (int k = 0; k < rows; k += 4) {
            float a = lds[ao + (k + kq) * d.ldy];
            float b = lds[bo + (k + kq) * d.ldx];
            a = mok ? a : 0.f;
            b = nok ? b : 0.f;
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[q], 0, 0, 0);
        }
    }
}

// Every wave's tiles into the workgroup's partial, which the caller has zeroed (pad slots, products that got no rows).
template <int PER_WAVE, int SLOTS>
__device__ __forceinline__ void dw_store_partial(const DwTable<SLOTS>& table, float* part, const f32x4 (&acc)[PER_WAVE],
                                                 int wave, int lane) {
    const int col = lane & 15, rq = lane >> 4;
#pragma unroll
    for (int q = 0; q < PER_WAVE; ++q) {
        const DwTile& d = table.t[4 * q + wave];
        const int nn = d.n0 + col;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = d.m0 + 4 * rq + e;
            if (m < d.M) {
                if (nn < d.Nw) part[d.w + m * d.ldw + nn] = acc[q][e];
                else if (nn == d.Nw && d.b >= 0) part[d.b + m] = acc[q][e];
            }
        }
    }
}

// Sum of the partials in workgroup order (fixed: bit-identical from run to run), one lane per float.  The body of each user's reduce
// kernel, a __global__ of its own as the bodies of gdb_costreg_body.h and gdb_costvol_body.h have.
__device__ __forceinline__ void dw_reduce(const float* __restrict__ partials, int nparts, int floats, float* __restrict__ out) {
    int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= floats) return;
    // a double accumulator: a small batch is one tile per workgroup, so this sum IS the sum over samples then, and a sequential fp32
    // chain over a few hundred cancelling terms loses against the blocked sums of a CPU GEMM (seen on sigma.0.bias: 3 x the bound)
    double s = 0.0;
    for (int w = 0; w < nparts; ++w) s += (double)partials[(size_t)w * floats + o];
    out[o] = (float)s;
}
#endif
