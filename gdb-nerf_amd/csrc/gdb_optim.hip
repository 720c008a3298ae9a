// The optimiser step of the training loop as ONE library call: clip_grad_value_ + Adam / AdamW over any number of fp32 tensors, for
// gfx950.  The definition is the header's (include/gdb_nerf_hip.h, "the optimiser step"); this file is how it is computed.
//
// * Why: the training recipe puts every parameter in a param group of its own (136 tensors for dtu_pretrain, median 64 elements), so
//   a per-group optimiser is a run of tiny launches per tensor.  Here a launch takes a BY-VALUE table of up to OPT_TABLE tensors in its
//   kernel arguments: no device-resident table (gradient addresses change every step under zero_grad(set_to_none=True)), no upload,
//   no workspace, no host synchronisation.  ceil(tensors / OPT_TABLE) launches per call.
// * Work split: a workgroup of OPT_THREADS lanes owns ONE chunk of OPT_CHUNK consecutive elements of ONE tensor.  It finds its tensor
//   by a binary search of the table's chunk-count prefix with blockIdx.x: every value in it is wave-uniform, so the table is read
//   through scalar loads of the kernel-argument segment and nothing is parked in private memory.
// * Access: where the four base pointers are 16-byte aligned (a chunk starts at a multiple of OPT_CHUNK floats, so the chunk starts
//   are then aligned too) a lane moves 16 bytes per array per access, lane i next to lane i + 1; a tail of fewer than four elements
//   and every tensor that is only 4-byte aligned (a view at an odd element offset) go one float per lane.  The choice is per tensor,
//   hence wave-uniform.  No LDS, no atomics, no cross-lane work: every element is read and written by exactly one lane, so two calls
//   from the same state give the same bits.
// * Arithmetic: fp32, one rounding per step in the header's order (the translation unit is built with -ffp-contract=off; hipcc's
//   fp32 divide and square root are correctly rounded by default).  The per-tensor scalars are formed on the host in double and
//   rounded to float once, as torch does with a Python-number step count.
#include "gdb_internal.h"

#include <math.h>

#define OPT_THREADS 256
#define OPT_CHUNK 2048   // elements per workgroup: two 16-byte accesses per lane and array
#define OPT_TABLE 48     // tensors per launch: sizeof(OptTable) + the two scalars stay inside the 4 KB of kernel arguments assumed
#define OPT_MAX_CHUNKS 0x7fffffffLL   // chunks per launch (the grid's x extent) at most

struct OptHyper {
    float omb1;        // 1 - beta1
    float beta2;
    float omb2;        // 1 - beta2
    float eps;
    float wd;          // weight_decay (Adam with L2: g += wd p)
    float decay;       // 1 - lr weight_decay (AdamW: p *= decay)
    float step_size;   // lr / (1 - beta1^t)
    float bc2_sqrt;    // sqrt(1 - beta2^t)
};

struct OptTable {
    float* p[OPT_TABLE];
    float* g[OPT_TABLE];
    float* m[OPT_TABLE];
    float* v[OPT_TABLE];
    long long numel[OPT_TABLE];
    OptHyper h[OPT_TABLE];
    int first[OPT_TABLE + 1];   // first[t] = chunks of tensors 0 .. t - 1; every tensor in the table has at least one chunk
    int n;
};
static_assert(sizeof(OptTable) + 2 * sizeof(int) <= 4096, "the by-value table must fit the kernel-argument segment");

// One element.  clip > 0: clamp as torch.clamp does (a NaN fails both comparisons and stays NaN; fminf / fmaxf would return the bound).
__device__ __forceinline__ void opt_element(float& p, float& g, float& m, float& v, const OptHyper& h, float clip, bool decoupled) {
    if (clip > 0.f) g = g < -clip ? -clip : (g > clip ? clip : g);
    float gg = g;
    if (h.wd != 0.f) {
        if (decoupled) p = p * h.decay;
        else gg = g + h.wd * p;
    }
    m = m + (gg - m) * h.omb1;
    v = v * h.beta2;
    v = v + h.omb2 * gg * gg;
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    p = p - h.step_size * (m / denom);
}

__global__ __launch_bounds__(OPT_THREADS) void k_adam_step(const OptTable T, const float clip, const int decoupled) {
    const int c = (int)blockIdx.x;
    int lo = 0, hi = T.n;   // the tensor t with first[t] <= c < first[t + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (T.first[mid] <= c) lo = mid; else hi = mid;
    }
    const int t = lo;
    const long long start = (long long)(c - T.first[t]) * OPT_CHUNK;
    const long long left = T.numel[t] - start;
    const int len = left < (long long)OPT_CHUNK ? (int)left : OPT_CHUNK;   // >= 1: the grid holds ceil(numel / OPT_CHUNK) chunks of t
    const OptHyper h = T.h[t];
    float* __restrict__ p = T.p[t] + start;
    float* __restrict__ g = T.g[t] + start;
    float* __restrict__ m = T.m[t] + start;
    float* __restrict__ v = T.v[t] + start;
    const bool wide = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    int done = 0;   // elements [0, done) are taken four per lane
    if (wide) {
        const int nv = len >> 2;
        done = nv << 2;
#pragma unroll
        for (int r = 0; r < OPT_CHUNK / 4 / OPT_THREADS; ++r) {
            const int i = (int)threadIdx.x + r * OPT_THREADS;
            if (i >= nv) break;
            f32x4 p4 = ((const f32x4*)p)[i], g4 = ((const f32x4*)g)[i], m4 = ((const f32x4*)m)[i], v4 = ((const f32x4*)v)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pe = p4[k], ge = g4[k], me = m4[k], ve = v4[k];
                opt_element(pe, ge, me, ve, h, clip, decoupled != 0);
                p4[k] = pe; g4[k] = ge; m4[k] = me; v4[k] = ve;
            }
            ((f32x4*)p)[i] = p4; ((f32x4*)m)[i] = m4; ((f32x4*)v)[i] = v4;
            if (clip > 0.f) ((f32x4*)g)[i] = g4;
        }
    }
    for (int i = done + (int)threadIdx.x; i < len; i += OPT_THREADS) {
        float pe = p[i], ge = g[i], me = m[i], ve = v[i];
        opt_element(pe, ge, me, ve, h, clip, decoupled != 0);
        p[i] = pe; m[i] = me; v[i] = ve;
        if (clip > 0.f) g[i] = ge;
    }
}

static int opt_launch(const OptTable& T, float clip, int decoupled, hipStream_t stream) {
    hipLaunchKernelGGL(k_adam_step, dim3((unsigned)T.first[T.n]), dim3(OPT_THREADS), 0, stream, T, clip, decoupled);
    LAUNCH_CHECK("k_adam_step");
    return GDB_OK;
}

extern "C" int gdb_adam_step(int32_t n, float* const* d_param, float* const* d_grad, float* const* d_exp_avg, float* const* d_exp_avg_sq,
                             const int64_t* numel, const double* lr, const double* beta1, const double* beta2, const double* eps,
                             const double* weight_decay, const int64_t* step, double clip_value, int32_t decoupled, void* stream_) {
    if (n < 0) return gdb_fail(GDB_E_BADARG, "adam_step: %d tensors", (int)n);
    if (n == 0) return GDB_OK;
    if (!d_param || !d_grad || !d_exp_avg || !d_exp_avg_sq || !numel || !lr || !beta1 || !beta2 || !eps || !weight_decay || !step)
        return gdb_fail(GDB_E_BADARG, "adam_step: NULL array");
    // every refusal comes before the first launch: a refused call has changed nothing
    for (int i = 0; i < n; ++i) {
        if (!d_param[i] || !d_grad[i] || !d_exp_avg[i] || !d_exp_avg_sq[i]) return gdb_fail(GDB_E_BADARG, "adam_step: tensor %d: NULL pointer", i);
        if (numel[i] < 0) return gdb_fail(GDB_E_SHAPE, "adam_step: tensor %d: numel %lld", i, (long long)numel[i]);
        if (step[i] < 1) return gdb_fail(GDB_E_BADARG, "adam_step: tensor %d: step %lld (the count after its increment: at least 1)", i, (long long)step[i]);
        if (!(beta1[i] >= 0.0 && beta1[i] < 1.0) || !(beta2[i] >= 0.0 && beta2[i] < 1.0))
            return gdb_fail(GDB_E_BADARG, "adam_step: tensor %d: betas (%g, %g) outside [0, 1)", i, beta1[i], beta2[i]);
        if (((long long)numel[i] + OPT_CHUNK - 1) / OPT_CHUNK > OPT_MAX_CHUNKS)
            return gdb_fail(GDB_E_SHAPE, "adam_step: tensor %d: %lld elements are too many for the launch grid", i, (long long)numel[i]);
    }
    hipStream_t stream = (hipStream_t)stream_;
    const float clip = clip_value > 0.0 ? (float)clip_value : 0.f;
    OptTable T;
    T.n = 0; T.first[0] = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] == 0) continue;
        const long long chunks = ((long long)numel[i] + OPT_CHUNK - 1) / OPT_CHUNK;
        if (T.n == OPT_TABLE || (long long)T.first[T.n] + chunks > OPT_MAX_CHUNKS) {
            const int rc = opt_launch(T, clip, decoupled, stream);
            if (rc != GDB_OK) return rc;
            T.n = 0;
        }
        const int k = T.n;
        T.p[k] = d_param[i]; T.g[k] = d_grad[i]; T.m[k] = d_exp_avg[i]; T.v[k] = d_exp_avg_sq[i];
        T.numel[k] = (long long)numel[i];
        const double bc1 = 1.0 - pow(beta1[i], (double)step[i]), bc2 = 1.0 - pow(beta2[i], (double)step[i]);
        OptHyper& h = T.h[k];
        h.omb1 = (float)(1.0 - beta1[i]); h.beta2 = (float)beta2[i]; h.omb2 = (float)(1.0 - beta2[i]);
        h.eps = (float)eps[i]; h.wd = (float)weight_decay[i]; h.decay = (float)(1.0 - lr[i] * weight_decay[i]);
        h.step_size = (float)(lr[i] / bc1); h.bc2_sqrt = (float)sqrt(bc2);
        T.first[k + 1] = T.first[k] + (int)chunks;
        T.n = k + 1;
    }
    return T.n ? opt_launch(T, clip, decoupled, stream) : GDB_OK;
}
