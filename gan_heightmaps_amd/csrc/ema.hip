// Exponential moving average of a flat parameter buffer, and the exchange of two flat buffers.
//   ghm_ema_update: ema[i] = fl(fl(decay * ema[i]) + fl(c * w[i])), c = (float)(1 - (double)decay) from the host
//   ghm_swap_f32:   a[i] <-> b[i] as 32-bit words (NaN payloads and -0 survive)
// Both have opt_update_kernel's shape (csrc/optim.hip): one float4 per thread, the ragged tail (n % 4) in the last thread,
// 64-bit indices, no LDS, no atomics.  The update keeps the optimisers' loss-scale contract: with a loss-scale state attached
// an overflowed step (ls[3] != 0) returns before touching anything, so a skipped fp16 step leaves the average alone too.
#include "common.h"

// two products and one sum, each rounded on its own (hipcc contracts a * b + c into an fma by default): the float32 numpy
// restatement (tests/ema_ref.py) then gives the same bits
#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ w, long n,
                                                         float decay, float c, const float* __restrict__ ls) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (ls && ls[3] != 0.f) return;     // {scale, 1/scale, good steps, overflow flag}: the optimiser skipped this step
    if (i + 3 < n) {
        float ev[4], wv[4];
        *reinterpret_cast<float4*>(ev) = *reinterpret_cast<const float4*>(ema + i);
        *reinterpret_cast<float4*>(wv) = *reinterpret_cast<const float4*>(w + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[j] = decay * ev[j] + c * wv[j];
        *reinterpret_cast<float4*>(ema + i) = *reinterpret_cast<const float4*>(ev);
    } else {
        for (long e = i; e < n; ++e) ema[e] = decay * ema[e] + c * w[e];
    }
}

__global__ __launch_bounds__(256) void swap_f32_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, long n) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 3 < n) {
        const uint4 av = *reinterpret_cast<const uint4*>(a + i);
        const uint4 bv = *reinterpret_cast<const uint4*>(b + i);
        *reinterpret_cast<uint4*>(a + i) = bv;
        *reinterpret_cast<uint4*>(b + i) = av;
    } else {
        for (long e = i; e < n; ++e) {
            const uint32_t t = a[e];
            a[e] = b[e];
            b[e] = t;
        }
    }
}

inline bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// do [a, a + n) and [b, b + n) floats share a byte?
inline bool overlap(const void* a, const void* b, int64_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)n * 4;
    return x < y + len && y < x + len;
}

}  // namespace

extern "C" {

int ghm_ema_update(ghm_ctx* ctx, float* ema, const float* w, int64_t n, float decay) {
    GHM_CHECK(ctx != nullptr, "ghm_ema_update: no context");
    GHM_CHECK(ema != nullptr && w != nullptr, "ghm_ema_update: ema and w must not be NULL");
    GHM_CHECK(aligned16(ema) && aligned16(w), "ghm_ema_update: ema and w must be 16-byte aligned");
    GHM_CHECK(n >= 0, "ghm_ema_update: n = %lld", (long long)n);
    GHM_CHECK(decay >= 0.f && decay < 1.f, "ghm_ema_update: decay %g is not in [0, 1)", (double)decay);   // (a NaN fails both)
    GHM_CHECK(!overlap(ema, w, n), "ghm_ema_update: ema and w overlap");
    if (n == 0) return 0;
    const float c = (float)(1.0 - (double)decay);
    hipLaunchKernelGGL(ema_update_kernel, EW_GRID((n + 3) / 4), ema, w, (long)n, decay, c, (const float*)ctx->ls_state);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_swap_f32(ghm_ctx* ctx, float* a, float* b, int64_t n) {
    GHM_CHECK(ctx != nullptr, "ghm_swap_f32: no context");
    GHM_CHECK(a != nullptr && b != nullptr, "ghm_swap_f32: a and b must not be NULL");
    GHM_CHECK(aligned16(a) && aligned16(b), "ghm_swap_f32: a and b must be 16-byte aligned");
    GHM_CHECK(n >= 0, "ghm_swap_f32: n = %lld", (long long)n);
    GHM_CHECK(!overlap(a, b, n), "ghm_swap_f32: a and b overlap");
    if (n == 0) return 0;
    hipLaunchKernelGGL(swap_f32_kernel, EW_GRID((n + 3) / 4), reinterpret_cast<uint32_t*>(a), reinterpret_cast<uint32_t*>(b),
                       (long)n);
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
