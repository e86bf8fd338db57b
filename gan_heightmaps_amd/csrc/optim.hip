// The rest of lasagne.updates as fused flat-buffer optimisers: sgd, momentum, nesterov_momentum, adagrad, adadelta,
// adamax, amsgrad (rmsprop / adam live in elementwise.hip and are unchanged).  One kernel template over the rule: one
// float4 of p, g and every state buffer per thread, the ragged tail (n % 4) in the last thread, no LDS, no atomics.
//
// The contract is rmsprop_kernel's / adam_kernel's: lr = hyper[0] and t = hyper[1] + 1 are read on the device (nothing
// step-dependent is baked into a recorded or captured launch); with a loss-scale state attached an overflowed step
// (ls[3] != 0) returns before touching anything, otherwise g is multiplied by 1/S = ls[1].  The step counter of adamax /
// amsgrad is advanced by ghm_adam_tick after the update.
#include "common.h"

namespace {

// hyper-parameters of a launch: the constants (h0, h1, h2 of the ABI) plus what the kernel derives from hyper[]
struct Coef {
    float lr, h0, h1, h2, c;    // c: the bias-corrected step size of adamax / amsgrad
};

// number of fp32 state buffers per rule (GHM_OPT_* order)
__host__ __device__ constexpr int n_state(int rule) {
    return rule == GHM_OPT_SGD ? 0 : rule == GHM_OPT_ADADELTA || rule == GHM_OPT_ADAMAX ? 2 : rule == GHM_OPT_AMSGRAD ? 3 : 1;
}

template <int R>
__device__ __forceinline__ void rule_step(float& p, float g, float& s0, float& s1, float& s2, const Coef& k) {
    if constexpr (R == GHM_OPT_SGD) {
        p -= k.lr * g;
    } else if constexpr (R == GHM_OPT_MOMENTUM) {              // h0 = momentum
        const float v = k.h0 * s0 - k.lr * g;
        s0 = v;
        p += v;
    } else if constexpr (R == GHM_OPT_NESTEROV) {              // h0 = momentum
        const float v = k.h0 * s0 - k.lr * g;
        s0 = v;
        p = p - k.lr * g + k.h0 * v;
    } else if constexpr (R == GHM_OPT_ADAGRAD) {               // h0 = epsilon
        const float a = s0 + g * g;
        s0 = a;
        p -= k.lr * g / sqrtf(a + k.h0);
    } else if constexpr (R == GHM_OPT_ADADELTA) {              // h0 = rho, h1 = epsilon; s0 = accu, s1 = delta_accu
        const float a = k.h0 * s0 + (1.f - k.h0) * g * g;
        const float u = g * sqrtf(s1 + k.h1) / sqrtf(a + k.h1);
        s0 = a;
        p -= k.lr * u;
        s1 = k.h0 * s1 + (1.f - k.h0) * u * u;
    } else if constexpr (R == GHM_OPT_ADAMAX) {                // h0 = beta1, h1 = beta2, h2 = epsilon; s0 = m, s1 = u
        const float m = k.h0 * s0 + (1.f - k.h0) * g;
        const float u = fmaxf(k.h1 * s1, fabsf(g));
        s0 = m;
        s1 = u;
        p -= k.c * m / (u + k.h2);
    } else {                                                   // amsgrad: h0 = beta1, h1 = beta2, h2 = epsilon; s0 = m, s1 = v, s2 = vhat
        const float m = k.h0 * s0 + (1.f - k.h0) * g;
        const float v = k.h1 * s1 + (1.f - k.h1) * g * g;
        const float vh = fmaxf(s2, v);
        s0 = m;
        s1 = v;
        s2 = vh;
        p -= k.c * m / (sqrtf(vh) + k.h2);
    }
}

template <int R>
__global__ __launch_bounds__(256) void opt_update_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ s0, float* __restrict__ s1, float* __restrict__ s2,
                                                         long n, const float* __restrict__ hyper, float h0, float h1, float h2,
                                                         float gscale, const float* __restrict__ ls) {
    constexpr int NS = n_state(R);
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (ls) {                           // {scale, 1/scale, good steps, overflow flag}: skip the update of an overflowed step
        if (ls[3] != 0.f) return;
        gscale *= ls[1];
    }
    Coef k{hyper[0], h0, h1, h2, 0.f};
    if constexpr (R == GHM_OPT_ADAMAX || R == GHM_OPT_AMSGRAD) {
        const float t = hyper[1] + 1.f;                         // t_prev + 1
        k.c = k.lr / (1.f - powf(h0, t));
        if constexpr (R == GHM_OPT_AMSGRAD) k.c *= sqrtf(1.f - powf(h1, t));
    }
    if (i + 3 < n) {
        float pv[4], gv[4], a[4] = {}, b[4] = {}, c[4] = {};
        *reinterpret_cast<float4*>(pv) = *reinterpret_cast<const float4*>(p + i);
        *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(g + i);
        if constexpr (NS > 0) *reinterpret_cast<float4*>(a) = *reinterpret_cast<const float4*>(s0 + i);
        if constexpr (NS > 1) *reinterpret_cast<float4*>(b) = *reinterpret_cast<const float4*>(s1 + i);
        if constexpr (NS > 2) *reinterpret_cast<float4*>(c) = *reinterpret_cast<const float4*>(s2 + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) rule_step<R>(pv[j], gv[j] * gscale, a[j], b[j], c[j], k);
        *reinterpret_cast<float4*>(p + i) = *reinterpret_cast<const float4*>(pv);
        if constexpr (NS > 0) *reinterpret_cast<float4*>(s0 + i) = *reinterpret_cast<const float4*>(a);
        if constexpr (NS > 1) *reinterpret_cast<float4*>(s1 + i) = *reinterpret_cast<const float4*>(b);
        if constexpr (NS > 2) *reinterpret_cast<float4*>(s2 + i) = *reinterpret_cast<const float4*>(c);
    } else {
        for (long e = i; e < n; ++e) {
            float a = NS > 0 ? s0[e] : 0.f, b = NS > 1 ? s1[e] : 0.f, c = NS > 2 ? s2[e] : 0.f;
            rule_step<R>(p[e], g[e] * gscale, a, b, c, k);
            if constexpr (NS > 0) s0[e] = a;
            if constexpr (NS > 1) s1[e] = b;
            if constexpr (NS > 2) s2[e] = c;
        }
    }
}

inline bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

template <int R>
int launch(ghm_ctx* ctx, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n, const float* hyper, float h0,
           float h1, float h2, float grad_scale) {
    hipLaunchKernelGGL((opt_update_kernel<R>), EW_GRID((n + 3) / 4), p, g, s0, s1, s2, (long)n, hyper, h0, h1, h2, grad_scale,
                       (const float*)ctx->ls_state);
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int ghm_opt_update(ghm_ctx* ctx, int32_t rule, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n,
                   const float* hyper, float h0, float h1, float h2, float grad_scale) {
    GHM_CHECK(rule >= GHM_OPT_SGD && rule <= GHM_OPT_AMSGRAD, "ghm_opt_update: unknown rule %d", (int)rule);
    if (n == 0) return 0;
    const int ns = n_state(rule);
    float* s[3] = {s0, s1, s2};
    for (int j = 0; j < 3; ++j)
        GHM_CHECK((j < ns) == (s[j] != nullptr), "ghm_opt_update: rule %d takes %d state buffers (s%d is %s)", (int)rule, ns, j,
                  s[j] ? "set" : "NULL");
    GHM_CHECK(aligned16(p) && aligned16(g) && aligned16(s0) && aligned16(s1) && aligned16(s2),
              "ghm_opt_update: parameter, gradient and state buffers must be 16-byte aligned");
    switch (rule) {
        case GHM_OPT_SGD: return launch<GHM_OPT_SGD>(ctx, p, g, s0, s1, s2, n, hyper, h0, h1, h2, grad_scale);
        case GHM_OPT_MOMENTUM: return launch<GHM_OPT_MOMENTUM>(ctx, p, g, s0, s1, s2, n, hyper, h0, h1, h2, grad_scale);
        case GHM_OPT_NESTEROV: return launch<GHM_OPT_NESTEROV>(ctx, p, g, s0, s1, s2, n, hyper, h0, h1, h2, grad_scale);
        case GHM_OPT_ADAGRAD: return launch<GHM_OPT_ADAGRAD>(ctx, p, g, s0, s1, s2, n, hyper, h0, h1, h2, grad_scale);
        case GHM_OPT_ADADELTA: return launch<GHM_OPT_ADADELTA>(ctx, p, g, s0, s1, s2, n, hyper, h0, h1, h2, grad_scale);
        case GHM_OPT_ADAMAX: return launch<GHM_OPT_ADAMAX>(ctx, p, g, s0, s1, s2, n, hyper, h0, h1, h2, grad_scale);
        default: return launch<GHM_OPT_AMSGRAD>(ctx, p, g, s0, s1, s2, n, hyper, h0, h1, h2, grad_scale);
    }
}

}  // extern "C"
