// Heightmaps of any size from a grid of latent vectors (gan_heightmaps_amd/terrain.py): the DCGAN generator's
// head runs per cell, its s x s maps are laid out (or bilinearly blended) into one seed canvas, and the fully convolutional
// trunk runs over the canvas in row windows.  Two HBM-bound streaming kernels around the trunk's forward pass:
//   seed : canvas seed rows [row0, row0 + rows) -> fp32 [C, rows, s*gx] at the trunk plan's input view;
//   emit : output rows [r0, r0 + n) of the trunk -> a staging buffer, as fp32 CHW or as the uint8 map of
//          util.to_uint8(util.convert_to_rgb(.)).
// No LDS, no reductions.  Lanes run along the canvas columns, 4 per thread where the row geometry allows 16-byte stores.
#include "common.h"

// no fused multiply-adds: the blend and the uint8 map round every product and sum on their own, as the host restatement and
// numpy's float32 evaluation of util.convert_to_rgb do (csrc/texture.hip: the same rule, the same reason)
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

// the cells of one axis that seed coordinate y reads, and their weights: ``two`` is false where one cell holds all the
// weight (mosaic, or bilinear corners clamped onto the same cell), which then weighs exactly 1
struct Cover {
    int a, b;
    float wa, wb;
    bool two;
};

__device__ __forceinline__ Cover ter_cover(int y, int s, int n, int bilinear) {
    Cover c;
    if (!bilinear) {
        c.a = c.b = y / s;
        c.wa = 1.0f;
        c.wb = 0.0f;
        c.two = false;
        return c;
    }
    // u = (y + 0.5) / s - 0.5 in cell coordinates; corners floor(u) and floor(u) + 1, clamped to the grid
    const float u = __fdiv_rn((float)y + 0.5f, (float)s) - 0.5f;
    const float f = floorf(u);
    const int i0 = (int)f;
    const float fy = u - f;
    c.a = min(max(i0, 0), n - 1);
    c.b = min(max(i0 + 1, 0), n - 1);
    c.two = c.a != c.b;
    c.wa = c.two ? 1.0f - fy : 1.0f;
    c.wb = c.two ? fy : 0.0f;
    return c;
}

// out[c][r][x] = sum over the covering cells (i, j) of wy_i wx_j P[i * gx + j][c][y mod s][x mod s], y = row0 + r
template <int VEC>
__global__ __launch_bounds__(256) void ter_seed_kernel(const float* __restrict__ P, long p_nstride, int gy, int gx, int C,
                                                       int s, int row0, int rows, int bilinear, float* __restrict__ out) {
    const int Wc = s * gx;
    const int per_row = Wc / VEC;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)C * rows * per_row) return;
    const int row = (int)(idx / per_row);             // c * rows + r
    const int x0 = (int)(idx - (long)row * per_row) * VEC;
    const int c = row / rows, r = row - c * rows;
    const int y = row0 + r;
    const Cover cy = ter_cover(y, s, gy, bilinear);
    const long cbase = (long)c * s * s + (long)(y % s) * s;
    float v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const int x = x0 + k;
        const Cover cx = ter_cover(x, s, gx, bilinear);
        const long off = cbase + x % s;
        const float* pa = P + (long)cy.a * gx * p_nstride + off;
        float ra = pa[(long)cx.a * p_nstride];
        if (cx.two) ra = add_rn(mul_rn(cx.wa, ra), mul_rn(cx.wb, pa[(long)cx.b * p_nstride]));
        if (cy.two) {
            const float* pb = P + (long)cy.b * gx * p_nstride + off;
            float rb = pb[(long)cx.a * p_nstride];
            if (cx.two) rb = add_rn(mul_rn(cx.wa, rb), mul_rn(cx.wb, pb[(long)cx.b * p_nstride]));
            ra = add_rn(mul_rn(cy.wa, ra), mul_rn(cy.wb, rb));
        }
        v[k] = ra;
    }
    float* op = out + (long)row * Wc + x0;
    if constexpr (VEC == 4)
        *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
    else
        op[0] = v[0];
}

// rows [r0, r0 + n) of src [C, H, W] -> fp32 [C, n, W], or uint8 [n, W] (C == 1) / [n, W, 3] (C == 3)
template <int VEC>
__global__ __launch_bounds__(256) void ter_emit_kernel(const float* __restrict__ src, int C, int H, int W, int r0, int n,
                                                       int out_u8, int grey, void* __restrict__ out) {
    const int per_row = W / VEC;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (!out_u8) {
        if (idx >= (long)C * n * per_row) return;
        const int row = (int)(idx / per_row);         // c * n + r
        const int x0 = (int)(idx - (long)row * per_row) * VEC;
        const int c = row / n, r = row - c * n;
        const float* sp = src + ((long)c * H + r0 + r) * W + x0;
        float* op = (float*)out + (long)row * W + x0;
        if constexpr (VEC == 4)
            *reinterpret_cast<float4*>(op) = *reinterpret_cast<const float4*>(sp);
        else
            op[0] = sp[0];
        return;
    }
    if (idx >= (long)n * per_row) return;
    const int r = (int)(idx / per_row);
    const int x0 = (int)(idx - (long)r * per_row) * VEC;
    // util.to_uint8(util.convert_to_rgb(v, is_grayscale=grey)): the tanh-range map in float32 as numpy evaluates it (no
    // contraction), clip to [0, 1], then rint(double * 255) -- half to even.  One channel comes out as one byte per pixel.
    const int nc = C == 1 ? 1 : 3;
    unsigned char px[3 * VEC];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (ch >= nc) break;
        const float* sp = src + ((long)ch * H + r0 + r) * W + x0;
        float q[VEC];
        if constexpr (VEC == 4) {
            const float4 t = *reinterpret_cast<const float4*>(sp);
            q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
        } else {
            q[0] = sp[0];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float f = q[k];
            if (!grey) f = __fdiv_rn(add_rn(mul_rn(f, 127.5f), 127.5f), 255.0f);
            f = fminf(fmaxf(f, 0.0f), 1.0f);
            px[nc * k + ch] = (unsigned char)(int)rint((double)f * 255.0);
        }
    }
    unsigned char* op = (unsigned char*)out + ((long)r * W + x0) * nc;
    if constexpr (VEC == 4) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(op);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (i >= nc) break;
            o32[i] = (uint32_t)px[4 * i] | ((uint32_t)px[4 * i + 1] << 8) | ((uint32_t)px[4 * i + 2] << 16) |
                     ((uint32_t)px[4 * i + 3] << 24);
        }
    } else {
        for (int ch = 0; ch < nc; ++ch) op[ch] = px[ch];
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int ghm_terrain_seed(ghm_ctx* ctx, const float* P, int64_t p_nstride, int32_t gy, int32_t gx, int32_t C, int32_t s,
                     int32_t row0, int32_t rows, int32_t blend, float* out, int64_t out_nstride) {
    GHM_CHECK(P && out && gy >= 1 && gx >= 1 && C >= 1 && s >= 1 && rows >= 1 && (blend == 0 || blend == 1),
              "ghm_terrain_seed: bad arguments (gy=%d gx=%d C=%d s=%d rows=%d blend=%d)", gy, gx, C, s, rows, blend);
    GHM_CHECK(p_nstride >= (int64_t)C * s * s, "ghm_terrain_seed: p_nstride=%lld < C s^2", (long long)p_nstride);
    GHM_CHECK(row0 >= 0 && row0 + rows <= s * gy, "ghm_terrain_seed: rows [%d, %d) outside the canvas of %d", row0,
              row0 + rows, s * gy);
    GHM_CHECK(out_nstride >= (int64_t)C * rows * s * gx, "ghm_terrain_seed: out_nstride=%lld too small",
              (long long)out_nstride);
    GHM_CHECK((int64_t)C * rows * s * gx < ((int64_t)1 << 31), "ghm_terrain_seed: window too large");
    const int Wc = s * gx;
    if (Wc % 4 == 0 && al16(out)) {
        hipLaunchKernelGGL(ter_seed_kernel<4>, EW_GRID((long)C * rows * (Wc / 4)), P, (long)p_nstride, gy, gx, C, s, row0,
                           rows, blend, out);
    } else {
        hipLaunchKernelGGL(ter_seed_kernel<1>, EW_GRID((long)C * rows * Wc), P, (long)p_nstride, gy, gx, C, s, row0, rows,
                           blend, out);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_terrain_emit(ghm_ctx* ctx, const float* src, int32_t C, int32_t H, int32_t W, int32_t r0, int32_t n,
                     int32_t out_u8, int32_t grey, void* out) {
    GHM_CHECK(src && out && C >= 1 && H >= 1 && W >= 1 && (!out_u8 || C == 1 || C == 3),
              "ghm_terrain_emit: bad arguments (C=%d H=%d W=%d out_u8=%d)", C, H, W, out_u8);
    GHM_CHECK(r0 >= 0 && n >= 0 && r0 + n <= H, "ghm_terrain_emit: rows [%d, %d) outside [0, %d)", r0, r0 + n, H);
    GHM_CHECK((int64_t)C * H * W < ((int64_t)1 << 31), "ghm_terrain_emit: source too large");
    if (n == 0) return 0;
    if (W % 4 == 0 && al16(src) && al16(out)) {
        hipLaunchKernelGGL(ter_emit_kernel<4>, EW_GRID((long)(out_u8 ? 1 : C) * n * (W / 4)), src, C, H, W, r0, n,
                           out_u8 ? 1 : 0, grey ? 1 : 0, out);
    } else {
        hipLaunchKernelGGL(ter_emit_kernel<1>, EW_GRID((long)(out_u8 ? 1 : C) * n * W), src, C, H, W, r0, n, out_u8 ? 1 : 0,
                           grey ? 1 : 0, out);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
