// Tiled inference over heightmaps of any size (gan_heightmaps_amd/texture.py): the canvas is cut into
// in_shp x in_shp tiles that overlap by ``o`` pixels, every tile goes through the U-Net's forward plan, and the overlaps are
// cross-faded with separable linear ramps.  Four HBM-bound streaming kernels around the forward pass:
//   gather   : a band of input rows (uint8 NHWC or normalised fp32 CHW) -> the plan's fp32 NCHW input view, with the
//              half-sample-symmetric 'reflect' rule of ghm_image_batch at all four canvas borders;
//   blend    : acc += w * u for the tiles of one forward batch, gather form (a thread owns its accumulator pixels and walks
//              the batch's tiles in order: no atomics, bit-repeatable);
//   finalize : acc / sum(w) of rows no later tile row touches, as fp32 CHW or as the uint8 HWC RGB of
//              util.to_uint8(util.convert_to_rgb(.)).  sum(w) is recomputed from the plan (no weight buffer);
//   scene    : the same fp32 values mapped to [0, 1] and written into the three texture planes of a render scene on the
//              device.
// No LDS, no reductions.  Lanes run along the canvas columns, 4 per thread where the row geometry allows 16-byte accesses.
#include "common.h"

// no fused multiply-adds: the weights, the blend and the uint8 map round every product and sum on its own, as the host
// restatement and numpy's float32 evaluation of util.convert_to_rgb do.  HIP's __fmul_rn / __fadd_rn are plain operators
// defined in a header that hipcc compiles with contraction on, so they would still fuse: these two are compiled here.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

// ghm_image_batch's reflect_coord on integer coordinates: period 2L, mirrored about the half-sample points -1/2 and L-1/2
__device__ __forceinline__ int tex_reflect(long c, int L) {
    if (L <= 1) return 0;
    const long p = 2L * L;
    long m = c % p;
    if (m < 0) m += p;
    return (int)(m >= L ? p - 1 - m : m);
}

// per-axis weight of tile i (of n) at tile-local coordinate t: ramps of width o towards the neighbours it has
__device__ __forceinline__ float tex_w(int i, int t, int n, int T, int o) {
    if (o > 0 && i > 0 && t < o) return __fdiv_rn((float)t + 0.5f, (float)o);
    if (o > 0 && i < n - 1 && t >= T - o) return __fdiv_rn((float)(T - t) - 0.5f, (float)o);
    return 1.0f;
}

// the (one or two) tiles of an axis that cover canvas coordinate y, in tile order: their weights there (w1 = 0 if one)
__device__ __forceinline__ void tex_cover(int y, int n, int pad, int T, int o, float& w0, float& w1) {
    const int s = T - o;
    int hi = (y + pad) / s;             // y + pad >= 0 for every canvas coordinate in [0, L)
    if (hi > n - 1) hi = n - 1;
    const bool two = hi > 0 && -pad + (hi - 1) * s + T > y;
    const int lo = two ? hi - 1 : hi;
    w0 = tex_w(lo, y + pad - lo * s, n, T, o);
    w1 = two ? tex_w(hi, y + pad - hi * s, n, T, o) : 0.0f;
}

// sum(w) at canvas column x of a row whose covering tile rows weigh wy0, wy1: the blend's order, tile rows, then tile
// columns (a missing second tile adds an exact 0)
__device__ __forceinline__ float tex_sum_w(float wy0, float wy1, int x, int nx, int pad_x, int T, int o) {
    float wx0, wx1;
    tex_cover(x, nx, pad_x, T, o, wx0, wx1);
    float z = mul_rn(wy0, wx0);
    if (wx1 != 0.0f) z = add_rn(z, mul_rn(wy0, wx1));
    if (wy1 != 0.0f) {
        z = add_rn(z, mul_rn(wy1, wx0));
        if (wx1 != 0.0f) z = add_rn(z, mul_rn(wy1, wx1));
    }
    return z;
}

template <int VEC>
__global__ __launch_bounds__(256) void tex_gather_kernel(const void* __restrict__ band, int u8, int C, int band_rows,
                                                         int band_row0, int H, int W, int y0, int x0, int s, int nvalid,
                                                         int B, int T, int tanh_range, float* __restrict__ dst,
                                                         long dst_nstride) {
    const int per_row = T / VEC;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * T * per_row) return;
    const int b = (int)(idx / ((long)T * per_row));
    const int rem = (int)(idx - (long)b * T * per_row);
    const int ty = rem / per_row, tx0 = (rem - ty * per_row) * VEC;
    const int xj = x0 + min(b, nvalid - 1) * s;        // a ragged batch repeats its last tile
    int gy = tex_reflect((long)y0 + ty, H) - band_row0;
    gy = min(max(gy, 0), band_rows - 1);
    int gx[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) gx[k] = tex_reflect((long)xj + tx0 + k, W);
    float* dp = dst + (long)b * dst_nstride + (long)ty * T + tx0;
    for (int c = 0; c < C; ++c) {
        float v[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (u8) {
                // the training path's normalisation (ghm_image_batch, ArrayIterator): x / 255 or (x - 127.5) / 127.5
                const float x = (float)((const unsigned char*)band)[((long)gy * W + gx[k]) * C + c];
                v[k] = tanh_range ? (x - 127.5f) / 127.5f : x / 255.0f;
            } else {
                v[k] = ((const float*)band)[((long)c * band_rows + gy) * W + gx[k]];
            }
        }
        if constexpr (VEC == 4)
            *reinterpret_cast<float4*>(dp + (long)c * T * T) = make_float4(v[0], v[1], v[2], v[3]);
        else
            dp[(long)c * T * T] = v[0];
    }
}

// acc[c][r][x] (+)= sum over the batch's tiles covering x of wy(r) wx(x - x_b) u_b[c][r][x - x_b], x in [xlo, xlo + xw)
template <int VEC>
__global__ __launch_bounds__(256) void tex_blend_kernel(float* __restrict__ acc, int W, int T, int C,
                                                        const float* __restrict__ u, long u_nstride, int nb, int iy, int ny,
                                                        int j0, int nx, int pad_x, int o, int xlo, int xw) {
    const int per_row = (xw + VEC - 1) / VEC;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)C * T * per_row) return;
    const int row = (int)(idx / per_row);              // c * T + r
    const int r = row % T, c = row / T;
    const int x0 = xlo + (int)(idx - (long)row * per_row) * VEC;
    const int s = T - o;
    const float wy = tex_w(iy, r, ny, T, o);
    float* ap = acc + (long)row * W + x0;
    float a[VEC];
    if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(ap);
        a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w;
    } else {
        a[0] = ap[0];
    }
    const float* ub = u + ((long)c * T + r) * T;
    for (int b = 0; b < nb; ++b) {
        const int xb = -pad_x + (j0 + b) * s;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int t = x0 + k - xb;
            if (t >= 0 && t < T && x0 + k < W) {
                const float w = mul_rn(wy, tex_w(j0 + b, t, nx, T, o));
                a[k] = add_rn(a[k], mul_rn(w, ub[(long)b * u_nstride + t]));
            }
        }
    }
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(ap) = make_float4(a[0], a[1], a[2], a[3]);
    } else {
        ap[0] = a[0];
    }
}

// rows [r0, r0 + nrows) of the accumulator (canvas rows yc0 + r0 + ...) -> acc / sum(w), fp32 CHW [C, nrows, W] or
// uint8 HWC [nrows, W, 3]
template <int VEC>
__global__ __launch_bounds__(256) void tex_finalize_kernel(const float* __restrict__ acc, int W, int T, int C, int r0,
                                                           int nrows, int yc0, int ny, int pad_y, int nx, int pad_x, int o,
                                                           int out_u8, int b_grey, void* __restrict__ out) {
    const int per_row = W / VEC;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)nrows * per_row) return;
    const int r = (int)(idx / per_row);
    const int x0 = (int)(idx - (long)r * per_row) * VEC;
    float wy0, wy1;
    tex_cover(yc0 + r0 + r, ny, pad_y, T, o, wy0, wy1);
    float sw[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) sw[k] = tex_sum_w(wy0, wy1, x0 + k, nx, pad_x, T, o);
    float v[3][VEC];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= C) break;
        const float* ap = acc + ((long)c * T + r0 + r) * W + x0;
        float q[VEC];
        if constexpr (VEC == 4) {
            const float4 t = *reinterpret_cast<const float4*>(ap);
            q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
        } else {
            q[0] = ap[0];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[c][k] = __fdiv_rn(q[k], sw[k]);
    }
    if (!out_u8) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= C) break;
            float* op = (float*)out + ((long)c * nrows + r) * W + x0;
            if constexpr (VEC == 4)
                *reinterpret_cast<float4*>(op) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            else
                op[0] = v[c][0];
        }
        return;
    }
    // util.to_uint8(util.convert_to_rgb(v, is_grayscale=b_grey)): the tanh-range map in float32 as numpy evaluates it (no
    // contraction), clip to [0, 1], then rint(double * 255) -- half to even.  One channel is replicated to three.
    unsigned char px[3 * VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float f = C == 1 ? v[0][k] : v[ch][k];
            if (!b_grey) f = __fdiv_rn(add_rn(mul_rn(f, 127.5f), 127.5f), 255.0f);
            f = fminf(fmaxf(f, 0.0f), 1.0f);
            px[3 * k + ch] = (unsigned char)(int)rint((double)f * 255.0);
        }
    }
    unsigned char* op = (unsigned char*)out + ((long)r * W + x0) * 3;
    if constexpr (VEC == 4) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(op);
#pragma unroll
        for (int i = 0; i < 3; ++i)
            o32[i] = (uint32_t)px[4 * i] | ((uint32_t)px[4 * i + 1] << 8) | ((uint32_t)px[4 * i + 2] << 16) |
                     ((uint32_t)px[4 * i + 3] << 24);
    } else {
        op[0] = px[0];
        op[1] = px[1];
        op[2] = px[2];
    }
}

// tex_finalize_kernel's fp32 values, written where a render scene keeps its texture: accumulator rows
// [r0, r0 + nrows) (canvas rows yc0 + r0 + ...) -> rows yc0 + r0 + ... of the three unit planes out [3, H, Ws], Ws <= W
// columns of each row.  v = acc / sum(w) by the very operations of the fp32 path above, in its order (sum(w): tile rows,
// then tile columns; then one __fdiv_rn); then render.Scene's host map of a texture: util.convert_to_rgb in float32 -- for
// the tanh range fl(fl(fl(v 127.5) + 127.5) / 255), three roundings kept apart by this file's `fp contract(off)` and the
// correctly rounded __fdiv_rn -- clipped to [0, 1] (the sign of a zero is no part of the contract, csrc/world.hip), one
// channel replicated to three planes.  A non-finite v sets *flag with a plain store.
template <int VEC>
__global__ __launch_bounds__(256) void tex_scene_kernel(const float* __restrict__ acc, int W, int T, int C, int r0, int nrows,
                                                        int yc0, int ny, int pad_y, int nx, int pad_x, int o, int b_grey,
                                                        float* __restrict__ out, int H, int Ws, int* __restrict__ flag) {
    const int per_row = Ws / VEC;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)nrows * per_row) return;
    const int r = (int)(idx / per_row);
    const int x0 = (int)(idx - (long)r * per_row) * VEC;
    float wy0, wy1;
    tex_cover(yc0 + r0 + r, ny, pad_y, T, o, wy0, wy1);
    float sw[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) sw[k] = tex_sum_w(wy0, wy1, x0 + k, nx, pad_x, T, o);
    bool bad = false;
    float* orow = out + (long)(yc0 + r0 + r) * Ws + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= C) break;
        const float* ap = acc + ((long)c * T + r0 + r) * W + x0;
        float q[VEC];
        if constexpr (VEC == 4) {
            const float4 t = *reinterpret_cast<const float4*>(ap);
            q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
        } else {
            q[0] = ap[0];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float f = __fdiv_rn(q[k], sw[k]);
            bad = bad || !isfinite(f);
            if (!b_grey) f = __fdiv_rn(add_rn(mul_rn(f, 127.5f), 127.5f), 255.0f);
            f = f > 0.0f ? f : 0.0f;
            q[k] = f < 1.0f ? f : 1.0f;
        }
        for (int p = c; p < (C == 1 ? 3 : c + 1); ++p) {
            float* op = orow + (long)p * H * Ws;
            if constexpr (VEC == 4)
                *reinterpret_cast<float4*>(op) = make_float4(q[0], q[1], q[2], q[3]);
            else
                op[0] = q[0];
        }
    }
    if (bad) *flag = 1;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int tex_check_axis(int L, int T, int o) {
    GHM_CHECK(L >= 1 && T >= 1 && o >= 0 && 2 * o <= T, "texture: bad axis (L=%d, T=%d, overlap=%d)", L, T, o);
    return 0;
}

}  // namespace

extern "C" {

int ghm_texture_gather(ghm_ctx* ctx, const void* band, int32_t band_u8, int32_t C, int32_t band_rows, int32_t band_row0,
                       int32_t H, int32_t W, int32_t y0, int32_t x0, int32_t stride, int32_t n_valid, int32_t B, int32_t T,
                       int32_t tanh_range, float* dst, int64_t dst_nstride) {
    GHM_CHECK(band && dst && C >= 1 && band_rows >= 1 && H >= 1 && W >= 1 && T >= 1 && stride >= 1,
              "ghm_texture_gather: bad arguments");
    GHM_CHECK(n_valid >= 1 && n_valid <= B && dst_nstride >= (int64_t)C * T * T,
              "ghm_texture_gather: n_valid=%d B=%d dst_nstride=%lld", n_valid, B, (long long)dst_nstride);
    GHM_CHECK(band_row0 >= 0 && band_row0 + band_rows <= H, "ghm_texture_gather: band rows [%d, %d) outside [0, %d)",
              band_row0, band_row0 + band_rows, H);
    if (T % 4 == 0 && dst_nstride % 4 == 0 && al16(dst)) {
        hipLaunchKernelGGL(tex_gather_kernel<4>, EW_GRID((long)B * T * (T / 4)), band, band_u8 ? 1 : 0, C, band_rows,
                           band_row0, H, W, y0, x0, stride, n_valid, B, T, tanh_range ? 1 : 0, dst, (long)dst_nstride);
    } else {
        hipLaunchKernelGGL(tex_gather_kernel<1>, EW_GRID((long)B * T * T), band, band_u8 ? 1 : 0, C, band_rows, band_row0,
                           H, W, y0, x0, stride, n_valid, B, T, tanh_range ? 1 : 0, dst, (long)dst_nstride);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_texture_blend(ghm_ctx* ctx, float* acc, int32_t W, int32_t T, int32_t C, const float* u, int64_t u_nstride,
                      int32_t nb, int32_t iy, int32_t ny, int32_t j0, int32_t nx, int32_t pad_x, int32_t overlap) {
    if (tex_check_axis(W, T, overlap)) return -2;
    GHM_CHECK(acc && u && C >= 1 && nb >= 1 && iy >= 0 && iy < ny && j0 >= 0 && j0 + nb <= nx && u_nstride >= (int64_t)C * T * T,
              "ghm_texture_blend: bad arguments");
    const int s = T - overlap;
    const int xlo = max(0, -pad_x + j0 * s), xhi = min(W, -pad_x + (j0 + nb - 1) * s + T);
    if (xhi <= xlo) return 0;
    if (W % 4 == 0 && al16(acc)) {
        const int a = xlo & ~3, w = ((xhi + 3) & ~3) - a;     // whole 16-byte groups of the row (W % 4 == 0: inside it)
        hipLaunchKernelGGL(tex_blend_kernel<4>, EW_GRID((long)C * T * (w / 4)), acc, W, T, C, u, (long)u_nstride, nb, iy,
                           ny, j0, nx, pad_x, overlap, a, w);
    } else {
        hipLaunchKernelGGL(tex_blend_kernel<1>, EW_GRID((long)C * T * (xhi - xlo)), acc, W, T, C, u, (long)u_nstride, nb,
                           iy, ny, j0, nx, pad_x, overlap, xlo, xhi - xlo);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_texture_finalize(ghm_ctx* ctx, const float* acc, int32_t W, int32_t T, int32_t C, int32_t r0, int32_t nrows,
                         int32_t yc0, int32_t ny, int32_t pad_y, int32_t nx, int32_t pad_x, int32_t overlap, int32_t out_u8,
                         int32_t b_grey, void* out) {
    if (tex_check_axis(W, T, overlap)) return -2;
    GHM_CHECK(acc && out && (C == 1 || C == 3 || !out_u8) && C >= 1 && C <= 3, "ghm_texture_finalize: bad arguments (C=%d)", C);
    GHM_CHECK(r0 >= 0 && nrows >= 0 && r0 + nrows <= T, "ghm_texture_finalize: rows [%d, %d) outside the band of %d", r0,
              r0 + nrows, T);
    GHM_CHECK(yc0 + r0 >= 0, "ghm_texture_finalize: rows above the canvas");
    if (nrows == 0) return 0;
    if (W % 4 == 0 && al16(acc) && al16(out)) {
        hipLaunchKernelGGL(tex_finalize_kernel<4>, EW_GRID((long)nrows * (W / 4)), acc, W, T, C, r0, nrows, yc0, ny, pad_y,
                           nx, pad_x, overlap, out_u8 ? 1 : 0, b_grey ? 1 : 0, out);
    } else {
        hipLaunchKernelGGL(tex_finalize_kernel<1>, EW_GRID((long)nrows * W), acc, W, T, C, r0, nrows, yc0, ny, pad_y, nx,
                           pad_x, overlap, out_u8 ? 1 : 0, b_grey ? 1 : 0, out);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_texture_finalize_scene(ghm_ctx* ctx, const float* acc, int32_t W, int32_t T, int32_t C, int32_t r0, int32_t nrows,
                               int32_t yc0, int32_t ny, int32_t pad_y, int32_t nx, int32_t pad_x, int32_t overlap,
                               int32_t b_grey, float* out, int32_t H, int32_t Ws, int32_t* flag) {
    if (tex_check_axis(W, T, overlap)) return -2;
    GHM_CHECK(acc && out && flag && (C == 1 || C == 3), "ghm_texture_finalize_scene: bad arguments (C=%d)", C);
    GHM_CHECK(r0 >= 0 && nrows >= 0 && r0 + nrows <= T, "ghm_texture_finalize_scene: rows [%d, %d) outside the band of %d", r0,
              r0 + nrows, T);
    GHM_CHECK(H >= 1 && Ws >= 1 && Ws <= W && (int64_t)H * Ws < ((int64_t)1 << 31),
              "ghm_texture_finalize_scene: a scene of %d x %d from an accumulator %d wide", H, Ws, W);
    GHM_CHECK((int64_t)yc0 + r0 >= 0 && (int64_t)yc0 + r0 + nrows <= H,
              "ghm_texture_finalize_scene: rows [%d, %d) outside the scene of %d", yc0 + r0, yc0 + r0 + nrows, H);
    if (nrows == 0) return 0;
    // Ws % 4 == 0 puts every row of every plane on a 16-byte boundary (a flight's windows are snapped to such widths)
    if (W % 4 == 0 && Ws % 4 == 0 && al16(acc) && al16(out)) {
        hipLaunchKernelGGL(tex_scene_kernel<4>, EW_GRID((long)nrows * (Ws / 4)), acc, W, T, C, r0, nrows, yc0, ny, pad_y, nx,
                           pad_x, overlap, b_grey ? 1 : 0, out, H, Ws, flag);
    } else {
        hipLaunchKernelGGL(tex_scene_kernel<1>, EW_GRID((long)nrows * Ws), acc, W, T, C, r0, nrows, yc0, ny, pad_y, nx, pad_x,
                           overlap, b_grey ? 1 : 0, out, H, Ws, flag);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
