// Regions of an unbounded seeded world, chunk by chunk (gan_heightmaps_amd/world.py): the seed canvas of
// terrain.hip without borders, cut into square chunks that are anchored to world coordinates.  Five HBM-bound streaming
// kernels around the trunk's and the U-Net's forward passes:
//   seed   : a rows x cols rectangle of the unbounded seed canvas at any integer origin -> fp32 [C, rows, cols] at the trunk
//            plan's input view, from a table of the head maps of the cell block the rectangle reads;
//   emit   : the centre K x K of the trunk's output -> a resident fp32 chunk buffer [C, K, K];
//   crop   : a sub-rectangle of a chunk buffer -> a staging buffer with a row pitch, as fp32 CHW or as the uint8 map of
//            util.to_uint8(util.convert_to_rgb(.));
//   scene  : a sub-rectangle of a chunk buffer -> the height plane of a render scene on the device, mapped to
//            [0, 1] as render.Scene maps it on the host, bit for bit;
//   gather : a batch of U-Net input tiles, each from the at most four chunk buffers it straddles -> the forward plan's input.
// No LDS, no reductions, no atomics.  Lanes run along the columns, 4 per thread where the geometry allows 16-byte accesses.
#include "common.h"

// no fused multiply-adds: the blend and the uint8 map round every product and sum on their own (csrc/terrain.hip: the same
// rule, the same reason -- and the same values where a finite canvas covers the same pixels)
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

__host__ __device__ __forceinline__ int floor_div(int a, int b) {          // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// the cells of one axis that seed coordinate y reads, and their weights.  ter_cover's arithmetic (csrc/terrain.hip) on
// y mod s: u = (y mod s + 0.5) / s - 0.5 lies in (-0.5, 0.5), so the corners are the cell of y and the one before or after
// it; the weights depend on y mod s alone, so whole-cell translations of the world leave them unchanged.  No clamping.
struct WCover {
    int a;              // first cell (world index); the second is a + 1
    int m;              // y mod s
    float wa, wb;
    bool two;
};

__host__ __device__ __forceinline__ WCover wld_cover(int y, int s, int bilinear) {
    WCover c;
    const int q = floor_div(y, s);
    c.m = y - q * s;
    if (!bilinear) {
        c.a = q;
        c.wa = 1.0f;
        c.wb = 0.0f;
        c.two = false;
        return c;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    const float u = __fdiv_rn((float)c.m + 0.5f, (float)s) - 0.5f;
#else
    const float u = ((float)c.m + 0.5f) / (float)s - 0.5f;
#endif
    const float f = floorf(u);
    const float fy = u - f;
    c.a = q + (int)f;
    c.two = true;
    c.wa = 1.0f - fy;
    c.wb = fy;
    return c;
}

// out[c][r][x] = sum over the covering cells (i, j) of wy_i wx_j P[(i - ci0) * ncx + (j - cj0)][c][y mod s][x mod s]
template <int VEC>
__global__ __launch_bounds__(256) void wld_seed_kernel(const float* __restrict__ P, long p_nstride, int ci0, int cj0,
                                                       int ncx, int C, int s, int y0, int x0, int rows, int cols,
                                                       int bilinear, float* __restrict__ out) {
    const int per_row = cols / VEC;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)C * rows * per_row) return;
    const int row = (int)(idx / per_row);             // c * rows + r
    const int xo = (int)(idx - (long)row * per_row) * VEC;
    const int c = row / rows, r = row - c * rows;
    const WCover cy = wld_cover(y0 + r, s, bilinear);
    const long cbase = (long)c * s * s + (long)cy.m * s;
    const float* prow_a = P + (long)(cy.a - ci0) * ncx * p_nstride;
    const float* prow_b = prow_a + (long)ncx * p_nstride;
    float v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const WCover cx = wld_cover(x0 + xo + k, s, bilinear);
        const long off = cbase + cx.m + (long)(cx.a - cj0) * p_nstride;
        float ra = prow_a[off];
        if (cx.two) ra = add_rn(mul_rn(cx.wa, ra), mul_rn(cx.wb, prow_a[off + p_nstride]));
        if (cy.two) {
            float rb = prow_b[off];
            if (cx.two) rb = add_rn(mul_rn(cx.wa, rb), mul_rn(cx.wb, prow_b[off + p_nstride]));
            ra = add_rn(mul_rn(cy.wa, ra), mul_rn(cy.wb, rb));
        }
        v[k] = ra;
    }
    float* op = out + (long)row * cols + xo;
    if constexpr (VEC == 4)
        *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
    else
        op[0] = v[0];
}

// rows [r0, r0 + K) x columns [c0, c0 + K) of src [C, H, W] -> dst [C, K, K]
template <int VEC>
__global__ __launch_bounds__(256) void wld_emit_kernel(const float* __restrict__ src, int C, int H, int W, int r0, int c0,
                                                       int K, float* __restrict__ dst) {
    const int per_row = K / VEC;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)C * K * per_row) return;
    const int row = (int)(idx / per_row);             // c * K + r
    const int xo = (int)(idx - (long)row * per_row) * VEC;
    const int c = row / K, r = row - c * K;
    const float* sp = src + ((long)c * H + r0 + r) * W + c0 + xo;
    float* dp = dst + (long)row * K + xo;
    if constexpr (VEC == 4)
        *reinterpret_cast<float4*>(dp) = *reinterpret_cast<const float4*>(sp);
    else
        dp[0] = sp[0];
}

// rows [r0, r0 + nr) x columns [c0, c0 + nc) of chunk [C, K, K] -> fp32 dst[c][r][xoff + x] (planes of nr rows of ``pitch``
// pixels), or uint8 dst[r][xoff + x] (C == 1) / dst[r][xoff + x][3] (C == 3)
template <int VEC>
__global__ __launch_bounds__(256) void wld_crop_kernel(const float* __restrict__ chunk, int C, int K, int r0, int c0, int nr,
                                                       int nc, int out_u8, int grey, void* __restrict__ dst, int pitch,
                                                       int xoff) {
    const int per_row = nc / VEC;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (!out_u8) {
        if (idx >= (long)C * nr * per_row) return;
        const int row = (int)(idx / per_row);         // c * nr + r
        const int xo = (int)(idx - (long)row * per_row) * VEC;
        const int c = row / nr, r = row - c * nr;
        const float* sp = chunk + ((long)c * K + r0 + r) * K + c0 + xo;
        float* dp = (float*)dst + (long)row * pitch + xoff + xo;
        if constexpr (VEC == 4)
            *reinterpret_cast<float4*>(dp) = *reinterpret_cast<const float4*>(sp);
        else
            dp[0] = sp[0];
        return;
    }
    if (idx >= (long)nr * per_row) return;
    const int r = (int)(idx / per_row);
    const int xo = (int)(idx - (long)r * per_row) * VEC;
    // util.to_uint8(util.convert_to_rgb(v, is_grayscale=grey)) as ter_emit_kernel evaluates it: the tanh-range map in
    // float32 without contraction, clip to [0, 1], then rint(double * 255) -- half to even
    const int nch = C == 1 ? 1 : 3;
    unsigned char px[3 * VEC];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (ch >= nch) break;
        const float* sp = chunk + ((long)ch * K + r0 + r) * K + c0 + xo;
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
            px[nch * k + ch] = (unsigned char)(int)rint((double)f * 255.0);
        }
    }
    unsigned char* op = (unsigned char*)dst + ((long)r * pitch + xoff + xo) * nch;
    if constexpr (VEC == 4) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(op);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (i >= nch) break;
            o32[i] = (uint32_t)px[4 * i] | ((uint32_t)px[4 * i + 1] << 8) | ((uint32_t)px[4 * i + 2] << 16) |
                     ((uint32_t)px[4 * i + 3] << 24);
        }
    } else {
        for (int ch = 0; ch < nch; ++ch) op[ch] = px[ch];
    }
}

// util.convert_to_rgb's map of one value to [0, 1] as numpy evaluates it in float32: the tanh range by three separately
// rounded operations (the product and the sum stay apart under this file's `fp contract(off)`; __fdiv_rn is the correctly
// rounded IEEE quotient whatever the division flags of the build), then the clip to [0, 1].  The sign of a zero is no part
// of the contract: numpy's own clip loops disagree on what becomes of -0, and -0 == +0 wherever the renderer compares
__device__ __forceinline__ float wld_unit(float f, int grey) {
    if (!grey) f = __fdiv_rn(add_rn(mul_rn(f, 127.5f), 127.5f), 255.0f);
    f = f > 0.0f ? f : 0.0f;
    return f < 1.0f ? f : 1.0f;
}

// rows [r0, r0 + nr) x columns [c0, c0 + nc) of chunk [C, K, K] -> the scene's height plane dst [H, W] at (y, x), as
// render.Scene maps a heightmap on the host: wld_unit per channel, and for C == 3 the mean of the three mapped channels as
// hm.astype(float64).mean(0).astype(float32) computes it -- ((a + b) + c) / 3 in double (the language's `/` on doubles is
// the correctly rounded IEEE division: no fast-math option is given to this build), rounded once to float32.
// A non-finite input sets *flag with a plain store (every thread that stores writes the same 1).
template <int VEC>
__global__ __launch_bounds__(256) void wld_scene_height_kernel(const float* __restrict__ chunk, int C, int K, int r0, int c0,
                                                               int nr, int nc, int grey, float* __restrict__ dst, int W,
                                                               int y, int x, int* __restrict__ flag) {
    const int per_row = nc / VEC;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)nr * per_row) return;
    const int r = (int)(idx / per_row);
    const int xo = (int)(idx - (long)r * per_row) * VEC;
    float q[3][VEC];
    bool bad = false;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (ch >= C) break;
        const float* sp = chunk + ((long)ch * K + r0 + r) * K + c0 + xo;
        if constexpr (VEC == 4) {
            const float4 t = *reinterpret_cast<const float4*>(sp);
            q[ch][0] = t.x; q[ch][1] = t.y; q[ch][2] = t.z; q[ch][3] = t.w;
        } else {
            q[ch][0] = sp[0];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            bad = bad || !isfinite(q[ch][k]);
            q[ch][k] = wld_unit(q[ch][k], grey);
        }
    }
    float v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        v[k] = C == 1 ? q[0][k] : (float)((((double)q[0][k] + (double)q[1][k]) + (double)q[2][k]) / 3.0);
    float* dp = dst + (long)(y + r) * W + x + xo;
    if constexpr (VEC == 4)
        *reinterpret_cast<float4*>(dp) = make_float4(v[0], v[1], v[2], v[3]);
    else
        dp[0] = v[0];
    if (bad) *flag = 1;
}

// the tiles of one forward batch, passed by value: the launch carries its own table, nothing is uploaded
struct WTiles {
    ghm_world_tile t[GHM_WORLD_MAX_TILES];
};

// dst[b][c][ty][tx] = chunk(b, ty, tx)[c][...]: tile b starts at (y0, x0) of its chunk[0] and runs on into chunk[1] (right),
// chunk[2] (below) and chunk[3] (below right); blockIdx.y is the batch slot, slots >= nv repeat tile nv - 1
template <int VEC>
__global__ __launch_bounds__(256) void wld_gather_kernel(const WTiles tiles, int nv, int C, int T, int K,
                                                         float* __restrict__ dst, long dst_nstride) {
    const int per_row = T / VEC;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * per_row) return;
    const int b = blockIdx.y;
    const ghm_world_tile& t = tiles.t[min(b, nv - 1)];
    const int ty = idx / per_row, tx = (idx - ty * per_row) * VEC;
    int yy = t.y0 + ty, xx = t.x0 + tx;
    int which = 0;
    if (yy >= K) { yy -= K; which = 2; }
    if (xx >= K) { xx -= K; which += 1; }          // a group of 4 never straddles: x0, K and T are multiples of 4 there
    const float* sp = t.chunk[which] + (long)yy * K + xx;
    float* dp = dst + (long)b * dst_nstride + (long)ty * T + tx;
    for (int c = 0; c < C; ++c) {
        if constexpr (VEC == 4)
            *reinterpret_cast<float4*>(dp + (long)c * T * T) = *reinterpret_cast<const float4*>(sp + (long)c * K * K);
        else
            dp[(long)c * T * T] = sp[(long)c * K * K];
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int ghm_world_seed(ghm_ctx* ctx, const float* P, int64_t p_nstride, int32_t ci0, int32_t cj0, int32_t ncy, int32_t ncx,
                   int32_t C, int32_t s, int32_t y0, int32_t x0, int32_t rows, int32_t cols, int32_t blend, float* out,
                   int64_t out_nstride) {
    GHM_CHECK(P && out && ncy >= 1 && ncx >= 1 && C >= 1 && s >= 1 && rows >= 1 && cols >= 1 && (blend == 0 || blend == 1),
              "ghm_world_seed: bad arguments (ncy=%d ncx=%d C=%d s=%d rows=%d cols=%d blend=%d)", ncy, ncx, C, s, rows, cols,
              blend);
    GHM_CHECK(p_nstride >= (int64_t)C * s * s, "ghm_world_seed: p_nstride=%lld < C s^2", (long long)p_nstride);
    const int64_t lim = ((int64_t)1 << 30);
    GHM_CHECK(y0 > -lim && x0 > -lim && (int64_t)y0 + rows < lim && (int64_t)x0 + cols < lim && ci0 > -lim && cj0 > -lim,
              "ghm_world_seed: origin (%d, %d) out of range", y0, x0);
    // every cell the rectangle reads lies in the table: the covers are monotone in the coordinate
    const WCover ya = wld_cover(y0, s, blend), yb = wld_cover(y0 + rows - 1, s, blend);
    const WCover xa = wld_cover(x0, s, blend), xb = wld_cover(x0 + cols - 1, s, blend);
    GHM_CHECK(ya.a >= ci0 && yb.a + blend < ci0 + ncy && xa.a >= cj0 && xb.a + blend < cj0 + ncx,
              "ghm_world_seed: the rectangle reads cells [%d, %d] x [%d, %d], the table holds [%d, %d) x [%d, %d)", ya.a,
              yb.a + blend, xa.a, xb.a + blend, ci0, ci0 + ncy, cj0, cj0 + ncx);
    GHM_CHECK(out_nstride >= (int64_t)C * rows * cols, "ghm_world_seed: out_nstride=%lld too small", (long long)out_nstride);
    GHM_CHECK((int64_t)C * rows * cols < ((int64_t)1 << 31), "ghm_world_seed: window too large");
    if (cols % 4 == 0 && al16(out)) {
        hipLaunchKernelGGL(wld_seed_kernel<4>, EW_GRID((long)C * rows * (cols / 4)), P, (long)p_nstride, ci0, cj0, ncx, C, s,
                           y0, x0, rows, cols, blend, out);
    } else {
        hipLaunchKernelGGL(wld_seed_kernel<1>, EW_GRID((long)C * rows * cols), P, (long)p_nstride, ci0, cj0, ncx, C, s, y0,
                           x0, rows, cols, blend, out);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_world_emit(ghm_ctx* ctx, const float* src, int32_t C, int32_t H, int32_t W, int32_t r0, int32_t c0, int32_t K,
                   float* dst) {
    GHM_CHECK(src && dst && C >= 1 && H >= 1 && W >= 1 && K >= 1, "ghm_world_emit: bad arguments (C=%d H=%d W=%d K=%d)", C,
              H, W, K);
    GHM_CHECK(r0 >= 0 && c0 >= 0 && (int64_t)r0 + K <= H && (int64_t)c0 + K <= W,
              "ghm_world_emit: [%d, %d) x [%d, %d) outside %d x %d", r0, r0 + K, c0, c0 + K, H, W);
    GHM_CHECK((int64_t)C * H * W < ((int64_t)1 << 31), "ghm_world_emit: source too large");
    if (K % 4 == 0 && W % 4 == 0 && c0 % 4 == 0 && al16(src) && al16(dst)) {
        hipLaunchKernelGGL(wld_emit_kernel<4>, EW_GRID((long)C * K * (K / 4)), src, C, H, W, r0, c0, K, dst);
    } else {
        hipLaunchKernelGGL(wld_emit_kernel<1>, EW_GRID((long)C * K * K), src, C, H, W, r0, c0, K, dst);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_world_crop(ghm_ctx* ctx, const float* chunk, int32_t C, int32_t K, int32_t r0, int32_t c0, int32_t nr, int32_t nc,
                   int32_t out_u8, int32_t grey, void* dst, int32_t pitch, int32_t xoff) {
    GHM_CHECK(chunk && dst && C >= 1 && K >= 1 && (!out_u8 || C == 1 || C == 3),
              "ghm_world_crop: bad arguments (C=%d K=%d out_u8=%d)", C, K, out_u8);
    GHM_CHECK(r0 >= 0 && c0 >= 0 && nr >= 0 && nc >= 0 && (int64_t)r0 + nr <= K && (int64_t)c0 + nc <= K,
              "ghm_world_crop: [%d, %d) x [%d, %d) outside the chunk of %d", r0, r0 + nr, c0, c0 + nc, K);
    GHM_CHECK(xoff >= 0 && (int64_t)xoff + nc <= pitch, "ghm_world_crop: columns [%d, %d) outside the pitch of %d", xoff,
              xoff + nc, pitch);
    GHM_CHECK((int64_t)C * K * K < ((int64_t)1 << 31) && (int64_t)C * nr * pitch < ((int64_t)1 << 31),
              "ghm_world_crop: too large");
    if (nr == 0 || nc == 0) return 0;
    const int planes = out_u8 ? 1 : C;
    if (K % 4 == 0 && c0 % 4 == 0 && nc % 4 == 0 && pitch % 4 == 0 && xoff % 4 == 0 && al16(chunk) && al16(dst)) {
        hipLaunchKernelGGL(wld_crop_kernel<4>, EW_GRID((long)planes * nr * (nc / 4)), chunk, C, K, r0, c0, nr, nc,
                           out_u8 ? 1 : 0, grey ? 1 : 0, dst, pitch, xoff);
    } else {
        hipLaunchKernelGGL(wld_crop_kernel<1>, EW_GRID((long)planes * nr * nc), chunk, C, K, r0, c0, nr, nc, out_u8 ? 1 : 0,
                           grey ? 1 : 0, dst, pitch, xoff);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_world_scene_height(ghm_ctx* ctx, const float* chunk, int32_t C, int32_t K, int32_t r0, int32_t c0, int32_t nr,
                           int32_t nc, int32_t grey, float* dst, int32_t H, int32_t W, int32_t y, int32_t x, int32_t* flag) {
    GHM_CHECK(chunk && dst && flag && (C == 1 || C == 3) && K >= 1, "ghm_world_scene_height: bad arguments (C=%d K=%d)", C, K);
    GHM_CHECK(r0 >= 0 && c0 >= 0 && nr >= 0 && nc >= 0 && (int64_t)r0 + nr <= K && (int64_t)c0 + nc <= K,
              "ghm_world_scene_height: [%d, %d) x [%d, %d) outside the chunk of %d", r0, r0 + nr, c0, c0 + nc, K);
    GHM_CHECK(H >= 1 && W >= 1 && y >= 0 && x >= 0 && (int64_t)y + nr <= H && (int64_t)x + nc <= W,
              "ghm_world_scene_height: rows [%d, %d) x columns [%d, %d) outside the scene of %d x %d", y, y + nr, x, x + nc, H,
              W);
    GHM_CHECK((int64_t)C * K * K < ((int64_t)1 << 31) && (int64_t)H * W < ((int64_t)1 << 31),
              "ghm_world_scene_height: too large");
    if (nr == 0 || nc == 0) return 0;
    // 16-byte groups need every row of both sides to start on one: a scene snapped to multiples of 4 (a flight's windows)
    // takes this form, any other rectangle the scalar one, whose rows are just as contiguous
    if (K % 4 == 0 && c0 % 4 == 0 && nc % 4 == 0 && W % 4 == 0 && x % 4 == 0 && al16(chunk) && al16(dst)) {
        hipLaunchKernelGGL(wld_scene_height_kernel<4>, EW_GRID((long)nr * (nc / 4)), chunk, C, K, r0, c0, nr, nc,
                           grey ? 1 : 0, dst, W, y, x, flag);
    } else {
        hipLaunchKernelGGL(wld_scene_height_kernel<1>, EW_GRID((long)nr * nc), chunk, C, K, r0, c0, nr, nc, grey ? 1 : 0, dst,
                           W, y, x, flag);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_world_gather(ghm_ctx* ctx, const ghm_world_tile* tiles, int32_t n_valid, int32_t B, int32_t C, int32_t T, int32_t K,
                     float* dst, int64_t dst_nstride) {
    GHM_CHECK(tiles && dst && C >= 1 && T >= 1 && K >= T, "ghm_world_gather: bad arguments (C=%d T=%d K=%d)", C, T, K);
    GHM_CHECK(n_valid >= 1 && n_valid <= B && B <= GHM_WORLD_MAX_TILES && dst_nstride >= (int64_t)C * T * T,
              "ghm_world_gather: n_valid=%d B=%d (at most %d) dst_nstride=%lld", n_valid, B, GHM_WORLD_MAX_TILES,
              (long long)dst_nstride);
    GHM_CHECK((int64_t)C * K * K < ((int64_t)1 << 31), "ghm_world_gather: chunk too large");
    WTiles tab = {};
    bool vec = T % 4 == 0 && K % 4 == 0 && dst_nstride % 4 == 0 && al16(dst);
    for (int b = 0; b < n_valid; ++b) {
        const ghm_world_tile& t = tiles[b];
        GHM_CHECK(t.y0 >= 0 && t.y0 < K && t.x0 >= 0 && t.x0 < K, "ghm_world_gather: tile %d starts at (%d, %d) of its chunk",
                  b, t.y0, t.x0);
        const bool down = t.y0 + T > K, right = t.x0 + T > K;
        GHM_CHECK(t.chunk[0] && (!right || t.chunk[1]) && (!down || t.chunk[2]) && (!(down && right) || t.chunk[3]),
                  "ghm_world_gather: tile %d straddles a chunk it has no buffer for", b);
        vec = vec && t.x0 % 4 == 0 && al16(t.chunk[0]) && al16(t.chunk[1]) && al16(t.chunk[2]) && al16(t.chunk[3]);
        tab.t[b] = t;
    }
    if (vec) {
        hipLaunchKernelGGL(wld_gather_kernel<4>, dim3(ceil_div((long)T * (T / 4), 256), B), dim3(256), 0, ctx->stream, tab,
                           n_valid, C, T, K, dst, (long)dst_nstride);
    } else {
        hipLaunchKernelGGL(wld_gather_kernel<1>, dim3(ceil_div((long)T * T, 256), B), dim3(256), 0, ctx->stream, tab,
                           n_valid, C, T, K, dst, (long)dst_nstride);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
