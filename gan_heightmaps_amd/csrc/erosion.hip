// Hydraulic erosion of a heightmap by the "virtual pipes" shallow-water model (gan_heightmaps_amd/erosion.py):
// Mei, Decaudin and Hu (2007), restated so that every step is a gather.  State of a cell, seven fp32 planes of H rows of
// ``pitch`` cells (plane p at p * H * pitch): ground b, water depth d, suspended sediment s, outflow fL fR fT fB towards
// columns j - 1, j + 1 and rows i - 1, i + 1.  The edge of the H x W array is a closed wall.  One iteration:
//   A (steps 1-2)  rain, then the outflow of every cell from the water surfaces of its four neighbours, scaled so that a
//                  cell never gives more water than it holds;
//   B (steps 3-4)  the new depth from the neighbours' outflow, the velocity, the transport capacity from tilt and speed,
//                  and what the ground gives to or takes from the suspended sediment;
//   C (steps 5-6)  the sediment moved against the velocity (one bilinear sample at most one cell away), evaporation.
// Two forms that run the same three device functions per cell, so their results agree bit for bit:
//   plain : three launches, every stage reads and writes global planes (28 plane passes per iteration);
//   fused : one launch; a block stages a 64 x 16 tile and its 3-cell apron in LDS, recomputes the apron's flux (reach 2)
//           and velocity (reach 1) there and writes the tile to the other state of a ping-pong pair (7 planes read with
//           the apron's overhead, 7 written).
// No atomics, no randomness, no reductions.  Planes are indexed in 64 bits.
#include "common.h"

// every product, sum, quotient and root is rounded on its own, in the order written (tests/erosion_ref.py restates it)
#pragma clang fp contract(off)

namespace {

constexpr int NPLANES = GHM_EROSION_PLANES;
constexpr int P_B = 0, P_D = 1, P_S = 2, P_F = 3;          // fL fR fT fB are planes 3 .. 6
constexpr int TW = GHM_EROSION_TILE_W, TH = GHM_EROSION_TILE_H;

typedef ghm_erosion_params EP;

__device__ __forceinline__ float ero_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---- stage A: the scaled outflow f'[4] of cell (i, j).  rb / rd read b and d at any cell of the array -------------------
template <class RB, class RD>
__device__ __forceinline__ void ero_flux(const EP& p, int i, int j, int H, int W, RB rb, RD rd, const float* fin,
                                         float* fout) {
    const float rn = p.dt * p.rain;
    const float k = (p.dt * p.pipe) * p.gravity;
    const float d1 = rd(i, j) + rn;
    const float h = rb(i, j) + d1;
    float g[4];
    g[0] = j > 0 ? fmaxf(0.0f, fin[0] + k * (h - (rb(i, j - 1) + (rd(i, j - 1) + rn)))) : 0.0f;
    g[1] = j < W - 1 ? fmaxf(0.0f, fin[1] + k * (h - (rb(i, j + 1) + (rd(i, j + 1) + rn)))) : 0.0f;
    g[2] = i > 0 ? fmaxf(0.0f, fin[2] + k * (h - (rb(i - 1, j) + (rd(i - 1, j) + rn)))) : 0.0f;
    g[3] = i < H - 1 ? fmaxf(0.0f, fin[3] + k * (h - (rb(i + 1, j) + (rd(i + 1, j) + rn)))) : 0.0f;
    const float S = ((g[0] + g[1]) + (g[2] + g[3])) * p.dt;
    const float K = S > d1 ? __fdiv_rn(d1, S) : 1.0f;
#pragma unroll
    for (int x = 0; x < 4; ++x) fout[x] = K * g[x];
}

struct EroB {
    float b, d2, u, v, s1;
};

// ---- stage B: rb reads b, rf(x, i, j) reads the new outflow f'[x]; d and s are the cell's own --------------------------
template <class RB, class RF>
__device__ __forceinline__ EroB ero_water(const EP& p, int i, int j, int H, int W, RB rb, RF rf, float d, float s) {
    const float d1 = d + p.dt * p.rain;
    const float fl = rf(0, i, j), fr = rf(1, i, j), ft = rf(2, i, j), fb = rf(3, i, j);
    const float inL = j > 0 ? rf(1, i, j - 1) : 0.0f;
    const float inR = j < W - 1 ? rf(0, i, j + 1) : 0.0f;
    const float inT = i > 0 ? rf(3, i - 1, j) : 0.0f;
    const float inB = i < H - 1 ? rf(2, i + 1, j) : 0.0f;
    const float inflow = (inL + inR) + (inT + inB);
    const float outflow = (fl + fr) + (ft + fb);
    EroB o;
    o.d2 = fmaxf(0.0f, d1 + p.dt * (inflow - outflow));
    const float wx = 0.5f * ((inL - fl) + (fr - inR));
    const float wy = 0.5f * ((inT - ft) + (fb - inB));
    const float dbar = fmaxf(0.5f * (d1 + o.d2), p.min_depth);
    o.u = ero_clamp(__fdiv_rn(wx, dbar), -p.max_speed, p.max_speed);
    o.v = ero_clamp(__fdiv_rn(wy, dbar), -p.max_speed, p.max_speed);
    const float gx = 0.5f * (rb(i, min(j + 1, W - 1)) - rb(i, max(j - 1, 0)));
    const float gy = 0.5f * (rb(min(i + 1, H - 1), j) - rb(max(i - 1, 0), j));
    const float g2 = gx * gx + gy * gy;
    const float tilt = fmaxf(__fsqrt_rn(__fdiv_rn(g2, 1.0f + g2)), p.min_tilt);
    const float cap = (p.capacity * tilt) * __fsqrt_rn(o.u * o.u + o.v * o.v);
    const float D = cap - s;
    const float e = D > 0.0f ? p.dissolve * D : p.deposit * D;
    o.b = rb(i, j) - e;
    o.s1 = s + e;
    return o;
}

// one axis of the backtrace: the first corner, the second corner and the weight of idx - clamp(vel dt, +-1) clamped to
// [0, n - 1].  The weight comes from the displacement alone, never from the absolute index: it does not depend on where
// the window's origin lies
__device__ __forceinline__ void ero_back(float vel, float dt, int idx, int n, int& c0, int& c1, float& t) {
    float o = -ero_clamp(vel * dt, -1.0f, 1.0f);
    if (idx == 0 && o < 0.0f) o = 0.0f;
    if (idx == n - 1 && o > 0.0f) o = 0.0f;
    const bool neg = o < 0.0f;
    const int x0 = neg ? idx - 1 : idx;
    t = neg ? o + 1.0f : o;
    c0 = min(max(x0, 0), n - 1);
    c1 = min(max(x0 + 1, 0), n - 1);
}

// ---- stage C: rs reads s1 ---------------------------------------------------------------------------------------------
template <class RS>
__device__ __forceinline__ float ero_transport(const EP& p, int i, int j, int H, int W, float u, float v, RS rs) {
    int x0, x1, y0, y1;
    float tx, ty;
    ero_back(u, p.dt, j, W, x0, x1, tx);
    ero_back(v, p.dt, i, H, y0, y1, ty);
    const float a0 = rs(y0, x0), a1 = rs(y0, x1), b0 = rs(y1, x0), b1 = rs(y1, x1);
    const float top = a0 + tx * (a1 - a0);
    const float bot = b0 + tx * (b1 - b0);
    return top + ty * (bot - top);
}

__device__ __forceinline__ float ero_evaporate(const EP& p, float d2) { return d2 * (1.0f - p.evaporation * p.dt); }

// ---- the plain form: blocks of 64 x 4 cells, one cell per thread --------------------------------------------------------
#define ERO_CELL()                                            \
    const int j = blockIdx.x * 64 + threadIdx.x;              \
    const int i = blockIdx.y * 4 + threadIdx.y;               \
    if (i >= H || j >= W) return;                             \
    const long ps = (long)H * pitch;                          \
    const long at = (long)i * pitch + j

__global__ __launch_bounds__(256) void ero_flux_kernel(const EP p, const float* __restrict__ src, float* __restrict__ dst,
                                                       int H, int W, int pitch) {
    ERO_CELL();
    auto rb = [&](int y, int x) { return src[P_B * ps + (long)y * pitch + x]; };
    auto rd = [&](int y, int x) { return src[P_D * ps + (long)y * pitch + x]; };
    float fin[4], fout[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) fin[x] = src[(P_F + x) * ps + at];
    ero_flux(p, i, j, H, W, rb, rd, fin, fout);
#pragma unroll
    for (int x = 0; x < 4; ++x) dst[(P_F + x) * ps + at] = fout[x];
}

// tmp: three planes u, v, s1
__global__ __launch_bounds__(256) void ero_water_kernel(const EP p, const float* __restrict__ src, float* __restrict__ dst,
                                                        float* __restrict__ tmp, int H, int W, int pitch) {
    ERO_CELL();
    auto rb = [&](int y, int x) { return src[P_B * ps + (long)y * pitch + x]; };
    auto rf = [&](int f, int y, int x) { return dst[(P_F + f) * ps + (long)y * pitch + x]; };
    const EroB o = ero_water(p, i, j, H, W, rb, rf, src[P_D * ps + at], src[P_S * ps + at]);
    dst[P_B * ps + at] = o.b;
    dst[P_D * ps + at] = o.d2;
    tmp[at] = o.u;
    tmp[ps + at] = o.v;
    tmp[2 * ps + at] = o.s1;
}

__global__ __launch_bounds__(256) void ero_transport_kernel(const EP p, float* __restrict__ dst,
                                                            const float* __restrict__ tmp, int H, int W, int pitch) {
    ERO_CELL();
    auto rs = [&](int y, int x) { return tmp[2 * ps + (long)y * pitch + x]; };
    dst[P_S * ps + at] = ero_transport(p, i, j, H, W, tmp[at], tmp[ps + at], rs);
    dst[P_D * ps + at] = ero_evaporate(p, dst[P_D * ps + at]);
}

// ---- the fused form -------------------------------------------------------------------------------------------------------
// LDS of a block: b, d over the tile + 3; the four outflows over the tile + 2; s, u, v over the tile + 1:
// (2 * 22 * 70 + 4 * 20 * 68 + 3 * 18 * 66) * 4 = 48336 bytes, three blocks per CU.  A cell outside the array is never
// loaded, computed or read: every read of a neighbour is guarded by the array's bounds exactly as in the plain form.
constexpr int W3 = TW + 6, H3 = TH + 6, W2 = TW + 4, H2 = TH + 4, W1 = TW + 2, H1 = TH + 2;

__global__ __launch_bounds__(256) void ero_fused_kernel(const EP p, const float* __restrict__ src, float* __restrict__ dst,
                                                        int H, int W, int pitch) {
    __shared__ float sb[H3 * W3], sd[H3 * W3];
    __shared__ float sf[4][H2 * W2];
    __shared__ float ss[H1 * W1], su[H1 * W1], sv[H1 * W1];
    const int ti = blockIdx.y * TH, tj = blockIdx.x * TW;     // the tile's first cell
    const long ps = (long)H * pitch;
    const int tid = threadIdx.x;

    for (int n = tid; n < H3 * W3; n += 256) {
        const int r = n / W3, c = n - r * W3;
        const int i = ti - 3 + r, j = tj - 3 + c;
        if (i >= 0 && i < H && j >= 0 && j < W) {
            const long at = (long)i * pitch + j;
            sb[n] = src[P_B * ps + at];
            sd[n] = src[P_D * ps + at];
        }
    }
    for (int n = tid; n < H2 * W2; n += 256) {
        const int r = n / W2, c = n - r * W2;
        const int i = ti - 2 + r, j = tj - 2 + c;
        if (i >= 0 && i < H && j >= 0 && j < W) {
            const long at = (long)i * pitch + j;
#pragma unroll
            for (int x = 0; x < 4; ++x) sf[x][n] = src[(P_F + x) * ps + at];
        }
    }
    for (int n = tid; n < H1 * W1; n += 256) {
        const int r = n / W1, c = n - r * W1;
        const int i = ti - 1 + r, j = tj - 1 + c;
        if (i >= 0 && i < H && j >= 0 && j < W) ss[n] = src[P_S * ps + (long)i * pitch + j];
    }
    __syncthreads();

    auto rb = [&](int y, int x) { return sb[(y - ti + 3) * W3 + (x - tj + 3)]; };
    auto rd = [&](int y, int x) { return sd[(y - ti + 3) * W3 + (x - tj + 3)]; };
    auto rf = [&](int f, int y, int x) { return sf[f][(y - ti + 2) * W2 + (x - tj + 2)]; };
    auto rs = [&](int y, int x) { return ss[(y - ti + 1) * W1 + (x - tj + 1)]; };

    // A over the tile + 2: a cell reads and writes its own outflow only, its neighbours' b and d
    for (int n = tid; n < H2 * W2; n += 256) {
        const int r = n / W2, c = n - r * W2;
        const int i = ti - 2 + r, j = tj - 2 + c;
        if (i >= 0 && i < H && j >= 0 && j < W) {
            float fin[4], fout[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) fin[x] = sf[x][n];
            ero_flux(p, i, j, H, W, rb, rd, fin, fout);
#pragma unroll
            for (int x = 0; x < 4; ++x) sf[x][n] = fout[x];
        }
    }
    __syncthreads();

    // B over the tile + 1: s becomes s1 in place (a cell reads its own s only); the tile's own cells leave for dst
    for (int n = tid; n < H1 * W1; n += 256) {
        const int r = n / W1, c = n - r * W1;
        const int i = ti - 1 + r, j = tj - 1 + c;
        if (i >= 0 && i < H && j >= 0 && j < W) {
            const EroB o = ero_water(p, i, j, H, W, rb, rf, rd(i, j), ss[n]);
            ss[n] = o.s1;
            su[n] = o.u;
            sv[n] = o.v;
            if (r >= 1 && r <= TH && c >= 1 && c <= TW) {
                const long at = (long)i * pitch + j;
                dst[P_B * ps + at] = o.b;
                dst[P_D * ps + at] = ero_evaporate(p, o.d2);
#pragma unroll
                for (int x = 0; x < 4; ++x) dst[(P_F + x) * ps + at] = rf(x, i, j);
            }
        }
    }
    __syncthreads();

    // C over the tile
    for (int n = tid; n < TH * TW; n += 256) {
        const int r = n / TW, c = n - r * TW;
        const int i = ti + r, j = tj + c;
        if (i < H && j < W) {
            const int m = (r + 1) * W1 + (c + 1);
            dst[P_S * ps + (long)i * pitch + j] = ero_transport(p, i, j, H, W, su[m], sv[m], rs);
        }
    }
}

// ---- init and emit ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ero_init_kernel(const float* __restrict__ hm, int src_pitch, float scale,
                                                       float* __restrict__ state, int H, int W, int pitch) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (i >= H || j >= W) return;
    const long ps = (long)H * pitch;
    const long at = (long)i * pitch + j;
    state[at] = hm[(long)i * src_pitch + j] * scale;
#pragma unroll
    for (int x = 1; x < NPLANES; ++x) state[x * ps + at] = 0.0f;
}

// clamp(b / scale, 0, 1) of rows [r0, r0 + nr) x columns [c0, c0 + nc) -> dst rows yoff .., columns xoff .. (rows of
// dst_pitch cells): fp32, or the uint8 map of ghm_world_crop for a unit-range plane: rint((double)v * 255), half to even
__global__ __launch_bounds__(256) void ero_emit_kernel(const float* __restrict__ b, int pitch, float scale, int r0, int c0,
                                                       int nr, int nc, int out_u8, void* __restrict__ dst, int dst_pitch,
                                                       int yoff, int xoff) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (i >= nr || j >= nc) return;
    float v = __fdiv_rn(b[(long)(r0 + i) * pitch + c0 + j], scale);
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    const long at = (long)(yoff + i) * dst_pitch + xoff + j;
    if (out_u8)
        ((unsigned char*)dst)[at] = (unsigned char)(int)rint((double)v * 255.0);
    else
        ((float*)dst)[at] = v;
}

inline dim3 ero_grid(int H, int W) { return dim3(ceil_div(W, 64), ceil_div(H, 4)); }

inline bool ero_params_ok(const EP* p) {
    if (!p) return false;
    const float v[12] = {p->dt, p->rain, p->evaporation, p->gravity, p->pipe, p->capacity, p->dissolve, p->deposit,
                         p->min_tilt, p->max_speed, p->min_depth, p->height_scale};
    for (float x : v)
        if (!(x >= 0.0f) || x > 3.0e38f) return false;          // finite, not negative, no NaN
    return p->dt > 0.0f && p->min_depth > 0.0f && p->max_speed > 0.0f && p->dt * p->max_speed <= 1.0f &&
           p->height_scale > 0.0f;
}

inline bool ero_shape_ok(int H, int W, int pitch) {
    // the kernels index in 64 bits; a plane stays below 2^31 cells and the launch grids inside their limits
    return H >= 1 && W >= 1 && pitch >= W && (int64_t)H * pitch < ((int64_t)1 << 31) && H <= 4 * 65535;
}

}  // namespace

extern "C" {

int ghm_erosion_init(ghm_ctx* ctx, const float* heightmap, int32_t H, int32_t W, int32_t src_pitch, float height_scale,
                     float* state, int32_t pitch) {
    GHM_CHECK(heightmap && state && ero_shape_ok(H, W, pitch) && src_pitch >= W,
              "ghm_erosion_init: bad arguments (H=%d W=%d src_pitch=%d pitch=%d)", H, W, src_pitch, pitch);
    GHM_CHECK(height_scale > 0.0f && height_scale <= 3.0e38f, "ghm_erosion_init: height_scale=%g", (double)height_scale);
    hipLaunchKernelGGL(ero_init_kernel, ero_grid(H, W), dim3(64, 4), 0, ctx->stream, heightmap, src_pitch, height_scale,
                       state, H, W, pitch);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_erosion_iterate(ghm_ctx* ctx, const ghm_erosion_params* params, float* state0, float* state1, float* tmp,
                        int32_t H, int32_t W, int32_t pitch, int32_t iterations, int32_t fused) {
    GHM_CHECK(state0 && state1 && state0 != state1 && ero_shape_ok(H, W, pitch),
              "ghm_erosion_iterate: bad arguments (H=%d W=%d pitch=%d)", H, W, pitch);
    GHM_CHECK(ero_params_ok(params), "ghm_erosion_iterate: parameters out of range (finite, >= 0, dt > 0, min_depth > 0, "
                                     "max_speed > 0, dt max_speed <= 1, height_scale > 0)");
    GHM_CHECK(iterations >= 0, "ghm_erosion_iterate: iterations=%d", iterations);
    GHM_CHECK(fused || tmp, "ghm_erosion_iterate: the plain form needs three planes of workspace");
    const EP p = *params;
    float *src = state0, *dst = state1;
    for (int it = 0; it < iterations; ++it) {
        if (fused) {
            hipLaunchKernelGGL(ero_fused_kernel, dim3(ceil_div(W, TW), ceil_div(H, TH)), dim3(256), 0, ctx->stream, p,
                               (const float*)src, dst, H, W, pitch);
        } else {
            hipLaunchKernelGGL(ero_flux_kernel, ero_grid(H, W), dim3(64, 4), 0, ctx->stream, p, (const float*)src, dst, H,
                               W, pitch);
            hipLaunchKernelGGL(ero_water_kernel, ero_grid(H, W), dim3(64, 4), 0, ctx->stream, p, (const float*)src, dst, tmp,
                               H, W, pitch);
            hipLaunchKernelGGL(ero_transport_kernel, ero_grid(H, W), dim3(64, 4), 0, ctx->stream, p, dst, (const float*)tmp,
                               H, W, pitch);
        }
        GHM_LAUNCH_CHECK();
        float* t = src;
        src = dst;
        dst = t;
    }
    return 0;
}

int ghm_erosion_emit(ghm_ctx* ctx, const float* state, int32_t H, int32_t W, int32_t pitch, float height_scale, int32_t r0,
                     int32_t c0, int32_t nr, int32_t nc, int32_t out_u8, void* dst, int32_t dst_rows, int32_t dst_pitch,
                     int32_t yoff, int32_t xoff) {
    GHM_CHECK(state && dst && ero_shape_ok(H, W, pitch), "ghm_erosion_emit: bad arguments (H=%d W=%d pitch=%d)", H, W, pitch);
    GHM_CHECK(height_scale > 0.0f && height_scale <= 3.0e38f, "ghm_erosion_emit: height_scale=%g", (double)height_scale);
    GHM_CHECK(r0 >= 0 && c0 >= 0 && nr >= 0 && nc >= 0 && (int64_t)r0 + nr <= H && (int64_t)c0 + nc <= W,
              "ghm_erosion_emit: [%d, %d) x [%d, %d) outside the map of %d x %d", r0, r0 + nr, c0, c0 + nc, H, W);
    GHM_CHECK(dst_rows >= 1 && dst_pitch >= 1 && yoff >= 0 && xoff >= 0 && (int64_t)yoff + nr <= dst_rows &&
                  (int64_t)xoff + nc <= dst_pitch && (int64_t)dst_rows * dst_pitch < ((int64_t)1 << 31),
              "ghm_erosion_emit: rows [%d, %d) x columns [%d, %d) outside the destination of %d x %d", yoff, yoff + nr, xoff,
              xoff + nc, dst_rows, dst_pitch);
    if (nr == 0 || nc == 0) return 0;
    hipLaunchKernelGGL(ero_emit_kernel, ero_grid(nr, nc), dim3(64, 4), 0, ctx->stream, state, pitch, height_scale, r0, c0,
                       nr, nc, out_u8 ? 1 : 0, dst, dst_pitch, yoff, xoff);
    GHM_LAUNCH_CHECK();
    return 0;
}

int32_t ghm_erosion_tile(int32_t axis) { return axis == 0 ? TH : TW; }

}  // extern "C"
