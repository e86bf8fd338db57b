// The light of the sky on a heightfield (gan_heightmaps_amd/skylight.py): per texel the share of a uniform sky a
// horizontal patch receives over the horizon the surrounding heights raise.  A table of directions x steps samples (built
// by the host in float64: integer offsets, bilinear weights, 1 / distance) is scanned per texel; per direction the largest
// slope towards a sample is the horizon's tangent T, its share of light 1 / (1 + (height_scale T)^2) = cos^2 of the
// horizon's elevation.  Positions enter through the table's offsets and weights alone, never through an absolute
// coordinate: a texel's value does not depend on the window it is baked in.
// Two forms that run the same per-sample function, so their results agree bit for bit:
//   plain : one thread per output texel, gathers from global memory with clamped indices;
//   tiled : a 256-thread block owns 32 x 32 outputs, stages their (32 + 2 reach + 1)^2 window in LDS (the clamping to the
//           source's edges resolved while staging) and gathers from there.
// The table is read with wave-uniform indices.  No atomics, no reductions.
#include "common.h"

// every product, sum and quotient is rounded on its own, in the order written (tests/skylight_ref.py restates it)
#pragma clang fp contract(off)

namespace {

constexpr int SKY_TILE = GHM_SKYLIGHT_TILE;
constexpr int SKY_MAX_LDS = GHM_SKYLIGHT_MAX_LDS;

typedef ghm_skylight_sample SS;

// the side of the window a tile of the tiled form stages
__host__ __device__ inline int sky_window(int reach) { return SKY_TILE + 2 * reach + 1; }

// the slope from a texel of height h0 towards one sample; rp(y, x) reads the plane at any position the table reaches
template <class RP>
__device__ __forceinline__ float sky_slope(RP rp, int i, int j, const SS& s, float h0) {
    const int y = i + s.iy, x = j + s.ix;
    const float a = rp(y, x), b = rp(y, x + 1), c = rp(y + 1, x), e = rp(y + 1, x + 1);
    const float t = a + s.wx * (b - a);
    const float u = c + s.wx * (e - c);
    const float hv = t + s.wy * (u - t);
    return (hv - h0) * s.inv_r;
}

// N texels at (i[n], j[n]) scanned together, so that every table entry is loaded once for all of them
template <int N, class RP>
__device__ __forceinline__ void sky_texels(RP rp, const SS* __restrict__ table, int directions, int steps, float hs,
                                           float strength, const int* i, const int* j, float* sky) {
    float h0[N], sum[N];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        h0[n] = rp(i[n], j[n]);
        sum[n] = 0.0f;
    }
    for (int d = 0; d < directions; ++d) {
        float T[N];
#pragma unroll
        for (int n = 0; n < N; ++n) T[n] = 0.0f;
        for (int m = 0; m < steps; ++m) {
            const SS s = table[d * steps + m];
#pragma unroll
            for (int n = 0; n < N; ++n) T[n] = fmaxf(T[n], sky_slope(rp, i[n], j[n], s, h0[n]));
        }
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const float q = hs * T[n];
            sum[n] = sum[n] + __fdiv_rn(1.0f, 1.0f + q * q);
        }
    }
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const float V = __fdiv_rn(sum[n], (float)directions);
        sky[n] = 1.0f - strength * (1.0f - V);
    }
}

// fp32, or the uint8 map of ghm_world_crop for a unit-range plane: rint((double)v * 255), half to even
__device__ __forceinline__ void sky_store(void* __restrict__ out, long at, float v, int out_u8) {
    if (out_u8)
        ((unsigned char*)out)[at] = (unsigned char)(int)rint((double)v * 255.0);
    else
        ((float*)out)[at] = v;
}

struct SkyArgs {
    const float* src;
    const SS* table;
    void* out;
    int rows, cols, pitch;          // the source plane
    int directions, steps, reach;
    int y0, x0, h, w;               // the rectangle of outputs inside the source
    int out_pitch, out_u8;
    float hs, strength;
};

// ---- the plain form: blocks of 64 x 4 texels, one texel per thread --------------------------------------------------------
__global__ __launch_bounds__(256) void sky_plain_kernel(const SkyArgs k) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    const int r = blockIdx.y * 4 + threadIdx.y;
    if (r >= k.h || c >= k.w) return;
    const float* __restrict__ src = k.src;
    auto rp = [&](int y, int x) {
        return src[(long)min(max(y, 0), k.rows - 1) * k.pitch + min(max(x, 0), k.cols - 1)];
    };
    const int i = k.y0 + r, j = k.x0 + c;
    float v;
    sky_texels<1>(rp, k.table, k.directions, k.steps, k.hs, k.strength, &i, &j, &v);
    sky_store(k.out, (long)r * k.out_pitch + c, v, k.out_u8);
}

// ---- the tiled form ---------------------------------------------------------------------------------------------------------
// staging: the window of the tile whose first output is (ty, tx) of the rectangle; element (r, c) of the window is the source
// at (y0 + ty - reach + r, x0 + tx - reach + c), clamped to the source
__device__ __forceinline__ void sky_stage(const SkyArgs& k, float* lds, int ty, int tx, int tid) {
    const int WW = sky_window(k.reach);
    const int wy0 = k.y0 + ty - k.reach, wx0 = k.x0 + tx - k.reach;
    const float* __restrict__ src = k.src;
    for (int n = tid; n < WW * WW; n += 256) {
        const int r = n / WW, c = n - r * WW;
        const int y = min(max(wy0 + r, 0), k.rows - 1), x = min(max(wx0 + c, 0), k.cols - 1);
        lds[n] = src[(long)y * k.pitch + x];
    }
}

// compute: thread tid owns the texels (tid / 32 + 8 n, tid % 32) of the tile, n = 0 .. 3
__device__ __forceinline__ void sky_compute(const SkyArgs& k, const float* lds, int ty, int tx, int tid) {
    const int WW = sky_window(k.reach);
    const int wy0 = k.y0 + ty - k.reach, wx0 = k.x0 + tx - k.reach;
    auto rp = [&](int y, int x) { return lds[(y - wy0) * WW + (x - wx0)]; };
    int i[4], j[4];
    float v[4];
    // a texel of the tile outside the rectangle lies inside the window all the same: it is computed and never stored
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        i[n] = k.y0 + ty + (tid >> 5) + 8 * n;
        j[n] = k.x0 + tx + (tid & 31);
    }
    sky_texels<4>(rp, k.table, k.directions, k.steps, k.hs, k.strength, i, j, v);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int r = ty + (tid >> 5) + 8 * n, c = tx + (tid & 31);
        if (r < k.h && c < k.w) sky_store(k.out, (long)r * k.out_pitch + c, v[n], k.out_u8);
    }
}

__global__ __launch_bounds__(256) void sky_tiled_kernel(const SkyArgs k) {
    HIP_DYNAMIC_SHARED(float, sky_lds)
    const int ty = blockIdx.y * SKY_TILE, tx = blockIdx.x * SKY_TILE;
    sky_stage(k, sky_lds, ty, tx, threadIdx.x);
    __syncthreads();
    sky_compute(k, sky_lds, ty, tx, threadIdx.x);
}

}  // namespace

extern "C" {

int64_t ghm_skylight_lds_bytes(int32_t reach) {
    if (reach < 1) return -1;
    const int64_t n = (int64_t)SKY_TILE + 2 * (int64_t)reach + 1;
    const int64_t bytes = n * n * (int64_t)sizeof(float);
    return bytes <= SKY_MAX_LDS ? bytes : -1;
}

int ghm_skylight_bake(ghm_ctx* ctx, const float* src, int32_t rows, int32_t cols, int32_t pitch,
                      const ghm_skylight_sample* table, int32_t directions, int32_t steps, int32_t reach, int32_t y0,
                      int32_t x0, int32_t h, int32_t w, float height_scale, float strength, int32_t tiled, int32_t out_u8,
                      void* out, int32_t out_pitch) {
    GHM_CHECK(src && table && out, "ghm_skylight_bake: null pointer");
    GHM_CHECK(rows >= 1 && cols >= 1 && pitch >= cols && (int64_t)rows * pitch < ((int64_t)1 << 31),
              "ghm_skylight_bake: source %d x %d with a pitch of %d out of range", rows, cols, pitch);
    GHM_CHECK(y0 >= 0 && x0 >= 0 && h >= 1 && w >= 1 && (int64_t)y0 + h <= rows && (int64_t)x0 + w <= cols,
              "ghm_skylight_bake: [%d, %d) x [%d, %d) outside the source of %d x %d", y0, y0 + h, x0, x0 + w, rows, cols);
    GHM_CHECK((int64_t)h * w < ((int64_t)1 << 31) && out_pitch >= w && (int64_t)h * out_pitch < ((int64_t)1 << 31) &&
                  h <= 4 * 65535,
              "ghm_skylight_bake: output %d x %d with a pitch of %d out of range", h, w, out_pitch);
    GHM_CHECK(directions >= 1 && directions <= GHM_SKYLIGHT_MAX_DIRECTIONS && steps >= 1 && steps <= GHM_SKYLIGHT_MAX_STEPS,
              "ghm_skylight_bake: directions=%d (1 .. %d), steps=%d (1 .. %d)", directions, GHM_SKYLIGHT_MAX_DIRECTIONS, steps,
              GHM_SKYLIGHT_MAX_STEPS);
    GHM_CHECK(reach >= 1, "ghm_skylight_bake: reach=%d", reach);
    GHM_CHECK(height_scale > 0.0f && height_scale <= 3.0e38f, "ghm_skylight_bake: height_scale=%g", (double)height_scale);
    GHM_CHECK(strength >= 0.0f && strength <= 1.0f, "ghm_skylight_bake: strength=%g outside [0, 1]", (double)strength);
    SkyArgs k;
    k.src = src;
    k.table = table;
    k.out = out;
    k.rows = rows;
    k.cols = cols;
    k.pitch = pitch;
    k.directions = directions;
    k.steps = steps;
    k.reach = reach;
    k.y0 = y0;
    k.x0 = x0;
    k.h = h;
    k.w = w;
    k.out_pitch = out_pitch;
    k.out_u8 = out_u8 ? 1 : 0;
    k.hs = height_scale;
    k.strength = strength;
    if (tiled) {
        const int64_t lds = ghm_skylight_lds_bytes(reach);
        GHM_CHECK(lds > 0, "ghm_skylight_bake: the tiled form's window for reach=%d exceeds %d bytes of LDS: use the plain form",
                  reach, SKY_MAX_LDS);
        static bool opted_in = false;
        if (!opted_in) {
            GHM_HIP(hipFuncSetAttribute((const void*)sky_tiled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        SKY_MAX_LDS));
            opted_in = true;
        }
        hipLaunchKernelGGL(sky_tiled_kernel, dim3(ceil_div(w, SKY_TILE), ceil_div(h, SKY_TILE)), dim3(256), (size_t)lds,
                           ctx->stream, k);
    } else {
        hipLaunchKernelGGL(sky_plain_kernel, dim3(ceil_div(w, 64), ceil_div(h, 4)), dim3(64, 4), 0, ctx->stream, k);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
