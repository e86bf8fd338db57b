// Sliced Wasserstein distance on Laplacian-pyramid patches (gan_heightmaps_amd/swd.py, include/ghm.h):
// the pyramid, the descriptor gather, per-channel statistics, the projection onto random directions, an exact column
// sort and the mean absolute difference.  fp32 throughout with `fp contract(off)` where the restatement
// (tests/swd_ref.py) is held to a derived bound; every reduction runs in double in a fixed order (no atomics), so a
// result never depends on scheduling.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int PATCH = GHM_SWD_PATCH;                 // 7
constexpr int PP = PATCH * PATCH;                    // 49 values per channel of a descriptor
constexpr int KMAX = GHM_SWD_MAX_K;                  // 196 = 4 channels
constexpr int NPART = GHM_SWD_PARTIALS;              // blocks of the two reductions
constexpr int SORT_MAX = GHM_SWD_SORT_MAX_CHUNK;     // 2^15 floats = 128 KiB of the CU's 160 KiB of LDS

// the reflection without repeating the edge: -1 -> 1, n -> n - 2 (|i| <= 2 beyond either end, n >= 3)
__device__ __forceinline__ int refl(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// ---- pyramid ------------------------------------------------------------------------------------------------------------
// a view: element (n, c, y, x) at n * ns + c * cs + y * pitch + x
struct View {
    long ns, cs;
    int pitch;
};

// G_{i+1}[n, c, i, j] = the binomial [1 4 6 4 1] / 16 along both axes of G_i around (2 i, 2 j)
__global__ __launch_bounds__(256) void swd_down_kernel(const float* __restrict__ src, View sv, float* __restrict__ dst,
                                                       View dv, int C, int H, int W) {
    const int Hd = H >> 1, Wd = W >> 1;
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    const int nc = blockIdx.z;
    if (i >= Hd || j >= Wd) return;
    const int n = nc / C, c = nc - n * C;
    const float* s = src + n * sv.ns + c * sv.cs;
    int xs[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) xs[t] = refl(2 * j + t - 2, W);
    float rows[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const float* r = s + (long)refl(2 * i + a - 2, H) * sv.pitch;
        rows[a] = ((r[xs[0]] + r[xs[4]]) + 4.0f * (r[xs[1]] + r[xs[3]]) + 6.0f * r[xs[2]]) * 0.0625f;
    }
    dst[n * dv.ns + c * dv.cs + (long)i * dv.pitch + j] =
        ((rows[0] + rows[4]) + 4.0f * (rows[1] + rows[3]) + 6.0f * rows[2]) * 0.0625f;
}

// one row of up(): the value at column x of the zero-stuffed row ``r`` of the coarse image filtered with [1 4 6 4 1] / 8
__device__ __forceinline__ float up_row(const float* __restrict__ r, int x, int W) {
    if (x & 1) return (r[(x - 1) >> 1] + r[refl(x + 1, W) >> 1]) * 0.5f;
    return ((r[refl(x - 2, W) >> 1] + r[refl(x + 2, W) >> 1]) + 6.0f * r[x >> 1]) * 0.125f;
}

// Lap_i = G_i - up(G_{i+1}) over the H x W cells of G_i (the reflection keeps the parity of an index: H and W are even)
__global__ __launch_bounds__(256) void swd_lap_kernel(const float* __restrict__ fine, View fv, const float* __restrict__ coarse,
                                                      View cv, float* __restrict__ dst, View dv, int C, int H, int W) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    const int nc = blockIdx.z;
    if (y >= H || x >= W) return;
    const int n = nc / C, c = nc - n * C;
    const float* g = coarse + n * cv.ns + c * cv.cs;
    float u;
    if (y & 1) {
        u = (up_row(g + (long)((y - 1) >> 1) * cv.pitch, x, W) + up_row(g + (long)(refl(y + 1, H) >> 1) * cv.pitch, x, W)) * 0.5f;
    } else {
        u = ((up_row(g + (long)(refl(y - 2, H) >> 1) * cv.pitch, x, W) + up_row(g + (long)(refl(y + 2, H) >> 1) * cv.pitch, x, W)) +
             6.0f * up_row(g + (long)(y >> 1) * cv.pitch, x, W)) * 0.125f;
    }
    dst[n * dv.ns + c * dv.cs + (long)y * dv.pitch + x] = fine[n * fv.ns + c * fv.cs + (long)y * fv.pitch + x] - u;
}

__global__ __launch_bounds__(256) void swd_copy_kernel(const float* __restrict__ src, View sv, float* __restrict__ dst, View dv,
                                                       int C, int H, int W) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    const int nc = blockIdx.z;
    if (y >= H || x >= W) return;
    const int n = nc / C, c = nc - n * C;
    dst[n * dv.ns + c * dv.cs + (long)y * dv.pitch + x] = src[n * sv.ns + c * sv.cs + (long)y * sv.pitch + x];
}

// ---- gather -------------------------------------------------------------------------------------------------------------
// desc[(row0 + r) * K + c * 49 + dy * 7 + dx] = img[r / P, c, cy + dy, cx + dx], (cy, cx) = corners[r].  The host refuses a
// corner outside [0, H - 7] x [0, W - 7] before it uploads the table; the clamp only keeps a bad table inside the image.
__global__ __launch_bounds__(256) void swd_gather_kernel(const float* __restrict__ img, View v, int H, int W,
                                                         const int* __restrict__ corners, int P, int K, long rows,
                                                         float* __restrict__ desc, long row0) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * K) return;
    const long r = t / K;
    const int k = (int)(t - r * K);
    const int c = k / PP, q = k - c * PP;
    const int dy = q / PATCH, dx = q - dy * PATCH;
    const int cy = min(max(corners[2 * r], 0), H - PATCH), cx = min(max(corners[2 * r + 1], 0), W - PATCH);
    desc[(row0 + r) * K + k] = img[(r / P) * v.ns + c * v.cs + (long)(cy + dy) * v.pitch + cx + dx];
}

// ---- reductions in double, fixed order --------------------------------------------------------------------------------
// 256 doubles summed by a tree whose shape depends on nothing but the thread index
__device__ __forceinline__ double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

// part[(c * NPART + b) * 2 + {0, 1}] = sum / sum of squares of channel c over block b's share of the N x 49 values
__global__ __launch_bounds__(256) void swd_stats_partial_kernel(const float* __restrict__ desc, long N, int K, double* __restrict__ part) {
    __shared__ double sh[256];
    const int b = blockIdx.x, c = blockIdx.y;
    const long total = N * PP;
    double s = 0.0, s2 = 0.0;
    for (long e = (long)b * 256 + threadIdx.x; e < total; e += (long)NPART * 256) {
        const long n = e / PP;
        const double v = (double)desc[n * K + c * PP + (int)(e - n * PP)];
        s += v;
        s2 += v * v;
    }
    const double S = block_sum(s, sh);
    const double S2 = block_sum(s2, sh);
    if (threadIdx.x == 0) {
        part[((long)c * NPART + b) * 2] = S;
        part[((long)c * NPART + b) * 2 + 1] = S2;
    }
}

// stats[2 c] = mean, stats[2 c + 1] = population standard deviation
__global__ __launch_bounds__(64) void swd_stats_finish_kernel(const double* __restrict__ part, long N, int C, float* __restrict__ stats) {
    const int c = threadIdx.x;
    if (c >= C) return;
    double s = 0.0, s2 = 0.0;
    for (int b = 0; b < NPART; ++b) {
        s += part[((long)c * NPART + b) * 2];
        s2 += part[((long)c * NPART + b) * 2 + 1];
    }
    const double cnt = (double)N * PP;
    const double mean = s / cnt;
    double var = s2 / cnt - mean * mean;
    // a constant channel: the one-pass variance is rounding noise of either sign around 0; against mean^2 it is nothing
    if (var <= mean * mean * 1e-13) var = 0.0;
    stats[2 * c] = (float)mean;
    stats[2 * c + 1] = (float)sqrt(var);
}

__global__ __launch_bounds__(256) void swd_l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, long n,
                                                             double* __restrict__ part) {
    __shared__ double sh[256];
    double s = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)NPART * 256) s += (double)fabsf(a[e] - b[e]);
    const double S = block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = S;
}

__global__ void swd_l1_finish_kernel(const double* __restrict__ part, long n, double* __restrict__ out) {
    double s = 0.0;
    for (int b = 0; b < NPART; ++b) s += part[b];
    out[0] = s / (double)n;
}

// ---- projection ---------------------------------------------------------------------------------------------------------
// out[m * N + n] = sum_k ((desc[n, k] - mean_c) / std_c) dirs[k * M + m]: a block stages 64 normalised rows in LDS (row
// stride K, odd: 49 C with C odd; with C even the 2-way conflict of the column read is paid), every wave then walks the
// directions with one m per wave at a time, so dirs[k, m] is a wave-uniform load and the store to out is coalesced
constexpr int PROJ_ROWS = 64;
__global__ __launch_bounds__(256) void swd_project_kernel(const float* __restrict__ desc, long N, int K, const float* __restrict__ dirs,
                                                          int M, const float* __restrict__ stats, float* __restrict__ out) {
    __shared__ float xs[PROJ_ROWS * KMAX];
    const long n0 = (long)blockIdx.x * PROJ_ROWS;
    const int rows = (int)(N - n0 < PROJ_ROWS ? N - n0 : PROJ_ROWS);
    for (int e = threadIdx.x; e < rows * K; e += 256) {
        const int r = e / K, k = e - r * K;
        const int c = k / PP;
        xs[e] = __fdiv_rn(desc[(n0 + r) * K + k] - stats[2 * c], stats[2 * c + 1]);
    }
    __syncthreads();
    const int r = threadIdx.x & 63;
    if (r >= rows) return;
    const float* x = xs + r * K;
    for (int m = threadIdx.x >> 6; m < M; m += 4) {
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) acc = fmaf(x[k], dirs[(long)k * M + m], acc);
        out[(long)m * N + n0 + r] = acc;
    }
}

// ---- sort ---------------------------------------------------------------------------------------------------------------
// A bitonic network in the form whose every compare-exchange leaves the smaller value at the lower index: a merge of
// size k starts with a "flip" (i against the mirror position of its k-block) and goes on with half-cleaners of stride
// k/4 .. 1.  With that form a column of any length N sorts in place as if padded to a power of two with +inf: a pair whose
// upper index is >= N would exchange with +inf, which is no exchange, so it is skipped and the padding never exists.
__device__ __forceinline__ void cmpx(float& a, float& b) {
    if (a > b) {
        const float t = a;
        a = b;
        b = t;
    }
}

// One workgroup per (chunk of ``cn`` cells, column), the chunk in LDS (padded there with +inf).  full: sort the chunk
// (every merge up to cn); otherwise: the half-cleaners of stride cn/2 .. 1 that finish a merge begun in global memory.
__global__ __launch_bounds__(1024) void swd_sort_lds_kernel(float* __restrict__ data, long N, int cn, int full) {
    extern __shared__ float s[];
    float* col = data + (long)blockIdx.y * N;
    const long base = (long)blockIdx.x * cn;
    const int T = blockDim.x, tid = threadIdx.x;
    for (int t = tid; t < cn; t += T) s[t] = base + t < N ? col[base + t] : INFINITY;
    __syncthreads();
    const int half = cn >> 1;
    for (int k = full ? 2 : cn; k <= cn; k <<= 1) {
        if (full) {
            for (int p = tid; p < half; p += T) {                     // the flip: i against the mirror of its k-block
                const int q = p & ((k >> 1) - 1);
                const int i = ((p - q) << 1) + q;
                cmpx(s[i], s[i + k - 1 - 2 * q]);
            }
            __syncthreads();
        }
        for (int j = full ? k >> 2 : k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < half; p += T) {
                const int q = p & (j - 1);
                const int i = ((p - q) << 1) + q;
                cmpx(s[i], s[i + j]);
            }
            __syncthreads();
        }
    }
    for (int t = tid; t < cn; t += T)
        if (base + t < N) col[base + t] = s[t];
}

// One compare-exchange pass through global memory over every column: flip != 0: the flip of the merge of size k;
// otherwise the half-cleaner of stride k.  Thread = one pair; pairs whose upper index is >= N are skipped.
__global__ __launch_bounds__(256) void swd_sort_global_kernel(float* __restrict__ data, long N, long pairs, long k, int flip) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    float* col = data + (long)blockIdx.y * N;
    long i, h;
    if (flip) {
        const long q = p & ((k >> 1) - 1);
        i = ((p - q) << 1) + q;
        h = i + k - 1 - 2 * q;
    } else {
        const long q = p & (k - 1);
        i = ((p - q) << 1) + q;
        h = i + k;
    }
    if (h >= N) return;
    const float a = col[i], b = col[h];
    if (a > b) {
        col[i] = b;
        col[h] = a;
    }
}

inline bool view_ok(int n, int C, int H, int W, long ns, long cs, int pitch) {
    return n >= 1 && C >= 1 && H >= 1 && W >= 1 && pitch >= W && cs >= (long)(H - 1) * pitch + W &&
           ns >= (long)(C - 1) * cs + (long)(H - 1) * pitch + W && (long)n * C <= 65535 && H <= 4 * 65535 &&
           (long)n * ns < ((long)1 << 40);
}

inline dim3 img_grid(int n, int C, int H, int W) { return dim3(ceil_div(W, 64), ceil_div(H, 4), n * C); }

inline int pow2_at_least(long n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

extern "C" {

int ghm_swd_pyramid_level(ghm_ctx* ctx, const float* g, int32_t n, int32_t C, int32_t H, int32_t W, int64_t g_nstride,
                          int64_t g_cstride, int32_t g_pitch, float* g_next, int32_t next_pitch, float* lap, int32_t lap_pitch) {
    GHM_CHECK(g && lap && view_ok(n, C, H, W, g_nstride, g_cstride, g_pitch) && lap_pitch >= W,
              "ghm_swd_pyramid_level: bad arguments (n=%d C=%d H=%d W=%d pitch=%d lap_pitch=%d)", n, C, H, W, g_pitch, lap_pitch);
    const View gv = {g_nstride, g_cstride, g_pitch};
    const View lv = {(long)C * H * lap_pitch, (long)H * lap_pitch, lap_pitch};
    if (!g_next) {                                            // the coarsest level: Lap = G
        hipLaunchKernelGGL(swd_copy_kernel, img_grid(n, C, H, W), dim3(64, 4), 0, ctx->stream, g, gv, lap, lv, C, H, W);
        GHM_LAUNCH_CHECK();
        return 0;
    }
    GHM_CHECK(H % 2 == 0 && W % 2 == 0 && H >= 4 && W >= 4 && next_pitch >= W / 2,
              "ghm_swd_pyramid_level: a level of %d x %d cannot be halved (next_pitch=%d)", H, W, next_pitch);
    const View nv = {(long)C * (H / 2) * next_pitch, (long)(H / 2) * next_pitch, next_pitch};
    hipLaunchKernelGGL(swd_down_kernel, img_grid(n, C, H / 2, W / 2), dim3(64, 4), 0, ctx->stream, g, gv, g_next, nv, C, H, W);
    hipLaunchKernelGGL(swd_lap_kernel, img_grid(n, C, H, W), dim3(64, 4), 0, ctx->stream, g, gv, (const float*)g_next, nv, lap,
                       lv, C, H, W);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_swd_gather(ghm_ctx* ctx, const float* img, int32_t n, int32_t C, int32_t H, int32_t W, int32_t pitch,
                   const int32_t* corners, int32_t patches, float* desc, int64_t row_offset, int64_t total_rows) {
    GHM_CHECK(img && corners && desc && n >= 1 && C >= 1 && C * PP <= KMAX && H >= PATCH && W >= PATCH && pitch >= W &&
                  patches >= 1 && row_offset >= 0 && row_offset + (int64_t)n * patches <= total_rows &&
                  total_rows * C * PP < ((int64_t)1 << 40) && (int64_t)n * patches * C * PP < ((int64_t)1 << 38),
              "ghm_swd_gather: bad arguments (n=%d C=%d H=%d W=%d pitch=%d patches=%d row_offset=%lld total_rows=%lld)", n, C, H,
              W, pitch, patches, (long long)row_offset, (long long)total_rows);
    const View v = {(long)C * H * pitch, (long)H * pitch, pitch};
    const long rows = (long)n * patches;
    hipLaunchKernelGGL(swd_gather_kernel, dim3(ceil_div(rows * C * PP, 256)), dim3(256), 0, ctx->stream, img, v, H, W, corners,
                       patches, C * PP, rows, desc, (long)row_offset);
    GHM_LAUNCH_CHECK();
    return 0;
}

int64_t ghm_swd_workspace(void) { return (int64_t)sizeof(double) * 2 * NPART * (KMAX / PP); }

int ghm_swd_stats(ghm_ctx* ctx, const float* desc, int64_t N, int32_t C, float* stats, void* workspace) {
    GHM_CHECK(desc && stats && workspace && N >= 1 && C >= 1 && C * PP <= KMAX && N * C * PP < ((int64_t)1 << 40),
              "ghm_swd_stats: bad arguments (N=%lld C=%d)", (long long)N, C);
    hipLaunchKernelGGL(swd_stats_partial_kernel, dim3(NPART, C), dim3(256), 0, ctx->stream, desc, (long)N, C * PP,
                       (double*)workspace);
    hipLaunchKernelGGL(swd_stats_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double*)workspace, (long)N, C, stats);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_swd_project(ghm_ctx* ctx, const float* desc, int64_t N, int32_t C, const float* dirs, int32_t M, const float* stats,
                    float* out) {
    GHM_CHECK(desc && dirs && stats && out && N >= 1 && C >= 1 && C * PP <= KMAX && M >= 1 && N * C * PP < ((int64_t)1 << 40) &&
                  N * M < ((int64_t)1 << 40) && N <= (int64_t)PROJ_ROWS * 0x7fffffff,
              "ghm_swd_project: bad arguments (N=%lld C=%d M=%d)", (long long)N, C, M);
    hipLaunchKernelGGL(swd_project_kernel, dim3(ceil_div(N, PROJ_ROWS)), dim3(256), 0, ctx->stream, desc, (long)N, C * PP, dirs,
                       M, stats, out);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_swd_sort_columns(ghm_ctx* ctx, float* data, int64_t N, int32_t M, int32_t chunk) {
    GHM_CHECK(data && N >= 1 && N <= ((int64_t)1 << 30) && M >= 1 && M <= 65535 && chunk >= 0 && N * M < ((int64_t)1 << 40),
              "ghm_swd_sort_columns: bad arguments (N=%lld M=%d chunk=%d)", (long long)N, M, chunk);
    if (N == 1) return 0;
    // the chunk an LDS workgroup holds: a power of two in [2, SORT_MAX]; 0 asks for the largest
    int cn = chunk == 0 ? SORT_MAX : chunk;
    cn = cn > SORT_MAX ? SORT_MAX : cn < 2 ? 2 : cn;
    while (cn & (cn - 1)) cn &= cn - 1;                       // round down to a power of two
    static bool opted_in = false;
    if (!opted_in) {
        GHM_HIP(hipFuncSetAttribute((const void*)swd_sort_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    SORT_MAX * (int)sizeof(float)));
        opted_in = true;
    }
    const long P = pow2_at_least(N);
    if (P <= cn) {                                            // the LDS form: the whole column in one workgroup
        const int c = (int)P;
        const int threads = c / 2 >= 1024 ? 1024 : c / 2 < 64 ? 64 : c / 2;
        hipLaunchKernelGGL(swd_sort_lds_kernel, dim3(1, M), dim3(threads), (size_t)c * sizeof(float), ctx->stream, data, (long)N,
                           c, 1);
        GHM_LAUNCH_CHECK();
        return 0;
    }
    // the global form: chunks sorted in LDS, then per merge the strides that span chunks through global memory and the rest
    // in LDS again
    const int threads = cn / 2 >= 1024 ? 1024 : cn / 2 < 64 ? 64 : cn / 2;
    const dim3 lds_grid(ceil_div(N, cn), M);
    const long pairs = P / 2;
    const dim3 glb_grid(ceil_div(pairs, 256), M);
    hipLaunchKernelGGL(swd_sort_lds_kernel, lds_grid, dim3(threads), (size_t)cn * sizeof(float), ctx->stream, data, (long)N, cn, 1);
    for (long k = 2L * cn; k <= P; k <<= 1) {
        hipLaunchKernelGGL(swd_sort_global_kernel, glb_grid, dim3(256), 0, ctx->stream, data, (long)N, pairs, k, 1);
        for (long j = k >> 2; j >= cn; j >>= 1)
            hipLaunchKernelGGL(swd_sort_global_kernel, glb_grid, dim3(256), 0, ctx->stream, data, (long)N, pairs, j, 0);
        hipLaunchKernelGGL(swd_sort_lds_kernel, lds_grid, dim3(threads), (size_t)cn * sizeof(float), ctx->stream, data, (long)N, cn,
                           0);
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int32_t ghm_swd_sort_max_chunk(void) { return SORT_MAX; }

int ghm_swd_l1(ghm_ctx* ctx, const float* a, const float* b, int64_t n, void* workspace, double* result) {
    GHM_CHECK(a && b && workspace && result && n >= 1 && n < ((int64_t)1 << 40), "ghm_swd_l1: bad arguments (n=%lld)",
              (long long)n);
    GHM_CHECK(!ctx->rec && !ctx->capturing, "ghm_swd_l1 returns its result to the host: not inside a recorded step or a capture");
    double* part = (double*)workspace;
    hipLaunchKernelGGL(swd_l1_partial_kernel, dim3(NPART), dim3(256), 0, ctx->stream, a, b, (long)n, part);
    hipLaunchKernelGGL(swd_l1_finish_kernel, dim3(1), dim3(1), 0, ctx->stream, (const double*)part, (long)n, part + NPART);
    GHM_LAUNCH_CHECK();
    GHM_HIP(hipMemcpyAsync(result, part + NPART, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
