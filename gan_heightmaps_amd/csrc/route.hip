// How to get from here to there on a heightfield (gan_heightmaps_amd/route.py): the least travel cost from a set of
// sources to every cell of the 8-neighbour grid, and the neighbour each cell leaves through.  Neighbours k = 0 .. 7 are
// N NE E SE S SW W NW, hydrology's order, so the parent plane reads as a direction plane.
//
// Edge weights (one launch).  z = height_scale (h + 0); P[c] = ((penalty[c] lake_c) ford_c), lake_c = lake where depth[c] >
// lake_min_depth, ford_c = ford where accumulation[c] >= river_threshold, 1 otherwise and where the plane is absent.  Between a
// cell a and its neighbour b in direction k, every float32 operation rounded on its own (no contraction, no division):
//   g = |z_a - z_b| R_k, R_k = 1 or 0.70710678f;  s = g inv_grade;  f = 1 + s s;  m = 0.5 (P_a + P_b);
//   w = (L_k m) f, L_k = 1 or 1.41421356f;  q = 0 (no edge) if w is not finite, else max(1, rint(min(64 w, 2^24))).
// Every operation is symmetric in a and b, so q_k(a) = q_{k+4}(b) in the same bits and four planes (E, SE, S, SW) hold all
// edges; an edge that leaves the plane is 0.
//
// The cost C (uint32, in units of 1 / 64) is the fixed point of
//   C[c] = 0 at a source, min over the present edges to reached neighbours of C[n_k] + q_k(c) elsewhere,
// the sum formed without wrapping and accepted only below UNREACHED = 0xFFFFFFFF, relaxed downward from UNREACHED.
// Why any schedule gives the same numbers.  The map is monotone: lower inputs never give a higher output.  The start lies at or
// above the fixed point, so every value ever computed, from inputs of any age, is (a) at or above the fixed point and (b) at or
// below what the cell held before -- the new value is the least of the old one and the candidates.  A cell is written by one
// owner only, and a 32-bit load cannot tear: it sees a value that was once stored.  So a tile may read its neighbours' cells of
// either generation, mid-launch: cross-tile reads may be stale, which makes them late, never wrong.  The values are integers in
// [0, 2^32), so the descent ends, at a state that one more pass leaves alone.  All weights are positive integers, so that state
// is unique and is what a heap Dijkstra gives: by induction along the order in which Dijkstra settles cells, a settled cell's
// value at the fixed point is its distance.  Integer sums do not round, so the two forms agree bit for bit:
//   plain : one launch is one Jacobi sweep between two global planes (the output and a workspace plane, alternating);
//   tiled : a 256-thread block stages a 32 x 32 tile of C and its one-cell apron in LDS, keeps the eight incoming weights of the
//           four cells each thread owns in registers, sweeps the tile in place until it stops changing -- at most RT_INNER
//           times, a compile-time cap -- and writes back the cells that fell.
// After k sweeps of either form a cell holds at most the cost of its best path of k edges, and no shortest path has more than
// H W - 1: sweep H W is the first that is sure to change nothing, so the host loop (relax.h) sends it out alone and refuses to
// go further.
//
// The parent of a cell (one launch): -1 at a source (cost 0: weights are >= 1, so no other cell has it), -2 at an unreached
// cell, else the lowest k with a present edge, a reached neighbour and C[n_k] + q_k(c) == C[c].  Parents strictly descend in
// cost: a forest rooted at the sources.
#include "common.h"
#include "relax.h"

// the weights' products, sums and the subtraction are rounded one by one (tests/route_ref.py restates them)
#pragma clang fp contract(off)

namespace {

constexpr int RT_TILE = GHM_ROUTE_TILE;
constexpr int RT_LDS = RT_TILE + 2;                   // the tile and its apron
constexpr int RT_INNER = GHM_ROUTE_INNER_SWEEPS;
constexpr unsigned RT_UNREACHED = GHM_ROUTE_UNREACHED;
constexpr int RT_GROUP_PLAIN = 8, RT_GROUP_TILED = 4;
constexpr int64_t RT_HEADER = 256;                    // bytes in front of the workspace: the device word
constexpr int64_t RT_SOURCE_BYTES = (int64_t)sizeof(int32_t) * GHM_ROUTE_MAX_SOURCES;

__host__ __device__ constexpr int rt_dy(int k) { return (k == 7 || k <= 1) ? -1 : (k >= 3 && k <= 5) ? 1 : 0; }
__host__ __device__ constexpr int rt_dx(int k) { return (k >= 1 && k <= 3) ? 1 : (k >= 5) ? -1 : 0; }

// the weight of the edge between the cell (r, c) and its neighbour k, 0 if there is none: the cell's own plane for E SE S SW,
// the neighbour's plane of the opposite direction for W NW N NE
__device__ __forceinline__ unsigned rt_q(const unsigned* __restrict__ q, size_t n, int r, int c, int H, int W, int k) {
    const int y = r + rt_dy(k), x = c + rt_dx(k);
    if (y < 0 || y >= H || x < 0 || x >= W) return 0u;
    return (k >= 2 && k <= 5) ? q[(size_t)(k - 2) * n + (size_t)r * W + c] : q[(size_t)((k + 4) % 8 - 2) * n + (size_t)y * W + x];
}

// ---- the edge weights -------------------------------------------------------------------------------------------------------
struct WeightArgs {
    const float *h, *penalty, *depth;
    const unsigned* acc;
    unsigned* q;
    int H, W, ph, pp, pd, pa;
    unsigned threshold;
    float scale, inv_grade, lake, ford, min_depth;
};

__device__ __forceinline__ float rt_penalty(const WeightArgs& a, int r, int c) {
    const float p = a.penalty ? a.penalty[(long)r * a.pp + c] : 1.0f;
    const float lake = (a.depth && a.depth[(long)r * a.pd + c] > a.min_depth) ? a.lake : 1.0f;
    const float ford = (a.acc && a.acc[(long)r * a.pa + c] >= a.threshold) ? a.ford : 1.0f;
    return (p * lake) * ford;
}

__global__ __launch_bounds__(256) void rt_weights_kernel(const WeightArgs a) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    if (r >= a.H || c >= a.W) return;
    const size_t n = (size_t)a.H * a.W, at = (size_t)r * a.W + c;
    const float za = a.scale * (a.h[(long)r * a.ph + c] + 0.0f);
    const float pa = rt_penalty(a, r, c);
#pragma unroll
    for (int k = 2; k <= 5; ++k) {
        const int y = r + rt_dy(k), x = c + rt_dx(k);
        unsigned q = 0u;
        if (y < a.H && x >= 0 && x < a.W) {
            const float zb = a.scale * (a.h[(long)y * a.ph + x] + 0.0f);
            const float d = za - zb;
            const float g = fabsf(d) * ((k & 1) ? 0.70710678f : 1.0f);
            const float s = g * a.inv_grade;
            const float ss = s * s;
            const float f = 1.0f + ss;
            const float sum = pa + rt_penalty(a, y, x);
            const float m = 0.5f * sum;
            const float lm = ((k & 1) ? 1.41421356f : 1.0f) * m;
            const float w = lm * f;
            if (fabsf(w) <= 3.4028235e38f) q = max(1u, (unsigned)rintf(fminf(w * (float)GHM_ROUTE_UNIT, (float)GHM_ROUTE_MAX_WEIGHT)));
        }
        a.q[(size_t)(k - 2) * n + at] = q;
    }
}

// ---- the cost ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rt_init_kernel(unsigned* __restrict__ cost, int pc, int H, int W) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    if (r >= H || c >= W) return;
    cost[(long)r * pc + c] = RT_UNREACHED;
}

// at[i]: the offset of source i in the cost plane, rows of its pitch (computed and checked on the host)
__global__ __launch_bounds__(256) void rt_seed_kernel(const int* __restrict__ at, int count, unsigned* __restrict__ cost) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) cost[at[i]] = 0u;
}

// the least of ``best`` and the candidate through a neighbour that holds cn over an edge of weight w (0: none); cn + w does not
// wrap and stays below UNREACHED exactly when w < UNREACHED - cn, which an unreached neighbour (a difference of 0) never meets
__device__ __forceinline__ unsigned rt_try(unsigned best, unsigned cn, unsigned w) {
    return (w != 0u && w < RT_UNREACHED - cn) ? min(best, cn + w) : best;
}

__global__ __launch_bounds__(256) void rt_plain_kernel(const unsigned* __restrict__ q, const unsigned* __restrict__ src, int ps,
                                                       unsigned* __restrict__ dst, int pd, int H, int W, int* word) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    int changed = 0;
    if (r < H && c < W) {
        const size_t n = (size_t)H * W;
        const unsigned old = src[(long)r * ps + c];
        unsigned best = old;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned w = rt_q(q, n, r, c, H, W, k);          // 0 wherever the neighbour is outside the plane
            if (w != 0u) best = rt_try(best, src[(long)(r + rt_dy(k)) * ps + (c + rt_dx(k))], w);
        }
        dst[(long)r * pd + c] = best;
        changed = best != old;
    }
    hyd_raise(changed, word);
}

// thread tid of a tile's block owns the cells (tid / 32 + 8 n, tid % 32) of the tile, n = 0 .. 3
__global__ __launch_bounds__(256) void rt_tiled_kernel(const unsigned* __restrict__ q, unsigned* cost, int pc, int H, int W,
                                                       int* word) {
    __shared__ unsigned t[RT_LDS][RT_LDS];
    const int tid = threadIdx.x, ty = blockIdx.y * RT_TILE, tx = blockIdx.x * RT_TILE;
    for (int i = tid; i < RT_LDS * RT_LDS; i += 256) {
        const int lr = i / RT_LDS, lc = i - lr * RT_LDS;
        const int r = ty - 1 + lr, c = tx - 1 + lc;
        t[lr][lc] = (r >= 0 && r < H && c >= 0 && c < W) ? cost[(long)r * pc + c] : RT_UNREACHED;
    }
    const int lc = (tid & 31) + 1, c = tx + (tid & 31);
    const size_t n = (size_t)H * W;
    unsigned qv[4][8], first[4];
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = ty + (tid >> 5) + 8 * i;
        live[i] = r < H && c < W;
#pragma unroll
        for (int k = 0; k < 8; ++k) qv[i][k] = live[i] ? rt_q(q, n, r, c, H, W, k) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) first[i] = t[(tid >> 5) + 8 * i + 1][lc];
    for (int s = 0; s < RT_INNER; ++s) {
        int ch = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!live[i]) continue;
            const int lr = (tid >> 5) + 8 * i + 1;
            const unsigned cur = t[lr][lc];
            unsigned best = cur;
#pragma unroll
            for (int k = 0; k < 8; ++k) best = rt_try(best, t[lr + rt_dy(k)][lc + rt_dx(k)], qv[i][k]);
            if (best != cur) {
                t[lr][lc] = best;
                ch = 1;
            }
        }
        if (!__syncthreads_or(ch)) break;
    }
    int changed = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!live[i]) continue;
        const int lr = (tid >> 5) + 8 * i + 1;
        const unsigned v = t[lr][lc];
        if (v != first[i]) {
            cost[(long)(ty + lr - 1) * pc + c] = v;
            changed = 1;
        }
    }
    hyd_raise(changed, word);
}

// ---- the parents ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rt_parents_kernel(const unsigned* __restrict__ q, const unsigned* __restrict__ cost, int pc,
                                                         int H, int W, signed char* __restrict__ parent, int pp) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    if (r >= H || c >= W) return;
    const size_t n = (size_t)H * W;
    const unsigned mine = cost[(long)r * pc + c];
    int best = mine == RT_UNREACHED ? GHM_ROUTE_NO_PARENT : -1;
    if (mine != RT_UNREACHED && mine != 0u) {
#pragma unroll
        for (int k = 7; k >= 0; --k) {
            const unsigned w = rt_q(q, n, r, c, H, W, k);
            if (w != 0u) {
                const unsigned cn = cost[(long)(r + rt_dy(k)) * pc + (c + rt_dx(k))];
                if (w < RT_UNREACHED - cn && cn + w == mine) best = k;
            }
        }
    }
    parent[(long)r * pp + c] = (signed char)best;
}

#define RT_PLANE_GRID(H, W) dim3(ceil_div((W), 64), ceil_div((H), 4)), dim3(64, 4), 0, ctx->stream
#define RT_TILE_GRID(H, W) dim3(ceil_div((W), RT_TILE), ceil_div((H), RT_TILE)), dim3(256), 0, ctx->stream

unsigned* rt_planes(void* workspace) { return (unsigned*)((char*)workspace + RT_HEADER + RT_SOURCE_BYTES); }

}  // namespace

extern "C" {

int64_t ghm_route_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return -1;
    return RT_HEADER + RT_SOURCE_BYTES + 5 * (int64_t)sizeof(uint32_t) * H * W;
}

int ghm_route_weights(ghm_ctx* ctx, const float* h, int32_t H, int32_t W, int32_t pitch, const float* penalty, int32_t p_pitch,
                      const float* depth, int32_t depth_pitch, const uint32_t* accumulation, int32_t a_pitch, float height_scale,
                      double grade, float lake, float ford, uint32_t river_threshold, float lake_min_depth, void* workspace) {
    GHM_CHECK(ctx && h && workspace, "ghm_route_weights: null pointer");
    if (int rc = hyd_check_plane("ghm_route_weights", H, W, pitch, "h")) return rc;
    if (penalty)
        if (int rc = hyd_check_plane("ghm_route_weights", H, W, p_pitch, "penalty")) return rc;
    if (depth)
        if (int rc = hyd_check_plane("ghm_route_weights", H, W, depth_pitch, "depth")) return rc;
    if (accumulation)
        if (int rc = hyd_check_plane("ghm_route_weights", H, W, a_pitch, "accumulation")) return rc;
    const float inv_grade = (float)(1.0 / grade);
    GHM_CHECK(grade > 0.0 && grade <= 1.0e300 && inv_grade > 0.0f && inv_grade <= 3.0e38f,
              "ghm_route_weights: grade=%g (positive and finite, and so must 1 / grade be in float32)", grade);
    GHM_CHECK(height_scale > 0.0f && height_scale <= 3.0e38f, "ghm_route_weights: height_scale=%g (positive and finite)",
              (double)height_scale);
    GHM_CHECK(lake >= 1.0f, "ghm_route_weights: lake=%g (>= 1; +inf makes lakes impassable)", (double)lake);
    GHM_CHECK(ford >= 1.0f && ford <= 3.0e38f, "ghm_route_weights: ford=%g (>= 1 and finite)", (double)ford);
    GHM_CHECK(lake_min_depth >= 0.0f && lake_min_depth <= 3.0e38f, "ghm_route_weights: lake_min_depth=%g", (double)lake_min_depth);
    WeightArgs a;
    a.h = h;
    a.penalty = penalty;
    a.depth = depth;
    a.acc = accumulation;
    a.q = rt_planes(workspace);
    a.H = H;
    a.W = W;
    a.ph = pitch;
    a.pp = p_pitch;
    a.pd = depth_pitch;
    a.pa = a_pitch;
    a.threshold = river_threshold;
    a.scale = height_scale;
    a.inv_grade = inv_grade;
    a.lake = lake;
    a.ford = ford;
    a.min_depth = lake_min_depth;
    hipLaunchKernelGGL(rt_weights_kernel, RT_PLANE_GRID(H, W), a);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_route_relax(ghm_ctx* ctx, int32_t H, int32_t W, const int32_t* sources, int32_t nsources, int32_t tiled, int32_t resume,
                    uint32_t* cost, int32_t c_pitch, void* workspace, int64_t* sweeps, int32_t* changed) {
    if (int rc = hyd_sync_ok(ctx, "ghm_route_relax")) return rc;
    GHM_CHECK(sources && cost && workspace, "ghm_route_relax: null pointer");
    if (int rc = hyd_check_plane("ghm_route_relax", H, W, c_pitch, "cost")) return rc;
    GHM_CHECK(nsources >= 1 && nsources <= GHM_ROUTE_MAX_SOURCES, "ghm_route_relax: %d sources (1 .. %d)", nsources,
              GHM_ROUTE_MAX_SOURCES);
    const int64_t cap = (int64_t)H * W;
    std::vector<int32_t> at((size_t)nsources);
    for (int i = 0; i < nsources; ++i) {
        GHM_CHECK(sources[i] >= 0 && sources[i] < cap, "ghm_route_relax: source %d, the flat index %d, lies outside the %d x %d plane",
                  i, sources[i], H, W);
        at[(size_t)i] = (sources[i] / W) * c_pitch + sources[i] % W;
    }
    int* word = (int*)workspace;
    int* d_at = (int*)((char*)workspace + RT_HEADER);
    const unsigned* q = rt_planes(workspace);
    unsigned* other = rt_planes(workspace) + 4 * (size_t)cap;
    GHM_HIP(hipMemcpyAsync(d_at, at.data(), sizeof(int32_t) * (size_t)nsources, hipMemcpyHostToDevice, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));            // ``at`` may go now
    if (!resume) hipLaunchKernelGGL(rt_init_kernel, RT_PLANE_GRID(H, W), cost, c_pitch, H, W);
    hipLaunchKernelGGL(rt_seed_kernel, dim3(ceil_div(nsources, 256)), dim3(256), 0, ctx->stream, d_at, nsources, cost);
    if (tiled)
        return hyd_relax(ctx, "ghm_route_relax", word, RT_GROUP_TILED, cap, [&](int64_t) {
            hipLaunchKernelGGL(rt_tiled_kernel, RT_TILE_GRID(H, W), q, cost, c_pitch, H, W, word);
        }, sweeps, changed, true);
    // the first group that changes nothing leaves the same plane on both sides, whatever the parity of the count
    return hyd_relax(ctx, "ghm_route_relax", word, RT_GROUP_PLAIN, cap, [&](int64_t i) {
        if (i & 1)
            hipLaunchKernelGGL(rt_plain_kernel, RT_PLANE_GRID(H, W), q, other, W, cost, c_pitch, H, W, word);
        else
            hipLaunchKernelGGL(rt_plain_kernel, RT_PLANE_GRID(H, W), q, cost, c_pitch, other, W, H, W, word);
    }, sweeps, changed, true);
}

int ghm_route_parents(ghm_ctx* ctx, const uint32_t* cost, int32_t c_pitch, int32_t H, int32_t W, int8_t* parent, int32_t p_pitch,
                      void* workspace) {
    GHM_CHECK(ctx && cost && parent && workspace, "ghm_route_parents: null pointer");
    if (int rc = hyd_check_plane("ghm_route_parents", H, W, c_pitch, "cost")) return rc;
    if (int rc = hyd_check_plane("ghm_route_parents", H, W, p_pitch, "parent")) return rc;
    hipLaunchKernelGGL(rt_parents_kernel, RT_PLANE_GRID(H, W), rt_planes(workspace), cost, c_pitch, H, W, (signed char*)parent,
                       p_pitch);
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
