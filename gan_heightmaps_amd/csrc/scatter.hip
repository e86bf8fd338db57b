// Scatter on a heightfield (gan_heightmaps_amd/scatter.py): where trees and rocks stand -- a Poisson-disk point set
// whose density follows the terrain, deterministic from a seed and from world coordinates.  Three steps.
//
// 1. The chance -- float32, each operation rounded on its own (no contraction), no sqrt and no division on the device: altitude,
//    slope and the distance to water enter through the host's tables.  chance[y, x] in [0, 2^24] is the probability, in units of
//    2^-24, that the cell is a candidate (include/ghm.h has the operations one by one; tests/scatter_ref.py restates them).
// 2. The candidates -- integers.  hash = the chained "lowbias32" mixer of include/ghm.h over (seed, stream, world row, world col).
//    state = 1 iff hash(stream 0) >> 8 < chance, priority = hash(stream 1): functions of the seed and the world position alone.
// 3. The thinning -- integers.  Two cells conflict iff dy^2 + dx^2 < s2; a candidate is earlier than another iff its
//    (priority, row, col) is less, a strict order.  Dart throwing in that order is the lexicographically first maximal independent
//    set of the conflict graph, and that set is the one fixed point of the local rule
//      an undecided candidate is REJECTED once one earlier candidate in conflict is KEPT,
//                             and KEPT once every earlier candidate in conflict is REJECTED
//    (induction along the order: the earliest undecided candidate always has all its earlier neighbours decided, so it is decided
//    by the next sweep, and by the greedy choice).  A decision is final and rests on final decisions only, so it does not matter
//    how stale the states are that a sweep reads: Jacobi sweeps, in-place sweeps and tiles with stale aprons end in the same bits.
//      plain : one launch per sweep, from one state plane into the other (the second lies in the workspace): every cell is copied,
//              every undecided candidate scans its window in global memory.
//      tiled : a 256-thread block owns a 32 x 32 tile.  A tile without an undecided candidate returns at once.  Otherwise the block
//              stages priorities and states of its (32 + 2R)^2 window in LDS (state 0 outside the plane), R the largest with
//              R^2 < s2, sweeps the tile's cells in place until a sweep decides nothing -- the apron stays as staged -- and writes
//              the decisions back.  Other blocks write their own tiles meanwhile: a staged apron state is that of the launch's
//              start or later, either of which is final if it is a decision.
//    LDS: 4 (32 + 2R)^2 bytes of priorities and (32 + 2R)^2 of states, each rounded up to 16: 44192 bytes at R = 31, three blocks
//    per CU of the MI355X's 160 KiB; at R <= 7 (s2 <= 64) it is under 12 KiB and the LDS does not limit the occupancy.
//    Both forms go through hyd_relax (relax.h): sweeps in groups, one change word read per group, a hard cap of H W + 1 sweeps --
//    a sweep that changes anything decides at least the earliest undecided candidate, so sweep H W + 1 changes nothing.
#include "common.h"
#include "relax.h"

// the chance's products and sums are rounded one by one (tests/scatter_ref.py restates them)
#pragma clang fp contract(off)

namespace {

constexpr int SC_TILE = GHM_SCATTER_TILE;
constexpr int SC_MAX_S2 = GHM_SCATTER_MAX_S2;
constexpr int SC_NONE = 0, SC_UNDECIDED = 1, SC_KEPT = 2, SC_REJECTED = 3;
constexpr int SC_GROUP_PLAIN = 8, SC_GROUP_TILED = 1;
constexpr int64_t SC_HEADER = 256;                     // bytes in front of the workspace's state plane: the device word
constexpr int SC_ALT = 0, SC_EDGES = 256, SC_SLOPE = 320;          // offsets into the tables, in floats

__host__ __device__ inline unsigned sc_mix(unsigned x) {
    x ^= x >> 16;
    x *= GHM_SCATTER_MIX_A;
    x ^= x >> 15;
    x *= GHM_SCATTER_MIX_B;
    x ^= x >> 16;
    return x;
}

__host__ __device__ inline unsigned sc_hash(unsigned seed_lo, unsigned seed_hi, unsigned stream, unsigned row, unsigned col) {
    unsigned x = sc_mix(seed_lo + GHM_SCATTER_MIX_STEP);
    x = sc_mix((x ^ seed_hi) + GHM_SCATTER_MIX_STEP);
    x = sc_mix((x ^ stream) + GHM_SCATTER_MIX_STEP);
    x = sc_mix((x ^ row) + GHM_SCATTER_MIX_STEP);
    return sc_mix((x ^ col) + GHM_SCATTER_MIX_STEP);
}

// the largest R with R^2 < s2
__host__ __device__ constexpr int sc_reach(int s2) {
    int R = 0;
    while ((R + 1) * (R + 1) < s2) ++R;
    return R;
}

// ---- the chance -------------------------------------------------------------------------------------------------------------
struct ScChance {
    const float *h, *tables, *water;
    const int* dist2;
    const unsigned* blocked;
    unsigned* chance;
    int H, W, ph, pd, pb, pc, water_n;
    unsigned threshold;
    float half_scale, density;
};

__device__ __forceinline__ void sc_chance_cell(const ScChance& a, int y, int x) {
    unsigned out = 0u;
    if (!(a.blocked && a.blocked[(long)y * a.pb + x] >= a.threshold)) {
        const float* row = a.h + (long)y * a.ph;
        const float h = row[x];
        const float t255 = h * 255.0f;
        const float t = t255 + 0.5f;
        const int ai = !(t >= 0.0f) ? 0 : t >= 255.0f ? 255 : (int)t;
        const float dxh = row[min(x + 1, a.W - 1)] - row[max(x - 1, 0)];
        const float dyh = a.h[(long)min(y + 1, a.H - 1) * a.ph + x] - a.h[(long)max(y - 1, 0) * a.ph + x];
        const float gx = dxh * a.half_scale, gy = dyh * a.half_scale;
        const float gxx = gx * gx, gyy = gy * gy;
        const float g2 = gxx + gyy;
        int bin = 0;                                   // the number of bounds <= g2: the bounds ascend, a NaN counts none
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1)
            if (bin + step <= 63 && a.tables[SC_EDGES + bin + step - 1] <= g2) bin += step;
        float p = a.tables[SC_ALT + ai] * a.tables[SC_SLOPE + bin];
        if (a.water) {
            const int d = a.dist2[(long)y * a.pd + x];
            p = p * a.water[(d >= 0 && d < a.water_n) ? d : a.water_n];
        }
        p = p * a.density;
        const float v = p * 16777216.0f;
        out = !(v >= 0.0f) ? 0u : v >= 16777216.0f ? GHM_SCATTER_ONE : (unsigned)v;
    }
    a.chance[(long)y * a.pc + x] = out;
}

__global__ __launch_bounds__(256) void sc_chance_kernel(const ScChance a) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (y < a.H && x < a.W) sc_chance_cell(a, y, x);
}

// ---- the candidates ---------------------------------------------------------------------------------------------------------
struct ScCand {
    const unsigned* chance;
    unsigned char* state;
    unsigned* prio;
    int H, W, pc, ps, pp;
    unsigned seed_lo, seed_hi, row0, col0;
};

__device__ __forceinline__ void sc_cand_cell(const ScCand& a, int y, int x) {
    const unsigned row = a.row0 + (unsigned)y, col = a.col0 + (unsigned)x;
    const unsigned draw = sc_hash(a.seed_lo, a.seed_hi, 0u, row, col) >> 8;
    a.state[(long)y * a.ps + x] = (unsigned char)(draw < a.chance[(long)y * a.pc + x] ? SC_UNDECIDED : SC_NONE);
    a.prio[(long)y * a.pp + x] = sc_hash(a.seed_lo, a.seed_hi, 1u, row, col);
}

__global__ __launch_bounds__(256) void sc_cand_kernel(const ScCand a) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (y < a.H && x < a.W) sc_cand_cell(a, y, x);
}

// ---- the thinning -----------------------------------------------------------------------------------------------------------
// the local rule for the undecided candidate at (y, x) of planes in rows of ps (states) and pp (priorities) cells, over the rows
// i0 .. i1 and columns j0 .. j1 of its window: its new state.  The states may change under the scan (the tiled form's sweeps are in
// place): each is read once, and whatever it reads is final if it is a decision.
__device__ __forceinline__ int sc_decide(const unsigned char* st, int ps, const unsigned* pr, int pp, int y, int x, int i0, int i1,
                                         int j0, int j1, int s2) {
    const unsigned mine = pr[(long)y * pp + x];
    int pending = 0;
    for (int i = i0; i <= i1; ++i) {
        const int dy = i - y, room = s2 - dy * dy;
        const unsigned char* srow = st + (long)i * ps;
        const unsigned* prow = pr + (long)i * pp;
        for (int j = j0; j <= j1; ++j) {
            const int dx = j - x;
            if (dx * dx >= room) continue;
            const int s = srow[j];
            if (s != SC_UNDECIDED && s != SC_KEPT) continue;
            const unsigned p = prow[j];
            if (!(p < mine || (p == mine && (dy < 0 || (dy == 0 && dx < 0))))) continue;       // not earlier (or the cell itself)
            if (s == SC_KEPT) return SC_REJECTED;
            pending = 1;
        }
    }
    return pending ? SC_UNDECIDED : SC_KEPT;
}

struct ScThin {
    const unsigned* prio;
    const unsigned char* src;      // plain: the states a sweep reads
    unsigned char* state;          // the states a sweep writes (tiled: reads and writes)
    int H, W, pp, pi, ps, s2, R;   // pi: the pitch of src
};

// returns whether the cell was decided
__device__ __forceinline__ int sc_plain_cell(const ScThin& a, int y, int x) {
    const int old = a.src[(long)y * a.pi + x];
    int now = old;
    if (old == SC_UNDECIDED)
        now = sc_decide(a.src, a.pi, a.prio, a.pp, y, x, max(0, y - a.R), min(a.H - 1, y + a.R), max(0, x - a.R),
                        min(a.W - 1, x + a.R), a.s2);
    a.state[(long)y * a.ps + x] = (unsigned char)now;
    return now != old;
}

__global__ __launch_bounds__(256) void sc_plain_kernel(const ScThin a, int* word) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    int changed = 0;
    if (y < a.H && x < a.W) changed = sc_plain_cell(a, y, x);
    hyd_raise(changed, word);
}

// ---- tiled: the phases of a block, thread t of 256; a barrier lies between two phases.  Thread t owns the tile's cells
// (t / 32 + 8 k, t % 32), k = 0 .. 3.  The window of the tile at (ty, tx) has n = 32 + 2R rows and columns and starts at
// (ty - R, tx - R) ---------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int sc_prio_bytes(int R) { return (4 * (SC_TILE + 2 * R) * (SC_TILE + 2 * R) + 15) / 16 * 16; }
__host__ __device__ constexpr int sc_state_bytes(int R) { return ((SC_TILE + 2 * R) * (SC_TILE + 2 * R) + 15) / 16 * 16; }

__device__ __forceinline__ int sc_live(const ScThin& a, int ty, int tx, int t) {
    const int x = tx + (t & 31);
    int any = 0;
    for (int tr = t >> 5; tr < SC_TILE; tr += 8) {
        const int y = ty + tr;
        if (y < a.H && x < a.W) any |= a.state[(long)y * a.ps + x] == SC_UNDECIDED;
    }
    return any;
}

__device__ __forceinline__ void sc_stage(const ScThin& a, unsigned* wp, unsigned char* ws, int ty, int tx, int t) {
    const int n = SC_TILE + 2 * a.R;
    for (int i = t; i < n * n; i += 256) {
        const int lr = i / n, lc = i - lr * n;
        const int r = ty - a.R + lr, c = tx - a.R + lc;
        const bool in = r >= 0 && r < a.H && c >= 0 && c < a.W;
        ws[i] = in ? a.state[(long)r * a.ps + c] : (unsigned char)SC_NONE;
        wp[i] = in ? a.prio[(long)r * a.pp + c] : 0u;
    }
}

// one sweep over the thread's cells, in place in LDS -> whether it decided any
__device__ __forceinline__ int sc_sweep(const ScThin& a, const unsigned* wp, unsigned char* ws, int t) {
    const int n = SC_TILE + 2 * a.R, lc = (t & 31) + a.R;
    int ch = 0;
    for (int tr = t >> 5; tr < SC_TILE; tr += 8) {
        const int lr = tr + a.R;
        if (ws[lr * n + lc] != SC_UNDECIDED) continue;
        const int now = sc_decide(ws, n, wp, n, lr, lc, lr - a.R, lr + a.R, lc - a.R, lc + a.R, a.s2);
        if (now != SC_UNDECIDED) {
            ws[lr * n + lc] = (unsigned char)now;
            ch = 1;
        }
    }
    return ch;
}

// the decisions of the tile's cells -> the plane; whether there were any
__device__ __forceinline__ int sc_store(const ScThin& a, const unsigned char* ws, int ty, int tx, int t) {
    const int n = SC_TILE + 2 * a.R, x = tx + (t & 31);
    int changed = 0;
    for (int tr = t >> 5; tr < SC_TILE; tr += 8) {
        const int y = ty + tr;
        if (y >= a.H || x >= a.W) continue;
        const int now = ws[(tr + a.R) * n + (t & 31) + a.R];
        if (now != SC_UNDECIDED && a.state[(long)y * a.ps + x] == SC_UNDECIDED) {
            a.state[(long)y * a.ps + x] = (unsigned char)now;
            changed = 1;
        }
    }
    return changed;
}

__global__ __launch_bounds__(256) void sc_tiled_kernel(const ScThin a, int* word) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sc_lds[];
    unsigned* wp = (unsigned*)sc_lds;
    unsigned char* ws = sc_lds + sc_prio_bytes(a.R);
    const int t = threadIdx.x, ty = blockIdx.y * SC_TILE, tx = blockIdx.x * SC_TILE;
#ifndef GHM_SCATTER_NO_SKIP /* a tuning build measures what the skip is worth (GHM_BUILD_DEFINES, csrc/build.py): the same bits */
    if (!__syncthreads_or(sc_live(a, ty, tx, t))) return;
#endif
    sc_stage(a, wp, ws, ty, tx, t);
    __syncthreads();
    // a sweep that decides anything decides one of at most 1024 cells: sweep 1025 decides nothing
    for (int s = 0; s <= SC_TILE * SC_TILE; ++s)
        if (!__syncthreads_or(sc_sweep(a, wp, ws, t))) break;
    hyd_raise(sc_store(a, ws, ty, tx, t), word);
}

#define SC_PLANE_GRID(H, W) dim3(ceil_div((W), 64), ceil_div((H), 4)), dim3(64, 4), 0, ctx->stream

}  // namespace

extern "C" {

int64_t ghm_scatter_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return -1;
    return SC_HEADER + (int64_t)H * W;
}

int64_t ghm_scatter_lds_bytes(int32_t s2) {
    if (s2 < 1 || s2 > SC_MAX_S2) return -1;
    return (int64_t)sc_prio_bytes(sc_reach(s2)) + sc_state_bytes(sc_reach(s2));
}

int ghm_scatter_chance(ghm_ctx* ctx, const float* h, int32_t h_pitch, int32_t H, int32_t W, const float* tables, double height_scale,
                       float density, const int32_t* dist2, int32_t d_pitch, const float* water, int32_t water_n,
                       const uint32_t* blocked, int32_t b_pitch, uint32_t threshold, uint32_t* chance, int32_t c_pitch) {
    GHM_CHECK(ctx && h && tables && chance, "ghm_scatter_chance: null pointer");
    if (int rc = hyd_check_plane("ghm_scatter_chance", H, W, h_pitch, "h")) return rc;
    if (int rc = hyd_check_plane("ghm_scatter_chance", H, W, c_pitch, "chance")) return rc;
    const float half_scale = (float)(height_scale / 2);
    GHM_CHECK(height_scale > 0.0 && half_scale > 0.0f && half_scale <= 3.0e38f,
              "ghm_scatter_chance: height_scale=%g (positive and finite, and so must its half be in float32)", height_scale);
    GHM_CHECK(density >= 0.0f && density <= 1.0f, "ghm_scatter_chance: density=%g (0 .. 1)", (double)density);
    if (water) {
        GHM_CHECK(dist2 != nullptr, "ghm_scatter_chance: null pointer: water weights without a dist2 plane");
        if (int rc = hyd_check_plane("ghm_scatter_chance", H, W, d_pitch, "dist2")) return rc;
        GHM_CHECK(water_n >= 1 && water_n <= 1025, "ghm_scatter_chance: water_n=%d (1 .. 1025)", water_n);
    }
    if (blocked) {
        if (int rc = hyd_check_plane("ghm_scatter_chance", H, W, b_pitch, "blocked")) return rc;
        GHM_CHECK(threshold >= 1u, "ghm_scatter_chance: threshold=0 would block every cell (>= 1)");
    }
    ScChance a;
    a.h = h;
    a.tables = tables;
    a.water = water;
    a.dist2 = dist2;
    a.blocked = blocked;
    a.chance = chance;
    a.H = H;
    a.W = W;
    a.ph = h_pitch;
    a.pd = d_pitch;
    a.pb = b_pitch;
    a.pc = c_pitch;
    a.water_n = water_n;
    a.threshold = threshold;
    a.half_scale = half_scale;
    a.density = density;
    hipLaunchKernelGGL(sc_chance_kernel, SC_PLANE_GRID(H, W), a);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_scatter_candidates(ghm_ctx* ctx, const uint32_t* chance, int32_t c_pitch, int32_t H, int32_t W, uint64_t seed,
                           int64_t origin_row, int64_t origin_col, uint8_t* state, int32_t s_pitch, uint32_t* priority,
                           int32_t p_pitch) {
    GHM_CHECK(ctx && chance && state && priority, "ghm_scatter_candidates: null pointer");
    if (int rc = hyd_check_plane("ghm_scatter_candidates", H, W, c_pitch, "chance")) return rc;
    if (int rc = hyd_check_plane("ghm_scatter_candidates", H, W, s_pitch, "state")) return rc;
    if (int rc = hyd_check_plane("ghm_scatter_candidates", H, W, p_pitch, "priority")) return rc;
    ScCand a;
    a.chance = chance;
    a.state = state;
    a.prio = priority;
    a.H = H;
    a.W = W;
    a.pc = c_pitch;
    a.ps = s_pitch;
    a.pp = p_pitch;
    a.seed_lo = (unsigned)seed;
    a.seed_hi = (unsigned)(seed >> 32);
    a.row0 = (unsigned)(uint64_t)origin_row;
    a.col0 = (unsigned)(uint64_t)origin_col;
    hipLaunchKernelGGL(sc_cand_kernel, SC_PLANE_GRID(H, W), a);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_scatter_thin(ghm_ctx* ctx, const uint32_t* priority, int32_t p_pitch, uint8_t* state, int32_t s_pitch, int32_t H, int32_t W,
                     int32_t s2, int32_t tiled, void* workspace, int64_t* sweeps) {
    if (int rc = hyd_sync_ok(ctx, "ghm_scatter_thin")) return rc;
    GHM_CHECK(priority && state && workspace, "ghm_scatter_thin: null pointer");
    if (int rc = hyd_check_plane("ghm_scatter_thin", H, W, p_pitch, "priority")) return rc;
    if (int rc = hyd_check_plane("ghm_scatter_thin", H, W, s_pitch, "state")) return rc;
    GHM_CHECK(s2 >= 1 && s2 <= SC_MAX_S2, "ghm_scatter_thin: s2=%d (1 .. %d)", s2, SC_MAX_S2);
    int* word = (int*)workspace;
    unsigned char* other = (unsigned char*)workspace + SC_HEADER;
    const int64_t cap = (int64_t)H * W + 1;
    ScThin a;
    a.prio = priority;
    a.src = state;
    a.state = state;
    a.H = H;
    a.W = W;
    a.pp = p_pitch;
    a.pi = s_pitch;
    a.ps = s_pitch;
    a.s2 = s2;
    a.R = sc_reach(s2);
    if (tiled)
        return hyd_relax(ctx, "ghm_scatter_thin", word, SC_GROUP_TILED, cap, [&](int64_t) {
            hipLaunchKernelGGL(sc_tiled_kernel, dim3(ceil_div(W, SC_TILE), ceil_div(H, SC_TILE)), dim3(256),
                               (size_t)ghm_scatter_lds_bytes(s2), ctx->stream, a, word);
        }, sweeps, nullptr, true);
    // the first group that changes nothing leaves the same plane on both sides, whatever the parity of the count
    return hyd_relax(ctx, "ghm_scatter_thin", word, SC_GROUP_PLAIN, cap, [&](int64_t i) {
        ScThin b = a;
        if (i & 1) {
            b.src = other, b.pi = W, b.state = state, b.ps = s_pitch;
        } else {
            b.src = state, b.pi = s_pitch, b.state = other, b.ps = W;
        }
        hipLaunchKernelGGL(sc_plain_kernel, SC_PLANE_GRID(H, W), b, word);
    }, sweeps, nullptr, true);
}

}  // extern "C"
