// Climate on a heightfield (gan_heightmaps_amd/climate.py): rain carried along the wind with orographic lift and a
// rain shadow, temperature from altitude and world latitude, a biome label per cell, and the rain-weighted discharge of a
// hydrology's directions.  Integers throughout: include/ghm.h states the definition, tests/climate_ref.py restates it in plain
// Python, and the kernels equal it bit for bit.
//
// Transport.  The plane is cut into wind lines -- rows for E and W, columns for N and S, the H + W - 1 diagonals for the other
// four winds -- and a line is one serial recurrence over the vapour m; lines do not interact, so a line is a lane.  In the
// normalised plane (u, v) = (rows, columns counted from the upwind edges) line l holds at step t the cell
//   KIND 0 (E, W): (l, t)       KIND 1 (N, S): (t, l)       KIND 2 (diagonals): (t, t + l - (H - 1)),
// wherever that lies inside the plane, so in KIND 1 and 2 the lanes of a wave read adjacent columns of one row at every step.
// Two forms, the same bits:
//   line   : a wave of 64 lines reads and writes global memory directly; the heights of CLM_AHEAD steps are loaded before the
//            recurrence runs over them, so only the recurrence is serial.  KIND 0 reads a pitch apart.
//   staged : a block of four waves takes 64 lines and moves tiles of 64 steps through LDS: wave 0 runs the recurrence over tile j
//            in place (heights in, rain out) while the other three load tile j + 1 and store tile j - 1, both row-wise, 64
//            consecutive cells per wave access in every KIND.  Three tiles of 64 x 65 words; the odd pitch keeps both the
//            transfers and the recurrence's accesses on distinct banks.
// No atomics: every cell of raw is written once, by the one lane that owns its line.
//
// Discharge.  The pointer doubling of hydrology.hip's accumulation with the rain as 64-bit weights: S_0 = rain, P_0 = the
// receiver; S_{k+1}[c] = S_k[c] + sum of S_k[d] over P_k(d) = c, P_{k+1} = P_k(P_k).  The sums are 64-bit integer atomicAdd: exact
// in any order.  At most GHM_CLIMATE_MAX_ROUNDS rounds: directions that hold a cycle are refused, not waited for.
#include "common.h"
#include "relax.h"      // hyd_raise, hyd_check_plane, hyd_sync_ok, hyd_read_word

// the paint's subtraction, product and sum are rounded one by one, as hyd_paint_kernel's
#pragma clang fp contract(off)

namespace {

constexpr int CLM_LINES = 64;                          // lines of a wave (line) or a block (staged)
constexpr int CLM_STEPS = 64;                          // steps of a staged tile
constexpr int CLM_LDS_PITCH = CLM_STEPS + 1;
constexpr int CLM_AHEAD = 16;                          // heights in flight in front of the recurrence
constexpr int CLM_MAX_ROUNDS = GHM_CLIMATE_MAX_ROUNDS;
constexpr int64_t CLM_HEADER = 256;                    // bytes in front of the workspace planes: the device word

const int CLM_DY[8] = {-1, -1, 0, 1, 1, 1, 0, -1};     // the hydrology's neighbours, N NE E SE S SW W NW: where a wind comes from
const int CLM_DX[8] = {0, 1, 1, 1, 0, -1, -1, -1};
__device__ __constant__ const int CLM_NY[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
__device__ __constant__ const int CLM_NX[8] = {0, 1, 1, 1, 0, -1, -1, -1};

struct Transport {
    const int* zq;
    unsigned* raw;
    int H, W, pz, pr, flipy, flipx, sea_q;
    unsigned hum_q, evap_q, base_q, up_q, rec_q;
};

// the cell of line ``line`` at step t -> its offsets in zq and raw; false outside the plane (and for a line past the last)
template <int KIND>
__device__ __forceinline__ bool clm_cell(const Transport& k, long line, int t, long& zi, long& ri) {
    long u, v;
    if (KIND == 0) {
        u = line;
        v = t;
    } else if (KIND == 1) {
        u = t;
        v = line;
    } else {
        u = t;
        v = t + line - (k.H - 1);
    }
    if (u < 0 || u >= k.H || v < 0 || v >= k.W) return false;
    const long r = k.flipy ? k.H - 1 - u : u, c = k.flipx ? k.W - 1 - v : v;
    zi = r * k.pz + c;
    ri = r * k.pr + c;
    return true;
}

// the steps [t0, t1) at which one of the 64 lines from ``first`` on can lie inside the plane
template <int KIND>
__device__ __forceinline__ void clm_span(const Transport& k, long first, int& t0, int& t1) {
    t0 = 0;
    t1 = KIND == 0 ? k.W : k.H;
    if (KIND == 2) {
        const long dmin = first - (k.H - 1), dmax = dmin + CLM_LINES - 1;          // v - u of the first and the last line
        t0 = (int)max(0L, -dmax);
        t1 = (int)min((long)k.H, k.W - dmin);
    }
}

struct Parcel {
    unsigned m;
    int before;
    bool started;
};

// one step of the recurrence, in the definition's order; every product is 32 x 32 -> 64 bits
__device__ __forceinline__ unsigned clm_step(const Transport& k, Parcel& p, int z) {
    const int s = max(z, k.sea_q);
    if (!p.started) {
        p.before = s;
        p.started = true;
    }
    const bool sea = z <= k.sea_q;
    if (sea) p.m += (unsigned)(((uint64_t)(65536u - p.m) * k.evap_q) >> 16);
    const int64_t climb = (int64_t)s - p.before;
    const uint64_t lift = climb > 0 ? (uint64_t)climb : 0;
    const uint64_t want = (uint64_t)k.base_q + ((lift * k.up_q) >> 8);
    const unsigned rate = want < 65536u ? (unsigned)want : 65536u;
    const unsigned r = (unsigned)(((uint64_t)p.m * rate) >> 16);
    p.m -= r;
    if (!sea) p.m += (unsigned)(((uint64_t)r * k.rec_q) >> 16);
    p.before = s;
    return r;
}

template <int KIND>
__global__ __launch_bounds__(CLM_LINES) void clm_line_kernel(const Transport k) {
    const long first = (long)blockIdx.x * CLM_LINES, line = first + threadIdx.x;
    int t0, t1;
    clm_span<KIND>(k, first, t0, t1);
    Parcel p = {k.hum_q, 0, false};
    for (int tb = t0; tb < t1; tb += CLM_AHEAD) {
        int z[CLM_AHEAD];
        long at[CLM_AHEAD];
        bool in[CLM_AHEAD];
#pragma unroll
        for (int i = 0; i < CLM_AHEAD; ++i) {
            long zi = 0;
            at[i] = 0;
            in[i] = tb + i < t1 && clm_cell<KIND>(k, line, tb + i, zi, at[i]);
            z[i] = in[i] ? k.zq[zi] : 0;
        }
#pragma unroll
        for (int i = 0; i < CLM_AHEAD; ++i)
            if (in[i]) k.raw[at[i]] = clm_step(k, p, z[i]);
    }
}

// element e of a tile's transfer by ``n`` threads: 64 consecutive e share the slow index and run along the plane's rows
template <int KIND>
__device__ __forceinline__ int clm_lds(int e, int& l, int& tt) {
    const int fast = e & 63, slow = e >> 6;
    l = KIND == 0 ? slow : fast;
    tt = KIND == 0 ? fast : slow;
    return slow * CLM_LDS_PITCH + fast;
}

template <int KIND>
__device__ __forceinline__ void clm_tile_load(const Transport& k, int* tile, long first, int tb, int t1, int w, int n) {
    for (int e = w; e < CLM_LINES * CLM_STEPS; e += n) {
        int l, tt;
        const int a = clm_lds<KIND>(e, l, tt);
        long zi = 0, ri = 0;
        const bool in = tb + tt < t1 && clm_cell<KIND>(k, first + l, tb + tt, zi, ri);
        tile[a] = in ? k.zq[zi] : 0;
    }
}

template <int KIND>
__device__ __forceinline__ void clm_tile_store(const Transport& k, const int* tile, long first, int tb, int t1, int w, int n) {
    for (int e = w; e < CLM_LINES * CLM_STEPS; e += n) {
        int l, tt;
        const int a = clm_lds<KIND>(e, l, tt);
        long zi = 0, ri = 0;
        if (tb + tt < t1 && clm_cell<KIND>(k, first + l, tb + tt, zi, ri)) k.raw[ri] = (unsigned)tile[a];
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void clm_staged_kernel(const Transport k) {
    __shared__ int tiles[3][CLM_LINES * CLM_LDS_PITCH];
    const int tid = threadIdx.x;
    const long first = (long)blockIdx.x * CLM_LINES;
    int t0, t1;
    clm_span<KIND>(k, first, t0, t1);
    const int count = (t1 - t0 + CLM_STEPS - 1) / CLM_STEPS;          // the same in every thread of the block
    if (count <= 0) return;
    clm_tile_load<KIND>(k, tiles[0], first, t0, t1, tid, 256);
    __syncthreads();
    Parcel p = {k.hum_q, 0, false};
    for (int j = 0; j < count; ++j) {
        const int tb = t0 + j * CLM_STEPS;
        if (tid < CLM_LINES) {
            int* tile = tiles[j % 3];
            for (int c = 0; c < CLM_STEPS; c += CLM_AHEAD) {
                int z[CLM_AHEAD];
#pragma unroll
                for (int i = 0; i < CLM_AHEAD; ++i) z[i] = tile[KIND == 0 ? tid * CLM_LDS_PITCH + c + i : (c + i) * CLM_LDS_PITCH + tid];
#pragma unroll
                for (int i = 0; i < CLM_AHEAD; ++i) {
                    long zi = 0, ri = 0;
                    if (tb + c + i < t1 && clm_cell<KIND>(k, first + tid, tb + c + i, zi, ri))
                        tile[KIND == 0 ? tid * CLM_LDS_PITCH + c + i : (c + i) * CLM_LDS_PITCH + tid] = (int)clm_step(k, p, z[i]);
                }
            }
        } else {
            if (j + 1 < count) clm_tile_load<KIND>(k, tiles[(j + 1) % 3], first, tb + CLM_STEPS, t1, tid - CLM_LINES, 256 - CLM_LINES);
            if (j > 0) clm_tile_store<KIND>(k, tiles[(j - 1) % 3], first, tb - CLM_STEPS, t1, tid - CLM_LINES, 256 - CLM_LINES);
        }
        __syncthreads();
    }
    clm_tile_store<KIND>(k, tiles[(count - 1) % 3], first, t0 + (count - 1) * CLM_STEPS, t1, tid, 256);
}

// ---- spread ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clm_spread_kernel(const unsigned* __restrict__ raw, int pr, int H, int W, int spread,
                                                         unsigned* __restrict__ rain, int po) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    if (r >= H || c >= W) return;
    uint64_t sum = 0;
    for (int dy = -spread; dy <= spread; ++dy) {
        const int y = min(max(r + dy, 0), H - 1);
        for (int dx = -spread; dx <= spread; ++dx) sum += raw[(long)y * pr + min(max(c + dx, 0), W - 1)];
    }
    const unsigned side = 2u * spread + 1u;
    rain[(long)r * po + c] = (unsigned)(sum / (side * side));
}

// ---- temperature and biome ----------------------------------------------------------------------------------------------------------
struct Chart {
    const int* zq;
    const unsigned* rain;
    int* temperature;
    int* biome;
    int H, W, pz, pr, pt, pb, sea_q, t0_q, n_t, n_r, ocean;
    unsigned lapse_q;
    int lat_q;
    int64_t origin_row;
    int t_edges[GHM_CLIMATE_MAX_EDGES];
    unsigned r_edges[GHM_CLIMATE_MAX_EDGES];
    int table[(GHM_CLIMATE_MAX_EDGES + 1) * (GHM_CLIMATE_MAX_EDGES + 1)];
};

__global__ __launch_bounds__(256) void clm_biome_kernel(const Chart k) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    if (r >= k.H || c >= k.W) return;
    const int z = k.zq[(long)r * k.pz + c];
    const int64_t above = max((int64_t)z - k.sea_q, (int64_t)0);
    const int64_t t = (int64_t)k.t0_q - ((above * (int64_t)k.lapse_q) >> 16) - (((k.origin_row + r) * (int64_t)k.lat_q) >> 16);
    const int tq = (int)t;
    k.temperature[(long)r * k.pt + c] = tq;
    int b = k.ocean;
    if (z > k.sea_q) {
        const unsigned wet = k.rain[(long)r * k.pr + c];
        int i = 0, j = 0;
        for (int e = 0; e < k.n_t; ++e) i += tq >= k.t_edges[e];
        for (int e = 0; e < k.n_r; ++e) j += wet >= k.r_edges[e];
        b = k.table[i * (k.n_r + 1) + j];
    }
    k.biome[(long)r * k.pb + c] = b;
}

// ---- discharge ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clm_dis_init_kernel(const signed char* __restrict__ dir, int pdir, const unsigned* __restrict__ rain,
                                                           int pr, int H, int W, unsigned long long* __restrict__ S, int* __restrict__ P,
                                                           int* word) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    int alive = 0;
    if (r < H && c < W) {
        const int d = dir[(long)r * pdir + c];
        const int idx = r * W + c;
        int p = -1;
        if (d >= 0 && d < 8) {                           // anything else, and a receiver outside the plane, ends the chain
            const int y = r + CLM_NY[d], x = c + CLM_NX[d];
            if (y >= 0 && y < H && x >= 0 && x < W) p = y * W + x;
        }
        S[idx] = rain[(long)r * pr + c];
        P[idx] = p;
        alive = p >= 0;
    }
    hyd_raise(alive, word);
}

// S1 holds a copy of S0 when this starts
__global__ __launch_bounds__(256) void clm_dis_round_kernel(const unsigned long long* __restrict__ S0, unsigned long long* S1,
                                                            const int* __restrict__ P0, int* __restrict__ P1, int n, int* word) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    int alive = 0;
    if (idx < n) {
        const int p = P0[idx];
        int pp = -1;
        if (p >= 0) {
            atomicAdd(&S1[p], S0[idx]);
            pp = P0[p];
        }
        P1[idx] = pp;
        alive = pp >= 0;
    }
    hyd_raise(alive, word);
}

__global__ __launch_bounds__(256) void clm_dis_emit_kernel(const unsigned long long* __restrict__ S, int H, int W, unsigned ref_q,
                                                           unsigned long long* __restrict__ discharge, int pq,
                                                           unsigned* __restrict__ effective, int pe) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    if (r >= H || c >= W) return;
    const unsigned long long q = S[r * W + c];
    discharge[(long)r * pq + c] = q;
    const unsigned long long a = q / ref_q;
    effective[(long)r * pe + c] = a < 0xffffffffull ? (unsigned)a : 0xffffffffu;
}

// ---- the biomes on a texture ----------------------------------------------------------------------------------------------------------
struct Palette {
    const int* biome;
    const float* tex;
    void* out;
    int H, W, pb, ptex, pout, channels, out_u8, count;
    float opacity;
    float colour[GHM_CLIMATE_MAX_LABELS][3];
    unsigned long long has;                              // bit b: biome b has a colour
};

__global__ __launch_bounds__(256) void clm_paint_kernel(const Palette k) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    if (r >= k.H || c >= k.W) return;
    const int b = k.biome[(long)r * k.pb + c];
    const bool on = b >= 0 && b < k.count && (k.has >> b & 1ull);
    for (int ch = 0; ch < k.channels; ++ch) {
        const float t = k.tex[((long)ch * k.H + r) * k.ptex + c];
        float v = t;
        if (on) {
            const float d = k.colour[b][ch] - t;
            const float p = k.opacity * d;
            v = t + p;
        }
        const long at = ((long)ch * k.H + r) * k.pout + c;
        if (k.out_u8)                                    // hyd_paint_kernel's map: rint((double)v * 255), half to even
            ((unsigned char*)k.out)[at] = (unsigned char)(int)rint((double)fminf(fmaxf(v, 0.0f), 1.0f) * 255.0);
        else
            ((float*)k.out)[at] = v;
    }
}

#define CLM_PLANE_GRID(H, W) dim3(ceil_div((W), 64), ceil_div((H), 4)), dim3(64, 4), 0, ctx->stream

template <int KIND>
void clm_launch_transport(ghm_ctx* ctx, const Transport& k, int form, long lines) {
    const dim3 grid(ceil_div(lines, CLM_LINES));
    if (form == GHM_CLIMATE_STAGED)
        hipLaunchKernelGGL(clm_staged_kernel<KIND>, grid, dim3(256), 0, ctx->stream, k);
    else
        hipLaunchKernelGGL(clm_line_kernel<KIND>, grid, dim3(CLM_LINES), 0, ctx->stream, k);
}

bool clm_share(int32_t v) { return v >= 0 && v <= 65536; }

}  // namespace

extern "C" {

int64_t ghm_climate_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31) || H > 4 * 65535) return -1;
    return CLM_HEADER + 24 * (int64_t)H * W;             // two planes of 64-bit sums, two of pointers
}

int ghm_climate_transport(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, int32_t H, int32_t W, int32_t wind, int32_t form,
                          int32_t sea_q, int32_t hum_q, int32_t evap_q, int32_t base_q, int32_t up_q, int32_t rec_q, uint32_t* raw,
                          int32_t r_pitch) {
    GHM_CHECK(ctx && zq && raw, "ghm_climate_transport: null pointer");
    if (int rc = hyd_check_plane("ghm_climate_transport", H, W, z_pitch, "zq")) return rc;
    if (int rc = hyd_check_plane("ghm_climate_transport", H, W, r_pitch, "raw")) return rc;
    GHM_CHECK(wind >= 0 && wind < 8, "ghm_climate_transport: wind=%d (0 .. 7: N NE E SE S SW W NW)", wind);
    GHM_CHECK(form == GHM_CLIMATE_LINE || form == GHM_CLIMATE_STAGED, "ghm_climate_transport: form=%d (0 line, 1 staged)", form);
    GHM_CHECK(clm_share(hum_q) && clm_share(evap_q) && clm_share(base_q) && clm_share(rec_q),
              "ghm_climate_transport: hum_q=%d, evap_q=%d, base_q=%d, rec_q=%d: each lies in [0, 65536]", hum_q, evap_q, base_q, rec_q);
    GHM_CHECK(up_q >= 0 && up_q <= 16 * 65536, "ghm_climate_transport: up_q=%d outside [0, 2^20]", up_q);
    Transport k;
    k.zq = zq;
    k.raw = raw;
    k.H = H;
    k.W = W;
    k.pz = z_pitch;
    k.pr = r_pitch;
    k.flipy = CLM_DY[wind] > 0;                          // a wind from the south enters at the last row
    k.flipx = CLM_DX[wind] > 0;
    k.sea_q = sea_q;
    k.hum_q = (unsigned)hum_q;
    k.evap_q = (unsigned)evap_q;
    k.base_q = (unsigned)base_q;
    k.up_q = (unsigned)up_q;
    k.rec_q = (unsigned)rec_q;
    if (CLM_DY[wind] == 0)
        clm_launch_transport<0>(ctx, k, form, H);
    else if (CLM_DX[wind] == 0)
        clm_launch_transport<1>(ctx, k, form, W);
    else
        clm_launch_transport<2>(ctx, k, form, (long)H + W - 1);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_climate_spread(ghm_ctx* ctx, const uint32_t* raw, int32_t r_pitch, int32_t H, int32_t W, int32_t spread, uint32_t* rain,
                       int32_t o_pitch) {
    GHM_CHECK(ctx && raw && rain, "ghm_climate_spread: null pointer");
    if (int rc = hyd_check_plane("ghm_climate_spread", H, W, r_pitch, "raw")) return rc;
    if (int rc = hyd_check_plane("ghm_climate_spread", H, W, o_pitch, "rain")) return rc;
    GHM_CHECK(spread >= 0 && spread <= GHM_CLIMATE_MAX_SPREAD, "ghm_climate_spread: spread=%d (0 .. %d)", spread, GHM_CLIMATE_MAX_SPREAD);
    GHM_CHECK(raw != rain, "ghm_climate_spread: rain may not be raw");
    hipLaunchKernelGGL(clm_spread_kernel, CLM_PLANE_GRID(H, W), raw, r_pitch, H, W, spread, rain, o_pitch);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_climate_biome(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, const uint32_t* rain, int32_t r_pitch, int32_t H, int32_t W,
                      int32_t sea_q, int32_t t0_q, int32_t lapse_q, int32_t lat_q, int64_t origin_row, const int32_t* t_edges,
                      int32_t n_t, const int32_t* r_edges, int32_t n_r, const int32_t* table, int32_t ocean, int32_t* temperature,
                      int32_t t_pitch, int32_t* biome, int32_t b_pitch) {
    GHM_CHECK(ctx && zq && rain && temperature && biome && table, "ghm_climate_biome: null pointer");
    if (int rc = hyd_check_plane("ghm_climate_biome", H, W, z_pitch, "zq")) return rc;
    if (int rc = hyd_check_plane("ghm_climate_biome", H, W, r_pitch, "rain")) return rc;
    if (int rc = hyd_check_plane("ghm_climate_biome", H, W, t_pitch, "temperature")) return rc;
    if (int rc = hyd_check_plane("ghm_climate_biome", H, W, b_pitch, "biome")) return rc;
    GHM_CHECK(n_t >= 0 && n_t <= GHM_CLIMATE_MAX_EDGES && n_r >= 0 && n_r <= GHM_CLIMATE_MAX_EDGES,
              "ghm_climate_biome: %d temperature and %d rain edges (0 .. %d each)", n_t, n_r, GHM_CLIMATE_MAX_EDGES);
    GHM_CHECK((n_t == 0 || t_edges) && (n_r == 0 || r_edges), "ghm_climate_biome: null pointer");
    GHM_CHECK(t0_q >= -25600 && t0_q <= 25600, "ghm_climate_biome: t0_q=%d outside [-25600, 25600]", t0_q);
    GHM_CHECK(lapse_q >= 0 && lapse_q <= 16 * 65536, "ghm_climate_biome: lapse_q=%d outside [0, 2^20]", lapse_q);
    GHM_CHECK(lat_q >= -(1 << 24) && lat_q <= (1 << 24), "ghm_climate_biome: lat_q=%d outside [-2^24, 2^24]", lat_q);
    GHM_CHECK(origin_row >= -((int64_t)1 << 31) && origin_row <= ((int64_t)1 << 31),
              "ghm_climate_biome: origin_row=%lld outside [-2^31, 2^31]", (long long)origin_row);
    for (int i = 1; i < n_t; ++i) GHM_CHECK(t_edges[i - 1] < t_edges[i], "ghm_climate_biome: the temperature edges do not ascend");
    for (int i = 0; i < n_r; ++i)
        GHM_CHECK(r_edges[i] >= 0 && (i == 0 || r_edges[i - 1] < r_edges[i]), "ghm_climate_biome: the rain edges are negative or do not ascend");
    GHM_CHECK(ocean >= 0, "ghm_climate_biome: ocean=%d is negative", ocean);
    for (int i = 0; i < (n_t + 1) * (n_r + 1); ++i) GHM_CHECK(table[i] >= 0, "ghm_climate_biome: table[%d]=%d is negative", i, table[i]);
    Chart k = {};
    k.zq = zq;
    k.rain = rain;
    k.temperature = temperature;
    k.biome = biome;
    k.H = H;
    k.W = W;
    k.pz = z_pitch;
    k.pr = r_pitch;
    k.pt = t_pitch;
    k.pb = b_pitch;
    k.sea_q = sea_q;
    k.t0_q = t0_q;
    k.n_t = n_t;
    k.n_r = n_r;
    k.ocean = ocean;
    k.lapse_q = (unsigned)lapse_q;
    k.lat_q = lat_q;
    k.origin_row = origin_row;
    for (int i = 0; i < n_t; ++i) k.t_edges[i] = t_edges[i];
    for (int i = 0; i < n_r; ++i) k.r_edges[i] = (unsigned)r_edges[i];
    for (int i = 0; i < (n_t + 1) * (n_r + 1); ++i) k.table[i] = table[i];
    hipLaunchKernelGGL(clm_biome_kernel, CLM_PLANE_GRID(H, W), k);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_climate_discharge(ghm_ctx* ctx, const int8_t* direction, int32_t d_pitch, const uint32_t* rain, int32_t r_pitch, int32_t H,
                          int32_t W, uint32_t ref_q, uint64_t* discharge, int32_t q_pitch, uint32_t* effective, int32_t e_pitch,
                          void* workspace, int32_t* rounds) {
    if (int rc = hyd_sync_ok(ctx, "ghm_climate_discharge")) return rc;
    GHM_CHECK(direction && rain && discharge && effective && workspace, "ghm_climate_discharge: null pointer");
    if (int rc = hyd_check_plane("ghm_climate_discharge", H, W, d_pitch, "direction")) return rc;
    if (int rc = hyd_check_plane("ghm_climate_discharge", H, W, r_pitch, "rain")) return rc;
    if (int rc = hyd_check_plane("ghm_climate_discharge", H, W, q_pitch, "discharge")) return rc;
    if (int rc = hyd_check_plane("ghm_climate_discharge", H, W, e_pitch, "effective_area")) return rc;
    GHM_CHECK(ref_q >= 1 && ref_q <= 65536, "ghm_climate_discharge: ref_q=%u outside [1, 65536]", ref_q);
    const int n = H * W;
    int* word = (int*)workspace;
    char* base = (char*)workspace + CLM_HEADER;
    const size_t cells = (size_t)n;
    unsigned long long* S[2] = {(unsigned long long*)base, (unsigned long long*)(base + 8 * cells)};
    int* P[2] = {(int*)(base + 16 * cells), (int*)(base + 20 * cells)};
    GHM_HIP(hipMemsetAsync(word, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(clm_dis_init_kernel, CLM_PLANE_GRID(H, W), (const signed char*)direction, d_pitch, rain, r_pitch, H, W, S[0], P[0],
                       word);
    int alive = 0, k = 0;
    if (int rc = hyd_read_word(ctx, word, &alive)) return rc;
    while (alive) {
        // a forest needs at most ceil(log2(H W)) rounds; directions that hold a cycle never run out of live pointers
        GHM_CHECK(k < CLM_MAX_ROUNDS, "ghm_climate_discharge: pointers still alive after %d rounds: the directions are no forest", k);
        const int a = k & 1, b = a ^ 1;
        GHM_HIP(hipMemsetAsync(word, 0, sizeof(int), ctx->stream));
        GHM_HIP(hipMemcpyAsync(S[b], S[a], 8 * cells, hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(clm_dis_round_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, S[a], S[b], P[a], P[b], n, word);
        if (int rc = hyd_read_word(ctx, word, &alive)) return rc;
        ++k;
    }
    hipLaunchKernelGGL(clm_dis_emit_kernel, CLM_PLANE_GRID(H, W), S[k & 1], H, W, ref_q, (unsigned long long*)discharge, q_pitch,
                       effective, e_pitch);
    GHM_LAUNCH_CHECK();
    if (rounds) *rounds = k;
    return 0;
}

int ghm_climate_paint(ghm_ctx* ctx, const int32_t* biome, int32_t b_pitch, int32_t H, int32_t W, const float* texture,
                      int32_t tex_pitch, int32_t channels, const float* palette, int32_t colours, float opacity, int32_t out_u8,
                      void* out, int32_t out_pitch) {
    GHM_CHECK(ctx && biome && texture && out, "ghm_climate_paint: null pointer");
    if (int rc = hyd_check_plane("ghm_climate_paint", H, W, b_pitch, "biome")) return rc;
    GHM_CHECK(channels == 1 || channels == 3, "ghm_climate_paint: channels=%d (1 or 3)", channels);
    GHM_CHECK(tex_pitch >= W && out_pitch >= W && (int64_t)channels * H * tex_pitch < ((int64_t)1 << 31) &&
                  (int64_t)channels * H * out_pitch < ((int64_t)1 << 31),
              "ghm_climate_paint: texture pitches %d, %d out of range for %d x %d x %d", tex_pitch, out_pitch, channels, H, W);
    GHM_CHECK(colours >= 0 && colours <= GHM_CLIMATE_MAX_LABELS, "ghm_climate_paint: %d colours (0 .. %d)", colours, GHM_CLIMATE_MAX_LABELS);
    GHM_CHECK(colours == 0 || palette, "ghm_climate_paint: null pointer");
    GHM_CHECK(opacity >= 0.0f && opacity <= 1.0f, "ghm_climate_paint: opacity=%g outside [0, 1]", (double)opacity);
    Palette k = {};
    for (int b = 0; b < colours; ++b) {
        const float* p = palette + 4 * b;
        if (!(p[3] > 0.0f)) continue;
        GHM_CHECK(fabsf(p[0]) <= 3.0e38f && fabsf(p[1]) <= 3.0e38f && fabsf(p[2]) <= 3.0e38f, "ghm_climate_paint: colour %d is not finite", b);
        for (int ch = 0; ch < 3; ++ch) k.colour[b][ch] = p[ch];
        k.has |= 1ull << b;
    }
    k.biome = biome;
    k.tex = texture;
    k.out = out;
    k.H = H;
    k.W = W;
    k.pb = b_pitch;
    k.ptex = tex_pitch;
    k.pout = out_pitch;
    k.channels = channels;
    k.out_u8 = out_u8 ? 1 : 0;
    k.count = colours;
    k.opacity = opacity;
    hipLaunchKernelGGL(clm_paint_kernel, CLM_PLANE_GRID(H, W), k);
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
