// Sunlight on a heightfield (gan_heightmaps_amd/sunlight.py): for a list of sun positions, which of them light each
// cell, for how many hours, and how much energy the cell's slope receives.  Integers throughout, so there are no tolerances;
// include/ghm.h, section "sunlight", has the definition and tests/sunlight_ref.py restates it.
//
// 1. The heights are the viewshed's zq (ghm_viewshed_quantise), the block maxima its top (ghm_viewshed_top); zmax, the plane's
//    largest zq, is the largest block maximum (ghm_sunlight_zmax, one block, into a device word: nothing waits for it).
// 2. A position travels as (rows, gmaj, gmin, m_q, rise_q, s_y, s_x, s_z, w_q): the major axis and the two signs, the minor advance
//    and the rise per major step in 1/65536, the unit vector to the sun in 1/16384 and the weight in 1/256 hour.
// 3. The slope: g_y = zq[r + 1, c] - zq[r - 1, c], g_x likewise, indices clamped; norm = floor(sqrt(g_y^2 + g_x^2 + 512^2)), exact: the
//    sum stays below 2^52, so a double holds it and its root is corrected by one.  dot = -g_y s_y - g_x s_x + 512 s_z.  It is folded
//    into the sun kernel: four loads and one root per cell and launch, against a ray per position.
// 4. The shadow ray of cell T under a position with dot > 0: for k = 1, 2, ... ray = 256 (zq[T] + target_q) + k rise_q; q, f =
//    divmod(k m_q, 65536), carried along by additions; cell a lies k major and q minor steps from T, b one minor step further
//    (read only if f > 0).  The ray ends LIT at the first k whose a (or b, if f > 0) lies outside the plane and IN SHADOW at the
//    first k with zq[a] (65536 - f) + zq[b] f > 256 ray; grazing is lit.
//    The bound: every sample is a weighted mean of two heights <= zmax, so zq[a] (65536 - f) + zq[b] f <= 65536 zmax, and the ray
//    only rises; once ray >= 256 zmax no later step can block and the ray ends lit.  That early exit is a no-op on the result.  It
//    also bounds the products: a step is tested only while ray < 256 zmax <= 2^32 (zq <= 2^24), so 256 ray < 2^40 and
//    zq (65536 - f) + zq f <= 2^40; ray itself stays below 2^33 + 2^40 + rise_q <= 2^42; w_q dot < 2^17 2^41.  All of it in int64,
//    nothing reaches 2^59.
//      plain : every k.
//      accel : the steps are taken in runs k0 .. k1 whose major coordinate stays inside one 16 x 16 block and inside the plane.  The
//              cells the run's samples touch have minor offsets q(k0) .. q(k1) + (f(k1) > 0); m_q <= 65536 and a run has at most 16
//              steps, so they lie in at most three blocks, side by side.  If all of them lie in the plane, M is the largest of the
//              three block maxima; every sample of the run is <= 65536 M and 256 ray(k) >= 256 ray(k0), so if
//              65536 M <= 256 ray(k0) no step of the run blocks (and none leaves the plane) and the run is jumped, q(k1), f(k1) by
//              one product, a shift and a mask.  Otherwise its steps are marched one by one by the plain form's own test.  A jump
//              is taken on that integer proof alone, so both forms give the same bits by construction.
//    The positions travel as kernel arguments, SUN_CHUNK to a launch: the entry point waits for nothing, needs no workspace and
//    can be recorded.  The first launch of a call stores the planes, a later one adds to what the earlier ones stored; there are
//    no atomics.  Launch shape: 16 x 16 threads on 16 x 16 cells, a wavefront on 4 rows of 16: under one position neighbouring
//    rays run through the same cache lines and (accel) through the same blocks.  No LDS in the sun kernel.
#include "common.h"
#include "relax.h"

namespace {

constexpr int SUN_B = GHM_VIEWSHED_BLOCK;
constexpr int SUN_SHIFT = 4;
static_assert((1 << SUN_SHIFT) == SUN_B, "the block is a power of two");
constexpr int SUN_CHUNK = GHM_SUNLIGHT_CHUNK;
static_assert(SUN_CHUNK >= 32, "a mask's positions go in one launch");
constexpr int SUN_ONE = 65536;

struct SunPos {
    int64_t rise_q;
    int m_q, w_q;
    short s_y, s_x, s_z;
    signed char rows, gmaj, gmin;
};

struct SunChunk {
    SunPos p[SUN_CHUNK];
};
static_assert(sizeof(SunChunk) <= 3072, "the positions of a launch travel as kernel arguments");

struct SunArgs {
    const int* zq;
    const int* top;
    const int* zmax;
    unsigned* lit;
    unsigned* mask;
    unsigned* hours;
    unsigned* energy;
    int H, W, pz, pl, pm, ph, pe, TW, n, first, target_q;
};

// floor(sqrt(v)), exactly, for 0 <= v < 2^52
__device__ __forceinline__ int64_t sun_isqrt(int64_t v) {
    int64_t n = (int64_t)sqrt((double)v);
    if (n * n > v) --n;
    else if ((n + 1) * (n + 1) <= v) ++n;
    return n;
}

// the ray's geometry along its two axes: flat strides, extents, signs
struct SunRay {
    const int* zq;
    long smaj, smin;              // the strides of the major and the minor axis in flat indices
    int nmaj, nmin, gmaj, gmin, m;
    int64_t rise, stop;           // stop = 256 zmax
};

// one step of the march at (cmaj, cmin, f) with the ray at ``ray``: 0 the ray goes on, 1 it ends lit, 2 it ends in shadow
__device__ __forceinline__ int sun_step(const SunRay& g, int cmaj, int cmin, int f, int64_t ray, unsigned& steps) {
    if ((unsigned)cmaj >= (unsigned)g.nmaj || (unsigned)cmin >= (unsigned)g.nmin) return 1;
    if (f && (unsigned)(cmin + g.gmin) >= (unsigned)g.nmin) return 1;
    if (ray >= g.stop) return 1;
    ++steps;
    const long idx = (long)cmaj * g.smaj + (long)cmin * g.smin;
    const int64_t za = g.zq[idx];
    const int64_t zb = f ? (int64_t)g.zq[idx + g.gmin * g.smin] : za;                  // (f > 0 only where m_q > 0, and then gmin != 0)
    return za * (SUN_ONE - f) + zb * f > 256 * ray ? 2 : 0;
}

// whether the cell at (tmaj, tmin) along the ray's axes, its ray starting at ``base``, is lit; steps: the steps tested are added
template <bool ACCEL>
__device__ __forceinline__ bool sun_lit(const SunRay& g, const int* top, long tmajs, long tmins, int tmaj, int tmin, int64_t base,
                                        unsigned& steps) {
    int cmaj = tmaj, cmin = tmin, f = 0;
    int64_t ray = base;
    if (!ACCEL) {
        for (;;) {
            ray += g.rise;
            cmaj += g.gmaj;
            f += g.m;
            if (f >= SUN_ONE) f -= SUN_ONE, cmin += g.gmin;
            const int s = sun_step(g, cmaj, cmin, f, ray, steps);
            if (s) return s == 1;
        }
    }
    int k = 0;
    for (;;) {
        ++k;
        ray += g.rise;
        cmaj += g.gmaj;
        f += g.m;
        if (f >= SUN_ONE) f -= SUN_ONE, cmin += g.gmin;
        if ((unsigned)cmaj >= (unsigned)g.nmaj || (unsigned)cmin >= (unsigned)g.nmin || ray >= g.stop) return true;
        // the run k .. k1: as far as the major coordinate stays in its block and in the plane
        const int inblock = g.gmaj > 0 ? SUN_B - 1 - (cmaj & (SUN_B - 1)) : cmaj & (SUN_B - 1);
        const int inplane = g.gmaj > 0 ? g.nmaj - 1 - cmaj : cmaj;
        const int k1 = k + min(inblock, inplane);
        const int64_t km = (int64_t)k1 * g.m;
        const int q1 = (int)(km >> 16), f1 = (int)(km & (SUN_ONE - 1));
        const int e1 = tmin + g.gmin * (q1 + (f1 > 0));                   // the furthest minor coordinate the run touches; cmin the nearest
        if ((unsigned)e1 < (unsigned)g.nmin) {
            const int lo = min(cmin, e1) >> SUN_SHIFT, hi = max(cmin, e1) >> SUN_SHIFT;
            const long trow = (long)(cmaj >> SUN_SHIFT) * tmajs;
            int M = top[trow + (long)lo * tmins];
            for (int b = lo + 1; b <= hi; ++b) M = max(M, top[trow + (long)b * tmins]);
            if ((int64_t)M * SUN_ONE <= 256 * ray) {                      // no step of the run blocks or leaves the plane
                ray += (int64_t)(k1 - k) * g.rise;
                cmaj += (k1 - k) * g.gmaj;
                cmin = tmin + g.gmin * q1;
                f = f1;
                k = k1;
                continue;
            }
        }
        for (;;) {
            const int s = sun_step(g, cmaj, cmin, f, ray, steps);
            if (s) return s == 1;
            if (k == k1) break;
            ++k;
            ray += g.rise;
            cmaj += g.gmaj;
            f += g.m;
            if (f >= SUN_ONE) f -= SUN_ONE, cmin += g.gmin;
        }
    }
}

// STEPS: the lit plane takes the steps tested in place of the positions that light the cell, nothing else is written
// (tools/sunlight_bench.py)
template <bool ACCEL, bool STEPS>
__device__ __forceinline__ void sun_cell(const SunArgs& a, const SunChunk& sun, int y, int x) {
    const long at = (long)y * a.pz + x;
    const int64_t z0 = a.zq[at];
    const int64_t gy = (int64_t)a.zq[(long)min(y + 1, a.H - 1) * a.pz + x] - a.zq[(long)max(y - 1, 0) * a.pz + x];
    const int64_t gx = (int64_t)a.zq[(long)y * a.pz + min(x + 1, a.W - 1)] - a.zq[(long)y * a.pz + max(x - 1, 0)];
    const int64_t norm = sun_isqrt(gy * gy + gx * gx + 512 * 512);
    const int64_t base = 256 * (z0 + a.target_q);
    SunRay g;
    g.zq = a.zq;
    g.stop = 256 * (int64_t)*a.zmax;
    unsigned lit = 0u, bits = 0u, hours = 0u, energy = 0u, steps = 0u;
    for (int i = 0; i < a.n; ++i) {
        const SunPos& p = sun.p[i];
        const int64_t dot = -gy * p.s_y - gx * p.s_x + 512 * (int64_t)p.s_z;
        if (dot <= 0) continue;                                          // self-shaded: no ray
        const bool rows = p.rows != 0;
        g.smaj = rows ? a.pz : 1;
        g.smin = rows ? 1 : a.pz;
        g.nmaj = rows ? a.H : a.W;
        g.nmin = rows ? a.W : a.H;
        g.gmaj = p.gmaj;
        g.gmin = p.gmin;
        g.m = p.m_q;
        g.rise = p.rise_q;
        if (!sun_lit<ACCEL>(g, a.top, rows ? a.TW : 1, rows ? 1 : a.TW, rows ? y : x, rows ? x : y, base, steps)) continue;
        lit += 1u;
        bits |= 1u << (i & 31);
        hours += (unsigned)p.w_q;
        energy += (unsigned)(((int64_t)p.w_q * dot) / norm);
    }
    unsigned* out = a.lit + (long)y * a.pl + x;
    if (STEPS) {
        *out = a.first ? steps : *out + steps;
        return;
    }
    unsigned* hq = a.hours + (long)y * a.ph + x;
    unsigned* en = a.energy + (long)y * a.pe + x;
    *out = a.first ? lit : *out + lit;
    *hq = a.first ? hours : *hq + hours;
    *en = a.first ? energy : *en + energy;
    if (a.mask) a.mask[(long)y * a.pm + x] = bits;
}

template <bool ACCEL, bool STEPS>
__global__ __launch_bounds__(256) void sun_kernel(const SunArgs a, const SunChunk sun) {
    const int x = blockIdx.x * SUN_B + threadIdx.x, y = blockIdx.y * SUN_B + threadIdx.y;
    if (y < a.H && x < a.W) sun_cell<ACCEL, STEPS>(a, sun, y, x);
}

#define SUN_GRID(H, W) dim3(ceil_div((W), SUN_B), ceil_div((H), SUN_B)), dim3(SUN_B, SUN_B), 0, ctx->stream

// ---- the largest block maximum ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sun_zmax_kernel(const int* top, long elems, int* zmax) {
    __shared__ int part[256];
    int best = INT32_MIN;
    for (long i = threadIdx.x; i < elems; i += 256) best = max(best, top[i]);
    part[threadIdx.x] = best;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] = max(part[threadIdx.x], part[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *zmax = part[0];
}

}  // namespace

extern "C" {

// the checks and the launches of ghm_sunlight_sun and ghm_sunlight_steps
static int sun_launch(ghm_ctx* ctx, const char* who, const int32_t* zq, int32_t z_pitch, int32_t H, int32_t W, const int64_t* table,
                      int32_t n, int32_t target_q, int32_t accel, const int32_t* top, const int32_t* zmax, uint32_t* lit, int32_t l_pitch,
                      uint32_t* mask, int32_t m_pitch, uint32_t* hours, int32_t h_pitch, uint32_t* energy, int32_t e_pitch, bool steps) {
    GHM_CHECK(ctx && zq && table && zmax && lit && (steps || (hours && energy)), "%s: null pointer", who);
    if (int rc = hyd_check_plane(who, H, W, z_pitch, "zq")) return rc;
    if (int rc = hyd_check_plane(who, H, W, l_pitch, steps ? "steps" : "lit")) return rc;
    if (!steps) {
        if (int rc = hyd_check_plane(who, H, W, h_pitch, "hours_q")) return rc;
        if (int rc = hyd_check_plane(who, H, W, e_pitch, "energy")) return rc;
    }
    GHM_CHECK(n >= 1 && n <= GHM_SUNLIGHT_MAX_POSITIONS, "%s: %d positions (1 .. %d)", who, n, GHM_SUNLIGHT_MAX_POSITIONS);
    GHM_CHECK(target_q >= 0 && target_q <= (1 << 24), "%s: target_q=%d (0 .. 2^24)", who, target_q);
    if (mask) {
        GHM_CHECK(n <= 32, "%s: a mask has 32 bits, there are %d positions", who, n);
        if (int rc = hyd_check_plane(who, H, W, m_pitch, "mask")) return rc;
    }
    GHM_CHECK(!accel || top, "%s: null pointer: accel needs the block maxima", who);
    int64_t weight = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t* p = table + GHM_SUNLIGHT_FIELDS * (size_t)i;
        GHM_CHECK((p[0] == 0 || p[0] == 1) && (p[1] == -1 || p[1] == 1) && p[2] >= -1 && p[2] <= 1,
                  "%s: position %d has axis %lld and signs %lld, %lld", who, i, (long long)p[0], (long long)p[1], (long long)p[2]);
        GHM_CHECK(p[3] >= 0 && p[3] <= SUN_ONE, "%s: position %d has m_q=%lld (0 .. 65536)", who, i, (long long)p[3]);
        GHM_CHECK((p[2] == 0) == (p[3] == 0), "%s: position %d has m_q=%lld and the minor sign %lld: one is 0 iff the other is", who, i,
                  (long long)p[3], (long long)p[2]);
        GHM_CHECK(p[4] >= 1 && p[4] <= ((int64_t)1 << 40), "%s: position %d has rise_q=%lld (1 .. 2^40)", who, i, (long long)p[4]);
        GHM_CHECK(p[5] >= -16384 && p[5] <= 16384 && p[6] >= -16384 && p[6] <= 16384 && p[7] >= 0 && p[7] <= 16384,
                  "%s: position %d has the unit vector s=(%lld, %lld, %lld) (|s_y|, |s_x| <= 16384, 0 <= s_z <= 16384)", who, i,
                  (long long)p[5], (long long)p[6], (long long)p[7]);
        GHM_CHECK(p[8] >= 0 && p[8] <= GHM_SUNLIGHT_MAX_WEIGHT, "%s: position %d has w_q=%lld (0 .. %d)", who, i, (long long)p[8],
                  GHM_SUNLIGHT_MAX_WEIGHT);
        weight += p[8];
    }
    GHM_CHECK(weight <= GHM_SUNLIGHT_MAX_WEIGHT, "%s: the positions' w_q sum to %lld (<= %d)", who, (long long)weight,
              GHM_SUNLIGHT_MAX_WEIGHT);
    SunArgs a;
    a.zq = zq;
    a.top = top;
    a.zmax = zmax;
    a.lit = lit;
    a.mask = steps ? nullptr : mask;
    a.hours = hours;
    a.energy = energy;
    a.H = H;
    a.W = W;
    a.pz = z_pitch;
    a.pl = l_pitch;
    a.pm = m_pitch;
    a.ph = h_pitch;
    a.pe = e_pitch;
    a.TW = ceil_div(W, SUN_B);
    a.target_q = target_q;
    for (int at = 0; at < n; at += SUN_CHUNK) {
        SunChunk sun = {};
        a.n = min(SUN_CHUNK, n - at);
        a.first = at == 0;
        for (int i = 0; i < a.n; ++i) {
            const int64_t* p = table + GHM_SUNLIGHT_FIELDS * (size_t)(at + i);
            SunPos& o = sun.p[i];
            o.rows = (signed char)p[0];
            o.gmaj = (signed char)p[1];
            o.gmin = (signed char)p[2];
            o.m_q = (int)p[3];
            o.rise_q = p[4];
            o.s_y = (short)p[5];
            o.s_x = (short)p[6];
            o.s_z = (short)p[7];
            o.w_q = (int)p[8];
        }
        if (steps) {
            if (accel)
                hipLaunchKernelGGL((sun_kernel<true, true>), SUN_GRID(H, W), a, sun);
            else
                hipLaunchKernelGGL((sun_kernel<false, true>), SUN_GRID(H, W), a, sun);
        } else {
            if (accel)
                hipLaunchKernelGGL((sun_kernel<true, false>), SUN_GRID(H, W), a, sun);
            else
                hipLaunchKernelGGL((sun_kernel<false, false>), SUN_GRID(H, W), a, sun);
        }
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_sunlight_zmax(ghm_ctx* ctx, const int32_t* top, int64_t top_elems, int32_t* zmax) {
    GHM_CHECK(ctx && top && zmax, "ghm_sunlight_zmax: null pointer");
    GHM_CHECK(top_elems >= 1 && top_elems < ((int64_t)1 << 31), "ghm_sunlight_zmax: %lld block maxima (1 .. 2^31 - 1)",
              (long long)top_elems);
    hipLaunchKernelGGL(sun_zmax_kernel, dim3(1), dim3(256), 0, ctx->stream, top, (long)top_elems, zmax);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_sunlight_sun(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, int32_t H, int32_t W, const int64_t* table, int32_t n,
                     int32_t target_q, int32_t accel, const int32_t* top, const int32_t* zmax, uint32_t* lit, int32_t l_pitch,
                     uint32_t* mask, int32_t m_pitch, uint32_t* hours_q, int32_t h_pitch, uint32_t* energy, int32_t e_pitch) {
    return sun_launch(ctx, "ghm_sunlight_sun", zq, z_pitch, H, W, table, n, target_q, accel, top, zmax, lit, l_pitch, mask, m_pitch,
                      hours_q, h_pitch, energy, e_pitch, false);
}

int ghm_sunlight_steps(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, int32_t H, int32_t W, const int64_t* table, int32_t n,
                       int32_t target_q, int32_t accel, const int32_t* top, const int32_t* zmax, uint32_t* steps, int32_t s_pitch) {
    return sun_launch(ctx, "ghm_sunlight_steps", zq, z_pitch, H, W, table, n, target_q, accel, top, zmax, steps, s_pitch, nullptr, 0,
                      nullptr, 0, nullptr, 0, true);
}

}  // extern "C"
