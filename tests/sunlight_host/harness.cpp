// The sun kernel of csrc/sunlight.hip compiled for the host (tests/test_sunlight_host.py): HIP's qualifiers are defined away and a
// launch is a loop over the blocks and their threads, one after the other -- the kernel has no barrier and no LDS.
// SUNLIGHT_DEVICE_INC is the part of the file in front of its launch macro.  The heights come in rows of W + 3 cells, the four
// planes go out in rows of W + 3 cells that start as 0xAB bytes, the block maxima are dense, and every buffer has exactly its
// size, so that an index past one is an error of its own under the sanitizers.  The block maxima, zmax and the chunks of
// positions are made here as the entry point makes them.
//   harness H W n target_q accel steps ZQ TABLE OUT        (OUT: lit, mask, hours_q, energy one after the other)
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ghm.h"
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
struct Dim3 {
    unsigned x, y, z;
};
static Dim3 threadIdx, blockIdx;
using std::max;
using std::min;
#include SUNLIGHT_DEVICE_INC

template <bool ACCEL, bool STEPS>
static void launch(const SunArgs& a, const SunChunk& sun) {
    for (unsigned by = 0; by < (unsigned)((a.H + SUN_B - 1) / SUN_B); ++by)
        for (unsigned bx = 0; bx < (unsigned)((a.W + SUN_B - 1) / SUN_B); ++bx)
            for (unsigned ty = 0; ty < (unsigned)SUN_B; ++ty)
                for (unsigned tx = 0; tx < (unsigned)SUN_B; ++tx) {
                    blockIdx = {bx, by, 0};
                    threadIdx = {tx, ty, 0};
                    sun_kernel<ACCEL, STEPS>(a, sun);
                }
}

int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int H = atoi(argv[1]), W = atoi(argv[2]), n = atoi(argv[3]), target_q = atoi(argv[4]);
    const bool accel = atoi(argv[5]) != 0, steps = atoi(argv[6]) != 0;
    if (H < 1 || W < 1 || n < 1 || n > GHM_SUNLIGHT_MAX_POSITIONS) return 2;
    const int P = W + 3, TH = (H + SUN_B - 1) / SUN_B, TW = (W + SUN_B - 1) / SUN_B;
    std::vector<int> zq((size_t)H * P);
    std::vector<int64_t> table((size_t)n * GHM_SUNLIGHT_FIELDS);
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(zq.data(), sizeof(int), zq.size(), f) != zq.size()) return 3;
    fclose(f);
    f = fopen(argv[8], "rb");
    if (!f || fread(table.data(), sizeof(int64_t), table.size(), f) != table.size()) return 3;
    fclose(f);
    std::vector<int> top((size_t)TH * TW, INT_MIN);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int& t = top[(size_t)(y / SUN_B) * TW + x / SUN_B];
            t = max(t, zq[(size_t)y * P + x]);
        }
    std::vector<int> zmax(1, *std::max_element(top.begin(), top.end()));
    std::vector<unsigned> planes[4];
    for (auto& p : planes) p.assign((size_t)H * P, 0xABABABABu);
    SunArgs a;
    a.zq = zq.data();
    a.top = accel ? top.data() : nullptr;
    a.zmax = zmax.data();
    a.lit = planes[0].data();
    a.mask = !steps && n <= 32 ? planes[1].data() : nullptr;
    a.hours = steps ? nullptr : planes[2].data();
    a.energy = steps ? nullptr : planes[3].data();
    a.H = H;
    a.W = W;
    a.pz = a.pl = a.pm = a.ph = a.pe = P;
    a.TW = TW;
    a.target_q = target_q;
    for (int at = 0; at < n; at += SUN_CHUNK) {
        SunChunk sun = {};
        a.n = min(SUN_CHUNK, n - at);
        a.first = at == 0;
        for (int i = 0; i < a.n; ++i) {
            const int64_t* p = table.data() + GHM_SUNLIGHT_FIELDS * (size_t)(at + i);
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
        if (steps)
            accel ? launch<true, true>(a, sun) : launch<false, true>(a, sun);
        else
            accel ? launch<true, false>(a, sun) : launch<false, false>(a, sun);
    }
    f = fopen(argv[9], "wb");
    if (!f) return 3;
    for (auto& p : planes)
        if (fwrite(p.data(), sizeof(unsigned), p.size(), f) != p.size()) return 3;
    fclose(f);
    return 0;
}
