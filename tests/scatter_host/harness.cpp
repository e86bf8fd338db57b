// The device code of csrc/scatter.hip compiled for the host (tests/test_scatter_host.py): HIP's qualifiers and the few built-ins
// the kernels use are defined away, a "launch" is a loop over blocks and threads.  SCATTER_DEVICE_INC is the part of the file
// before its extern "C" entry points.  The plain thinning is swept from one plane into the other until a sweep changes nothing; the
// tiled one is run phase by phase: every thread of a block runs a phase before any runs the next, on LDS arrays of exactly the
// window's sizes that hold garbage before each block.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ghm.h"
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__
struct Dim3 {
    unsigned x, y, z;
};
static Dim3 threadIdx, blockIdx;
static inline void __syncthreads() {}
static inline int __syncthreads_or(int v) { return v; }
static inline void hyd_raise(int, int*) {}
using std::max;
using std::min;
#include SCATTER_DEVICE_INC

static bool read_all(const char* path, std::vector<char>& buf) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    buf.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    const bool ok = fread(buf.data(), 1, buf.size(), f) == buf.size();
    fclose(f);
    return ok;
}

// Jacobi sweeps between ``state`` (pitch ps) and a second plane of pitch W, as the entry point issues them -> the sweeps, the last,
// which changed nothing, included
static int64_t thin_plain(ScThin a, unsigned char* state, int ps) {
    std::vector<unsigned char> other((size_t)a.H * a.W, (unsigned char)0xCD);
    for (int64_t i = 0;; ++i) {
        if (i & 1)
            a.src = other.data(), a.pi = a.W, a.state = state, a.ps = ps;
        else
            a.src = state, a.pi = ps, a.state = other.data(), a.ps = a.W;
        int changed = 0;
        for (int y = 0; y < a.H; ++y)
            for (int x = 0; x < a.W; ++x) changed |= sc_plain_cell(a, y, x);
        if (!changed) return i + 1;
        if (i > (int64_t)a.H * a.W) return -1;
    }
}

// launches of the tiled kernel over every tile until one changes nothing -> the launches
static int64_t thin_tiled(ScThin a) {
    const int n = SC_TILE + 2 * a.R;
    // two separate arrays of the exact sizes, so that an index past either is an error of its own under the sanitizers
    std::vector<unsigned> wp((size_t)n * n);
    std::vector<unsigned char> ws((size_t)n * n);
    for (int64_t i = 0;; ++i) {
        int changed = 0;
        for (int ty = 0; ty < a.H; ty += SC_TILE)
            for (int tx = 0; tx < a.W; tx += SC_TILE) {
                std::fill(wp.begin(), wp.end(), 0xCDCDCDCDu);
                std::fill(ws.begin(), ws.end(), (unsigned char)0x01);         // garbage that looks like a candidate
                int live = 0;
                for (int t = 0; t < 256; ++t) live |= sc_live(a, ty, tx, t);
                if (!live) continue;
                for (int t = 0; t < 256; ++t) sc_stage(a, wp.data(), ws.data(), ty, tx, t);
                for (int s = 0; s <= SC_TILE * SC_TILE; ++s) {
                    int ch = 0;
                    for (int t = 0; t < 256; ++t) ch |= sc_sweep(a, wp.data(), ws.data(), t);
                    if (!ch) break;
                }
                for (int t = 0; t < 256; ++t) changed |= sc_store(a, ws.data(), ty, tx, t);
            }
        if (!changed) return i + 1;
        if (i > (int64_t)a.H * a.W) return -1;
    }
}

// thin H W pitch s2 in out
//   in:  state uint8 [H, pitch], priority uint32 [H, pitch]; the cells beyond W hold what the caller likes
//   out: the states of the plain and of the tiled form, uint8 [H, pitch] each, thinned in place, then two int64: the plain form's
//        sweeps and the tiled form's launches
static int run_thin(char** argv) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), pi = atoi(argv[4]), s2 = atoi(argv[5]);
    if (H < 1 || W < 1 || pi < W || s2 < 1 || s2 > GHM_SCATTER_MAX_S2) return 2;
    std::vector<char> in;
    const size_t cells = (size_t)H * pi;
    if (!read_all(argv[6], in) || in.size() != cells * 5) return 3;
    std::vector<unsigned> prio(cells);
    memcpy(prio.data(), in.data() + cells, cells * 4);
    std::vector<unsigned char> out[2];
    int64_t counts[2];
    for (int tiled = 0; tiled < 2; ++tiled) {
        out[tiled].assign((const unsigned char*)in.data(), (const unsigned char*)in.data() + cells);
        ScThin a;
        a.prio = prio.data();
        a.src = a.state = out[tiled].data();
        a.H = H, a.W = W, a.pp = pi, a.pi = pi, a.ps = pi, a.s2 = s2, a.R = sc_reach(s2);
        counts[tiled] = tiled ? thin_tiled(a) : thin_plain(a, out[tiled].data(), pi);
    }
    FILE* fo = fopen(argv[7], "wb");
    if (!fo) return 4;
    for (int tiled = 0; tiled < 2; ++tiled) fwrite(out[tiled].data(), 1, out[tiled].size(), fo);
    fwrite(counts, 8, 2, fo);
    fclose(fo);
    return 0;
}

// chance H W in_pitch out_pitch seed origin_row origin_col height_scale density water_n threshold in out
//   in:  h float32, dist2 int32, blocked uint32, each [H, in_pitch]; the tables, 384 float32; water_n + 1 float32
//        water_n = 0: no water factor; threshold = 0: no blocked plane
//   out: chance uint32, priority uint32 [H, out_pitch], state uint8 [H, out_pitch]; cells beyond W keep the byte 0xAB
static int run_chance(char** argv) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), pi = atoi(argv[4]), po = atoi(argv[5]);
    const uint64_t seed = strtoull(argv[6], nullptr, 10);
    const long long r0 = atoll(argv[7]), c0 = atoll(argv[8]);
    const double height_scale = atof(argv[9]);
    const float density = (float)atof(argv[10]);
    const int water_n = atoi(argv[11]);
    const unsigned threshold = (unsigned)strtoul(argv[12], nullptr, 10);
    if (H < 1 || W < 1 || pi < W || po < W || water_n < 0 || water_n > 1025) return 2;
    std::vector<char> in;
    const size_t plane = (size_t)H * pi * 4;
    if (!read_all(argv[13], in) || in.size() != 3 * plane + 4 * (size_t)(GHM_SCATTER_TABLE_FLOATS + water_n + 1)) return 3;
    const size_t cells = (size_t)H * po;
    std::vector<unsigned> chance(cells, 0xABABABABu), prio(cells, 0xABABABABu);
    std::vector<unsigned char> state(cells, (unsigned char)0xAB);
    ScChance a;
    a.h = (const float*)in.data();
    a.dist2 = (const int*)(in.data() + plane);
    a.blocked = threshold ? (const unsigned*)(in.data() + 2 * plane) : nullptr;
    a.tables = (const float*)(in.data() + 3 * plane);
    a.water = water_n ? a.tables + GHM_SCATTER_TABLE_FLOATS : nullptr;
    a.chance = chance.data();
    a.H = H, a.W = W, a.ph = pi, a.pd = pi, a.pb = pi, a.pc = po, a.water_n = water_n, a.threshold = threshold;
    a.half_scale = (float)(height_scale / 2), a.density = density;
    ScCand c;
    c.chance = chance.data(), c.state = state.data(), c.prio = prio.data();
    c.H = H, c.W = W, c.pc = po, c.ps = po, c.pp = po;
    c.seed_lo = (unsigned)seed, c.seed_hi = (unsigned)(seed >> 32);
    c.row0 = (unsigned)(uint64_t)(int64_t)r0, c.col0 = (unsigned)(uint64_t)(int64_t)c0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            sc_chance_cell(a, y, x);
            sc_cand_cell(c, y, x);
        }
    FILE* fo = fopen(argv[14], "wb");
    if (!fo) return 4;
    fwrite(chance.data(), 4, cells, fo);
    fwrite(prio.data(), 4, cells, fo);
    fwrite(state.data(), 1, cells, fo);
    fclose(fo);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 8 && std::string(argv[1]) == "thin") return run_thin(argv);
    if (argc == 15 && std::string(argv[1]) == "chance") return run_chance(argv);
    return 2;
}
