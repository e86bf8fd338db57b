// The device code of csrc/earthworks.hip compiled for the host (tests/test_earthworks_host.py): HIP's qualifiers and the few
// built-ins the kernels use are defined away, a "launch" is a loop over blocks and threads.  EARTHWORKS_DEVICE_INC is the part of
// the file before its extern "C" entry points.  The tiled kernel is run phase by phase: every thread of a block runs a phase
// before any runs the next, on LDS arrays of exactly the window's and the column offsets' sizes that hold garbage before each block.
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
using std::max;
using std::min;
#include EARTHWORKS_DEVICE_INC

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

static void nearest_plain(const EwNear& a) {
    for (int y = 0; y < a.H; ++y)
        for (int x = 0; x < a.W; ++x) ew_plain_cell(a, y, x);
}

static void nearest_tiled(const EwNear& a) {
    const int n = EW_TILE + 2 * a.R;
    // two separate arrays of the exact sizes, so that an index past either is an error of its own under the sanitizers
    std::vector<unsigned char> win((size_t)n * n);
    std::vector<signed char> col((size_t)EW_TILE * n);
    for (int ty = 0; ty < a.H; ty += EW_TILE)
        for (int tx = 0; tx < a.W; tx += EW_TILE) {
            std::fill(win.begin(), win.end(), (unsigned char)0xCD);
            std::fill(col.begin(), col.end(), (signed char)0x5A);
            int any = 0;
            for (int t = 0; t < 256; ++t) any |= ew_stage(a, win.data(), ty, tx, t);
            if (!any) {
                for (int t = 0; t < 256; ++t) ew_none(a, ty, tx, t);
                continue;
            }
            for (int t = 0; t < 256; ++t) ew_columns(a, win.data(), col.data(), t);
            for (int t = 0; t < 256; ++t) ew_rows(a, col.data(), ty, tx, t);
        }
}

// run H W in_pitch out_pitch R threshold mode in out
// in:  marks uint32 [H, in_pitch], h float32 [H, in_pitch], target float32 [H, in_pitch], table float32 [R R + 1, 2]
// out: five planes [H, out_pitch] whose cells beyond W keep the byte 0xAB: nearest and dist2 of the plain form, of the tiled
//      form, and the shaped heights (from the tiled form's planes)
int main(int argc, char** argv) {
    if (argc != 11 || std::string(argv[1]) != "run") return 2;
    const int H = atoi(argv[2]), W = atoi(argv[3]), pi = atoi(argv[4]), po = atoi(argv[5]), R = atoi(argv[6]);
    const unsigned threshold = (unsigned)strtoul(argv[7], nullptr, 10);
    const int mode = atoi(argv[8]);
    if (H < 1 || W < 1 || pi < W || po < W || R < 0 || R > GHM_EARTHWORKS_MAX_REACH || threshold < 1 || mode < 0 || mode > 2) return 2;
    std::vector<char> in;
    const size_t plane = (size_t)H * pi * 4, table_bytes = (size_t)(R * R + 1) * 8;
    if (!read_all(argv[9], in) || in.size() != 3 * plane + table_bytes) return 3;
    const size_t cells = (size_t)H * po;
    std::vector<int32_t> near[2], d2[2];
    EwNear a;
    a.marks = (const unsigned*)in.data();
    a.H = H, a.W = W, a.pm = pi, a.pn = po, a.pd = po, a.R = R, a.threshold = threshold;
    for (int tiled = 0; tiled < 2; ++tiled) {
        near[tiled].assign(cells, (int32_t)0xABABABAB);
        d2[tiled].assign(cells, (int32_t)0xABABABAB);
        a.nearest = near[tiled].data(), a.dist2 = d2[tiled].data();
        if (tiled)
            nearest_tiled(a);
        else
            nearest_plain(a);
    }
    std::vector<float> out(cells);
    memset(out.data(), 0xAB, cells * 4);
    EwShape s;
    s.h = (const float*)(in.data() + plane), s.target = (const float*)(in.data() + 2 * plane);
    s.table = (const float*)(in.data() + 3 * plane);
    s.nearest = near[1].data(), s.dist2 = d2[1].data(), s.out = out.data();
    s.H = H, s.W = W, s.ph = pi, s.pn = po, s.pd = po, s.pt = pi, s.po = po, s.R = R, s.mode = mode;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) ew_shape_cell(s, y, x);
    FILE* fo = fopen(argv[10], "wb");
    if (!fo) return 4;
    for (int tiled = 0; tiled < 2; ++tiled) {
        fwrite(near[tiled].data(), 4, cells, fo);
        fwrite(d2[tiled].data(), 4, cells, fo);
    }
    fwrite(out.data(), 4, cells, fo);
    fclose(fo);
    return 0;
}
