// The device code of csrc/viewshed.hip compiled for the host (tests/test_viewshed_host.py): HIP's qualifiers are defined away, a
// "launch" is a loop over the cells.  VIEWSHED_DEVICE_INC is the part of the file before its extern "C" entry points.  The
// observers go to the sight lines in chunks of GHM_VIEWSHED_CHUNK, the first of which stores and the later ones add, as the
// entry point issues them; the block maxima lie in an array of exactly their size, so that an index past it is an error of its
// own under the sanitizers.
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
struct Dim3 {
    unsigned x, y, z;
};
static Dim3 threadIdx, blockIdx;
using std::max;
using std::min;
#include VIEWSHED_DEVICE_INC

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

// quantise H W in_pitch out_pitch height_scale in out
//   in:  h float32 [H, in_pitch]; out: zq int32 [H, out_pitch]; cells beyond W keep the byte 0xAB
static int run_quantise(char** argv) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), pi = atoi(argv[4]), po = atoi(argv[5]);
    const double height_scale = atof(argv[6]);
    if (H < 1 || W < 1 || pi < W || po < W) return 2;
    std::vector<char> in;
    if (!read_all(argv[7], in) || in.size() != (size_t)H * pi * 4) return 3;
    std::vector<int> zq((size_t)H * po, (int)0xABABABABu);
    VsQuant a;
    a.h = (const float*)in.data();
    a.zq = zq.data();
    a.H = H, a.W = W, a.ph = pi, a.pz = po;
    a.scale = (float)(height_scale * 256.0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) vs_quantise_cell(a, y, x);
    FILE* fo = fopen(argv[8], "wb");
    if (!fo) return 4;
    fwrite(zq.data(), 4, zq.size(), fo);
    fclose(fo);
    return 0;
}

template <bool ACCEL, bool STEPS>
static void sight(VsSight a, const int* observers, int n, unsigned* out) {
    a.count = out;
    for (int at = 0; at < n; at += VS_CHUNK) {
        VsObs obs = {};
        a.n = std::min(VS_CHUNK, n - at);
        a.first = at == 0;
        for (int i = 0; i < a.n; ++i)
            for (int j = 0; j < 4; ++j) obs.v[i][j] = observers[4 * (size_t)(at + i) + j];
        for (int y = 0; y < a.H; ++y)
            for (int x = 0; x < a.W; ++x) vs_sight_cell<ACCEL, STEPS>(a, obs, y, x);
    }
}

// sight H W z_pitch out_pitch n target_q in out
//   in:  zq int32 [H, z_pitch], the observers int32 [n, 4]
//   out: the block maxima int32 [ceil(H / B), ceil(W / B)], then for the plain and for the accel form the count, the mask (left
//        alone beyond 32 observers) and the steps tested, uint32 [H, out_pitch] each; cells beyond W keep the byte 0xAB
static int run_sight(char** argv) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), pz = atoi(argv[4]), po = atoi(argv[5]), n = atoi(argv[6]);
    const int target_q = atoi(argv[7]);
    if (H < 1 || W < 1 || pz < W || po < W || n < 1 || n > GHM_VIEWSHED_MAX_OBSERVERS || target_q < 0) return 2;
    std::vector<char> in;
    const size_t plane = (size_t)H * pz * 4;
    if (!read_all(argv[8], in) || in.size() != plane + 16 * (size_t)n) return 3;
    const int* observers = (const int*)(in.data() + plane);
    for (int i = 0; i < n; ++i)
        if (observers[4 * i] < 0 || observers[4 * i] >= H || observers[4 * i + 1] < 0 || observers[4 * i + 1] >= W) return 2;
    VsTop t;
    t.zq = (const int*)in.data();
    t.H = H, t.W = W, t.pz = pz, t.TH = (H + VS_B - 1) / VS_B, t.TW = (W + VS_B - 1) / VS_B;
    std::vector<int> top((size_t)t.TH * t.TW);
    t.top = top.data();
    for (int by = 0; by < t.TH; ++by)
        for (int bx = 0; bx < t.TW; ++bx) vs_top_cell(t, by, bx);
    const size_t cells = (size_t)H * po;
    std::vector<unsigned> out[2][3];
    for (int accel = 0; accel < 2; ++accel) {
        for (int k = 0; k < 3; ++k) out[accel][k].assign(cells, 0xABABABABu);
        VsSight a;
        a.zq = t.zq;
        a.top = accel ? top.data() : nullptr;
        a.mask = n <= 32 ? out[accel][1].data() : nullptr;
        a.H = H, a.W = W, a.pz = pz, a.pc = po, a.pm = po, a.TW = t.TW, a.target_q = target_q;
        if (accel) {
            sight<true, false>(a, observers, n, out[accel][0].data());
            sight<true, true>(a, observers, n, out[accel][2].data());
        } else {
            sight<false, false>(a, observers, n, out[accel][0].data());
            sight<false, true>(a, observers, n, out[accel][2].data());
        }
    }
    FILE* fo = fopen(argv[9], "wb");
    if (!fo) return 4;
    fwrite(top.data(), 4, top.size(), fo);
    for (int accel = 0; accel < 2; ++accel)
        for (int k = 0; k < 3; ++k) fwrite(out[accel][k].data(), 4, cells, fo);
    fclose(fo);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 9 && std::string(argv[1]) == "quantise") return run_quantise(argv);
    if (argc == 10 && std::string(argv[1]) == "sight") return run_sight(argv);
    return 2;
}
