// The device code of csrc/peaks.hip compiled for the host (tests/test_peaks_host.py): HIP's qualifiers are defined away, a "launch"
// is a loop over the cells, the summits or the list's entries, the two atomics are serial stand-ins.  PEAKS_DEVICE_INC is the part
// of the file before its extern "C" entry points, ghm_peaks_merge's body (pk_merge) included.  The rounds are issued as the entry
// point issues them; every array has exactly the size the entry points give it, so that an index past it is an error of its own
// under the sanitizers.  The labels and areas, which the device takes from ghm_hydrology_accumulate, are climbed cell by cell here.
#include <algorithm>
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
#define __shared__
#define __constant__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __syncthreads()
struct Dim3 {
    unsigned x, y, z;
};
static Dim3 threadIdx, blockIdx;
using std::max;
using std::min;
static inline void hyd_raise(int, int*) {}
static inline unsigned long long atomicMax(unsigned long long* at, unsigned long long v) {
    const unsigned long long old = *at;
    if (v > old) *at = v;
    return old;
}
static inline unsigned atomicOr(unsigned* at, unsigned v) {
    const unsigned old = *at;
    *at = old | v;
    return old;
}
#include PEAKS_DEVICE_INC

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

// the three kernels of a scan, in place over io[0 .. n]; returns the total
static int64_t scan(int* io, long n) {
    const long nb = (n + 255) / 256;
    std::vector<int64_t> sums((size_t)nb + 1, -1);
    int sm[256], own[256];
    int64_t sg[16], sv[256], before[256];
    for (long b = 0; b < nb; ++b) {
        for (int t = 0; t < 256; ++t) sm[t] = pk_scan_load(io, n, b, t);
        for (int t = 0; t < 256; ++t) pk_scan_groups(sm, sg, t);
        sums[b] = pk_scan_before(sm, sg, 256);
    }
    for (int t = 0; t < 256; ++t) pk_scan_chunks(sums.data(), nb, sv, t);
    for (int t = 0; t < 256; ++t) pk_scan_spread(sums.data(), nb, sv, t);
    for (long b = 0; b < nb; ++b) {
        for (int t = 0; t < 256; ++t) own[t] = sm[t] = pk_scan_load(io, n, b, t);
        for (int t = 0; t < 256; ++t) pk_scan_groups(sm, sg, t);
        for (int t = 0; t < 256; ++t) before[t] = pk_scan_before(sm, sg, t);
        for (int t = 0; t < 256; ++t) pk_scan_put(n, sums.data(), io, b, t, own[t], before[t]);
    }
    return sums[(size_t)nb];
}

// run H W z_pitch pitch form in out
//   in:  zq int32 [H, z_pitch]
//   out: int64 P, T, rounds, E, jumps; ascent int8 [H, pitch]; label int32, area uint32, mask uint32 [H, pitch] each, cells beyond W
//        keep the byte 0xAB; summit int32 [P]; area uint32 [P]; tree int32 [T, 3]; col, parent, prominence_q int32 [P]
static int run(char** argv) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), pz = atoi(argv[4]), pp = atoi(argv[5]), form = atoi(argv[6]);
    if (H < 1 || W < 1 || pz < W || pp < W || (form != 0 && form != 1)) return 2;
    std::vector<char> in;
    if (!read_all(argv[7], in) || in.size() != (size_t)H * pz * 4) return 3;
    const int* zq = (const int*)in.data();
    const int n = H * W;
    std::vector<signed char> asc((size_t)H * pp, (signed char)0xAB);
    std::vector<int> label((size_t)H * pp, (int)0xABABABABu);
    std::vector<unsigned> area((size_t)H * pp, 0xABABABABu), mask((size_t)H * pp, 0xABABABABu);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) asc[(size_t)r * pp + c] = (signed char)pk_ascent_cell(zq, pz, H, W, r, c);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) area[(size_t)r * pp + c] = 0;
    for (int i = 0; i < n; ++i) {
        int r = i / W, c = i % W;
        for (int hops = 0;; ++hops) {
            if (hops > n) return 5;
            area[(size_t)r * pp + c] += 1;
            const int k = asc[(size_t)r * pp + c];
            if (k < 0) break;
            r += PK_DY[k], c += PK_DX[k];
            if (r < 0 || r >= H || c < 0 || c >= W) return 5;
        }
        label[(size_t)(i / W) * pp + i % W] = r * W + c;
    }

    PkPlane p;
    p.zq = zq, p.label = label.data();
    p.H = H, p.W = W, p.pz = pz, p.pl = pp, p.n = n;
    std::vector<int> sidx((size_t)n + 1, -1), eoff((size_t)n + 1, -1);
    for (int i = 0; i < n; ++i)
        if (pk_flag_cell(p, i, sidx.data(), eoff.data())) return 6;
    const int64_t P = scan(sidx.data(), n), E = scan(eoff.data(), n);
    if (P < 1 || P != sidx[(size_t)n] || E != eoff[(size_t)n]) return 7;
    std::vector<int> summit((size_t)P, -1), comp((size_t)n, -1), hook((size_t)n, -1);
    std::vector<pk_u64> best((size_t)n, ~0ull);
    PkState s = {};
    s.sidx = sidx.data(), s.summit = summit.data(), s.comp = comp.data(), s.hook = hook.data(), s.best = best.data();
    s.mask = mask.data(), s.pm = pp, s.P = (int)P;
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) mask[(size_t)r * pp + c] = 0u;
    for (int i = 0; i < n; ++i) pk_list_cell(s, i);

    std::vector<pk_u64> list[2];
    std::vector<int> alive;
    long left = 0;
    int cur = 0;
    if (form == 1) {
        list[0].assign((size_t)E, 0), list[1].assign((size_t)E, 0);
        alive.assign((size_t)E + 1, -1);
        left = (long)E;
        for (int i = 0; i < n; ++i) pk_fill_cell(p, eoff.data(), i, list[0].data());
    }
    int64_t rounds = 0, jumps = 0;
    for (;;) {
        for (int j = 0; j < P; ++j) pk_clear_summit(s, j);
        if (form == 1) {
            if (left == 0) break;
            for (long i = 0; i < left; ++i) pk_pick_item(p, s, list[cur].data(), i, alive.data());
            const long kept = (long)scan(alive.data(), left);
            if (kept == 0) break;
            if (rounds == GHM_PEAKS_MAX_ROUNDS) return 8;
            for (long i = 0; i < left; ++i) pk_keep_item(list[cur].data(), alive.data(), i, list[cur ^ 1].data());
            cur ^= 1;
            left = kept;
        } else {
            int found = 0;
            for (int i = 0; i < n; ++i) found |= pk_pick_cell(p, s, i);
            if (!found) break;
            if (rounds == GHM_PEAKS_MAX_ROUNDS) return 8;
        }
        for (int j = 0; j < P; ++j) pk_hook_summit(p, s, j);
        for (int j = 0; j < P; ++j) pk_apply_summit(s, j);
        for (int pass = 0;; ++pass) {
            if (pass == 64) return 9;
            int any = 0;
            for (int j = 0; j < P; ++j) any |= pk_jump_summit(s, j);
            ++jumps;
            if (!any) break;
        }
        ++rounds;
    }
    for (int i = 0; i < n; ++i) pk_marks_cell(mask.data(), pp, W, i, eoff.data());
    const int64_t T = scan(eoff.data(), n);
    if (T != P - 1) return 10;

    std::vector<int> summit_out((size_t)P, -1), tree((size_t)(3 * T), -1);
    std::vector<unsigned> area_out((size_t)P, 0xABABABABu);
    PkOut o = {};
    o.summit = summit.data(), o.area = area.data(), o.toff = eoff.data(), o.mask = mask.data();
    o.pa = pp, o.pm = pp, o.P = (int)P;
    o.summit_out = summit_out.data(), o.area_out = area_out.data(), o.tree = tree.data();
    for (int j = 0; j < P; ++j) pk_out_summit(o, W, j);
    for (int i = 0; i < n; ++i) pk_out_cell(p, o, i);

    std::vector<int32_t> szq((size_t)P), ezq((size_t)T), col((size_t)P, -7), parent((size_t)P, -7), prom((size_t)P, -7);
    int32_t lowest = zq[0];
    for (int i = 0; i < n; ++i) lowest = min(lowest, zq[(size_t)(i / W) * pz + i % W]);
    for (int64_t j = 0; j < P; ++j) szq[(size_t)j] = zq[(size_t)(summit_out[(size_t)j] / W) * pz + summit_out[(size_t)j] % W];
    for (int64_t j = 0; j < T; ++j) ezq[(size_t)j] = zq[(size_t)(tree[(size_t)(3 * j)] / W) * pz + tree[(size_t)(3 * j)] % W];
    const int rc = pk_merge(summit_out.data(), szq.data(), P, tree.data(), ezq.data(), T, lowest, col.data(), parent.data(), prom.data());
    if (rc) return 20 + rc;

    FILE* fo = fopen(argv[8], "wb");
    if (!fo) return 4;
    const int64_t head[5] = {P, T, rounds, E, jumps};
    fwrite(head, 8, 5, fo);
    fwrite(asc.data(), 1, asc.size(), fo);
    fwrite(label.data(), 4, label.size(), fo);
    fwrite(area.data(), 4, area.size(), fo);
    fwrite(mask.data(), 4, mask.size(), fo);
    fwrite(summit_out.data(), 4, summit_out.size(), fo);
    fwrite(area_out.data(), 4, area_out.size(), fo);
    fwrite(tree.data(), 4, tree.size(), fo);
    fwrite(col.data(), 4, col.size(), fo);
    fwrite(parent.data(), 4, parent.size(), fo);
    fwrite(prom.data(), 4, prom.size(), fo);
    fclose(fo);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 9 && std::string(argv[1]) == "run") return run(argv);
    return 2;
}
