// The device code of csrc/contour.hip compiled for the host (tests/test_contour_host.py): HIP's qualifiers are defined away, a
// "launch" is a loop over the cells or the segments, a kernel with barriers runs phase by phase over its block's threads.
// CONTOUR_DEVICE_INC is the part of the file before its extern "C" entry points.  The doubling rounds alternate between two pairs
// of buffers as the entry point issues them, one by one until a round changes nothing; every array has exactly the size the entry
// points give it, so that an index past it is an error of its own under the sanitizers.
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
#define __shared__
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
#include CONTOUR_DEVICE_INC

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

// the three kernels of a scan; out may be in
template <class Out>
static void scan(const int* in, long n, std::vector<int64_t>& sums, Out* out, bool write) {
    const long nb = (n + 255) / 256;
    sums.assign((size_t)nb + 1, -1);
    int sm[256], own[256];
    int64_t sg[16], sv[256], before[256];
    for (long b = 0; b < nb; ++b) {
        for (int t = 0; t < 256; ++t) sm[t] = ct_scan_load(in, n, b, t);
        for (int t = 0; t < 256; ++t) ct_scan_groups(sm, sg, t);
        sums[b] = ct_scan_before(sm, sg, 256);
    }
    for (int t = 0; t < 256; ++t) ct_scan_chunks(sums.data(), nb, sv, t);
    for (int t = 0; t < 256; ++t) ct_scan_spread(sums.data(), nb, sv, t);
    if (!write) return;
    for (long b = 0; b < nb; ++b) {
        for (int t = 0; t < 256; ++t) own[t] = sm[t] = ct_scan_load(in, n, b, t);
        for (int t = 0; t < 256; ++t) ct_scan_groups(sm, sg, t);
        for (int t = 0; t < 256; ++t) before[t] = ct_scan_before(sm, sg, t);
        for (int t = 0; t < 256; ++t) ct_scan_put<Out>(n, sums.data(), out, b, t, own[t], before[t]);
    }
}

// trace H W z_pitch m_pitch base_q interval_q count index_every in out
//   in:  zq int32 [H, z_pitch]
//   out: int64 S, L, V, rounds; edge int32 [V, 3]; t double [V]; offsets int64 [L + 1]; level int32 [L]; closed uint8 [L];
//        marks uint32 [H, m_pitch], cells beyond W keep the byte 0xAB
static int run_trace(char** argv) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), pz = atoi(argv[4]), pm = atoi(argv[5]);
    const int base_q = atoi(argv[6]), iq = atoi(argv[7]), count = atoi(argv[8]), index_every = atoi(argv[9]);
    if (H < 1 || W < 1 || pz < W || pm < W || iq < 1 || index_every < 1 || count == 0 || count < -1) return 2;
    std::vector<char> in;
    if (!read_all(argv[10], in) || in.size() != (size_t)H * pz * 4) return 3;
    CtPlane p;
    p.zq = (const int*)in.data();
    p.H = H, p.W = W, p.pz = pz;
    p.lv.base_q = base_q, p.lv.iq = iq;
    p.lv.jlo = count < 0 ? -CT_LEVEL_LIMIT : 0;
    p.lv.jhi = count < 0 ? CT_LEVEL_LIMIT : count;

    const long cells = H < 2 || W < 2 ? 0 : (long)(H - 1) * (W - 1);
    std::vector<int> off((size_t)cells + 1, 0);
    std::vector<int64_t> sums;
    int64_t S = 0, L = 0, V = 0, rounds = 0;
    if (cells > 0) {
        for (long n = 0; n < cells; ++n) ct_count_cell(p, n, off.data());
        scan<int>(off.data(), cells, sums, off.data(), true);
        S = sums[(size_t)((cells + 255) / 256)];
        if (S != off[(size_t)cells] || S >= ((int64_t)1 << 31)) return 5;
    }
    std::vector<int> edge, level;
    std::vector<double> t;
    std::vector<int64_t> offsets(1, 0);
    std::vector<uint8_t> closed;
    if (S > 0) {
        std::vector<int> cell((size_t)S), succ((size_t)S), pred((size_t)S), pair[2][2];
        for (auto& pr : pair)
            for (auto& v : pr) v.assign((size_t)S + 1, (int)0xABABABABu);
        CtSegs a;
        a.p = p;
        a.off = off.data();
        a.cell = cell.data(), a.succ = succ.data(), a.pred = pred.data();
        a.cells = cells, a.S = S;
        for (long n = 0; n < cells; ++n) ct_fill_cell(a, n);
        for (long s = 0; s < S; ++s) ct_link_seg(a, (int)s, pair[0][0].data(), pair[0][1].data());
        for (long s = 0; s < S; ++s)
            if (succ[s] < -1 || succ[s] >= S || pred[s] < -1 || pred[s] >= S) return 6;
        int at = 0;
        for (int i = 0;; ++i) {
            if (i == GHM_CONTOUR_MAX_ROUNDS) return 7;
            int any = 0;
            for (long s = 0; s < S; ++s)
                any |= ct_min_seg((int)s, pair[at][0].data(), pair[at][1].data(), pair[at ^ 1][0].data(), pair[at ^ 1][1].data());
            at ^= 1;
            if (!any) break;
        }
        for (long s = 0; s < S; ++s)
            ct_cut_seg((int)s, pair[at][0].data(), pair[at][1].data(), pred.data(), pair[at ^ 1][0].data(), pair[at ^ 1][1].data());
        at ^= 1;
        for (int i = 0;; ++i) {
            if (i == GHM_CONTOUR_MAX_ROUNDS) return 7;
            int any = 0;
            for (long s = 0; s < S; ++s)
                any |= ct_rank_seg((int)s, pair[at][0].data(), pair[at][1].data(), pair[at ^ 1][0].data(), pair[at ^ 1][1].data());
            at ^= 1;
            ++rounds;
            if (!any) break;
        }
        CtLines l = {};
        l.a = a;
        l.p = pair[at][0].data(), l.d = pair[at][1].data();
        l.line = pair[at ^ 1][0].data(), l.vcount = pair[at ^ 1][1].data();
        for (long s = 0; s < S; ++s) ct_flag_seg(l, (int)s);
        scan<int>(l.line, S, sums, l.line, true);
        L = sums[(size_t)((S + 255) / 256)];
        if (L < 1 || L > S) return 8;
        for (long s = 0; s < S; ++s) ct_tail_seg(l, (int)s);
        scan<int64_t>(l.vcount, L, sums, nullptr, false);
        V = sums[(size_t)((L + 255) / 256)];
        edge.assign((size_t)(3 * V), (int)0xABABABABu);
        t.assign((size_t)V, -1.0);
        offsets.assign((size_t)L + 1, -1);
        level.assign((size_t)L, (int)0xABABABABu);
        closed.assign((size_t)L, 0xAB);
        l.offsets = offsets.data();
        l.edge = edge.data(), l.t = t.data(), l.level = level.data(), l.closed = closed.data();
        scan<int64_t>(l.vcount, L, sums, offsets.data(), true);
        for (long s = 0; s < S; ++s) ct_write_seg(l, (int)s);
    }
    std::vector<uint32_t> marks((size_t)H * pm, 0xABABABABu);
    CtMarks m;
    m.p = p;
    m.marks = marks.data();
    m.pm = pm, m.index_every = index_every;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) ct_marks_cell(m, y, x);

    FILE* fo = fopen(argv[11], "wb");
    if (!fo) return 4;
    const int64_t head[4] = {S, L, V, rounds};
    fwrite(head, 8, 4, fo);
    fwrite(edge.data(), 4, edge.size(), fo);
    fwrite(t.data(), 8, t.size(), fo);
    fwrite(offsets.data(), 8, offsets.size(), fo);
    fwrite(level.data(), 4, level.size(), fo);
    fwrite(closed.data(), 1, closed.size(), fo);
    fwrite(marks.data(), 4, marks.size(), fo);
    fclose(fo);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 12 && std::string(argv[1]) == "trace") return run_trace(argv);
    return 2;
}
