// The device code of csrc/rivers.hip compiled for the host (tests/test_rivers_host.py): HIP's qualifiers are defined away and a
// "launch" is a loop over the cells, the list's entries or the reaches.  RIVERS_DEVICE_INC is the part of the file before its
// extern "C" entry points, ghm_rivers_order's body (rv_order) included.  The rounds are issued as the entry point issues them,
// between two buffer pairs; every array has exactly the size the entry points give it, so that an index past it is an error of
// its own under the sanitizers.
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
#define __syncthreads_count(x) (x)
struct Dim3 {
    unsigned x, y, z;
};
static Dim3 threadIdx, blockIdx;
using std::max;
using std::min;
static inline void hyd_raise(int, int*) {}
#include RIVERS_DEVICE_INC

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
        for (int t = 0; t < 256; ++t) sm[t] = rv_scan_load(io, n, b, t);
        for (int t = 0; t < 256; ++t) rv_scan_groups(sm, sg, t);
        sums[b] = rv_scan_before(sm, sg, 256);
    }
    for (int t = 0; t < 256; ++t) rv_scan_chunks(sums.data(), nb, sv, t);
    for (int t = 0; t < 256; ++t) rv_scan_spread(sums.data(), nb, sv, t);
    for (long b = 0; b < nb; ++b) {
        for (int t = 0; t < 256; ++t) own[t] = sm[t] = rv_scan_load(io, n, b, t);
        for (int t = 0; t < 256; ++t) rv_scan_groups(sm, sg, t);
        for (int t = 0; t < 256; ++t) before[t] = rv_scan_before(sm, sg, t);
        for (int t = 0; t < 256; ++t) rv_scan_put(n, sums.data(), io, b, t, own[t], before[t]);
    }
    return sums[(size_t)nb];
}

// run H W in_pitch out_pitch T form in out
//   in:  accumulation uint32 [H, in_pitch], then direction int8 [H, in_pitch]
//   out: int64 cells, R, sources, confluences, mouths, isolated, V, rounds; kind uint8 [H, out_pitch], cells beyond W keep the byte
//        0xAB; vertex int32 [V]; offsets int64 [R + 1]; downstream int32 [R]; area uint32 [R]; order, magnitude int32 [R]; main
//        uint8 [R]
// exit code 6: a refusal of the planes (7, 8, 9: which)
static int run(char** argv) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), pi = atoi(argv[4]), po = atoi(argv[5]), form = atoi(argv[7]);
    const unsigned T = (unsigned)strtoul(argv[6], nullptr, 10);
    if (H < 1 || W < 1 || pi < W || po < W || T < 1 || (form != 0 && form != 1)) return 2;
    std::vector<char> in;
    if (!read_all(argv[8], in) || in.size() != (size_t)H * pi * 5) return 3;
    const int n = H * W;
    RvPlane p;
    p.acc = (const unsigned*)in.data(), p.dir = (const signed char*)(in.data() + 4 * (size_t)H * pi);
    p.H = H, p.W = W, p.pd = pi, p.pa = pi, p.n = n, p.T = T;

    // the count
    std::vector<unsigned char> kind((size_t)H * po, 0xAB);
    std::vector<int> ridx((size_t)n + 1, -1), cidx((size_t)n + 1, -1);
    int64_t tally[4] = {0, 0, 0, 0};
    int errs = 0;
    for (int i = 0; i < n; ++i) {
        int err = 0;
        const int k = rv_flag_cell(p, i, kind.data(), po, ridx.data(), cidx.data(), err);
        errs |= err;
        const int bits = rv_tally_bits(k);
        for (int j = 0; j < 4; ++j) tally[j] += bits >> j & 1;
    }
    if (errs) return errs & 1 ? 7 : errs & 2 ? 8 : 9;
    const int64_t R = scan(ridx.data(), n), cells = scan(cidx.data(), n);
    if (R != ridx[(size_t)n] || cells != cidx[(size_t)n]) return 10;

    // the trace
    RvNet g;
    g.dir = p.dir, g.kind = kind.data(), g.ridx = ridx.data(), g.cidx = cidx.data();
    g.H = H, g.W = W, g.pd = pi, g.pk = po, g.n = n, g.R = (int)R;
    const long N = form == 1 ? (long)cells : n;
    std::vector<int> cell((size_t)(form == 1 ? cells : 0), -1), pb[2], db[2];
    for (int i = 0; i < 2; ++i) pb[i].assign((size_t)N, -1), db[i].assign((size_t)N, -1);
    for (int i = 0; i < n; ++i) {
        if (form == 1)
            rv_init_list_cell(g, i, cell.data(), pb[0].data(), db[0].data());
        else
            rv_init_plain_cell(g, i, pb[0].data(), db[0].data());
    }
    int launched = 0, needed = N > 0 ? 0 : 1;
    while (!needed) {
        if (launched > GHM_RIVERS_MAX_ROUNDS) return 11;
        const int a = launched & 1;
        int changed = 0;
        for (long s = 0; s < N; ++s) changed |= rv_rank_item((int)s, pb[a].data(), db[a].data(), pb[a ^ 1].data(), db[a ^ 1].data());
        ++launched;
        if (!changed) needed = launched;
    }
    // rounds past the fixed point, as a group issues them, leave the same values in the other pair
    for (int extra = 0; extra < 3 && N > 0; ++extra, ++launched) {
        const int a = launched & 1;
        for (long s = 0; s < N; ++s)
            if (rv_rank_item((int)s, pb[a].data(), db[a].data(), pb[a ^ 1].data(), db[a ^ 1].data())) return 12;
    }
    const int at = launched & 1;
    std::vector<int> rlen((size_t)R + 1, 0), rdown((size_t)R, -1);
    int64_t V = 0;
    if (R > 0) {
        for (long s = 0; s < N; ++s) {
            if (form == 1)
                rv_tail_cell(g, cell[(size_t)s], cell[(size_t)pb[at][(size_t)s]], db[at][(size_t)s], rlen.data(), rdown.data());
            else
                rv_tail_cell(g, (int)s, pb[at][(size_t)s], db[at][(size_t)s], rlen.data(), rdown.data());
        }
        V = scan(rlen.data(), (long)R);
        if (V != rlen[(size_t)R] || V < 2 * R) return 13;
    }

    // the extraction
    std::vector<int> vertex((size_t)V, -1), downstream((size_t)R, -7);
    std::vector<int64_t> offsets((size_t)R + 1, -7);
    if (R > 0) {
        for (long s = 0; s < N; ++s) {
            if (form == 1)
                rv_vertex_cell(g, cell[(size_t)s], cell[(size_t)pb[at][(size_t)s]], db[at][(size_t)s], rlen.data(), vertex.data());
            else
                rv_vertex_cell(g, (int)s, pb[at][(size_t)s], db[at][(size_t)s], rlen.data(), vertex.data());
        }
        for (long i = 0; i <= R; ++i) rv_out_reach(i, (long)R, rlen.data(), rdown.data(), offsets.data(), downstream.data());
    } else {
        offsets[0] = 0;
    }
    for (int64_t i = 0; i < V; ++i)
        if (vertex[(size_t)i] < 0 || vertex[(size_t)i] >= n) return 14;

    // the areas (the host's, as gan_heightmaps_amd/rivers.py takes them) and the orders
    std::vector<uint32_t> area((size_t)R, 0);
    for (int64_t r = 0; r < R; ++r) {
        const int end = vertex[(size_t)offsets[(size_t)r + 1] - 1], k = kind[(size_t)(end / W) * po + end % W];
        const int own = (k & GHM_RIVERS_MOUTH) && (k >> 4) == 1 ? end : vertex[(size_t)offsets[(size_t)r + 1] - 2];
        area[(size_t)r] = p.acc[(size_t)(own / W) * pi + own % W];
    }
    std::vector<int32_t> order((size_t)R, -7), magnitude((size_t)R, -7);
    std::vector<uint8_t> main_stem((size_t)R, 0xAB);
    const int rc = rv_order(downstream.data(), area.data(), R, order.data(), magnitude.data(), main_stem.data());
    if (rc) return 20 + rc;

    FILE* fo = fopen(argv[9], "wb");
    if (!fo) return 4;
    const int64_t head[8] = {cells, R, tally[0], tally[1], tally[2], tally[3], V, needed - 1};
    fwrite(head, 8, 8, fo);
    fwrite(kind.data(), 1, kind.size(), fo);
    fwrite(vertex.data(), 4, vertex.size(), fo);
    fwrite(offsets.data(), 8, offsets.size(), fo);
    fwrite(downstream.data(), 4, downstream.size(), fo);
    fwrite(area.data(), 4, area.size(), fo);
    fwrite(order.data(), 4, order.size(), fo);
    fwrite(magnitude.data(), 4, magnitude.size(), fo);
    fwrite(main_stem.data(), 1, main_stem.size(), fo);
    fclose(fo);
    return 0;
}

// order R in out: downstream int32 [R] then area uint32 [R] -> the exit code 20 + rv_order's, or 0 and order, magnitude, main
static int order_only(char** argv) {
    const long R = atol(argv[2]);
    std::vector<char> in;
    if (R < 0 || !read_all(argv[3], in) || in.size() != (size_t)R * 8) return 3;
    std::vector<int32_t> order((size_t)R), magnitude((size_t)R);
    std::vector<uint8_t> main_stem((size_t)R);
    const int rc = rv_order((const int32_t*)in.data(), (const uint32_t*)(in.data() + 4 * (size_t)R), R, order.data(), magnitude.data(),
                            main_stem.data());
    if (rc) return 20 + rc;
    FILE* fo = fopen(argv[4], "wb");
    if (!fo) return 4;
    fwrite(order.data(), 4, order.size(), fo);
    fwrite(magnitude.data(), 4, magnitude.size(), fo);
    fwrite(main_stem.data(), 1, main_stem.size(), fo);
    fclose(fo);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 10 && std::string(argv[1]) == "run") return run(argv);
    if (argc == 5 && std::string(argv[1]) == "order") return order_only(argv);
    return 2;
}
