// The device code of csrc/regions.hip compiled for the host (tests/test_regions_host.py): HIP's qualifiers are defined away and a
// "launch" is a loop over the tiles, the cells, the edges or the rings.  REGIONS_DEVICE_INC is the part of the file before its
// extern "C" entry points, the buffers' layouts included.  A tile's iteration runs in place, one slot after the other, to the same
// fixed point the block reaches; the sweeps, the union's three passes and the doubling rounds are issued as the entry points issue
// them.  The workspace is one buffer of ghm_regions_workspace's size laid out by rg_work, as on the device, so every scan -- the
// count's over the cells, the trace's over the edges and the rings -- shares the one sums area and what lies behind it; the trace
// runs twice over that workspace, as a caller may run it, and what the count left there must be untouched by it.  The per-edge
// arrays and the dense outputs have exactly the size the entry points need of them, so that an index past one is an error of its
// own under the sanitizers.
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
#define __syncthreads_or(x) (x)
struct Dim3 {
    unsigned x, y, z;
};
static Dim3 threadIdx, blockIdx;
using std::max;
using std::min;
static inline void hyd_raise(int, int*) {}
static inline int atomicMin(int* p, int v) {
    const int old = *p;
    if (v < old) *p = v;
    return old;
}
static inline unsigned atomicAdd(unsigned* p, unsigned v) {
    const unsigned old = *p;
    *p = old + v;
    return old;
}
#include REGIONS_DEVICE_INC

// fwrite takes no null pointer, which an empty vector's data may be
static void put(const void* data, size_t size, size_t count, FILE* f) {
    if (count) fwrite(data, size, count, f);
}

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

// the three kernels of a scan, in place over io[0 .. n], in the workspace's sums area; returns the total
static int64_t scan(int* io, long n, int64_t* sums) {
    const long nb = rg_blocks(n);
    int sm[256], own[256];
    int64_t sg[16], sv[256], before[256];
    for (long b = 0; b < nb; ++b) {
        for (int t = 0; t < 256; ++t) sm[t] = rg_scan_load(io, n, b, t);
        for (int t = 0; t < 256; ++t) rg_scan_groups(sm, sg, t);
        sums[b] = rg_scan_before(sm, sg, 256);
    }
    for (int t = 0; t < 256; ++t) rg_scan_chunks(sums, nb, sv, t);
    for (int t = 0; t < 256; ++t) rg_scan_spread(sums, nb, sv, t);
    for (long b = 0; b < nb; ++b) {
        for (int t = 0; t < 256; ++t) own[t] = sm[t] = rg_scan_load(io, n, b, t);
        for (int t = 0; t < 256; ++t) rg_scan_groups(sm, sg, t);
        for (int t = 0; t < 256; ++t) before[t] = rg_scan_before(sm, sg, t);
        for (int t = 0; t < 256; ++t) rg_scan_put(n, sums, io, b, t, own[t], before[t]);
    }
    return sums[nb];
}

// what a trace and an extraction give
struct Traced {
    int64_t R = 0, V = 0;
    int rounds = 0;
    std::vector<int> vertex, ring_polygon, seed, label, polygon;
    std::vector<int64_t> ring_offsets;
    std::vector<unsigned char> ring_hole;
    std::vector<unsigned> cells;
};

// ghm_regions_trace and ghm_regions_extract over a counted workspace; 0 or the exit code
static int trace(const RgPlane& p, const RgWork& w, int64_t E, int64_t P, int po, Traced& out) {
    const int H = p.H, W = p.W, n = p.n;
    RgGrid g;
    g.mask = w.mask, g.eoff = w.eoff, g.H = H, g.W = W, g.n = n;
    std::vector<int> pb[2], mb[2], qb[2], cb[2], pred((size_t)E, -1), corner((size_t)E, -1), cell((size_t)E, -1), ridx((size_t)E + 1, -1);
    for (int i = 0; i < 2; ++i) pb[i].assign((size_t)E, -1), mb[i].assign((size_t)E, -1), qb[i].assign((size_t)E, -1), cb[i].assign((size_t)E, -1);
    for (int i = 0; i < n; ++i) rg_link_cell(g, i, pb[0].data(), mb[0].data(), pred.data(), corner.data(), cell.data());
    for (int64_t e = 0; e < E; ++e)
        if (pb[0][(size_t)e] < 0 || pb[0][(size_t)e] >= E || pred[(size_t)e] < 0 || pred[(size_t)e] >= E) return 11;
    int launched = 0, needed = E > 0 ? 0 : 1;
    while (!needed) {
        if (launched > GHM_REGIONS_MAX_ROUNDS) return 12;
        const int a = launched & 1;
        int changed = 0;
        for (long e = 0; e < E; ++e) changed |= rg_min_item((int)e, pb[a].data(), mb[a].data(), pb[a ^ 1].data(), mb[a ^ 1].data());
        ++launched;
        if (!changed) needed = launched;
    }
    // rounds past the fixed point, as a group issues them, leave the same minima in the other pair
    for (int extra = 0; extra < 3 && E > 0; ++extra, ++launched) {
        const int a = launched & 1;
        for (long e = 0; e < E; ++e)
            if (rg_min_item((int)e, pb[a].data(), mb[a].data(), pb[a ^ 1].data(), mb[a ^ 1].data())) return 13;
    }
    const std::vector<int>& m = mb[launched & 1];
    for (long e = 0; e < E; ++e) rg_cut_item((int)e, m.data(), pred.data(), corner.data(), qb[0].data(), cb[0].data(), ridx.data());
    launched = 0, needed = E > 0 ? 0 : 1;
    while (!needed) {
        if (launched > GHM_REGIONS_MAX_ROUNDS) return 14;
        const int a = launched & 1;
        int changed = 0;
        for (long e = 0; e < E; ++e) changed |= rg_rank_item((int)e, qb[a].data(), cb[a].data(), qb[a ^ 1].data(), cb[a ^ 1].data());
        ++launched;
        if (!changed) needed = launched;
    }
    for (int extra = 0; extra < 3 && E > 0; ++extra, ++launched) {
        const int a = launched & 1;
        for (long e = 0; e < E; ++e)
            if (rg_rank_item((int)e, qb[a].data(), cb[a].data(), qb[a ^ 1].data(), cb[a ^ 1].data())) return 15;
    }
    const int at = launched & 1;
    int64_t R = 0, V = 0;
    std::vector<int> rlen(1, 0);
    if (E > 0) {
        R = scan(ridx.data(), (long)E, w.sums);
        if (R != ridx[(size_t)E]) return 16;
        rlen.assign((size_t)R + 1, 0);
        for (long e = 0; e < E; ++e) rg_ring_item((int)e, m.data(), pred.data(), cb[at].data(), corner.data(), ridx.data(), (long)R, rlen.data());
        V = scan(rlen.data(), (long)R, w.sums);
        if (V != rlen[(size_t)R] || V < 4 * R || V > E) return 17;
    }

    // the extraction
    out.R = R, out.V = V, out.rounds = needed - 1;
    out.vertex.assign((size_t)V, -1), out.ring_polygon.assign((size_t)R, -7), out.seed.assign((size_t)P, -7), out.label.assign((size_t)P, -7);
    out.ring_offsets.assign((size_t)R + 1, -7), out.ring_hole.assign((size_t)R, 0xAB), out.cells.assign((size_t)P, 0xABABABABu);
    out.polygon.assign((size_t)H * po, (int)0xABABABAB);
    RgOut o;
    o.vertex = out.vertex.data(), o.ring_offsets = out.ring_offsets.data(), o.ring_polygon = out.ring_polygon.data();
    o.ring_hole = out.ring_hole.data(), o.seed = out.seed.data(), o.label = out.label.data(), o.cells = out.cells.data();
    o.polygon = out.polygon.data(), o.pp = po;
    for (long e = 0; e < E; ++e)
        rg_vertex_item(p, (int)e, m.data(), cb[at].data(), corner.data(), cell.data(), ridx.data(), rlen.data(), w.pidx, (long)R, o);
    for (long i = 0; i <= R; ++i) out.ring_offsets[(size_t)i] = rlen[(size_t)i];
    for (int i = 0; i < n; ++i) rg_polygon_cell(p, i, w.pidx, w.pcells, (long)P, o);
    for (int64_t i = 0; i < V; ++i)
        if (out.vertex[(size_t)i] < 0 || out.vertex[(size_t)i] >= (H + 1) * (W + 1)) {
            fprintf(stderr, "vertex %lld of %lld was not written or lies outside the grid: %d\n", (long long)i, (long long)V, out.vertex[(size_t)i]);
            return 18;
        }
    return 0;
}

// one launch of the tile kernel: every tile to its own fixed point; returns whether a cell changed
template <bool INIT, bool HALO>
static bool tiles(const RgPlane& p) {
    bool changed = false;
    std::vector<int> sl(RG_S * RG_S), sv(RG_S * RG_S), first(RG_S * RG_S);
    for (int y0 = 0; y0 < p.H; y0 += RG_T)
        for (int x0 = 0; x0 < p.W; x0 += RG_T) {
            for (int slot = 0; slot < RG_S * RG_S; ++slot) rg_tile_load<INIT, HALO>(p, y0, x0, slot, sl.data(), sv.data());
            first = sv;
            for (int it = 0; it < RG_T * RG_T; ++it) {
                bool moved = false;
                for (int ty = 0; ty < RG_T; ++ty)
                    for (int tx = 0; tx < RG_T; ++tx) {
                        const int slot = (ty + 1) * RG_S + tx + 1, v = rg_tile_min(sl.data(), sv.data(), slot);
                        moved |= v != sv[slot];
                        sv[slot] = v;
                    }
                if (!moved) break;
            }
            for (int ty = 0; ty < RG_T; ++ty)
                for (int tx = 0; tx < RG_T; ++tx) {
                    const int slot = (ty + 1) * RG_S + tx + 1, y = y0 + ty, x = x0 + tx;
                    if (y >= p.H || x >= p.W) continue;
                    if (INIT || sv[slot] != first[slot]) p.comp[(long)y * p.pc + x] = sv[slot];
                    changed |= sv[slot] != first[slot];
                }
        }
    return changed;
}

// run H W in_pitch out_pitch form in out
//   in:  labels int32 [H, in_pitch]
//   out: int64 edges, polygons, rings, vertices, rounds, sweeps, 0, 0; component then polygon, int32 [H, out_pitch] each, cells
//        beyond W keep the bytes 0xAB; vertex int32 [V]; ring_offsets int64 [R + 1]; ring_polygon int32 [R]; ring_hole uint8 [R];
//        seed, label int32 [P]; cells uint32 [P]
static int run(char** argv) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), pi = atoi(argv[4]), po = atoi(argv[5]), form = atoi(argv[6]);
    if (H < 1 || W < 1 || pi < W || po < W || (form != 0 && form != 1)) return 2;
    std::vector<char> in;
    if (!read_all(argv[7], in) || in.size() != (size_t)H * pi * 4) return 3;
    const int n = H * W;
    std::vector<int> comp((size_t)H * po, (int)0xABABABAB);
    RgPlane p;
    p.lab = (const int*)in.data(), p.comp = comp.data();
    p.H = H, p.W = W, p.pl = pi, p.pc = po, p.n = n;

    // the labelling
    int64_t sweeps = 1;
    if (form == GHM_REGIONS_UNION) {
        tiles<true, false>(p);
        for (int i = 0; i < n; ++i) rg_border_cell(p, i);
        for (int i = 0; i < n; ++i) rg_flatten_cell(p, i);
    } else {
        bool changed = tiles<true, true>(p);
        while (changed) {
            if (sweeps > GHM_REGIONS_MAX_SWEEPS) return 5;
            for (int i = 0; i < n; ++i) rg_jump_cell(p, i);
            changed = tiles<false, true>(p);
            ++sweeps;
        }
    }

    // the count, in a workspace of the entry points' size and layout
    std::vector<char> ws(rg_work_bytes(n), (char)0xAB);
    const RgWork w = rg_work(ws.data(), n);
    for (int i = 0; i < n; ++i) {
        int err = 0;
        rg_flag_cell(p, i, w.mask, w.eoff, w.pidx, err);
        if (err) return 6;
    }
    const int64_t E = scan(w.eoff, n, w.sums), P = scan(w.pidx, n, w.sums);
    if (E != w.eoff[n] || P != w.pidx[n]) return 10;
    memset(w.pcells, 0, 4 * (size_t)(P + 1));
    for (int i = 0; i < n; ++i) rg_cells_cell(p, i, w.pidx, w.pcells);

    // the trace and the extraction, twice over the one workspace: the second must find what the count left and give the same
    const std::vector<char> counted(ws.begin() + RG_HEAD_BYTES + rg_sums_bytes(n), ws.end());
    Traced first, got;
    if (int rc = trace(p, w, E, P, po, first)) return rc;
    if (memcmp(counted.data(), ws.data() + RG_HEAD_BYTES + rg_sums_bytes(n), counted.size()) != 0) return 19;
    if (int rc = trace(p, w, E, P, po, got)) return 20 + rc;
    if (got.R != first.R || got.V != first.V || got.rounds != first.rounds || got.vertex != first.vertex || got.ring_offsets != first.ring_offsets ||
        got.ring_polygon != first.ring_polygon || got.ring_hole != first.ring_hole || got.seed != first.seed || got.label != first.label ||
        got.cells != first.cells || got.polygon != first.polygon)
        return 40;

    FILE* fo = fopen(argv[8], "wb");
    if (!fo) return 4;
    const int64_t head[8] = {E, P, got.R, got.V, got.rounds, sweeps, 0, 0};
    fwrite(head, 8, 8, fo);
    put(comp.data(), 4, comp.size(), fo);
    put(got.polygon.data(), 4, got.polygon.size(), fo);
    put(got.vertex.data(), 4, got.vertex.size(), fo);
    put(got.ring_offsets.data(), 8, got.ring_offsets.size(), fo);
    put(got.ring_polygon.data(), 4, got.ring_polygon.size(), fo);
    put(got.ring_hole.data(), 1, got.ring_hole.size(), fo);
    put(got.seed.data(), 4, got.seed.size(), fo);
    put(got.label.data(), 4, got.label.size(), fo);
    put(got.cells.data(), 4, got.cells.size(), fo);
    fclose(fo);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 9 && std::string(argv[1]) == "run") return run(argv);
    return 2;
}
