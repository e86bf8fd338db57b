// Regions of a label plane (gan_heightmaps_amd/regions.py): lakes, basins and territories as polygons with holes --
// the connected components of equal non-negative labels, their boundary rings in order, which ring is the outer one and which are
// holes, and the cells of each.  Integers throughout, so there are no tolerances; include/ghm.h, section "regions", has the
// definition and tests/regions_ref.py restates it cell by cell.
//
// 1. Label: component[cell] = the least flat index of the cell's 4-connected component, -1 where the label is negative.  Two
//    forms, the same bits, because that fixed point is unique.  sweep: tiles of 32 x 32 cells are taken to their own fixed point
//    of min over equal-label 4-neighbours in LDS, the halo read from the plane as it stands; between sweeps a jump
//    component[i] = component[component[i]]; sweeps are issued in groups (hyd_relax) until one group changes nothing.  union: the
//    tiles resolve themselves in LDS without a halo, a border pass hooks the larger root under the smaller with atomicMin, a
//    flatten pass jumps every cell to its root.  In both forms parent[i] <= i, so every chase ends after fewer than H W steps; no
//    kernel waits for another block.
// 2. Count: a thread per cell computes the cell's boundary sides (a 4-bit mask, kept) and checks the component plane; two
//    exclusive scans number the edges by their key (row, col, side) and the seeds, the polygons; cells[p] by integer atomicAdd.
// 3. Trace: every edge's successor and predecessor from the neighbouring masks and scan offsets -- nothing is searched for;
//    pointer doubling with min gives every edge its ring's least edge; the ring is cut in front of it and pointer doubling over
//    the predecessors ranks the edges, carrying the corner edges so far (the hops themselves nobody reads); every round reads one buffer set and writes the
//    other.  A scan of the ring flags numbers the rings, a scan of their corner counts gives the offsets.  No atomics.
// 4. Extract: every corner edge writes its start corner to vertex[offset[ring] + corners before it]; every ring's least edge
//    writes the ring's polygon and whether it is a hole; every cell its polygon, every seed its polygon's seed, label and cells.
// The scan is a copy of the contour's, the peaks' and the rivers', which are private to their files.
#include "common.h"
#include "relax.h"

namespace {

constexpr int RG_MAX_ROUNDS = GHM_REGIONS_MAX_ROUNDS;
constexpr int RG_GROUP = 4;                       // doubling rounds, or sweeps, per read of the changed words
constexpr int RG_T = 32, RG_S = RG_T + 2;         // a tile and its halo
constexpr int64_t RG_MAX_SWEEPS = GHM_REGIONS_MAX_SWEEPS;
constexpr int64_t RG_MAGIC = 0x736e6f6967657267;  // the header of a counted workspace

struct RgPlane {
    const int* lab;
    int* comp;
    int H, W, pl, pc, n;
};

// ---- the labelling ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rg_label_at(const RgPlane& p, int y, int x) {
    if (y < 0 || y >= p.H || x < 0 || x >= p.W) return -1;
    const int l = p.lab[(long)y * p.pl + x];
    return l < 0 ? -1 : l;
}
__device__ __forceinline__ long rg_comp_at(const RgPlane& p, int idx) {
    const int r = idx / p.W;
    return (long)r * p.pc + (idx - r * p.W);
}
// slot of the tile at (y0, x0) with its halo: the label (-1: none) and the value -- the cell's own index (init) or the plane's
template <bool INIT, bool HALO>
__device__ __forceinline__ void rg_tile_load(const RgPlane& p, int y0, int x0, int slot, int* sl, int* sv) {
    const int ly = slot / RG_S, lx = slot - ly * RG_S, y = y0 + ly - 1, x = x0 + lx - 1;
    const bool inner = ly >= 1 && ly <= RG_T && lx >= 1 && lx <= RG_T;
    const int l = (inner || HALO) ? rg_label_at(p, y, x) : -1;
    sl[slot] = l;
    sv[slot] = l < 0 ? -1 : INIT ? y * p.W + x : p.comp[(long)y * p.pc + x];
}
// the least value of an inner slot and its equal-label 4-neighbours
__device__ __forceinline__ int rg_tile_min(const int* sl, const int* sv, int slot) {
    const int l = sl[slot];
    int v = sv[slot];
    if (l < 0) return v;
    if (sl[slot - RG_S] == l) v = min(v, sv[slot - RG_S]);
    if (sl[slot - 1] == l) v = min(v, sv[slot - 1]);
    if (sl[slot + 1] == l) v = min(v, sv[slot + 1]);
    if (sl[slot + RG_S] == l) v = min(v, sv[slot + RG_S]);
    return v;
}
// words[0]: a tile changed a cell; words[1]: the plane holds a region at all (init only).  A block of 1024 threads, one per cell;
// at most RG_T RG_T iterations: a value travels a cell per iteration and the tile has that many
template <bool INIT, bool HALO>
__global__ __launch_bounds__(1024) void rg_tile_kernel(const RgPlane p, int* words) {
    __shared__ int sl[RG_S * RG_S], sv[RG_S * RG_S];
    const int tid = threadIdx.x, y0 = blockIdx.y * RG_T, x0 = blockIdx.x * RG_T;
    for (int slot = tid; slot < RG_S * RG_S; slot += 1024) rg_tile_load<INIT, HALO>(p, y0, x0, slot, sl, sv);
    __syncthreads();
    const int ty = tid / RG_T, tx = tid - ty * RG_T, slot = (ty + 1) * RG_S + tx + 1;
    const int first = sv[slot];
    for (int it = 0; it < RG_T * RG_T; ++it) {
        const int v = rg_tile_min(sl, sv, slot);
        __syncthreads();
        const int moved = v != sv[slot];
        sv[slot] = v;
        if (!__syncthreads_or(moved)) break;
    }
    const int y = y0 + ty, x = x0 + tx, v = sv[slot];
    const bool in = y < p.H && x < p.W;
    if (in && (INIT || v != first)) p.comp[(long)y * p.pc + x] = v;
    hyd_raise(in && v != first, words);
    if (INIT) hyd_raise(in && sl[slot] >= 0, words + 1);
}
// between sweeps: component[i] = component[component[i]]; a racing read sees an older or a newer value of the same chain
__device__ __forceinline__ void rg_jump_cell(const RgPlane& p, int idx) {
    const long at = rg_comp_at(p, idx);
    const int v = p.comp[at];
    if (v < 0 || v >= idx) return;
    const int vv = p.comp[rg_comp_at(p, v)];
    if (vv >= 0 && vv < v) p.comp[at] = vv;
}
__global__ __launch_bounds__(256) void rg_jump_kernel(const RgPlane p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < p.n) rg_jump_cell(p, (int)idx);
}
// the root of cell i: parent[i] <= i, so fewer than n steps
__device__ __forceinline__ int rg_find(const RgPlane& p, int i) {
    for (int guard = 0; guard < p.n; ++guard) {
        const int v = __atomic_load_n(p.comp + rg_comp_at(p, i), __ATOMIC_RELAXED);
        if (v < 0 || v >= i) break;
        i = v;
    }
    return i;
}
// hooks the larger root under the smaller; a hook that finds its root taken goes on from what took it: a + b falls every turn
__device__ __forceinline__ void rg_unite(const RgPlane& p, int a, int b) {
    for (long guard = 0; guard < 2L * p.n; ++guard) {
        a = rg_find(p, a), b = rg_find(p, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(p.comp + rg_comp_at(p, a), b);
        if (old == a) return;
        a = old;
    }
}
// a cell on a tile's upper or left border and its equal-label neighbour across it
__device__ __forceinline__ void rg_border_cell(const RgPlane& p, int idx) {
    const int y = idx / p.W, x = idx - y * p.W, l = rg_label_at(p, y, x);
    if (l < 0) return;
    if (x % RG_T == 0 && rg_label_at(p, y, x - 1) == l) rg_unite(p, idx, idx - 1);
    if (y % RG_T == 0 && rg_label_at(p, y - 1, x) == l) rg_unite(p, idx, idx - p.W);
}
__global__ __launch_bounds__(256) void rg_border_kernel(const RgPlane p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < p.n) rg_border_cell(p, (int)idx);
}
__device__ __forceinline__ void rg_flatten_cell(const RgPlane& p, int idx) {
    const long at = rg_comp_at(p, idx);
    if (p.comp[at] < 0) return;
    const int root = rg_find(p, idx);
    if (root != idx) p.comp[at] = root;
}
__global__ __launch_bounds__(256) void rg_flatten_kernel(const RgPlane p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < p.n) rg_flatten_cell(p, (int)idx);
}

// ---- the count --------------------------------------------------------------------------------------------------------------------
// the flat step across side N, E, S, W
__device__ __forceinline__ int rg_step(int W, int s) { return s == 0 ? -W : s == 1 ? 1 : s == 2 ? W : -1; }
// the cell's boundary sides, bit s for side s
__device__ __forceinline__ int rg_sides(const RgPlane& p, int y, int x) {
    const int l = rg_label_at(p, y, x);
    if (l < 0) return 0;
    return (rg_label_at(p, y - 1, x) != l ? 1 : 0) | (rg_label_at(p, y, x + 1) != l ? 2 : 0) | (rg_label_at(p, y + 1, x) != l ? 4 : 0) |
           (rg_label_at(p, y, x - 1) != l ? 8 : 0);
}
// err: the component plane is not the labelling's -- a region's cell whose component lies outside [0, idx] or has another label,
// a cell without a region whose component is not -1
__device__ __forceinline__ void rg_flag_cell(const RgPlane& p, int idx, unsigned char* mask, int* eflag, int* sflag, int& err) {
    const int y = idx / p.W, x = idx - y * p.W, l = rg_label_at(p, y, x), v = p.comp[(long)y * p.pc + x];
    const int m = rg_sides(p, y, x);
    err = l < 0 ? v != -1 : (v < 0 || v > idx || rg_label_at(p, v / p.W, v % p.W) != l);
    mask[idx] = (unsigned char)m;
    eflag[idx] = __builtin_popcount(m);
    sflag[idx] = (l >= 0 && v == idx) ? 1 : 0;
}
__global__ __launch_bounds__(256) void rg_flag_kernel(const RgPlane p, unsigned char* mask, int* eflag, int* sflag, int* word) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    int err = 0;
    if (idx < p.n) rg_flag_cell(p, (int)idx, mask, eflag, sflag, err);
    hyd_raise(err, word);
}
// pidx: the scan of the seed flags; every cell of a region adds one to its polygon
__device__ __forceinline__ void rg_cells_cell(const RgPlane& p, int idx, const int* pidx, unsigned* pcells) {
    const int v = p.comp[rg_comp_at(p, idx)];
    if (v >= 0) atomicAdd(pcells + pidx[v], 1u);
}
__global__ __launch_bounds__(256) void rg_cells_kernel(const RgPlane p, const int* pidx, unsigned* pcells) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < p.n) rg_cells_cell(p, (int)idx, pidx, pcells);
}

// ---- an exclusive scan of n int32 values in place: the blocks' sums, their scan by one block, the write (the contour's) --------
__device__ __forceinline__ int rg_scan_load(const int* in, long n, long block, int tid) {
    const long i = block * 256 + tid;
    return i < n ? in[i] : 0;
}
__device__ __forceinline__ void rg_scan_groups(const int* sm, int64_t* sg, int tid) {
    if (tid >= 16) return;
    int64_t a = 0;
    for (int i = 0; i < 16; ++i) a += sm[16 * tid + i];
    sg[tid] = a;
}
// the sum of the values of the threads before tid (tid = 256: of the block)
__device__ __forceinline__ int64_t rg_scan_before(const int* sm, const int64_t* sg, int tid) {
    int64_t a = 0;
    for (int g = 0; g < (tid >> 4); ++g) a += sg[g];
    for (int i = tid & ~15; i < tid; ++i) a += sm[i];
    return a;
}
__global__ __launch_bounds__(256) void rg_scan_sums_kernel(const int* in, long n, int64_t* sums) {
    __shared__ int sm[256];
    __shared__ int64_t sg[16];
    sm[threadIdx.x] = rg_scan_load(in, n, blockIdx.x, threadIdx.x);
    __syncthreads();
    rg_scan_groups(sm, sg, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = rg_scan_before(sm, sg, 256);
}
__device__ __forceinline__ void rg_scan_chunks(const int64_t* sums, long nb, int64_t* sv, int tid) {
    const long chunk = (nb + 255) / 256, lo = min(tid * chunk, nb), hi = min(lo + chunk, nb);
    int64_t a = 0;
    for (long i = lo; i < hi; ++i) a += sums[i];
    sv[tid] = a;
}
__device__ __forceinline__ void rg_scan_spread(int64_t* sums, long nb, const int64_t* sv, int tid) {
    const long chunk = (nb + 255) / 256, lo = min(tid * chunk, nb), hi = min(lo + chunk, nb);
    int64_t a = 0;
    for (int i = 0; i < tid; ++i) a += sv[i];
    for (long i = lo; i < hi; ++i) {
        const int64_t v = sums[i];
        sums[i] = a;
        a += v;
    }
    if (tid == 255) sums[nb] = a;                // the last thread's running sum has passed every block
}
__global__ __launch_bounds__(256) void rg_scan_blocks_kernel(int64_t* sums, long nb) {
    __shared__ int64_t sv[256];
    rg_scan_chunks(sums, nb, sv, threadIdx.x);
    __syncthreads();
    rg_scan_spread(sums, nb, sv, threadIdx.x);
}
// out[i] = the sum of the values before i, out[n] = the total (clamped: the host reads the 64-bit total and refuses 2^31 on)
__device__ __forceinline__ void rg_scan_put(long n, const int64_t* sums, int* out, long block, int tid, int own, int64_t before) {
    const long i = block * 256 + tid;
    if (i >= n) return;
    const int64_t at = sums[block] + before, top = 0x7fffffff;
    out[i] = (int)min(at, top);
    if (i == n - 1) out[n] = (int)min(at + own, top);
}
__global__ __launch_bounds__(256) void rg_scan_write_kernel(int* io, long n, const int64_t* sums) {
    __shared__ int sm[256];
    __shared__ int64_t sg[16];
    const int own = rg_scan_load(io, n, blockIdx.x, threadIdx.x);
    sm[threadIdx.x] = own;
    __syncthreads();
    rg_scan_groups(sm, sg, threadIdx.x);
    __syncthreads();
    rg_scan_put(n, sums, io, blockIdx.x, threadIdx.x, own, rg_scan_before(sm, sg, threadIdx.x));
}

// ---- the trace --------------------------------------------------------------------------------------------------------------------
// the per-edge arrays, E + 1 each: p, m two pairs (successor pointers and ring minima); pred; q, cnt two pairs (the ranking);
// corner: the edge's start corner, ~corner for an edge that is no corner edge; cell: the edge's cell; ridx, rlen: the rings
struct RgTrace {
    int *p[2], *m[2], *pred, *q[2], *cnt[2], *corner, *cell, *ridx, *rlen;
};
struct RgGrid {
    const unsigned char* mask;
    const int* eoff;
    int H, W, n;
};
// the number of side s of a cell, which is a boundary edge
__device__ __forceinline__ int rg_edge(const RgGrid& g, int cell, int s) {
    return g.eoff[cell] + __builtin_popcount(g.mask[cell] & ((1 << s) - 1));
}
// the edge that starts where side s of ``cell`` ends: turn right, else straight on, else turn left
__device__ __forceinline__ int rg_succ(const RgGrid& g, int cell, int s) {
    const int t = (s + 1) & 3;
    if (g.mask[cell] >> t & 1) return rg_edge(g, cell, t);
    const int n1 = cell + rg_step(g.W, t);
    if (g.mask[n1] >> s & 1) return rg_edge(g, n1, s);
    return rg_edge(g, n1 + rg_step(g.W, s), (s + 3) & 3);
}
// its mirror image: the edge that ends where side s starts, and that edge's side
__device__ __forceinline__ int rg_pred(const RgGrid& g, int cell, int s, int& side) {
    const int t = (s + 3) & 3;
    side = t;
    if (g.mask[cell] >> t & 1) return rg_edge(g, cell, t);
    const int n1 = cell + rg_step(g.W, t);
    side = s;
    if (g.mask[n1] >> s & 1) return rg_edge(g, n1, s);
    side = (s + 1) & 3;
    return rg_edge(g, n1 + rg_step(g.W, s), side);
}
__device__ __forceinline__ void rg_link_cell(const RgGrid& g, int idx, int* p, int* m, int* pred, int* corner, int* cell) {
    const int mask = g.mask[idx], y = idx / g.W, x = idx - y * g.W;
    for (int s = 0; s < 4; ++s) {
        if (!(mask >> s & 1)) continue;
        const int e = rg_edge(g, idx, s);
        int side;
        p[e] = rg_succ(g, idx, s);
        m[e] = e;
        pred[e] = rg_pred(g, idx, s, side);
        const int at = (y + (s == 2 || s == 3 ? 1 : 0)) * (g.W + 1) + x + (s == 1 || s == 2 ? 1 : 0);
        corner[e] = side != s ? at : ~at;
        cell[e] = idx;
    }
}
__global__ __launch_bounds__(256) void rg_link_kernel(const RgGrid g, int* p, int* m, int* pred, int* corner, int* cell) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < g.n) rg_link_cell(g, (int)idx, p, m, pred, corner, cell);
}
// a doubling round of the ring minima: m = the least edge among the next 2^k of the ring
__device__ __forceinline__ int rg_min_item(int e, const int* p0, const int* m0, int* p1, int* m1) {
    const int p = p0[e], v = min(m0[e], m0[p]);
    p1[e] = p0[p];
    m1[e] = v;
    return v != m0[e];
}
__global__ __launch_bounds__(256) void rg_min_kernel(long E, const int* p0, const int* m0, int* p1, int* m1, int* word) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    hyd_raise(e < E ? rg_min_item((int)e, p0, m0, p1, m1) : 0, word);
}
// the ring is cut in front of its least edge, which is the ranking's terminal; rflag: 1 at a ring's least edge
__device__ __forceinline__ void rg_cut_item(int e, const int* m, const int* pred, const int* corner, int* q, int* cnt, int* rflag) {
    const bool least = m[e] == e;
    q[e] = least ? e : pred[e];
    cnt[e] = !least && corner[e] >= 0 ? 1 : 0;
    rflag[e] = least ? 1 : 0;
}
__global__ __launch_bounds__(256) void rg_cut_kernel(long E, const int* m, const int* pred, const int* corner, int* q, int* cnt,
                                                     int* rflag) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < E) rg_cut_item((int)e, m, pred, corner, q, cnt, rflag);
}
// a doubling round of the ranking: q = the edge 2^k back or the terminal, cnt = the corner edges on the way to it
__device__ __forceinline__ int rg_rank_item(int e, const int* q0, const int* c0, int* q1, int* c1) {
    const int q = q0[e], qq = q0[q];
    q1[e] = qq;
    c1[e] = c0[e] + c0[q];
    return qq != q;
}
__global__ __launch_bounds__(256) void rg_rank_kernel(long E, const int* q0, const int* c0, int* q1, int* c1, int* word) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    hyd_raise(e < E ? rg_rank_item((int)e, q0, c0, q1, c1) : 0, word);
}
// a ring's least edge stores the ring's vertices: the corner edges up to its predecessor, the ring's last edge, and itself if it
// is one (an outer ring's least edge is, a hole's -- a side S of the cell above the hole -- need not be)
__device__ __forceinline__ void rg_ring_item(int e, const int* m, const int* pred, const int* cnt, const int* corner, const int* ridx, long R,
                                             int* rlen) {
    if (m[e] != e) return;
    const int ring = ridx[e];
    if (ring < R) rlen[ring] = cnt[pred[e]] + (corner[e] >= 0 ? 1 : 0);
}
__global__ __launch_bounds__(256) void rg_ring_kernel(long E, const int* m, const int* pred, const int* cnt, const int* corner,
                                                      const int* ridx, long R, int* rlen) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < E) rg_ring_item((int)e, m, pred, cnt, corner, ridx, R, rlen);
}

// ---- the extraction ---------------------------------------------------------------------------------------------------------------
struct RgOut {
    int* vertex;
    int64_t* ring_offsets;
    int* ring_polygon;
    unsigned char* ring_hole;
    int *seed, *label;
    unsigned* cells;
    int* polygon;
    int pp;
};
// roff: the scan of the rings' vertices, R + 1; no vertex is written outside its ring's own range
__device__ __forceinline__ void rg_vertex_item(const RgPlane& p, int e, const int* m, const int* cnt, const int* corner, const int* cell,
                                               const int* ridx, const int* roff, const int* pidx, long R, const RgOut& o) {
    const int least = m[e], ring = ridx[least];
    if (ring >= R) return;
    if (corner[e] >= 0) {
        // cnt counts the corner edges after the least edge up to e, e included; the least edge comes first if it is one
        const long at = least == e ? roff[ring] : (long)roff[ring] + cnt[e] - 1 + (corner[least] >= 0 ? 1 : 0);
        if (at >= roff[ring] && at < roff[ring + 1]) o.vertex[at] = corner[e];
    }
    if (least != e) return;
    const int c = cell[e], v = c >= 0 && c < p.n ? p.comp[rg_comp_at(p, c)] : -1;
    o.ring_polygon[ring] = v >= 0 && v < p.n ? pidx[v] : -1;
    // side N starts at the cell's own corner: the outer ring's least edge is side N of the seed
    o.ring_hole[ring] = (v == c && corner[e] == c / p.W * (p.W + 1) + c % p.W) ? 0 : 1;
}
__global__ __launch_bounds__(256) void rg_vertex_kernel(const RgPlane p, long E, const int* m, const int* cnt, const int* corner,
                                                        const int* cell, const int* ridx, const int* roff, const int* pidx, long R,
                                                        const RgOut o) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < E) rg_vertex_item(p, (int)e, m, cnt, corner, cell, ridx, roff, pidx, R, o);
}
__global__ __launch_bounds__(256) void rg_offsets_kernel(long R, const int* roff, int64_t* ring_offsets) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i <= R) ring_offsets[i] = roff[i];
}
__device__ __forceinline__ void rg_polygon_cell(const RgPlane& p, int idx, const int* pidx, const unsigned* pcells, long P, const RgOut& o) {
    const int y = idx / p.W, x = idx - y * p.W, v = p.comp[(long)y * p.pc + x];
    const int poly = v >= 0 && v < p.n ? pidx[v] : -1;
    if (o.polygon) o.polygon[(long)y * o.pp + x] = poly;
    if (v != idx || poly < 0 || poly >= P) return;
    o.seed[poly] = idx;
    o.label[poly] = p.lab[(long)y * p.pl + x];
    o.cells[poly] = pcells[poly];
}
__global__ __launch_bounds__(256) void rg_polygon_kernel(const RgPlane p, const int* pidx, const unsigned* pcells, long P, const RgOut o) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < p.n) rg_polygon_cell(p, (int)idx, pidx, pcells, P, o);
}

// ---- the layouts, on the host; tests/regions_host/harness.cpp lays its buffers out with them too ------------------------------------
inline long rg_blocks(long n) { return (n + 255) / 256; }
inline size_t rg_round(size_t bytes) { return (bytes + 255) / 256 * 256; }

// the workspace: a header (the words at byte 128), the blocks' sums -- for the largest scan, the trace's over the edges, of which a
// cell has four at most --, the masks (n bytes), eoff, pidx and pcells (n + 1 each)
struct RgHeader {
    int64_t magic, H, W, E, P, R, V, at;
};
struct RgWork {
    RgHeader* head;
    int* words;
    int64_t* sums;
    unsigned char* mask;
    int *eoff, *pidx;
    unsigned* pcells;
};
constexpr size_t RG_HEAD_BYTES = 512;
inline size_t rg_sums_bytes(long n) { return rg_round(8 * (size_t)(rg_blocks(4 * n) + 1)); }
inline RgWork rg_work(void* ws, long n) {
    RgWork w;
    char* at = (char*)ws;
    w.head = (RgHeader*)at;
    w.words = (int*)(at + 128);                  // RG_MAX_ROUNDS + 1 of them
    at += RG_HEAD_BYTES;
    w.sums = (int64_t*)at;
    at += rg_sums_bytes(n);
    w.mask = (unsigned char*)at;
    at += rg_round((size_t)n);
    const size_t one = rg_round(4 * (size_t)(n + 1));
    w.eoff = (int*)at, w.pidx = (int*)(at + one), w.pcells = (unsigned*)(at + 2 * one);
    return w;
}
inline size_t rg_work_bytes(long n) { return RG_HEAD_BYTES + rg_sums_bytes(n) + rg_round((size_t)n) + 3 * rg_round(4 * (size_t)(n + 1)); }
constexpr int RG_TRACE_ARRAYS = 13;
inline RgTrace rg_trace(void* buf, long E) {
    RgTrace t;
    char* at = (char*)buf;
    const size_t one = rg_round(4 * (size_t)(E + 1));
    int** all[RG_TRACE_ARRAYS] = {&t.p[0], &t.p[1], &t.m[0], &t.m[1], &t.pred, &t.q[0], &t.q[1], &t.cnt[0],
                                  &t.cnt[1], &t.corner, &t.cell, &t.ridx, &t.rlen};
    for (int i = 0; i < RG_TRACE_ARRAYS; ++i) *all[i] = (int*)(at + i * one);
    return t;
}
inline size_t rg_trace_size(long E) { return RG_TRACE_ARRAYS * rg_round(4 * (size_t)(E + 1)); }

#define RG_FLAT(total) dim3((unsigned)(((long)(total) + 255) / 256)), dim3(256), 0, ctx->stream

}  // namespace

extern "C" {

// ---- the host side: checks, launches -------------------------------------------------------------------------------------------
static void rg_scan(ghm_ctx* ctx, int* io, long n, int64_t* sums) {
    const long nb = rg_blocks(n);
    hipLaunchKernelGGL(rg_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, io, n, sums);
    hipLaunchKernelGGL(rg_scan_blocks_kernel, dim3(1), dim3(256), 0, ctx->stream, sums, nb);
    hipLaunchKernelGGL(rg_scan_write_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, io, n, sums);
}

static int rg_read(ghm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    GHM_LAUNCH_CHECK();
    GHM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

static int rg_check_planes(const char* who, int32_t H, int32_t W, int32_t l_pitch, int32_t c_pitch) {
    if (int rc = hyd_check_plane(who, H, W, l_pitch, "labels")) return rc;
    if (int rc = hyd_check_plane(who, H, W, c_pitch, "component")) return rc;
    GHM_CHECK(((int64_t)H + 1) * ((int64_t)W + 1) < ((int64_t)1 << 31), "%s: a plane of %d x %d has 2^31 grid corners or more", who, H, W);
    return 0;
}

static RgPlane rg_plane(const int32_t* labels, int32_t l_pitch, const int32_t* component, int32_t c_pitch, int32_t H, int32_t W) {
    RgPlane p;
    p.lab = labels, p.comp = const_cast<int*>(component);
    p.H = H, p.W = W, p.pl = l_pitch, p.pc = c_pitch, p.n = H * W;
    return p;
}

int64_t ghm_regions_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31) || ((int64_t)H + 1) * ((int64_t)W + 1) >= ((int64_t)1 << 31) || H > 4 * 65535)
        return -1;
    const long n = (long)H * W;
    return (int64_t)rg_work_bytes(n);
}

int64_t ghm_regions_trace_bytes(int64_t edges) {
    if (edges < 0 || edges >= ((int64_t)1 << 31)) return -1;
    return (int64_t)rg_trace_size((long)edges);
}

int ghm_regions_label(ghm_ctx* ctx, const int32_t* labels, int32_t l_pitch, int32_t H, int32_t W, int32_t form, int32_t* component,
                      int32_t c_pitch, void* workspace, int64_t* sweeps) {
    const char* who = "ghm_regions_label";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(labels && component && workspace && sweeps, "%s: null pointer", who);
    if (int rc = rg_check_planes(who, H, W, l_pitch, c_pitch)) return rc;
    GHM_CHECK(form == GHM_REGIONS_SWEEP || form == GHM_REGIONS_UNION, "%s: form=%d (0 sweep, 1 union)", who, form);
    const RgPlane p = rg_plane(labels, l_pitch, component, c_pitch, H, W);
    const RgWork w = rg_work(workspace, p.n);
    const dim3 tiles((unsigned)((W + RG_T - 1) / RG_T), (unsigned)((H + RG_T - 1) / RG_T));
    GHM_HIP(hipMemsetAsync(w.head, 0, RG_HEAD_BYTES, ctx->stream));         // a labelling forgets an earlier count
    int words[2] = {};
    if (form == GHM_REGIONS_UNION) {
        hipLaunchKernelGGL((rg_tile_kernel<true, false>), tiles, dim3(1024), 0, ctx->stream, p, w.words);
        hipLaunchKernelGGL(rg_border_kernel, RG_FLAT(p.n), p);
        hipLaunchKernelGGL(rg_flatten_kernel, RG_FLAT(p.n), p);
        if (int rc = rg_read(ctx, words, w.words, sizeof(words))) return rc;
        *sweeps = words[1] ? 1 : 0;
        return 0;
    }
    // the first sweep needs no plane: every halo value is the neighbour's own index
    hipLaunchKernelGGL((rg_tile_kernel<true, true>), tiles, dim3(1024), 0, ctx->stream, p, w.words);
    if (int rc = rg_read(ctx, words, w.words, sizeof(words))) return rc;
    *sweeps = words[1] ? 1 : 0;
    if (!words[0]) return 0;
    const int64_t cap = min((int64_t)p.n + 1, RG_MAX_SWEEPS);
    int64_t more = 0;
    auto sweep = [&](int64_t) {
        hipLaunchKernelGGL(rg_jump_kernel, RG_FLAT(p.n), p);
        hipLaunchKernelGGL((rg_tile_kernel<false, true>), tiles, dim3(1024), 0, ctx->stream, p, w.words);
    };
    if (int rc = hyd_relax(ctx, who, w.words, RG_GROUP, cap, sweep, &more, nullptr)) return rc;
    *sweeps = 1 + more;
    return 0;
}

int ghm_regions_count(ghm_ctx* ctx, const int32_t* labels, int32_t l_pitch, const int32_t* component, int32_t c_pitch, int32_t H, int32_t W,
                      int64_t max_edges, void* workspace, int64_t* counts) {
    const char* who = "ghm_regions_count";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(labels && component && workspace && counts, "%s: null pointer", who);
    if (int rc = rg_check_planes(who, H, W, l_pitch, c_pitch)) return rc;
    GHM_CHECK(max_edges >= 0 && max_edges < ((int64_t)1 << 31), "%s: max_edges=%lld (0 <= max_edges < 2^31)", who, (long long)max_edges);
    const RgPlane p = rg_plane(labels, l_pitch, component, c_pitch, H, W);
    const long n = p.n, nb = rg_blocks(n);
    const RgWork w = rg_work(workspace, n);
    GHM_HIP(hipMemsetAsync(w.head, 0, RG_HEAD_BYTES, ctx->stream));
    hipLaunchKernelGGL(rg_flag_kernel, RG_FLAT(n), p, w.mask, w.eoff, w.pidx, w.words);
    int err = 0;
    if (int rc = rg_read(ctx, &err, w.words, sizeof(err))) return rc;
    GHM_CHECK(!err, "%s: the component plane is not ghm_regions_label's of these labels", who);
    RgHeader head = {RG_MAGIC, H, W, 0, 0, -1, -1, -1};
    rg_scan(ctx, w.eoff, n, w.sums);
    if (int rc = rg_read(ctx, &head.E, w.sums + nb, sizeof(int64_t))) return rc;
    GHM_CHECK(head.E <= max_edges, "%s: the plane of %d x %d has %lld boundary edges, more than max_edges = %lld", who, H, W,
              (long long)head.E, (long long)max_edges);
    rg_scan(ctx, w.pidx, n, w.sums);
    if (int rc = rg_read(ctx, &head.P, w.sums + nb, sizeof(int64_t))) return rc;
    GHM_HIP(hipMemsetAsync(w.pcells, 0, 4 * (size_t)(head.P + 1), ctx->stream));
    if (head.P > 0) hipLaunchKernelGGL(rg_cells_kernel, RG_FLAT(n), p, w.pidx, w.pcells);
    GHM_LAUNCH_CHECK();
    GHM_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    counts[0] = head.E, counts[1] = head.P;
    return 0;
}

static int rg_header(ghm_ctx* ctx, const char* who, const RgWork& w, int32_t H, int32_t W, int64_t edges, int64_t polygons, RgHeader& head) {
    if (int rc = rg_read(ctx, &head, w.head, sizeof(head))) return rc;
    const bool ok = head.magic == RG_MAGIC;
    GHM_CHECK(ok && head.H == H && head.W == W && head.E == edges && head.P == polygons,
              "%s: the workspace was counted with %lld edges and %lld polygons on %lld x %lld, the call says %lld and %lld on %d x %d", who,
              (long long)(ok ? head.E : -1), (long long)(ok ? head.P : -1), (long long)(ok ? head.H : -1), (long long)(ok ? head.W : -1),
              (long long)edges, (long long)polygons, H, W);
    return 0;
}

// doubling rounds in groups until one changes nothing; one more than max_rounds may be issued, the one that shows the rest.
// round(i) issues round number i with words + i as its changed word; *needed: the first round that changed nothing, counted from 1
extern "C++" {
template <class Round>
static int rg_double(ghm_ctx* ctx, const char* who, const char* what, int* words, int max_rounds, Round round, int* launched, int* needed) {
    GHM_HIP(hipMemsetAsync(words, 0, 4 * (RG_MAX_ROUNDS + 1), ctx->stream));
    for (*launched = 0, *needed = 0; !*needed;) {
        GHM_CHECK(*launched <= max_rounds, "%s: the %s has not come to rest after %d rounds", who, what, max_rounds);
        const int group = min(RG_GROUP, max_rounds + 1 - *launched);
        for (int i = 0; i < group; ++i, ++*launched) round(*launched);
        int changed[RG_GROUP] = {};
        if (int rc = rg_read(ctx, changed, words + *launched - group, 4 * (size_t)group)) return rc;
        for (int i = 0; i < group && !*needed; ++i)
            if (!changed[i]) *needed = *launched - group + i + 1;
    }
    return 0;
}
}  // extern "C++"

int ghm_regions_trace(ghm_ctx* ctx, int32_t H, int32_t W, int32_t max_rounds, void* workspace, void* trace, int64_t edges, int64_t polygons,
                      int64_t* counts, int32_t* rounds) {
    const char* who = "ghm_regions_trace";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(workspace && trace && counts && rounds, "%s: null pointer", who);
    if (int rc = rg_check_planes(who, H, W, W, W)) return rc;
    GHM_CHECK(max_rounds >= 1 && max_rounds <= RG_MAX_ROUNDS, "%s: max_rounds=%d (1 .. %d)", who, max_rounds, RG_MAX_ROUNDS);
    const long n = (long)H * W;
    const RgWork w = rg_work(workspace, n);
    RgHeader head = {};
    if (int rc = rg_header(ctx, who, w, H, W, edges, polygons, head)) return rc;
    head.R = head.V = head.at = -1;              // what an earlier trace left is forgotten
    GHM_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    const long E = (long)head.E;
    const RgTrace t = rg_trace(trace, E);
    int64_t R = 0, V = 0;
    int at = 0, needed = 1;
    if (E > 0) {
        RgGrid g;
        g.mask = w.mask, g.eoff = w.eoff, g.H = H, g.W = W, g.n = (int)n;
        hipLaunchKernelGGL(rg_link_kernel, RG_FLAT(n), g, t.p[0], t.m[0], t.pred, t.corner, t.cell);
        int launched = 0, rest = 0;
        auto least = [&](int i) {
            hipLaunchKernelGGL(rg_min_kernel, RG_FLAT(E), E, t.p[i & 1], t.m[i & 1], t.p[(i & 1) ^ 1], t.m[(i & 1) ^ 1], w.words + i);
        };
        if (int rc = rg_double(ctx, who, "search for the rings' least edges", w.words, max_rounds, least, &launched, &rest)) return rc;
        const int* m = t.m[launched & 1];
        if (launched & 1) GHM_HIP(hipMemcpyAsync(t.m[0], m, 4 * (size_t)E, hipMemcpyDeviceToDevice, ctx->stream));        // m[0] holds the minima
        hipLaunchKernelGGL(rg_cut_kernel, RG_FLAT(E), E, t.m[0], t.pred, t.corner, t.q[0], t.cnt[0], t.ridx);
        auto rank = [&](int i) {
            const int a = i & 1, b = a ^ 1;
            hipLaunchKernelGGL(rg_rank_kernel, RG_FLAT(E), E, t.q[a], t.cnt[a], t.q[b], t.cnt[b], w.words + i);
        };
        if (int rc = rg_double(ctx, who, "ranking", w.words, max_rounds, rank, &launched, &needed)) return rc;
        at = launched & 1;
        rg_scan(ctx, t.ridx, E, w.sums);
        if (int rc = rg_read(ctx, &R, w.sums + rg_blocks(E), sizeof(int64_t))) return rc;
        GHM_HIP(hipMemsetAsync(t.rlen, 0, 4 * (size_t)(R + 1), ctx->stream));
        hipLaunchKernelGGL(rg_ring_kernel, RG_FLAT(E), E, t.m[0], t.pred, t.cnt[at], t.corner, t.ridx, (long)R, t.rlen);
        rg_scan(ctx, t.rlen, (long)R, w.sums);
        if (int rc = rg_read(ctx, &V, w.sums + rg_blocks((long)R), sizeof(int64_t))) return rc;
        GHM_CHECK(V >= 4 * R && V <= E, "%s: %lld vertices for %lld rings of %lld edges: the workspace is not the count's", who, (long long)V,
                  (long long)R, (long long)E);
    }
    head.R = R, head.V = V, head.at = at;
    GHM_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    counts[0] = R, counts[1] = V;
    *rounds = needed - 1;
    return 0;
}

int ghm_regions_extract(ghm_ctx* ctx, const int32_t* labels, int32_t l_pitch, const int32_t* component, int32_t c_pitch, int32_t H, int32_t W,
                        const void* workspace, const void* trace, int64_t edges, int64_t polygons, int64_t rings, int64_t vertices,
                        int32_t* vertex, int64_t* ring_offsets, int32_t* ring_polygon, uint8_t* ring_hole, int32_t* seed, int32_t* label,
                        uint32_t* cells, int32_t* polygon, int32_t p_pitch) {
    const char* who = "ghm_regions_extract";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(labels && component && workspace && ring_offsets && (edges == 0 || trace) && (vertices == 0 || vertex) &&
                  (rings == 0 || (ring_polygon && ring_hole)) && (polygons == 0 || (seed && label && cells)),
              "%s: null pointer", who);
    if (int rc = rg_check_planes(who, H, W, l_pitch, c_pitch)) return rc;
    if (polygon)
        if (int rc = hyd_check_plane(who, H, W, p_pitch, "polygon")) return rc;
    const long n = (long)H * W;
    const RgWork w = rg_work(const_cast<void*>(workspace), n);
    RgHeader head = {};
    if (int rc = rg_header(ctx, who, w, H, W, edges, polygons, head)) return rc;
    GHM_CHECK(head.R >= 0, "%s: the workspace holds no trace: ghm_regions_trace comes first", who);
    GHM_CHECK(head.R == rings && head.V == vertices, "%s: the workspace was traced with %lld rings and %lld vertices, the call says %lld and %lld",
              who, (long long)head.R, (long long)head.V, (long long)rings, (long long)vertices);
    const RgPlane p = rg_plane(labels, l_pitch, component, c_pitch, H, W);
    RgOut o;
    o.vertex = vertex, o.ring_offsets = ring_offsets, o.ring_polygon = ring_polygon, o.ring_hole = ring_hole;
    o.seed = seed, o.label = label, o.cells = cells, o.polygon = polygon, o.pp = p_pitch;
    const long E = (long)head.E, R = (long)head.R;
    if (E > 0) {
        const RgTrace t = rg_trace(const_cast<void*>(trace), E);
        hipLaunchKernelGGL(rg_vertex_kernel, RG_FLAT(E), p, E, t.m[0], t.cnt[head.at], t.corner, t.cell, t.ridx, t.rlen, w.pidx, R, o);
        hipLaunchKernelGGL(rg_offsets_kernel, RG_FLAT(R + 1), R, t.rlen, ring_offsets);
    } else {
        GHM_HIP(hipMemsetAsync(ring_offsets, 0, sizeof(int64_t), ctx->stream));
    }
    if (polygon || head.P > 0) hipLaunchKernelGGL(rg_polygon_kernel, RG_FLAT(n), p, w.pidx, w.pcells, (long)head.P, o);
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
