// Contours of a heightfield (gan_heightmaps_amd/contour.py): topographic isolines as ordered polylines, traced on the
// device.  Integers throughout but for one IEEE double division per vertex, so there are no tolerances; include/ghm.h, section
// "contour", has the definition and tests/contour_ref.py restates it.
//
// 1. Levels.  With Z = 2 zq (even) and lam_j = 2 (base_q + j interval_q) + 1 (odd), a corner is above level j iff j < A(zq) =
//    ceil((zq - base_q) / interval_q), clipped to the levels that are asked for.  The levels that cross a cell are the contiguous
//    range [min A, max A) of its corners' A, its saddle levels a contiguous sub-range: both follow from four integers per cell.
// 2. Count: a thread per cell writes its segments' number; an exclusive scan over the cells (blocks' sums in int64, one block
//    scans them, the blocks write) turns them into offsets, so a segment's id follows its key (row, col, level, entry edge).
// 3. Link: a thread per segment finds its cell (stored by a thread per cell), its level and entry edge from its id by arithmetic,
//    and the ids of its successor and predecessor from the offset of the cell across the exit or entry edge and that cell's own
//    four integers: nothing is searched for.
// 4. Loops: pointer doubling with min over the successors gives every segment of a loop the loop's least id; on an open line the
//    pointer runs off the end instead.  The loop is cut in front of its least id.
// 5. Rank: pointer doubling over the predecessors gives every segment its line's start and its hops from it (Wyllie).
// 6. Lines: a scan of the start flags numbers the lines in the order of their start ids, a scan of their vertex counts places
//    them; a thread per segment writes its entry vertex, the last segment of an open line its exit vertex too.
// Every doubling round reads one pair of buffers and writes the other (Jacobi); the only shared word is "changed", one per round,
// stored by a block that changed anything and read once per group of CT_GROUP rounds.  A round past the fixed point changes
// nothing, so the rounds of a group that were not needed do no harm.  No atomics, no LDS but the scans' 256 + 16 words.
#include "common.h"
#include "relax.h"

namespace {

constexpr int CT_GROUP = 4;                      // doubling rounds per read of the changed words
constexpr int CT_MAX_ROUNDS = GHM_CONTOUR_MAX_ROUNDS;
constexpr int CT_LEVEL_LIMIT = 1 << 28;          // levels are counted for j in [-2^28, 2^28): a cell's count fits 31 bits
constexpr int64_t CT_MAGIC = 0x72756f746e6f6367; // the header of a traced workspace

// ---- the levels ---------------------------------------------------------------------------------------------------------------
struct CtLv {
    int base_q, iq, jlo, jhi;                    // the levels asked for: j in [jlo, jhi)
};

// the number A such that a corner of height zq is above level j iff j < A, clipped to [jlo, jhi]
__device__ __forceinline__ int ct_above(const CtLv& v, int zq) {
    const int64_t d = (int64_t)zq - v.base_q;
    int64_t q = d / v.iq;
    if (d - q * v.iq > 0) ++q;                   // the division truncates towards zero: the ceiling is one more for a positive rest
    return (int)(q < v.jlo ? v.jlo : q > v.jhi ? v.jhi : q);
}

__device__ __forceinline__ int64_t ct_lambda(const CtLv& v, int j) { return 2 * ((int64_t)v.base_q + (int64_t)j * v.iq) + 1; }

struct CtPlane {
    const int* zq;
    int H, W, pz;
    CtLv lv;
};

// a cell: its corners' heights and A in the clockwise order TL, TR, BR, BL, its levels [lo, hi) and its saddle levels [s0, s1)
struct CtCell {
    int z0, z1, z2, z3;
    int a0, a1, a2, a3;
    int lo, hi, s0, s1;
};

__device__ __forceinline__ CtCell ct_cell(const CtPlane& p, int r, int c) {
    CtCell k;
    const int* z = p.zq + (long)r * p.pz + c;
    k.z0 = z[0], k.z1 = z[1], k.z2 = z[p.pz + 1], k.z3 = z[p.pz];
    k.a0 = ct_above(p.lv, k.z0), k.a1 = ct_above(p.lv, k.z1), k.a2 = ct_above(p.lv, k.z2), k.a3 = ct_above(p.lv, k.z3);
    k.lo = min(min(k.a0, k.a1), min(k.a2, k.a3));
    k.hi = max(max(k.a0, k.a1), max(k.a2, k.a3));
    // TL and BR above, TR and BL below: max(a1, a3) <= j < min(a0, a2); or the other way round; at most one range is not empty
    const int p0 = max(k.a1, k.a3), p1 = min(k.a0, k.a2), q0 = max(k.a0, k.a2), q1 = min(k.a1, k.a3);
    if (p1 > p0)
        k.s0 = p0, k.s1 = p1;
    else if (q1 > q0)
        k.s0 = q0, k.s1 = q1;
    else
        k.s0 = k.s1 = k.hi;
    return k;
}

__device__ __forceinline__ int ct_cell_count(const CtCell& k) { return (k.hi - k.lo) + (k.s1 - k.s0); }

// bit e: corner e (TL, TR, BR, BL) is above level j
__device__ __forceinline__ int ct_code(const CtCell& k, int j) {
    return (j < k.a0 ? 1 : 0) | (j < k.a1 ? 2 : 0) | (j < k.a2 ? 4 : 0) | (j < k.a3 ? 8 : 0);
}
// edge e leads from corner e to corner e + 1: the entry edges go from above to below, the exit edges from below to above
__device__ __forceinline__ int ct_rot(int code) { return ((code >> 1) | (code << 3)) & 15; }
__device__ __forceinline__ int ct_entries(int code) { return code & ~ct_rot(code) & 15; }
__device__ __forceinline__ int ct_exits(int code) { return ~code & ct_rot(code) & 15; }
__device__ __forceinline__ bool ct_centre_above(const CtPlane& p, const CtCell& k, int j) {
    return (int64_t)k.z0 + k.z1 + k.z2 + k.z3 > 2 * ct_lambda(p.lv, j);          // 2 (z0 + z1 + z2 + z3) > 4 lam
}
// the edge the segment of level j that enters through e leaves through
__device__ __forceinline__ int ct_exit_of(const CtPlane& p, const CtCell& k, int j, int e) {
    const int code = ct_code(k, j), en = ct_entries(code);
    if (en & (en - 1)) return (e + (ct_centre_above(p, k, j) ? 1 : 3)) & 3;
    return __builtin_ctz((unsigned)ct_exits(code));
}
// the edge the segment of level j that leaves through x enters through
__device__ __forceinline__ int ct_entry_of(const CtPlane& p, const CtCell& k, int j, int x) {
    const int en = ct_entries(ct_code(k, j));
    if (en & (en - 1)) return (x + (ct_centre_above(p, k, j) ? 3 : 1)) & 3;
    return __builtin_ctz((unsigned)en);
}
// the place among its cell's segments of the one of level j that enters through e: levels in order, a saddle's two by entry edge
__device__ __forceinline__ int ct_local(const CtCell& k, int j, int e) {
    const int before = min(max(j - k.s0, 0), k.s1 - k.s0);
    return (j - k.lo) + before + ((j >= k.s0 && j < k.s1 && e >= 2) ? 1 : 0);
}
// the level and the entry edge of the cell's segment number i
__device__ __forceinline__ void ct_unlocal(const CtCell& k, int i, int& j, int& e) {
    const int n0 = k.s0 - k.lo, n1 = 2 * (k.s1 - k.s0);
    int second = 0;
    if (i < n0) {
        j = k.lo + i;
    } else if (i < n0 + n1) {
        j = k.s0 + ((i - n0) >> 1);
        second = (i - n0) & 1;
    } else {
        j = k.lo + i - (k.s1 - k.s0);
    }
    const unsigned en = (unsigned)ct_entries(ct_code(k, j));
    e = second ? 31 - __builtin_clz(en) : __builtin_ctz(en);
}

// the crossing of level j with edge e of cell (r, c)
struct CtVertex {
    int r, c, axis;
    double t;
};
__device__ __forceinline__ CtVertex ct_vertex(const CtPlane& p, const CtCell& k, int r, int c, int e, int j) {
    CtVertex v;
    v.r = r + (e == 2 ? 1 : 0);
    v.c = c + (e == 1 ? 1 : 0);
    v.axis = e & 1;
    const int z0 = k.z0, z1 = k.z1, z2 = k.z2, z3 = k.z3;          // values, so that the choice below is one of registers
    const int za = (e == 0 || e == 3) ? z0 : e == 1 ? z1 : z3;
    const int zb = e == 0 ? z1 : e == 3 ? z3 : z2;
    v.t = (double)(ct_lambda(p.lv, j) - 2 * (int64_t)za) / (double)(2 * ((int64_t)zb - za));
    return v;
}

// ---- the count ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ct_count_cell(const CtPlane& p, long n, int* cnt) {
    const int W1 = p.W - 1, r = (int)(n / W1), c = (int)(n - (long)r * W1);
    cnt[n] = ct_cell_count(ct_cell(p, r, c));
}
__global__ __launch_bounds__(256) void ct_count_kernel(const CtPlane p, long cells, int* cnt) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n < cells) ct_count_cell(p, n, cnt);
}

// ---- an exclusive scan of n int32 values: the blocks' sums, their scan by one block, the write ---------------------------------
__device__ __forceinline__ int ct_scan_load(const int* in, long n, long block, int tid) {
    const long i = block * 256 + tid;
    return i < n ? in[i] : 0;
}
__device__ __forceinline__ void ct_scan_groups(const int* sm, int64_t* sg, int tid) {
    if (tid >= 16) return;
    int64_t a = 0;
    for (int i = 0; i < 16; ++i) a += sm[16 * tid + i];
    sg[tid] = a;
}
// the sum of the values of the threads before tid (tid = 256: of the block)
__device__ __forceinline__ int64_t ct_scan_before(const int* sm, const int64_t* sg, int tid) {
    int64_t a = 0;
    for (int g = 0; g < (tid >> 4); ++g) a += sg[g];
    for (int i = tid & ~15; i < tid; ++i) a += sm[i];
    return a;
}
__global__ __launch_bounds__(256) void ct_scan_sums_kernel(const int* in, long n, int64_t* sums) {
    __shared__ int sm[256];
    __shared__ int64_t sg[16];
    sm[threadIdx.x] = ct_scan_load(in, n, blockIdx.x, threadIdx.x);
    __syncthreads();
    ct_scan_groups(sm, sg, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = ct_scan_before(sm, sg, 256);
}
// one block: the exclusive scan of the nb sums in place, the total behind them
__device__ __forceinline__ void ct_scan_chunks(const int64_t* sums, long nb, int64_t* sv, int tid) {
    const long chunk = (nb + 255) / 256, lo = min(tid * chunk, nb), hi = min(lo + chunk, nb);
    int64_t a = 0;
    for (long i = lo; i < hi; ++i) a += sums[i];
    sv[tid] = a;
}
__device__ __forceinline__ void ct_scan_spread(int64_t* sums, long nb, const int64_t* sv, int tid) {
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
__global__ __launch_bounds__(256) void ct_scan_blocks_kernel(int64_t* sums, long nb) {
    __shared__ int64_t sv[256];
    ct_scan_chunks(sums, nb, sv, threadIdx.x);
    __syncthreads();
    ct_scan_spread(sums, nb, sv, threadIdx.x);
}
// out[i] = the sum of the values before i, out[n] = the total; out may be ``in`` itself: a block has read its values by then
template <class Out>
__device__ __forceinline__ void ct_scan_put(long n, const int64_t* sums, Out* out, long block, int tid, int own, int64_t before) {
    const long i = block * 256 + tid;
    if (i >= n) return;
    const int64_t at = sums[block] + before;
    out[i] = (Out)at;
    if (i == n - 1) out[n] = (Out)(at + own);
}
template <class Out>
__global__ __launch_bounds__(256) void ct_scan_write_kernel(const int* in, long n, const int64_t* sums, Out* out) {
    __shared__ int sm[256];
    __shared__ int64_t sg[16];
    const int own = ct_scan_load(in, n, blockIdx.x, threadIdx.x);
    sm[threadIdx.x] = own;
    __syncthreads();
    ct_scan_groups(sm, sg, threadIdx.x);
    __syncthreads();
    ct_scan_put<Out>(n, sums, out, blockIdx.x, threadIdx.x, own, ct_scan_before(sm, sg, threadIdx.x));
}

// ---- the segments -------------------------------------------------------------------------------------------------------------
struct CtSegs {
    CtPlane p;
    const int* off;                // the cells' offsets, cells + 1 of them
    int* cell;                     // per segment: its cell
    int* succ;                     // the segment the line goes on with, -1 where it leaves the plane
    int* pred;                     // the segment it comes from, -1 where it enters the plane
    long cells, S;
};

__device__ __forceinline__ void ct_fill_cell(const CtSegs& a, long n) {
    const int hi = a.off[n + 1];
    for (int s = a.off[n]; s < hi; ++s) a.cell[s] = (int)n;
}
__global__ __launch_bounds__(256) void ct_fill_kernel(const CtSegs a) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n < a.cells) ct_fill_cell(a, n);
}

// what a segment is, from its id
struct CtSeg {
    CtCell k;
    int r, c, j, e, x;
};
__device__ __forceinline__ CtSeg ct_seg(const CtSegs& a, int s) {
    CtSeg g;
    const int n = a.cell[s], W1 = a.p.W - 1;
    g.r = n / W1, g.c = n - g.r * W1;
    g.k = ct_cell(a.p, g.r, g.c);
    ct_unlocal(g.k, s - a.off[n], g.j, g.e);
    g.x = ct_exit_of(a.p, g.k, g.j, g.e);
    return g;
}
// the cell across edge e of (r, c), or -1 outside the plane
__device__ __forceinline__ int ct_across(const CtSegs& a, int r, int c, int e, int& nr, int& nc) {
    nr = r + (e == 2 ? 1 : e == 0 ? -1 : 0);
    nc = c + (e == 1 ? 1 : e == 3 ? -1 : 0);
    if (nr < 0 || nc < 0 || nr >= a.p.H - 1 || nc >= a.p.W - 1) return -1;
    return nr * (a.p.W - 1) + nc;
}
// the successor enters the cell across the exit edge through that edge; the predecessor leaves the cell across the entry edge
// through it; the minimum's doubling starts from (s, succ)
__device__ __forceinline__ void ct_link_seg(const CtSegs& a, int s, int* m, int* nx) {
    const CtSeg g = ct_seg(a, s);
    int nr, nc, to = -1, from = -1;
    int n = ct_across(a, g.r, g.c, g.x, nr, nc);
    if (n >= 0) to = a.off[n] + ct_local(ct_cell(a.p, nr, nc), g.j, (g.x + 2) & 3);
    n = ct_across(a, g.r, g.c, g.e, nr, nc);
    if (n >= 0) {
        const CtCell k = ct_cell(a.p, nr, nc);
        from = a.off[n] + ct_local(k, g.j, ct_entry_of(a.p, k, g.j, (g.e + 2) & 3));
    }
    a.succ[s] = to;
    a.pred[s] = from;
    m[s] = s;
    nx[s] = to;
}
__global__ __launch_bounds__(256) void ct_link_kernel(const CtSegs a, int* m, int* nx) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s < a.S) ct_link_seg(a, (int)s, m, nx);
}

// ---- the loops' least ids: m = the least id among the next 2^k segments, nx = the segment 2^k further or -1 beyond the end ------
__device__ __forceinline__ int ct_min_seg(int s, const int* m0, const int* n0, int* m1, int* n1) {
    const int m = m0[s], n = n0[s];
    int mm = m, nn = n;
    if (n >= 0) mm = min(m, m0[n]), nn = n0[n];
    m1[s] = mm;
    n1[s] = nn;
    return mm != m || (nn < 0 && n >= 0);
}
__global__ __launch_bounds__(256) void ct_min_kernel(long S, const int* m0, const int* n0, int* m1, int* n1, int* word) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    hyd_raise(s < S ? ct_min_seg((int)s, m0, n0, m1, n1) : 0, word);
}
// a segment starts its line if nothing precedes it, or if it is the least of a loop (a pointer that never ran off an end)
__device__ __forceinline__ void ct_cut_seg(int s, const int* m, const int* nx, const int* pred, int* p, int* d) {
    const int from = pred[s];
    const bool start = from < 0 || (nx[s] >= 0 && m[s] == s);
    p[s] = start ? s : from;
    d[s] = start ? 0 : 1;
}
__global__ __launch_bounds__(256) void ct_cut_kernel(long S, const int* m, const int* nx, const int* pred, int* p, int* d) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s < S) ct_cut_seg((int)s, m, nx, pred, p, d);
}

// ---- the ranks: p = the segment 2^k back or the line's start, d = the hops to it -----------------------------------------------
__device__ __forceinline__ int ct_rank_seg(int s, const int* p0, const int* d0, int* p1, int* d1) {
    const int p = p0[s], pp = p0[p];
    p1[s] = pp;
    d1[s] = d0[s] + d0[p];
    return pp != p;
}
__global__ __launch_bounds__(256) void ct_rank_kernel(long S, const int* p0, const int* d0, int* p1, int* d1, int* word) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    hyd_raise(s < S ? ct_rank_seg((int)s, p0, d0, p1, d1) : 0, word);
}

// ---- the lines ----------------------------------------------------------------------------------------------------------------
struct CtLines {
    CtSegs a;
    const int* p;                  // per segment: its line's start
    const int* d;                  // its hops from it
    int* line;                     // 1 at a start; after the scan the line's number, S + 1 of them
    int* vcount;                   // per line: its vertices
    const int64_t* offsets;
    int32_t* edge;
    double* t;
    int32_t* level;
    uint8_t* closed;
};
__device__ __forceinline__ void ct_flag_seg(const CtLines& l, int s) { l.line[s] = l.p[s] == s ? 1 : 0; }
__global__ __launch_bounds__(256) void ct_flag_kernel(const CtLines l) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s < l.a.S) ct_flag_seg(l, (int)s);
}
// the last segment of a line: the line leaves the plane behind it, or goes on with the line's own start (a loop)
__device__ __forceinline__ void ct_tail_seg(const CtLines& l, int s) {
    const int to = l.a.succ[s], start = l.p[s];
    if (to >= 0 && to != start) return;
    l.vcount[l.line[start]] = l.d[s] + (to >= 0 ? 1 : 2);
}
__global__ __launch_bounds__(256) void ct_tail_kernel(const CtLines l) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s < l.a.S) ct_tail_seg(l, (int)s);
}
__device__ __forceinline__ void ct_put_vertex(const CtLines& l, int64_t at, const CtVertex& v) {
    l.edge[3 * at] = v.r, l.edge[3 * at + 1] = v.c, l.edge[3 * at + 2] = v.axis;
    l.t[at] = v.t;
}
__device__ __forceinline__ void ct_write_seg(const CtLines& l, int s) {
    const CtSeg g = ct_seg(l.a, s);
    const int to = l.a.succ[s], start = l.p[s], n = l.line[start];
    const int64_t at = l.offsets[n] + l.d[s];
    ct_put_vertex(l, at, ct_vertex(l.a.p, g.k, g.r, g.c, g.e, g.j));
    if (to >= 0 && to != start) return;
    l.level[n] = g.j;
    l.closed[n] = to >= 0 ? 1 : 0;
    if (to < 0) ct_put_vertex(l, at + 1, ct_vertex(l.a.p, g.k, g.r, g.c, g.x, g.j));
}
__global__ __launch_bounds__(256) void ct_write_kernel(const CtLines l) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s < l.a.S) ct_write_seg(l, (int)s);
}

// ---- the marks: what the paint reads ------------------------------------------------------------------------------------------
struct CtMarks {
    CtPlane p;
    uint32_t* marks;
    int pm, index_every;
};
// 0: no level between the two heights; 2: an index contour (j a multiple of index_every) among them; else 1
__device__ __forceinline__ unsigned ct_between(const CtMarks& a, int A, int B) {
    const int lo = min(A, B), hi = max(A, B);
    if (hi <= lo) return 0u;
    const int m = lo % a.index_every;                                          // has the sign of lo
    const int64_t first = (int64_t)lo - m + (m > 0 ? a.index_every : 0);       // the least multiple of index_every >= lo
    return first < hi ? 2u : 1u;
}
__device__ __forceinline__ void ct_marks_cell(const CtMarks& a, int y, int x) {
    const int* z = a.p.zq + (long)y * a.p.pz + x;
    const int A = ct_above(a.p.lv, z[0]);
    unsigned m = 0u;
    if (x + 1 < a.p.W) m = max(m, ct_between(a, A, ct_above(a.p.lv, z[1])));
    if (y + 1 < a.p.H) m = max(m, ct_between(a, A, ct_above(a.p.lv, z[a.p.pz])));
    a.marks[(long)y * a.pm + x] = m;
}
__global__ __launch_bounds__(256) void ct_marks_kernel(const CtMarks a) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (y < a.p.H && x < a.p.W) ct_marks_cell(a, y, x);
}

#define CT_FLAT(total) dim3((unsigned)(((long)(total) + 255) / 256)), dim3(256), 0, ctx->stream

}  // namespace

extern "C" {

// ---- the host side: layouts, checks, launches -----------------------------------------------------------------------------------
static long ct_cells(int32_t H, int32_t W) { return H < 2 || W < 2 ? 0 : (long)(H - 1) * (W - 1); }
static long ct_blocks(long n) { return (n + 255) / 256; }
static size_t ct_round(size_t bytes) { return (bytes + 255) / 256 * 256; }

// the cells' buffer: the offsets int32 [cells + 1], the blocks' sums int64 [blocks + 1]
struct CtCellsBuf {
    int* off;
    int64_t* sums;
};
static CtCellsBuf ct_cells_buf(void* buf, long cells) {
    CtCellsBuf b;
    b.off = (int*)buf;
    b.sums = (int64_t*)((char*)buf + ct_round(4 * (size_t)(cells + 1)));
    return b;
}

// the workspace: a header (magic, S, L, V, where the ranks lie; then the changed words), the blocks' sums, seven int32 arrays of
// S + 1: cell, succ, pred and two pairs the doubling alternates between
struct CtHeader {
    int64_t magic, S, L, V, ranks;
};
struct CtWork {
    CtHeader* head;
    int* words;
    int64_t* sums;
    int* cell;
    int* succ;
    int* pred;
    int* pair[2][2];
};
static size_t ct_work_array(long S) { return ct_round(4 * (size_t)(S + 1)); }
static CtWork ct_work(void* ws, long S) {
    CtWork w;
    char* at = (char*)ws;
    w.head = (CtHeader*)at;
    w.words = (int*)(at + 64);
    at += 256;
    w.sums = (int64_t*)at;
    at += ct_round(8 * (size_t)(ct_blocks(S) + 1));
    const size_t n = ct_work_array(S);
    w.cell = (int*)at, w.succ = (int*)(at + n), w.pred = (int*)(at + 2 * n);
    for (int i = 0; i < 4; ++i) w.pair[i >> 1][i & 1] = (int*)(at + (3 + i) * n);
    return w;
}

static int ct_check(const char* who, const int32_t* zq, int32_t z_pitch, int32_t H, int32_t W, int32_t base_q, int32_t interval_q,
                    int32_t count, CtPlane& p) {
    GHM_CHECK(zq, "%s: null pointer", who);
    if (int rc = hyd_check_plane(who, H, W, z_pitch, "zq")) return rc;
    GHM_CHECK(interval_q >= 1, "%s: interval_q=%d (interval_q >= 1)", who, interval_q);
    GHM_CHECK(base_q >= -(1 << 30) && base_q <= (1 << 30), "%s: base_q=%d outside [-2^30, 2^30]", who, base_q);
    GHM_CHECK(count == -1 || (count >= 1 && count <= CT_LEVEL_LIMIT), "%s: count=%d (-1 for every level, or 1 .. 2^28)", who, count);
    p.zq = zq;
    p.H = H, p.W = W, p.pz = z_pitch;
    p.lv.base_q = base_q, p.lv.iq = interval_q;
    p.lv.jlo = count < 0 ? -CT_LEVEL_LIMIT : 0;
    p.lv.jhi = count < 0 ? CT_LEVEL_LIMIT : count;
    return 0;
}

extern "C++" {
// the exclusive scan of in[0 .. n) -> out[0 .. n], n >= 1; write = false: the sums and the total alone
template <class Out>
static void ct_scan(ghm_ctx* ctx, const int* in, long n, int64_t* sums, Out* out, bool write) {
    const long nb = ct_blocks(n);
    hipLaunchKernelGGL(ct_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, in, n, sums);
    hipLaunchKernelGGL(ct_scan_blocks_kernel, dim3(1), dim3(256), 0, ctx->stream, sums, nb);
    if (write) hipLaunchKernelGGL((ct_scan_write_kernel<Out>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, in, n, sums, out);
}
}  // extern "C++"

static int ct_read(ghm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    GHM_LAUNCH_CHECK();
    GHM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C++" {
// doubling rounds in groups of CT_GROUP until one changes nothing; round(i, word) issues round i.  *launched: the rounds issued
// (the result lies where the last of them wrote); *needed: the rounds up to the first that changed nothing, that one included
template <class Round>
static int ct_double(ghm_ctx* ctx, const char* who, const char* what, int* words, Round round, int* launched, int* needed) {
    GHM_HIP(hipMemsetAsync(words, 0, 4 * CT_MAX_ROUNDS, ctx->stream));
    int done = 0;
    for (;;) {
        GHM_CHECK(done < CT_MAX_ROUNDS, "%s: %s did not come to rest within %d doubling rounds", who, what, CT_MAX_ROUNDS);
        const int n = min(CT_GROUP, CT_MAX_ROUNDS - done);
        for (int i = 0; i < n; ++i) round(done + i, words + done + i);
        int w[CT_GROUP] = {};
        if (int rc = ct_read(ctx, w, words + done, 4 * (size_t)n)) return rc;
        done += n;
        for (int i = 0; i < n; ++i)
            if (!w[i]) {
                *launched = done;
                *needed = done - n + i + 1;
                return 0;
            }
    }
}
}  // extern "C++"

int64_t ghm_contour_cells_bytes(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31) || H > 4 * 65535) return -1;
    const long cells = ct_cells(H, W);
    return (int64_t)(ct_round(4 * (size_t)(cells + 1)) + ct_round(8 * (size_t)(ct_blocks(cells) + 1)));
}

int64_t ghm_contour_workspace(int32_t H, int32_t W, int64_t segments) {
    if (ghm_contour_cells_bytes(H, W) < 0 || segments < 0 || segments >= ((int64_t)1 << 31)) return -1;
    return (int64_t)(256 + ct_round(8 * (size_t)(ct_blocks(segments) + 1)) + 7 * ct_work_array(segments));
}

int ghm_contour_count(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, int32_t H, int32_t W, int32_t base_q, int32_t interval_q,
                      int32_t count, void* cells_buf, int64_t* segments) {
    if (int rc = hyd_sync_ok(ctx, "ghm_contour_count")) return rc;
    GHM_CHECK(cells_buf && segments, "ghm_contour_count: null pointer");
    CtPlane p;
    if (int rc = ct_check("ghm_contour_count", zq, z_pitch, H, W, base_q, interval_q, count, p)) return rc;
    const long cells = ct_cells(H, W);
    if (cells == 0) {                            // no cells: no segments, and not an error
        *segments = 0;
        return 0;
    }
    const CtCellsBuf b = ct_cells_buf(cells_buf, cells);
    hipLaunchKernelGGL(ct_count_kernel, CT_FLAT(cells), p, cells, b.off);
    ct_scan<int>(ctx, b.off, cells, b.sums, b.off, true);
    int64_t total = 0;
    if (int rc = ct_read(ctx, &total, b.sums + ct_blocks(cells), sizeof(total))) return rc;
    *segments = total;
    return 0;
}

int ghm_contour_trace(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, int32_t H, int32_t W, int32_t base_q, int32_t interval_q,
                      int32_t count, const void* cells_buf, void* workspace, int64_t segments, int64_t* lines, int64_t* vertices,
                      int32_t* rounds) {
    const char* who = "ghm_contour_trace";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(cells_buf && workspace && lines && vertices, "%s: null pointer", who);
    CtPlane p;
    if (int rc = ct_check(who, zq, z_pitch, H, W, base_q, interval_q, count, p)) return rc;
    GHM_CHECK(segments >= 0 && segments < ((int64_t)1 << 31), "%s: %lld segments (0 <= segments < 2^31)", who, (long long)segments);
    const long cells = ct_cells(H, W), S = (long)segments;
    int64_t total = 0;
    if (cells > 0) {
        const CtCellsBuf b = ct_cells_buf(const_cast<void*>(cells_buf), cells);
        if (int rc = ct_read(ctx, &total, b.sums + ct_blocks(cells), sizeof(total))) return rc;
    }
    GHM_CHECK(total == segments, "%s: the cells hold %lld segments, the call says %lld", who, (long long)total, (long long)segments);
    const CtWork w = ct_work(workspace, S);
    CtHeader head = {CT_MAGIC, segments, 0, 0, 0};
    int needed = 0;
    if (S > 0) {
        CtSegs a;
        a.p = p;
        a.off = ct_cells_buf(const_cast<void*>(cells_buf), cells).off;
        a.cell = w.cell, a.succ = w.succ, a.pred = w.pred;
        a.cells = cells, a.S = S;
        hipLaunchKernelGGL(ct_fill_kernel, CT_FLAT(cells), a);
        hipLaunchKernelGGL(ct_link_kernel, CT_FLAT(S), a, w.pair[0][0], w.pair[0][1]);
        int launched = 0, unused = 0;
        auto least = [&](int i, int* word) {
            int* const* src = w.pair[i & 1];
            int* const* dst = w.pair[(i + 1) & 1];
            hipLaunchKernelGGL(ct_min_kernel, CT_FLAT(S), S, src[0], src[1], dst[0], dst[1], word);
        };
        if (int rc = ct_double(ctx, who, "a loop's least id", w.words, least, &launched, &unused)) return rc;
        int at = launched & 1;                   // the pair the last round wrote
        hipLaunchKernelGGL(ct_cut_kernel, CT_FLAT(S), S, w.pair[at][0], w.pair[at][1], w.pred, w.pair[at ^ 1][0], w.pair[at ^ 1][1]);
        at ^= 1;
        const int first = at;
        auto rank = [&](int i, int* word) {
            int* const* src = w.pair[(first + i) & 1];
            int* const* dst = w.pair[(first + i + 1) & 1];
            hipLaunchKernelGGL(ct_rank_kernel, CT_FLAT(S), S, src[0], src[1], dst[0], dst[1], word);
        };
        if (int rc = ct_double(ctx, who, "a line's ranking", w.words, rank, &launched, &needed)) return rc;
        at = (first + launched) & 1;
        head.ranks = at;
        CtLines l = {};
        l.a = a;
        l.p = w.pair[at][0], l.d = w.pair[at][1];
        l.line = w.pair[at ^ 1][0], l.vcount = w.pair[at ^ 1][1];
        hipLaunchKernelGGL(ct_flag_kernel, CT_FLAT(S), l);
        ct_scan<int>(ctx, l.line, S, w.sums, l.line, true);
        if (int rc = ct_read(ctx, &head.L, w.sums + ct_blocks(S), sizeof(int64_t))) return rc;
        GHM_CHECK(head.L >= 1 && head.L <= S, "%s: %lld lines of %ld segments", who, (long long)head.L, S);
        hipLaunchKernelGGL(ct_tail_kernel, CT_FLAT(S), l);
        ct_scan<int64_t>(ctx, l.vcount, (long)head.L, w.sums, nullptr, false);
        if (int rc = ct_read(ctx, &head.V, w.sums + ct_blocks((long)head.L), sizeof(int64_t))) return rc;
    }
    GHM_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    *lines = head.L;
    *vertices = head.V;
    if (rounds) *rounds = needed;
    return 0;
}

int ghm_contour_extract(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, int32_t H, int32_t W, int32_t base_q, int32_t interval_q,
                        int32_t count, const void* cells_buf, void* workspace, int64_t segments, int64_t lines, int64_t vertices,
                        int32_t* edge, double* t, int64_t* offsets, int32_t* level, uint8_t* closed) {
    const char* who = "ghm_contour_extract";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(cells_buf && workspace && offsets, "%s: null pointer", who);
    GHM_CHECK(lines == 0 || (edge && t && level && closed), "%s: null pointer", who);
    CtPlane p;
    if (int rc = ct_check(who, zq, z_pitch, H, W, base_q, interval_q, count, p)) return rc;
    GHM_CHECK(segments >= 0 && segments < ((int64_t)1 << 31), "%s: %lld segments (0 <= segments < 2^31)", who, (long long)segments);
    const long cells = ct_cells(H, W), S = (long)segments;
    const CtWork w = ct_work(workspace, S);
    CtHeader head = {};
    if (int rc = ct_read(ctx, &head, w.head, sizeof(head))) return rc;
    int64_t total = 0;
    if (cells > 0) {
        const CtCellsBuf b = ct_cells_buf(const_cast<void*>(cells_buf), cells);
        if (int rc = ct_read(ctx, &total, b.sums + ct_blocks(cells), sizeof(total))) return rc;
    }
    // the arrays were sized by ghm_contour_trace: nothing is written where they do not fit
    GHM_CHECK(head.magic == CT_MAGIC && head.S == segments && total == segments && head.L == lines && head.V == vertices &&
                  (head.ranks == 0 || head.ranks == 1),
              "%s: the workspace was traced with %lld segments, %lld lines and %lld vertices, the call says %lld, %lld and %lld", who,
              (long long)(head.magic == CT_MAGIC ? head.S : -1), (long long)(head.magic == CT_MAGIC ? head.L : -1),
              (long long)(head.magic == CT_MAGIC ? head.V : -1), (long long)segments, (long long)lines, (long long)vertices);
    if (lines == 0) {
        GHM_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), ctx->stream));
        return 0;
    }
    const int at = (int)head.ranks;
    CtLines l = {};
    l.a.p = p;
    l.a.off = ct_cells_buf(const_cast<void*>(cells_buf), cells).off;
    l.a.cell = w.cell, l.a.succ = w.succ, l.a.pred = w.pred;
    l.a.cells = cells, l.a.S = S;
    l.p = w.pair[at][0], l.d = w.pair[at][1];
    l.line = w.pair[at ^ 1][0], l.vcount = w.pair[at ^ 1][1];
    l.offsets = offsets;
    l.edge = edge, l.t = t, l.level = level, l.closed = closed;
    ct_scan<int64_t>(ctx, l.vcount, (long)lines, w.sums, offsets, true);
    hipLaunchKernelGGL(ct_write_kernel, CT_FLAT(S), l);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_contour_marks(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, int32_t H, int32_t W, int32_t base_q, int32_t interval_q,
                      int32_t count, int32_t index_every, uint32_t* marks, int32_t m_pitch) {
    const char* who = "ghm_contour_marks";
    GHM_CHECK(ctx && marks, "%s: null pointer", who);
    CtMarks a;
    if (int rc = ct_check(who, zq, z_pitch, H, W, base_q, interval_q, count, a.p)) return rc;
    if (int rc = hyd_check_plane(who, H, W, m_pitch, "marks")) return rc;
    GHM_CHECK(index_every >= 1, "%s: index_every=%d (index_every >= 1)", who, index_every);
    a.marks = marks;
    a.pm = m_pitch;
    a.index_every = index_every;
    hipLaunchKernelGGL(ct_marks_kernel, dim3(ceil_div(W, 64), ceil_div(H, 4)), dim3(64, 4), 0, ctx->stream, a);
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
