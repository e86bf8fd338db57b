// Peaks of a heightfield (gan_heightmaps_amd/peaks.py): summits, their key cols, parents and prominences.  Integers
// throughout, so there are no tolerances; include/ghm.h, section "peaks", has the definition and tests/peaks_ref.py restates it.
//
// Cells are totally ordered by key(c) = (zq[c], idx(c)), idx = row W + col.
// 1. Ascent: a thread per cell writes the direction of its neighbour of greatest key if that key is above its own, else -1: a
//    summit.  ghm_hydrology_accumulate over these directions gives every cell its summit (label) and every summit its region's
//    size (area): no kernel of this file.
// 2. Count: a thread per cell flags the summits and counts the cell's edges -- (c, k) with key(n_k) > key(c) and another label on
//    the far side; two exclusive scans number both.  The weight of an edge packs (zq[c] + 2^25, idx(c), k) and 1 is added, so
//    weights are unique and 0 means "no edge".
// 3. Tree: the maximum spanning forest of the regions under these weights, by Boruvka rounds.  comp[s] is the component of summit
//    cell s.  A round: (a) best = 0 at every summit; (b) every edge whose ends lie in different components offers its weight to
//    both roots (64-bit atomicMax: any order, the same result); (c) every root that was offered an edge marks it (atomicOr of bit
//    k into the cell's mask) and writes the root across it to hook[s] -- in a mutual pick of one edge the root with the smaller
//    index keeps itself -- and a second launch moves hook to comp, so that (c) reads comp as the round found it; (d) pointer
//    jumping in place until a pass changes nothing: a pass can only read a pointer that is newer than its launch, which is an
//    ancestor all the same, and roots are never written.  The rounds end when (b) finds no edge.
//    Two forms, the same bits: plain -- (b) is a thread per cell over the whole plane; list -- the edges are compacted once into
//    a list of weights, (b) is a thread per entry, and the entries whose ends have merged are dropped by a scan and a scatter
//    after every round.
// 4. Extract: the summits in cell order with their areas; the marked edges in (cell, k) order as (cell, label, label across).
// ghm_peaks_merge (host, no device): the marked edges sorted by their cell's key, descending, all edges of one cell taken
// together, over a union-find of the summits -- what the definition's sweep does when it visits that cell.
#include <algorithm>
#include <vector>

#include "common.h"
#include "relax.h"

namespace {

constexpr int PK_MAX_ROUNDS = GHM_PEAKS_MAX_ROUNDS;
constexpr int PK_ZQ_LIMIT = 1 << 25;             // |zq| below this: a weight fits 26 + 31 + 3 bits
constexpr int PK_JUMP_GROUP = 4, PK_JUMP_CAP = 64;
constexpr int64_t PK_MAGIC = 0x73746d6d75736b70;  // the header of a counted workspace

__device__ __constant__ const int PK_DY[8] = {-1, -1, 0, 1, 1, 1, 0, -1};      // the hydrology's directions: N NE E SE S SW W NW
__device__ __constant__ const int PK_DX[8] = {0, 1, 1, 1, 0, -1, -1, -1};

typedef unsigned long long pk_u64;

struct PkPlane {
    const int* zq;
    const int* label;
    int H, W, pz, pl, n;
};

__device__ __forceinline__ bool pk_above(int za, int ia, int zb, int ib) { return za > zb || (za == zb && ia > ib); }

// ---- the ascent ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pk_ascent_cell(const int* zq, int pz, int H, int W, int r, int c) {
    int best = -1, bz = zq[(long)r * pz + c], bi = r * W + c;
    for (int k = 0; k < 8; ++k) {
        const int y = r + PK_DY[k], x = c + PK_DX[k];
        if (y < 0 || y >= H || x < 0 || x >= W) continue;
        const int z = zq[(long)y * pz + x], i = y * W + x;
        if (pk_above(z, i, bz, bi)) bz = z, bi = i, best = k;
    }
    return best;
}
__global__ __launch_bounds__(256) void pk_ascent_kernel(const int* __restrict__ zq, int pz, int H, int W, signed char* __restrict__ dir,
                                                        int pd) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    if (r < H && c < W) dir[(long)r * pd + c] = (signed char)pk_ascent_cell(zq, pz, H, W, r, c);
}

// ---- edges and weights --------------------------------------------------------------------------------------------------------
// is (cell idx, direction k) an edge?  la, lb: the labels on its two sides, both inside [0, n)
__device__ __forceinline__ bool pk_edge(const PkPlane& p, int idx, int k, int& la, int& lb) {
    const int r = idx / p.W, c = idx - r * p.W, y = r + PK_DY[k], x = c + PK_DX[k];
    if (y < 0 || y >= p.H || x < 0 || x >= p.W) return false;
    if (!pk_above(p.zq[(long)y * p.pz + x], y * p.W + x, p.zq[(long)r * p.pz + c], idx)) return false;
    la = p.label[(long)r * p.pl + c], lb = p.label[(long)y * p.pl + x];
    return la != lb && (unsigned)la < (unsigned)p.n && (unsigned)lb < (unsigned)p.n;
}
__device__ __forceinline__ pk_u64 pk_weight(int zq, int idx, int k) {
    return (((pk_u64)(unsigned)(zq + PK_ZQ_LIMIT) << 34) | ((pk_u64)(unsigned)idx << 3) | (pk_u64)k) + 1;
}
__device__ __forceinline__ void pk_unweight(pk_u64 w, int& idx, int& k) {
    w -= 1;
    k = (int)(w & 7);
    idx = (int)((w >> 3) & 0x7fffffffu);
}
__device__ __forceinline__ int pk_zq_at(const PkPlane& p, int idx) {
    const int r = idx / p.W;
    return p.zq[(long)r * p.pz + (idx - r * p.W)];
}

// ---- the count: sflag[idx] = 1 at a summit, ecount[idx] = the cell's edges; 1 is returned for a height out of range or a label
// that is no summit (a cell of the plane that is its own label) ------------------------------------------------------------------
__device__ __forceinline__ int pk_flag_cell(const PkPlane& p, int idx, int* sflag, int* ecount) {
    const int r = idx / p.W, c = idx - r * p.W;
    const int z = p.zq[(long)r * p.pz + c], l = p.label[(long)r * p.pl + c];
    sflag[idx] = l == idx ? 1 : 0;
    int e = 0, la, lb;
    for (int k = 0; k < 8; ++k) e += pk_edge(p, idx, k, la, lb) ? 1 : 0;
    ecount[idx] = e;
    bool stray = (unsigned)l >= (unsigned)p.n;
    if (!stray) {
        const int lr = l / p.W;
        stray = p.label[(long)lr * p.pl + (l - lr * p.W)] != l;
    }
    return stray || z <= -PK_ZQ_LIMIT || z >= PK_ZQ_LIMIT;
}
__global__ __launch_bounds__(256) void pk_flag_kernel(const PkPlane p, int* sflag, int* ecount, int* word) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    hyd_raise(idx < p.n ? pk_flag_cell(p, (int)idx, sflag, ecount) : 0, word);
}

// ---- an exclusive scan of n int32 values in place: the blocks' sums, their scan by one block, the write (the contour's) --------
__device__ __forceinline__ int pk_scan_load(const int* in, long n, long block, int tid) {
    const long i = block * 256 + tid;
    return i < n ? in[i] : 0;
}
__device__ __forceinline__ void pk_scan_groups(const int* sm, int64_t* sg, int tid) {
    if (tid >= 16) return;
    int64_t a = 0;
    for (int i = 0; i < 16; ++i) a += sm[16 * tid + i];
    sg[tid] = a;
}
// the sum of the values of the threads before tid (tid = 256: of the block)
__device__ __forceinline__ int64_t pk_scan_before(const int* sm, const int64_t* sg, int tid) {
    int64_t a = 0;
    for (int g = 0; g < (tid >> 4); ++g) a += sg[g];
    for (int i = tid & ~15; i < tid; ++i) a += sm[i];
    return a;
}
__global__ __launch_bounds__(256) void pk_scan_sums_kernel(const int* in, long n, int64_t* sums) {
    __shared__ int sm[256];
    __shared__ int64_t sg[16];
    sm[threadIdx.x] = pk_scan_load(in, n, blockIdx.x, threadIdx.x);
    __syncthreads();
    pk_scan_groups(sm, sg, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = pk_scan_before(sm, sg, 256);
}
__device__ __forceinline__ void pk_scan_chunks(const int64_t* sums, long nb, int64_t* sv, int tid) {
    const long chunk = (nb + 255) / 256, lo = min(tid * chunk, nb), hi = min(lo + chunk, nb);
    int64_t a = 0;
    for (long i = lo; i < hi; ++i) a += sums[i];
    sv[tid] = a;
}
__device__ __forceinline__ void pk_scan_spread(int64_t* sums, long nb, const int64_t* sv, int tid) {
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
__global__ __launch_bounds__(256) void pk_scan_blocks_kernel(int64_t* sums, long nb) {
    __shared__ int64_t sv[256];
    pk_scan_chunks(sums, nb, sv, threadIdx.x);
    __syncthreads();
    pk_scan_spread(sums, nb, sv, threadIdx.x);
}
// out[i] = the sum of the values before i, out[n] = the total; a block has read its values by then
__device__ __forceinline__ void pk_scan_put(long n, const int64_t* sums, int* out, long block, int tid, int own, int64_t before) {
    const long i = block * 256 + tid;
    if (i >= n) return;
    const int64_t at = sums[block] + before;
    out[i] = (int)at;
    if (i == n - 1) out[n] = (int)(at + own);
}
__global__ __launch_bounds__(256) void pk_scan_write_kernel(int* io, long n, const int64_t* sums) {
    __shared__ int sm[256];
    __shared__ int64_t sg[16];
    const int own = pk_scan_load(io, n, blockIdx.x, threadIdx.x);
    sm[threadIdx.x] = own;
    __syncthreads();
    pk_scan_groups(sm, sg, threadIdx.x);
    __syncthreads();
    pk_scan_put(n, sums, io, blockIdx.x, threadIdx.x, own, pk_scan_before(sm, sg, threadIdx.x));
}

// ---- the summits' list and the components ---------------------------------------------------------------------------------------
struct PkState {
    const int* sidx;               // the scan of the summit flags, n + 1
    int* summit;                   // the summit cells, ascending, P of them
    int* comp;                     // by summit cell: its component, a summit cell
    int* hook;                     // by summit cell: what a root's comp becomes
    pk_u64* best;                  // by summit cell: the greatest weight a root was offered this round
    unsigned* mask;                // the plane of marked edges, bit k
    int pm, P;
};
__device__ __forceinline__ void pk_list_cell(const PkState& s, int idx) {
    const bool summit = s.sidx[idx + 1] != s.sidx[idx];
    s.comp[idx] = summit ? idx : -1;             // a label that is no summit has no component: its edges are never offered
    if (summit) s.summit[s.sidx[idx]] = idx;
}
__global__ __launch_bounds__(256) void pk_list_kernel(const PkState s, int n) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < n) pk_list_cell(s, (int)idx);
}
__global__ __launch_bounds__(256) void pk_mask_clear_kernel(unsigned* mask, int pm, int H, int W) {
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    if (r < H && c < W) mask[(long)r * pm + c] = 0u;
}

// (a)
__device__ __forceinline__ void pk_clear_summit(const PkState& s, int j) { s.best[s.summit[j]] = 0; }
__global__ __launch_bounds__(256) void pk_clear_kernel(const PkState s) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j < s.P) pk_clear_summit(s, (int)j);
}
// (b) the edge of weight w between the labels la and lb: 1 if its ends lie in different components
__device__ __forceinline__ int pk_offer(const PkState& s, int la, int lb, pk_u64 w) {
    const int ra = s.comp[la], rb = s.comp[lb];
    if (ra == rb || (ra | rb) < 0) return 0;
    atomicMax(&s.best[ra], w);
    atomicMax(&s.best[rb], w);
    return 1;
}
__device__ __forceinline__ int pk_pick_cell(const PkPlane& p, const PkState& s, int idx) {
    int any = 0, la, lb;
    for (int k = 0; k < 8; ++k)
        if (pk_edge(p, idx, k, la, lb)) any |= pk_offer(s, la, lb, pk_weight(pk_zq_at(p, idx), idx, k));
    return any;
}
__global__ __launch_bounds__(256) void pk_pick_plain_kernel(const PkPlane p, const PkState s, int* word) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    hyd_raise(idx < p.n ? pk_pick_cell(p, s, (int)idx) : 0, word);
}
// the labels across the edge of weight w, which is an edge
__device__ __forceinline__ void pk_ends(const PkPlane& p, pk_u64 w, int& idx, int& k, int& la, int& lb) {
    pk_unweight(w, idx, k);
    const int r = idx / p.W, c = idx - r * p.W;
    la = p.label[(long)r * p.pl + c];
    lb = p.label[(long)(r + PK_DY[k]) * p.pl + (c + PK_DX[k])];
}
__device__ __forceinline__ void pk_pick_item(const PkPlane& p, const PkState& s, const pk_u64* list, long i, int* alive) {
    int idx, k, la, lb;
    pk_ends(p, list[i], idx, k, la, lb);
    alive[i] = pk_offer(s, la, lb, list[i]);
}
__global__ __launch_bounds__(256) void pk_pick_list_kernel(const PkPlane p, const PkState s, const pk_u64* list, long E, int* alive) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < E) pk_pick_item(p, s, list, i, alive);
}
// the list: a cell's edges at eoff[idx], in the order of k
__device__ __forceinline__ void pk_fill_cell(const PkPlane& p, const int* eoff, int idx, pk_u64* list) {
    int at = eoff[idx], la, lb;
    if (eoff[idx + 1] == at) return;
    for (int k = 0; k < 8; ++k)
        if (pk_edge(p, idx, k, la, lb)) list[at++] = pk_weight(pk_zq_at(p, idx), idx, k);
}
__global__ __launch_bounds__(256) void pk_fill_kernel(const PkPlane p, const int* eoff, pk_u64* list) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < p.n) pk_fill_cell(p, eoff, (int)idx, list);
}
// off: the scan of the alive flags, E + 1
__device__ __forceinline__ void pk_keep_item(const pk_u64* in, const int* off, long i, pk_u64* out) {
    if (off[i + 1] != off[i]) out[off[i]] = in[i];
}
__global__ __launch_bounds__(256) void pk_keep_kernel(const pk_u64* in, const int* off, long E, pk_u64* out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < E) pk_keep_item(in, off, i, out);
}
// (c)
__device__ __forceinline__ void pk_hook_summit(const PkPlane& p, const PkState& s, int j) {
    const int me = s.summit[j];
    if (s.comp[me] != me) return;
    const pk_u64 w = s.best[me];
    int to = me;
    if (w != 0) {
        int idx, k, la, lb;
        pk_ends(p, w, idx, k, la, lb);
        const int ra = s.comp[la], rb = s.comp[lb];
        const int other = ra == me ? rb : ra;
        if (!(s.best[other] == w && me < other)) to = other;
        const int r = idx / p.W;
        atomicOr(&s.mask[(long)r * s.pm + (idx - r * p.W)], 1u << k);
    }
    s.hook[me] = to;
}
__global__ __launch_bounds__(256) void pk_hook_kernel(const PkPlane p, const PkState s) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j < s.P) pk_hook_summit(p, s, (int)j);
}
__device__ __forceinline__ void pk_apply_summit(const PkState& s, int j) {
    const int me = s.summit[j];
    if (s.comp[me] == me) s.comp[me] = s.hook[me];
}
__global__ __launch_bounds__(256) void pk_apply_kernel(const PkState s) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j < s.P) pk_apply_summit(s, (int)j);
}
// (d)
__device__ __forceinline__ int pk_jump_summit(const PkState& s, int j) {
    const int me = s.summit[j], c = s.comp[me], cc = s.comp[c];
    if (cc == c) return 0;
    s.comp[me] = cc;
    return 1;
}
__global__ __launch_bounds__(256) void pk_jump_kernel(const PkState s, int* word) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    hyd_raise(j < s.P ? pk_jump_summit(s, (int)j) : 0, word);
}

// ---- the extraction -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pk_marks_cell(const unsigned* mask, int pm, int W, int idx, int* count) {
    const int r = idx / W;
    count[idx] = __builtin_popcount(mask[(long)r * pm + (idx - r * W)] & 255u);
}
__global__ __launch_bounds__(256) void pk_marks_kernel(const unsigned* mask, int pm, int W, int n, int* count) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < n) pk_marks_cell(mask, pm, W, (int)idx, count);
}
struct PkOut {
    const int* summit;             // the workspace's list
    const unsigned* area;          // the accumulation plane
    const int* toff;               // the scan of the marked edges per cell, n + 1
    const unsigned* mask;
    int pa, pm, P;
    int* summit_out;
    unsigned* area_out;
    int* tree;
};
__device__ __forceinline__ void pk_out_summit(const PkOut& o, int W, int j) {
    const int idx = o.summit[j], r = idx / W;
    o.summit_out[j] = idx;
    o.area_out[j] = o.area[(long)r * o.pa + (idx - r * W)];
}
__global__ __launch_bounds__(256) void pk_out_summit_kernel(const PkOut o, int W) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j < o.P) pk_out_summit(o, W, (int)j);
}
__device__ __forceinline__ void pk_out_cell(const PkPlane& p, const PkOut& o, int idx) {
    int at = o.toff[idx];
    if (o.toff[idx + 1] == at) return;
    const int r = idx / p.W, c = idx - r * p.W;
    const unsigned m = o.mask[(long)r * o.pm + c];
    for (int k = 0; k < 8; ++k) {
        if (!(m >> k & 1u)) continue;
        const int y = min(max(r + PK_DY[k], 0), p.H - 1), x = min(max(c + PK_DX[k], 0), p.W - 1);      // a mask is the caller's
        int* row = o.tree + 3 * (long)at++;
        row[0] = idx, row[1] = p.label[(long)r * p.pl + c], row[2] = p.label[(long)y * p.pl + x];
    }
}
__global__ __launch_bounds__(256) void pk_out_cell_kernel(const PkPlane p, const PkOut o) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < p.n) pk_out_cell(p, o, (int)idx);
}

// ---- the merge, on the host -----------------------------------------------------------------------------------------------------
// summit: P cells ascending; szq: their heights; tree: T rows (cell, label, label); ezq: the heights of the rows' cells.
// 0, or 1: T != P - 1; 2: a label that is no summit; 3: the rows are no spanning tree; 4: a prominence beyond 32 bits
int pk_merge(const int32_t* summit, const int32_t* szq, int64_t P, const int32_t* tree, const int32_t* ezq, int64_t T, int32_t min_zq,
             int32_t* col, int32_t* parent, int32_t* prom) {
    if (P < 1 || T != P - 1) return 1;
    std::vector<int32_t> uf((size_t)P), top((size_t)P);
    for (int64_t i = 0; i < P; ++i) uf[(size_t)i] = top[(size_t)i] = (int32_t)i;
    auto find = [&](int32_t x) {
        while (uf[(size_t)x] != x) {
            uf[(size_t)x] = uf[(size_t)uf[(size_t)x]];
            x = uf[(size_t)x];
        }
        return x;
    };
    auto number = [&](int32_t cell) -> int64_t {
        const int32_t* at = std::lower_bound(summit, summit + P, cell);
        return at != summit + P && *at == cell ? at - summit : -1;
    };
    // summits ascend in cell order, so of two of one height the later number has the greater key
    auto higher = [&](int32_t a, int32_t b) { return szq[a] > szq[b] || (szq[a] == szq[b] && a > b); };
    std::vector<int64_t> order((size_t)T);
    for (int64_t i = 0; i < T; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        if (ezq[a] != ezq[b]) return ezq[a] > ezq[b];
        if (tree[3 * a] != tree[3 * b]) return tree[3 * a] > tree[3 * b];
        return a < b;
    });
    std::vector<int32_t> roots;
    int64_t merged = 0;
    for (int64_t i = 0; i < T;) {
        const int32_t cell = tree[3 * order[(size_t)i]], z = ezq[order[(size_t)i]];
        roots.clear();
        for (; i < T && tree[3 * order[(size_t)i]] == cell; ++i)
            for (int side = 1; side <= 2; ++side) {
                const int64_t s = number(tree[3 * order[(size_t)i] + side]);
                if (s < 0) return 2;
                roots.push_back(find((int32_t)s));
            }
        std::sort(roots.begin(), roots.end());
        roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
        if (roots.size() < 2) return 3;
        int32_t keep = roots[0];
        for (int32_t r : roots)
            if (higher(top[(size_t)r], top[(size_t)keep])) keep = r;
        for (int32_t r : roots) {
            if (r == keep) continue;
            const int32_t t = top[(size_t)r];
            const int64_t d = (int64_t)szq[t] - z;
            if (d < 0 || d > 0x7fffffff) return 4;
            col[t] = cell, parent[t] = top[(size_t)keep], prom[t] = (int32_t)d;
            uf[(size_t)r] = keep;
            ++merged;
        }
    }
    if (merged != P - 1) return 3;
    const int32_t t = top[(size_t)find(0)];
    const int64_t d = (int64_t)szq[t] - min_zq;
    if (d < 0 || d > 0x7fffffff) return 4;
    col[t] = -1, parent[t] = -1, prom[t] = (int32_t)d;
    return 0;
}

#define PK_FLAT(total) dim3((unsigned)(((long)(total) + 255) / 256)), dim3(256), 0, ctx->stream
#define PK_PLANE_GRID(H, W) dim3(ceil_div((W), 64), ceil_div((H), 4)), dim3(64, 4), 0, ctx->stream

}  // namespace

extern "C" {

// ---- the host side: layouts, checks, launches -----------------------------------------------------------------------------------
static long pk_blocks(long n) { return (n + 255) / 256; }
static size_t pk_round(size_t bytes) { return (bytes + 255) / 256 * 256; }

// the workspace: a header (and the device word at byte 64), the blocks' sums, sidx and eoff (n + 1 each), summit, comp, hook (n
// each), best (n of 64 bits)
struct PkHeader {
    int64_t magic, H, W, P, E, T;
};
struct PkWork {
    PkHeader* head;
    int* word;
    int64_t* sums;
    int *sidx, *eoff, *summit, *comp, *hook;
    pk_u64* best;
};
static PkWork pk_work(void* ws, long n) {
    PkWork w;
    char* at = (char*)ws;
    w.head = (PkHeader*)at;
    w.word = (int*)(at + 64);
    at += 256;
    w.sums = (int64_t*)at;
    at += pk_round(8 * (size_t)(pk_blocks(n) + 1));
    const size_t one = pk_round(4 * (size_t)(n + 1));
    w.sidx = (int*)at, w.eoff = (int*)(at + one), w.summit = (int*)(at + 2 * one), w.comp = (int*)(at + 3 * one);
    w.hook = (int*)(at + 4 * one);
    w.best = (pk_u64*)(at + 5 * one);
    return w;
}
// the list buffer: two lists of E weights, the alive flags and their scan (E + 1), the blocks' sums
struct PkList {
    pk_u64* list[2];
    int* alive;
    int64_t* sums;
};
static PkList pk_list(void* buf, long E) {
    PkList l;
    char* at = (char*)buf;
    const size_t one = pk_round(8 * (size_t)(E + 1));
    l.list[0] = (pk_u64*)at, l.list[1] = (pk_u64*)(at + one);
    l.alive = (int*)(at + 2 * one);
    l.sums = (int64_t*)(at + 2 * one + pk_round(4 * (size_t)(E + 1)));
    return l;
}

static int pk_check(const char* who, const int32_t* zq, int32_t z_pitch, const int32_t* label, int32_t l_pitch, int32_t H, int32_t W,
                    PkPlane& p) {
    GHM_CHECK(zq && label, "%s: null pointer", who);
    if (int rc = hyd_check_plane(who, H, W, z_pitch, "zq")) return rc;
    if (int rc = hyd_check_plane(who, H, W, l_pitch, "label")) return rc;
    p.zq = zq, p.label = label;
    p.H = H, p.W = W, p.pz = z_pitch, p.pl = l_pitch, p.n = H * W;
    return 0;
}

static void pk_scan(ghm_ctx* ctx, int* io, long n, int64_t* sums) {
    const long nb = pk_blocks(n);
    hipLaunchKernelGGL(pk_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, io, n, sums);
    hipLaunchKernelGGL(pk_scan_blocks_kernel, dim3(1), dim3(256), 0, ctx->stream, sums, nb);
    hipLaunchKernelGGL(pk_scan_write_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, io, n, sums);
}

static int pk_read(ghm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    GHM_LAUNCH_CHECK();
    GHM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int64_t ghm_peaks_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31) || H > 4 * 65535) return -1;
    const long n = (long)H * W;
    return (int64_t)(256 + pk_round(8 * (size_t)(pk_blocks(n) + 1)) + 5 * pk_round(4 * (size_t)(n + 1)) + pk_round(8 * (size_t)n));
}

int64_t ghm_peaks_list_bytes(int64_t edges) {
    if (edges < 0 || edges >= ((int64_t)1 << 31)) return -1;
    const long E = (long)edges;
    return (int64_t)(2 * pk_round(8 * (size_t)(E + 1)) + pk_round(4 * (size_t)(E + 1)) + pk_round(8 * (size_t)(pk_blocks(E) + 1)));
}

int ghm_peaks_ascent(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, int32_t H, int32_t W, int8_t* ascent, int32_t a_pitch) {
    const char* who = "ghm_peaks_ascent";
    GHM_CHECK(ctx && zq && ascent, "%s: null pointer", who);
    if (int rc = hyd_check_plane(who, H, W, z_pitch, "zq")) return rc;
    if (int rc = hyd_check_plane(who, H, W, a_pitch, "ascent")) return rc;
    hipLaunchKernelGGL(pk_ascent_kernel, PK_PLANE_GRID(H, W), zq, z_pitch, H, W, (signed char*)ascent, a_pitch);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_peaks_count(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, const int32_t* label, int32_t l_pitch, int32_t H, int32_t W,
                    void* workspace, int64_t* summits, int64_t* edges) {
    const char* who = "ghm_peaks_count";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(workspace && summits && edges, "%s: null pointer", who);
    PkPlane p;
    if (int rc = pk_check(who, zq, z_pitch, label, l_pitch, H, W, p)) return rc;
    const long n = p.n;
    const PkWork w = pk_work(workspace, n);
    GHM_HIP(hipMemsetAsync(w.head, 0, 256, ctx->stream));
    hipLaunchKernelGGL(pk_flag_kernel, PK_FLAT(n), p, w.sidx, w.eoff, w.word);
    int high = 0;
    if (int rc = hyd_read_word(ctx, w.word, &high)) return rc;
    GHM_CHECK(!high, "%s: a height outside (-2^25, 2^25), or a label that is no summit: the labels are not an ascent's", who);
    PkHeader head = {PK_MAGIC, H, W, 0, 0, -1};
    pk_scan(ctx, w.sidx, n, w.sums);
    if (int rc = pk_read(ctx, &head.P, w.sums + pk_blocks(n), sizeof(int64_t))) return rc;
    pk_scan(ctx, w.eoff, n, w.sums);
    if (int rc = pk_read(ctx, &head.E, w.sums + pk_blocks(n), sizeof(int64_t))) return rc;
    GHM_CHECK(head.P >= 1, "%s: no cell is its own label: the labels are not an ascent's", who);
    PkState s = {};
    s.sidx = w.sidx, s.summit = w.summit, s.comp = w.comp;
    hipLaunchKernelGGL(pk_list_kernel, PK_FLAT(n), s, (int)n);
    GHM_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    *summits = head.P;
    *edges = head.E;
    return 0;
}

static int pk_header(ghm_ctx* ctx, const char* who, const PkWork& w, int32_t H, int32_t W, int64_t summits, PkHeader& head) {
    if (int rc = pk_read(ctx, &head, w.head, sizeof(head))) return rc;
    GHM_CHECK(head.magic == PK_MAGIC && head.H == H && head.W == W && head.P == summits,
              "%s: the workspace was counted with %lld summits on %lld x %lld, the call says %lld on %d x %d", who,
              (long long)(head.magic == PK_MAGIC ? head.P : -1), (long long)(head.magic == PK_MAGIC ? head.H : -1),
              (long long)(head.magic == PK_MAGIC ? head.W : -1), (long long)summits, H, W);
    return 0;
}

int ghm_peaks_tree(ghm_ctx* ctx, const int32_t* zq, int32_t z_pitch, const int32_t* label, int32_t l_pitch, int32_t H, int32_t W,
                   int32_t form, int32_t max_rounds, uint32_t* mask, int32_t m_pitch, void* workspace, void* list, int64_t summits,
                   int64_t edges, int32_t* rounds) {
    const char* who = "ghm_peaks_tree";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(mask && workspace && rounds, "%s: null pointer", who);
    PkPlane p;
    if (int rc = pk_check(who, zq, z_pitch, label, l_pitch, H, W, p)) return rc;
    if (int rc = hyd_check_plane(who, H, W, m_pitch, "mask")) return rc;
    GHM_CHECK(form == GHM_PEAKS_PLAIN || form == GHM_PEAKS_LIST, "%s: form=%d (0 plain, 1 list)", who, form);
    GHM_CHECK(max_rounds >= 1 && max_rounds <= PK_MAX_ROUNDS, "%s: max_rounds=%d (1 .. %d)", who, max_rounds, PK_MAX_ROUNDS);
    const long n = p.n;
    const PkWork w = pk_work(workspace, n);
    PkHeader head = {};
    if (int rc = pk_header(ctx, who, w, H, W, summits, head)) return rc;
    GHM_CHECK(head.E == edges, "%s: the workspace was counted with %lld edges, the call says %lld", who, (long long)head.E,
              (long long)edges);
    if (form == GHM_PEAKS_LIST) {
        GHM_CHECK(edges < ((int64_t)1 << 31), "%s: %lld edges are too many for the list form (< 2^31)", who, (long long)edges);
        GHM_CHECK(list, "%s: the list form needs the list buffer", who);
    }
    PkState s = {};
    s.sidx = w.sidx, s.summit = w.summit, s.comp = w.comp, s.hook = w.hook, s.best = w.best;
    s.mask = mask, s.pm = m_pitch, s.P = (int)head.P;
    hipLaunchKernelGGL(pk_mask_clear_kernel, PK_PLANE_GRID(H, W), mask, m_pitch, H, W);
    hipLaunchKernelGGL(pk_list_kernel, PK_FLAT(n), s, (int)n);       // the components of an earlier call are forgotten
    PkList l = {};
    long E = 0;
    int cur = 0;
    if (form == GHM_PEAKS_LIST) {
        l = pk_list(list, (long)edges);
        E = (long)edges;
        if (E > 0) hipLaunchKernelGGL(pk_fill_kernel, PK_FLAT(n), p, w.eoff, l.list[0]);
    }
    int done = 0;
    for (;;) {
        hipLaunchKernelGGL(pk_clear_kernel, PK_FLAT(s.P), s);
        if (form == GHM_PEAKS_LIST) {
            if (E == 0) break;
            hipLaunchKernelGGL(pk_pick_list_kernel, PK_FLAT(E), p, s, l.list[cur], E, l.alive);
            pk_scan(ctx, l.alive, E, l.sums);
            int64_t left = 0;
            if (int rc = pk_read(ctx, &left, l.sums + pk_blocks(E), sizeof(left))) return rc;
            if (left == 0) break;
            GHM_CHECK(done < max_rounds, "%s: edges are left after %d rounds", who, done);
            hipLaunchKernelGGL(pk_keep_kernel, PK_FLAT(E), l.list[cur], l.alive, E, l.list[cur ^ 1]);
            cur ^= 1;
            E = (long)left;
        } else {
            GHM_HIP(hipMemsetAsync(w.word, 0, sizeof(int), ctx->stream));
            hipLaunchKernelGGL(pk_pick_plain_kernel, PK_FLAT(n), p, s, w.word);
            int found = 0;
            if (int rc = hyd_read_word(ctx, w.word, &found)) return rc;
            if (!found) break;
            GHM_CHECK(done < max_rounds, "%s: edges are left after %d rounds", who, done);
        }
        hipLaunchKernelGGL(pk_hook_kernel, PK_FLAT(s.P), p, s);
        hipLaunchKernelGGL(pk_apply_kernel, PK_FLAT(s.P), s);
        if (int rc = hyd_relax(ctx, who, w.word, PK_JUMP_GROUP, PK_JUMP_CAP, [&](int64_t) {
                hipLaunchKernelGGL(pk_jump_kernel, PK_FLAT(s.P), s, w.word);
            }, nullptr, nullptr))
            return rc;
        ++done;
    }
    // the marked edges per cell and their scan: what ghm_peaks_extract places the rows by
    hipLaunchKernelGGL(pk_marks_kernel, PK_FLAT(n), mask, m_pitch, W, (int)n, w.eoff);
    pk_scan(ctx, w.eoff, n, w.sums);
    if (int rc = pk_read(ctx, &head.T, w.sums + pk_blocks(n), sizeof(int64_t))) return rc;
    GHM_CHECK(head.T == head.P - 1, "%s: %lld edges were marked for %lld summits: the labels are not an ascent's", who,
              (long long)head.T, (long long)head.P);
    head.E = -1;                                 // eoff no longer holds the edges' offsets
    GHM_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    *rounds = done;
    return 0;
}

int ghm_peaks_extract(ghm_ctx* ctx, const int32_t* label, int32_t l_pitch, const uint32_t* area, int32_t a_pitch, const uint32_t* mask,
                      int32_t m_pitch, int32_t H, int32_t W, const void* workspace, int64_t summits, int32_t* summit, uint32_t* area_out,
                      int32_t* tree) {
    const char* who = "ghm_peaks_extract";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(label && area && mask && workspace && summit && area_out && tree, "%s: null pointer", who);
    if (int rc = hyd_check_plane(who, H, W, l_pitch, "label")) return rc;
    if (int rc = hyd_check_plane(who, H, W, a_pitch, "area")) return rc;
    if (int rc = hyd_check_plane(who, H, W, m_pitch, "mask")) return rc;
    const long n = (long)H * W;
    const PkWork w = pk_work(const_cast<void*>(workspace), n);
    PkHeader head = {};
    if (int rc = pk_header(ctx, who, w, H, W, summits, head)) return rc;
    GHM_CHECK(head.T == head.P - 1, "%s: the workspace holds no tree: ghm_peaks_tree comes first", who);
    PkPlane p = {};
    p.label = label, p.H = H, p.W = W, p.pl = l_pitch, p.n = (int)n;
    PkOut o = {};
    o.summit = w.summit, o.area = area, o.toff = w.eoff, o.mask = mask;
    o.pa = a_pitch, o.pm = m_pitch, o.P = (int)head.P;
    o.summit_out = summit, o.area_out = area_out, o.tree = tree;
    hipLaunchKernelGGL(pk_out_summit_kernel, PK_FLAT(o.P), o, W);
    if (head.T > 0) hipLaunchKernelGGL(pk_out_cell_kernel, PK_FLAT(n), p, o);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_peaks_merge(const int32_t* summit, const int32_t* summit_zq, int64_t summits, const int32_t* tree, const int32_t* saddle_zq,
                    int64_t edges, int32_t min_zq, int32_t* col, int32_t* parent, int32_t* prominence_q) {
    const char* who = "ghm_peaks_merge";
    GHM_CHECK(summit && summit_zq && col && parent && prominence_q && (edges == 0 || (tree && saddle_zq)), "%s: null pointer", who);
    GHM_CHECK(summits >= 1 && summits < ((int64_t)1 << 31), "%s: %lld summits (1 <= summits < 2^31)", who, (long long)summits);
    for (int64_t i = 1; i < summits; ++i)
        GHM_CHECK(summit[i - 1] < summit[i], "%s: the summits do not ascend at %lld", who, (long long)i);
    const int rc = pk_merge(summit, summit_zq, summits, tree, saddle_zq, edges, min_zq, col, parent, prominence_q);
    GHM_CHECK(rc != 1, "%s: %lld edges for %lld summits (summits - 1)", who, (long long)edges, (long long)summits);
    GHM_CHECK(rc != 2, "%s: an edge names a label that is no summit", who);
    GHM_CHECK(rc != 3, "%s: the edges are no spanning tree of the summits", who);
    GHM_CHECK(rc != 4, "%s: a prominence is negative or beyond 32 bits: the heights are not the plane's", who);
    return 0;
}

}  // extern "C"
