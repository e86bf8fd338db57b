// Rivers of a drainage (gan_heightmaps_amd/rivers.py): the stream network as ordered reaches with their Strahler orders,
// Shreve magnitudes and main stems.  Integers throughout, so there are no tolerances; include/ghm.h, section "rivers", has the
// definition and tests/rivers_ref.py restates it cell by cell.
//
// The planes are the hydrology's direction (int8, k = 0 .. 7 = N NE E SE S SW W NW, -1: the water leaves the plane) and accumulation
// (uint32); a cell is a stream cell iff its accumulation reaches the threshold T.
// 1. Count: a thread per cell gathers its eight neighbours' (direction, accumulation), counts the stream cells that flow into it and
//    writes kind; it raises one of three error words for a direction outside [-1, 7], a receiver outside the plane, a stream cell
//    whose receiver has no greater accumulation.  Two exclusive scans number the reach starts and the stream cells; the sources,
//    confluences, mouths and isolated cells are counted per block (__syncthreads_count) and summed by the scan's middle kernel.
//    A gather: no atomics.
// 2. Trace: every stream cell with exactly one inflow points to that donor with distance 1 -- which neighbour it is is read off the
//    neighbourhood --, every other cell to itself with distance 0.  Pointer doubling of (hop, distance) between two buffer pairs
//    (Jacobi) until a round changes nothing; one changed word per round, read once per group of RV_GROUP rounds, as the contour's
//    ranking reads them.  Then every reach's one tail -- the ranked or start cell whose receiver is a confluence, or which is itself a
//    one-inflow mouth -- stores the reach's length and downstream reach with plain stores, and a scan of the lengths gives the
//    offsets.  Two forms, the same bits: plain -- a round is a thread per cell of the plane; list -- the stream cells are compacted
//    once, pointers are list positions, and a round is a thread per entry.  No atomics.
// 3. Extract: every ranked or start cell writes vertex[offsets[reach] + rank]; the tail also writes the end.
// ghm_rivers_order (host, no device): Kahn's algorithm over the reaches, because reach numbers are not topological.
// The scan is a copy of the contour's and the peaks', which are private to their files.
#include <vector>

#include "common.h"
#include "relax.h"

namespace {

constexpr int RV_MAX_ROUNDS = GHM_RIVERS_MAX_ROUNDS;
constexpr int RV_GROUP = 4;                      // doubling rounds per read of the changed words
constexpr int64_t RV_MAGIC = 0x7372657669726776;  // the header of a counted workspace

__device__ __constant__ const int RV_DY[8] = {-1, -1, 0, 1, 1, 1, 0, -1};      // the hydrology's directions: N NE E SE S SW W NW
__device__ __constant__ const int RV_DX[8] = {0, 1, 1, 1, 0, -1, -1, -1};

struct RvPlane {
    const signed char* dir;
    const unsigned* acc;
    int H, W, pd, pa, n;
    unsigned T;
};

// ---- the count ------------------------------------------------------------------------------------------------------------------
// the kind of cell idx; err: bit 0 a direction outside [-1, 7], bit 1 a receiver outside the plane, bit 2 a stream cell whose
// receiver has no greater accumulation
__device__ __forceinline__ int rv_kind_cell(const RvPlane& p, int idx, int& err) {
    const int r = idx / p.W, c = idx - r * p.W;
    const int d = p.dir[(long)r * p.pd + c];
    const unsigned a = p.acc[(long)r * p.pa + c];
    const bool stream = a >= p.T;
    err = 0;
    if (d < -1 || d > 7) {
        err = 1;
    } else if (d >= 0) {
        const int y = r + RV_DY[d], x = c + RV_DX[d];
        if (y < 0 || y >= p.H || x < 0 || x >= p.W)
            err = 2;
        else if (stream && !(p.acc[(long)y * p.pa + x] > a))
            err = 4;
    }
    if (!stream) return 0;
    int in = 0;
    for (int k = 0; k < 8; ++k) {
        const int y = r + RV_DY[k], x = c + RV_DX[k];
        if (y < 0 || y >= p.H || x < 0 || x >= p.W) continue;
        in += (p.acc[(long)y * p.pa + x] >= p.T && p.dir[(long)y * p.pd + x] == ((k + 4) & 7)) ? 1 : 0;
    }
    return GHM_RIVERS_STREAM | (in == 0 ? GHM_RIVERS_SOURCE : 0) | (in >= 2 ? GHM_RIVERS_CONFLUENCE : 0) |
           (d == -1 ? GHM_RIVERS_MOUTH : 0) | (in << 4);
}
// a reach starts at a source or a confluence that is no mouth
__device__ __forceinline__ bool rv_is_start(int kind) {
    return (kind & (GHM_RIVERS_SOURCE | GHM_RIVERS_CONFLUENCE)) != 0 && !(kind & GHM_RIVERS_MOUTH);
}
// bit 0 source, 1 confluence, 2 mouth, 3 isolated: what the blocks count
__device__ __forceinline__ int rv_tally_bits(int kind) {
    const int iso = GHM_RIVERS_SOURCE | GHM_RIVERS_MOUTH;
    return (kind >> 1 & 7) | ((kind & iso) == iso ? 8 : 0);
}
__device__ __forceinline__ int rv_flag_cell(const RvPlane& p, int idx, unsigned char* kind, int pk, int* sflag, int* cflag, int& err) {
    const int k = rv_kind_cell(p, idx, err), r = idx / p.W;
    kind[(long)r * pk + (idx - r * p.W)] = (unsigned char)k;
    sflag[idx] = rv_is_start(k) ? 1 : 0;
    cflag[idx] = k & 1;
    return k;
}
// tally: four rows of ``stride`` block counts; words: the three error words
__global__ __launch_bounds__(256) void rv_flag_kernel(const RvPlane p, unsigned char* kind, int pk, int* sflag, int* cflag, int64_t* tally,
                                                      long stride, int* words) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    int err = 0, k = 0;
    if (idx < p.n) k = rv_flag_cell(p, (int)idx, kind, pk, sflag, cflag, err);
    hyd_raise(err & 1, words);
    hyd_raise(err & 2, words + 1);
    hyd_raise(err & 4, words + 2);
    const int bits = rv_tally_bits(k);
    for (int j = 0; j < 4; ++j) {
        const int count = __syncthreads_count(bits >> j & 1);
        if (threadIdx.x == 0) tally[j * stride + blockIdx.x] = count;
    }
}

// ---- an exclusive scan of n int32 values in place: the blocks' sums, their scan by one block, the write (the contour's) --------
__device__ __forceinline__ int rv_scan_load(const int* in, long n, long block, int tid) {
    const long i = block * 256 + tid;
    return i < n ? in[i] : 0;
}
__device__ __forceinline__ void rv_scan_groups(const int* sm, int64_t* sg, int tid) {
    if (tid >= 16) return;
    int64_t a = 0;
    for (int i = 0; i < 16; ++i) a += sm[16 * tid + i];
    sg[tid] = a;
}
// the sum of the values of the threads before tid (tid = 256: of the block)
__device__ __forceinline__ int64_t rv_scan_before(const int* sm, const int64_t* sg, int tid) {
    int64_t a = 0;
    for (int g = 0; g < (tid >> 4); ++g) a += sg[g];
    for (int i = tid & ~15; i < tid; ++i) a += sm[i];
    return a;
}
__global__ __launch_bounds__(256) void rv_scan_sums_kernel(const int* in, long n, int64_t* sums) {
    __shared__ int sm[256];
    __shared__ int64_t sg[16];
    sm[threadIdx.x] = rv_scan_load(in, n, blockIdx.x, threadIdx.x);
    __syncthreads();
    rv_scan_groups(sm, sg, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = rv_scan_before(sm, sg, 256);
}
__device__ __forceinline__ void rv_scan_chunks(const int64_t* sums, long nb, int64_t* sv, int tid) {
    const long chunk = (nb + 255) / 256, lo = min(tid * chunk, nb), hi = min(lo + chunk, nb);
    int64_t a = 0;
    for (long i = lo; i < hi; ++i) a += sums[i];
    sv[tid] = a;
}
__device__ __forceinline__ void rv_scan_spread(int64_t* sums, long nb, const int64_t* sv, int tid) {
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
__global__ __launch_bounds__(256) void rv_scan_blocks_kernel(int64_t* sums, long nb) {
    __shared__ int64_t sv[256];
    rv_scan_chunks(sums, nb, sv, threadIdx.x);
    __syncthreads();
    rv_scan_spread(sums, nb, sv, threadIdx.x);
}
// out[i] = the sum of the values before i, out[n] = the total; a block has read its values by then
__device__ __forceinline__ void rv_scan_put(long n, const int64_t* sums, int* out, long block, int tid, int own, int64_t before) {
    const long i = block * 256 + tid;
    if (i >= n) return;
    const int64_t at = sums[block] + before;
    out[i] = (int)at;
    if (i == n - 1) out[n] = (int)(at + own);
}
__global__ __launch_bounds__(256) void rv_scan_write_kernel(int* io, long n, const int64_t* sums) {
    __shared__ int sm[256];
    __shared__ int64_t sg[16];
    const int own = rv_scan_load(io, n, blockIdx.x, threadIdx.x);
    sm[threadIdx.x] = own;
    __syncthreads();
    rv_scan_groups(sm, sg, threadIdx.x);
    __syncthreads();
    rv_scan_put(n, sums, io, blockIdx.x, threadIdx.x, own, rv_scan_before(sm, sg, threadIdx.x));
}

// ---- the trace ------------------------------------------------------------------------------------------------------------------
// what the trace and the extraction read of the plane: the directions and the count's kind; ridx, cidx: the scans of the reach
// starts and of the stream cells, n + 1 each
struct RvNet {
    const signed char* dir;
    const unsigned char* kind;
    const int* ridx;
    const int* cidx;
    int H, W, pd, pk, n, R;
};
__device__ __forceinline__ int rv_kind_at(const RvNet& g, int idx) {
    const int r = idx / g.W;
    return g.kind[(long)r * g.pk + (idx - r * g.W)];
}
// the predecessor of cell idx: the one stream cell that flows into a stream cell with one inflow; idx itself for every other cell
__device__ __forceinline__ int rv_pred(const RvNet& g, int idx) {
    const int kind = rv_kind_at(g, idx);
    if (!(kind & GHM_RIVERS_STREAM) || (kind >> 4) != 1) return idx;
    const int r = idx / g.W, c = idx - r * g.W;
    for (int k = 0; k < 8; ++k) {
        const int y = r + RV_DY[k], x = c + RV_DX[k];
        if (y < 0 || y >= g.H || x < 0 || x >= g.W) continue;
        if ((g.kind[(long)y * g.pk + x] & GHM_RIVERS_STREAM) && g.dir[(long)y * g.pd + x] == ((k + 4) & 7)) return y * g.W + x;
    }
    return idx;                                  // a kind that is not the count's
}
__device__ __forceinline__ void rv_init_plain_cell(const RvNet& g, int idx, int* p, int* d) {
    const int from = rv_pred(g, idx);
    p[idx] = from;
    d[idx] = from != idx ? 1 : 0;
}
__global__ __launch_bounds__(256) void rv_init_plain_kernel(const RvNet g, int* p, int* d) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < g.n) rv_init_plain_cell(g, (int)idx, p, d);
}
// the list: entry cidx[idx] is stream cell idx; pointers are entries
__device__ __forceinline__ void rv_init_list_cell(const RvNet& g, int idx, int* cell, int* p, int* d) {
    const int at = g.cidx[idx];
    if (g.cidx[idx + 1] == at) return;
    int from = rv_pred(g, idx);
    if (g.cidx[from + 1] == g.cidx[from]) from = idx;          // a kind that is not the count's: no entry to point to
    cell[at] = idx;
    p[at] = g.cidx[from];
    d[at] = from != idx ? 1 : 0;
}
__global__ __launch_bounds__(256) void rv_init_list_kernel(const RvNet g, int* cell, int* p, int* d) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < g.n) rv_init_list_cell(g, (int)idx, cell, p, d);
}
// a doubling round: p = the cell 2^k back or the terminal, d = the hops to it (the contour's ranking)
__device__ __forceinline__ int rv_rank_item(int s, const int* p0, const int* d0, int* p1, int* d1) {
    const int p = p0[s], pp = p0[p];
    p1[s] = pp;
    d1[s] = d0[s] + d0[p];
    return pp != p;
}
__global__ __launch_bounds__(256) void rv_rank_kernel(long N, const int* p0, const int* d0, int* p1, int* d1, int* word) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    hyd_raise(s < N ? rv_rank_item((int)s, p0, d0, p1, d1) : 0, word);
}
// what cell idx is to its reach: 0 no vertex of its own (no stream cell, an isolated cell, an end that is a confluence); 1 a vertex;
// 2 the tail, and ``end`` is the cell after it; 3 the tail and the end itself (a mouth with one inflow)
__device__ __forceinline__ int rv_member(const RvNet& g, int idx, int& end) {
    const int kind = rv_kind_at(g, idx);
    if (!(kind & GHM_RIVERS_STREAM) || !(rv_is_start(kind) || (kind >> 4) == 1)) return 0;
    end = idx;
    if (kind & GHM_RIVERS_MOUTH) return 3;
    const int r = idx / g.W, c = idx - r * g.W, k = g.dir[(long)r * g.pd + c];
    if (k < 0 || k > 7) return 1;
    const int y = r + RV_DY[k], x = c + RV_DX[k];
    if (y < 0 || y >= g.H || x < 0 || x >= g.W) return 1;
    if (!(g.kind[(long)y * g.pk + x] & GHM_RIVERS_CONFLUENCE)) return 1;
    end = y * g.W + x;
    return 2;
}
// the tail of a reach stores its length and the reach that starts at its end (-1: the end is a mouth); top: the ranked cell's
// terminal, a reach start; rank: its hops to it
__device__ __forceinline__ void rv_tail_cell(const RvNet& g, int idx, int top, int rank, int* rlen, int* rdown) {
    int end;
    const int m = rv_member(g, idx, end);
    if (m < 2) return;
    const int reach = g.ridx[top];
    if (reach >= g.R) return;                    // a kind that is not the count's
    rlen[reach] = rank + (m == 2 ? 2 : 1);
    rdown[reach] = (rv_kind_at(g, end) & GHM_RIVERS_MOUTH) ? -1 : g.ridx[end];
}
__global__ __launch_bounds__(256) void rv_tail_plain_kernel(const RvNet g, const int* p, const int* d, int* rlen, int* rdown) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < g.n) rv_tail_cell(g, (int)idx, p[idx], d[idx], rlen, rdown);
}
__global__ __launch_bounds__(256) void rv_tail_list_kernel(const RvNet g, long N, const int* cell, const int* p, const int* d, int* rlen,
                                                           int* rdown) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < N) rv_tail_cell(g, cell[i], cell[p[i]], d[i], rlen, rdown);
}

// ---- the extraction ---------------------------------------------------------------------------------------------------------------
// roff: the scan of the lengths, R + 1; no vertex is written outside its reach's own range
__device__ __forceinline__ void rv_vertex_cell(const RvNet& g, int idx, int top, int rank, const int* roff, int* vertex) {
    int end;
    const int m = rv_member(g, idx, end);
    if (m == 0) return;
    const int reach = g.ridx[top];
    if (reach >= g.R) return;
    const long at = (long)roff[reach] + rank, hi = roff[reach + 1];
    if (at < hi) vertex[at] = idx;
    if (m == 2 && at + 1 < hi) vertex[at + 1] = end;
}
__global__ __launch_bounds__(256) void rv_vertex_plain_kernel(const RvNet g, const int* p, const int* d, const int* roff, int* vertex) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < g.n) rv_vertex_cell(g, (int)idx, p[idx], d[idx], roff, vertex);
}
__global__ __launch_bounds__(256) void rv_vertex_list_kernel(const RvNet g, long N, const int* cell, const int* p, const int* d,
                                                             const int* roff, int* vertex) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < N) rv_vertex_cell(g, cell[i], cell[p[i]], d[i], roff, vertex);
}
__device__ __forceinline__ void rv_out_reach(long i, long R, const int* roff, const int* rdown, int64_t* offsets, int* downstream) {
    offsets[i] = roff[i];
    if (i < R) downstream[i] = rdown[i];
}
__global__ __launch_bounds__(256) void rv_out_kernel(long R, const int* roff, const int* rdown, int64_t* offsets, int* downstream) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i <= R) rv_out_reach(i, R, roff, rdown, offsets, downstream);
}

// ---- the orders, on the host ------------------------------------------------------------------------------------------------------
// Kahn's algorithm from the reaches without an upstream reach.  0, or 1: an index outside [-1, R); 2: a reach that is its own
// downstream; 3: a cycle
int rv_order(const int32_t* down, const uint32_t* area, int64_t R, int32_t* order, int32_t* magnitude, uint8_t* main_stem) {
    std::vector<int32_t> waiting((size_t)R, 0), top((size_t)R, 0), tops((size_t)R, 0), best((size_t)R, -1), queue;
    std::vector<int64_t> mag((size_t)R, 0);
    for (int64_t r = 0; r < R; ++r) {
        const int32_t d = down[r];
        if (d < -1 || d >= R) return 1;
        if (d == r) return 2;
        if (d < 0) continue;
        ++waiting[(size_t)d];
        if (best[(size_t)d] < 0 || area[r] > area[best[(size_t)d]]) best[(size_t)d] = (int32_t)r;      // ascending r: the lowest number stays
    }
    queue.reserve((size_t)R);
    for (int64_t r = 0; r < R; ++r)
        if (!waiting[(size_t)r]) queue.push_back((int32_t)r);
    for (size_t at = 0; at < queue.size(); ++at) {
        const int32_t r = queue[at], d = down[r];
        const int32_t o = tops[(size_t)r] == 0 ? 1 : top[(size_t)r] + (tops[(size_t)r] >= 2 ? 1 : 0);
        const int64_t m = tops[(size_t)r] == 0 ? 1 : mag[(size_t)r];
        order[r] = o;
        magnitude[r] = (int32_t)(m > 0x7fffffff ? 0x7fffffff : m);
        main_stem[r] = d < 0 || best[(size_t)d] == r ? 1 : 0;
        if (d < 0) continue;
        if (o > top[(size_t)d])
            top[(size_t)d] = o, tops[(size_t)d] = 1;
        else if (o == top[(size_t)d])
            ++tops[(size_t)d];
        mag[(size_t)d] += m;
        if (--waiting[(size_t)d] == 0) queue.push_back(d);
    }
    return (int64_t)queue.size() == R ? 0 : 3;
}

#define RV_FLAT(total) dim3((unsigned)(((long)(total) + 255) / 256)), dim3(256), 0, ctx->stream

}  // namespace

extern "C" {

// ---- the host side: layouts, checks, launches -----------------------------------------------------------------------------------
static long rv_blocks(long n) { return (n + 255) / 256; }
static size_t rv_round(size_t bytes) { return (bytes + 255) / 256 * 256; }

// the workspace: a header (the three error words at byte 128, the rounds' changed words behind them), the blocks' sums, four rows
// of block counts, ridx and cidx (n + 1 each), the plain form's two buffer pairs (n each), rlen (n + 1) and rdown (n)
struct RvHeader {
    int64_t magic, H, W, T, cells, R, V, form, at;
};
struct RvWork {
    RvHeader* head;
    int *errs, *words;
    int64_t *sums, *tally;
    long stride;
    int *ridx, *cidx, *p[2], *d[2], *rlen, *rdown;
};
constexpr size_t RV_HEAD_BYTES = 512;
static RvWork rv_work(void* ws, long n) {
    RvWork w;
    char* at = (char*)ws;
    w.head = (RvHeader*)at;
    w.errs = (int*)(at + 128);
    w.words = (int*)(at + 144);                  // RV_MAX_ROUNDS + 1 of them
    at += RV_HEAD_BYTES;
    w.stride = rv_blocks(n) + 1;
    const size_t row = rv_round(8 * (size_t)w.stride);
    w.sums = (int64_t*)at;
    w.tally = (int64_t*)(at + row);
    at += 5 * row;
    const size_t one = rv_round(4 * (size_t)(n + 1));
    w.ridx = (int*)at, w.cidx = (int*)(at + one);
    w.p[0] = (int*)(at + 2 * one), w.d[0] = (int*)(at + 3 * one), w.p[1] = (int*)(at + 4 * one), w.d[1] = (int*)(at + 5 * one);
    w.rlen = (int*)(at + 6 * one), w.rdown = (int*)(at + 7 * one);
    return w;
}
// the list buffer: the entries' cells and two buffer pairs, ``cells`` each
struct RvList {
    int *cell, *p[2], *d[2];
};
static RvList rv_list(void* buf, long cells) {
    RvList l;
    char* at = (char*)buf;
    const size_t one = rv_round(4 * (size_t)(cells + 1));
    l.cell = (int*)at;
    l.p[0] = (int*)(at + one), l.d[0] = (int*)(at + 2 * one), l.p[1] = (int*)(at + 3 * one), l.d[1] = (int*)(at + 4 * one);
    return l;
}

static void rv_scan(ghm_ctx* ctx, int* io, long n, int64_t* sums) {
    const long nb = rv_blocks(n);
    hipLaunchKernelGGL(rv_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, io, n, sums);
    hipLaunchKernelGGL(rv_scan_blocks_kernel, dim3(1), dim3(256), 0, ctx->stream, sums, nb);
    hipLaunchKernelGGL(rv_scan_write_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, io, n, sums);
}

static int rv_read(ghm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    GHM_LAUNCH_CHECK();
    GHM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int64_t ghm_rivers_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31) || H > 4 * 65535) return -1;
    const long n = (long)H * W;
    return (int64_t)(RV_HEAD_BYTES + 5 * rv_round(8 * (size_t)(rv_blocks(n) + 1)) + 8 * rv_round(4 * (size_t)(n + 1)));
}

int64_t ghm_rivers_list_bytes(int64_t cells) {
    if (cells < 0 || cells >= ((int64_t)1 << 31)) return -1;
    return (int64_t)(5 * rv_round(4 * (size_t)(cells + 1)));
}

int ghm_rivers_count(ghm_ctx* ctx, const int8_t* direction, int32_t d_pitch, const uint32_t* accumulation, int32_t a_pitch, int32_t H,
                     int32_t W, uint32_t threshold, uint8_t* kind, int32_t k_pitch, void* workspace, int64_t* counts) {
    const char* who = "ghm_rivers_count";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(direction && accumulation && kind && workspace && counts, "%s: null pointer", who);
    if (int rc = hyd_check_plane(who, H, W, d_pitch, "direction")) return rc;
    if (int rc = hyd_check_plane(who, H, W, a_pitch, "accumulation")) return rc;
    if (int rc = hyd_check_plane(who, H, W, k_pitch, "kind")) return rc;
    GHM_CHECK(threshold >= 1, "%s: threshold=0 (>= 1)", who);
    RvPlane p;
    p.dir = (const signed char*)direction, p.acc = accumulation;
    p.H = H, p.W = W, p.pd = d_pitch, p.pa = a_pitch, p.n = H * W, p.T = threshold;
    const long n = p.n, nb = rv_blocks(n);
    const RvWork w = rv_work(workspace, n);
    GHM_HIP(hipMemsetAsync(w.head, 0, RV_HEAD_BYTES, ctx->stream));
    hipLaunchKernelGGL(rv_flag_kernel, RV_FLAT(n), p, kind, k_pitch, w.ridx, w.cidx, w.tally, w.stride, w.errs);
    int errs[3] = {};
    if (int rc = rv_read(ctx, errs, w.errs, sizeof(errs))) return rc;
    GHM_CHECK(!errs[0], "%s: a direction outside [-1, 7]", who);
    GHM_CHECK(!errs[1], "%s: a receiver outside the plane", who);
    GHM_CHECK(!errs[2], "%s: the accumulation is not a drainage's: a stream cell's receiver must have a greater accumulation", who);
    RvHeader head = {RV_MAGIC, H, W, (int64_t)threshold, 0, 0, -1, -1, -1};
    rv_scan(ctx, w.ridx, n, w.sums);
    if (int rc = rv_read(ctx, &head.R, w.sums + nb, sizeof(int64_t))) return rc;
    rv_scan(ctx, w.cidx, n, w.sums);
    if (int rc = rv_read(ctx, &head.cells, w.sums + nb, sizeof(int64_t))) return rc;
    int64_t sums[4] = {};
    for (int j = 0; j < 4; ++j) {
        hipLaunchKernelGGL(rv_scan_blocks_kernel, dim3(1), dim3(256), 0, ctx->stream, w.tally + j * w.stride, nb);
        GHM_HIP(hipMemcpyAsync(&sums[j], w.tally + j * w.stride + nb, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    GHM_LAUNCH_CHECK();
    GHM_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    counts[0] = head.cells, counts[1] = head.R;
    for (int j = 0; j < 4; ++j) counts[2 + j] = sums[j];
    return 0;
}

static int rv_header(ghm_ctx* ctx, const char* who, const RvWork& w, int32_t H, int32_t W, int64_t cells, int64_t reaches,
                     RvHeader& head) {
    if (int rc = rv_read(ctx, &head, w.head, sizeof(head))) return rc;
    const bool ok = head.magic == RV_MAGIC;
    GHM_CHECK(ok && head.H == H && head.W == W && head.cells == cells && head.R == reaches,
              "%s: the workspace was counted with %lld cells and %lld reaches on %lld x %lld, the call says %lld and %lld on %d x %d", who,
              (long long)(ok ? head.cells : -1), (long long)(ok ? head.R : -1), (long long)(ok ? head.H : -1),
              (long long)(ok ? head.W : -1), (long long)cells, (long long)reaches, H, W);
    return 0;
}

static RvNet rv_net(const int8_t* direction, int32_t d_pitch, const uint8_t* kind, int32_t k_pitch, int32_t H, int32_t W, const RvWork& w,
                    int64_t R) {
    RvNet g;
    g.dir = (const signed char*)direction, g.kind = kind, g.ridx = w.ridx, g.cidx = w.cidx;
    g.H = H, g.W = W, g.pd = d_pitch, g.pk = k_pitch, g.n = H * W, g.R = (int)R;
    return g;
}

int ghm_rivers_trace(ghm_ctx* ctx, const int8_t* direction, int32_t d_pitch, const uint8_t* kind, int32_t k_pitch, int32_t H, int32_t W,
                     int32_t form, int32_t max_rounds, void* workspace, void* list, int64_t cells, int64_t reaches, int64_t* vertices,
                     int32_t* rounds) {
    const char* who = "ghm_rivers_trace";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(direction && kind && workspace && vertices && rounds, "%s: null pointer", who);
    if (int rc = hyd_check_plane(who, H, W, d_pitch, "direction")) return rc;
    if (int rc = hyd_check_plane(who, H, W, k_pitch, "kind")) return rc;
    GHM_CHECK(form == GHM_RIVERS_PLAIN || form == GHM_RIVERS_LIST, "%s: form=%d (0 plain, 1 list)", who, form);
    GHM_CHECK(max_rounds >= 1 && max_rounds <= RV_MAX_ROUNDS, "%s: max_rounds=%d (1 .. %d)", who, max_rounds, RV_MAX_ROUNDS);
    const long n = (long)H * W;
    const RvWork w = rv_work(workspace, n);
    RvHeader head = {};
    if (int rc = rv_header(ctx, who, w, H, W, cells, reaches, head)) return rc;
    if (form == GHM_RIVERS_LIST) GHM_CHECK(list, "%s: the list form needs the list buffer", who);
    head.V = head.form = head.at = -1;           // what an earlier trace left is forgotten
    GHM_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    const RvNet g = rv_net(direction, d_pitch, kind, k_pitch, H, W, w, head.R);
    const long R = (long)head.R, N = form == GHM_RIVERS_LIST ? (long)head.cells : n;
    RvList l = {};
    int *p[2] = {w.p[0], w.p[1]}, *d[2] = {w.d[0], w.d[1]};
    if (form == GHM_RIVERS_LIST) {
        l = rv_list(list, (long)head.cells);
        p[0] = l.p[0], p[1] = l.p[1], d[0] = l.d[0], d[1] = l.d[1];
        if (N > 0) hipLaunchKernelGGL(rv_init_list_kernel, RV_FLAT(n), g, l.cell, p[0], d[0]);
    } else {
        hipLaunchKernelGGL(rv_init_plain_kernel, RV_FLAT(n), g, p[0], d[0]);
    }
    // doubling rounds in groups until one changes nothing; one more than max_rounds may be issued, the one that shows the rest
    int launched = 0, needed = 1;
    if (N > 0) {
        GHM_HIP(hipMemsetAsync(w.words, 0, 4 * (RV_MAX_ROUNDS + 1), ctx->stream));
        for (needed = 0; !needed;) {
            GHM_CHECK(launched <= max_rounds, "%s: the ranking has not come to rest after %d rounds", who, max_rounds);
            const int group = min(RV_GROUP, max_rounds + 1 - launched);
            for (int i = 0; i < group; ++i, ++launched)
                hipLaunchKernelGGL(rv_rank_kernel, RV_FLAT(N), N, p[launched & 1], d[launched & 1], p[(launched & 1) ^ 1],
                                   d[(launched & 1) ^ 1], w.words + launched);
            int changed[RV_GROUP] = {};
            if (int rc = rv_read(ctx, changed, w.words + launched - group, 4 * (size_t)group)) return rc;
            for (int i = 0; i < group && !needed; ++i)
                if (!changed[i]) needed = launched - group + i + 1;
        }
    }
    const int at = launched & 1;
    int64_t V = 0;
    if (R > 0) {
        GHM_HIP(hipMemsetAsync(w.rlen, 0, 4 * (size_t)(R + 1), ctx->stream));
        GHM_HIP(hipMemsetAsync(w.rdown, 0xff, 4 * (size_t)R, ctx->stream));
        if (form == GHM_RIVERS_LIST)
            hipLaunchKernelGGL(rv_tail_list_kernel, RV_FLAT(N), g, N, l.cell, p[at], d[at], w.rlen, w.rdown);
        else
            hipLaunchKernelGGL(rv_tail_plain_kernel, RV_FLAT(n), g, p[at], d[at], w.rlen, w.rdown);
        rv_scan(ctx, w.rlen, R, w.sums);
        if (int rc = rv_read(ctx, &V, w.sums + rv_blocks(R), sizeof(int64_t))) return rc;
        GHM_CHECK(V >= 2 * (int64_t)R && V < ((int64_t)1 << 31), "%s: %lld vertices for %lld reaches: the kind plane is not the count's",
                  who, (long long)V, (long long)R);
    }
    head.V = V, head.form = form, head.at = at;
    GHM_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    *vertices = V;
    *rounds = needed - 1;
    return 0;
}

int ghm_rivers_extract(ghm_ctx* ctx, const int8_t* direction, int32_t d_pitch, const uint8_t* kind, int32_t k_pitch, int32_t H, int32_t W,
                       const void* workspace, const void* list, int64_t cells, int64_t reaches, int64_t vertices, int32_t* vertex,
                       int64_t* offsets, int32_t* downstream) {
    const char* who = "ghm_rivers_extract";
    if (int rc = hyd_sync_ok(ctx, who)) return rc;
    GHM_CHECK(direction && kind && workspace && offsets && (vertices == 0 || vertex) && (reaches == 0 || downstream), "%s: null pointer",
              who);
    if (int rc = hyd_check_plane(who, H, W, d_pitch, "direction")) return rc;
    if (int rc = hyd_check_plane(who, H, W, k_pitch, "kind")) return rc;
    const long n = (long)H * W;
    const RvWork w = rv_work(const_cast<void*>(workspace), n);
    RvHeader head = {};
    if (int rc = rv_header(ctx, who, w, H, W, cells, reaches, head)) return rc;
    GHM_CHECK(head.V >= 0, "%s: the workspace holds no trace: ghm_rivers_trace comes first", who);
    GHM_CHECK(head.V == vertices, "%s: the workspace was traced with %lld vertices, the call says %lld", who, (long long)head.V,
              (long long)vertices);
    if (head.form == GHM_RIVERS_LIST) GHM_CHECK(list, "%s: the workspace was traced in the list form: the list buffer is needed", who);
    const RvNet g = rv_net(direction, d_pitch, kind, k_pitch, H, W, w, head.R);
    const long R = (long)head.R;
    const int at = (int)head.at;
    if (R > 0) {
        if (head.form == GHM_RIVERS_LIST) {
            const RvList l = rv_list(const_cast<void*>(list), (long)head.cells);
            hipLaunchKernelGGL(rv_vertex_list_kernel, RV_FLAT(head.cells), g, (long)head.cells, l.cell, l.p[at], l.d[at], w.rlen, vertex);
        } else {
            hipLaunchKernelGGL(rv_vertex_plain_kernel, RV_FLAT(n), g, w.p[at], w.d[at], w.rlen, vertex);
        }
        hipLaunchKernelGGL(rv_out_kernel, RV_FLAT(R + 1), R, w.rlen, w.rdown, offsets, downstream);
    } else {
        GHM_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), ctx->stream));
    }
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_rivers_order(const int32_t* downstream, const uint32_t* area, int64_t reaches, int32_t* order, int32_t* magnitude,
                     uint8_t* main_stem) {
    const char* who = "ghm_rivers_order";
    GHM_CHECK(reaches >= 0 && reaches < ((int64_t)1 << 31), "%s: %lld reaches (0 <= reaches < 2^31)", who, (long long)reaches);
    GHM_CHECK(reaches == 0 || (downstream && area && order && magnitude && main_stem), "%s: null pointer", who);
    const int rc = rv_order(downstream, area, reaches, order, magnitude, main_stem);
    GHM_CHECK(rc != 1, "%s: a downstream reach outside [-1, %lld)", who, (long long)reaches);
    GHM_CHECK(rc != 2, "%s: a reach is its own downstream", who);
    GHM_CHECK(rc != 3, "%s: the downstream reaches form a cycle: they are no forest", who);
    return 0;
}

}  // extern "C"
