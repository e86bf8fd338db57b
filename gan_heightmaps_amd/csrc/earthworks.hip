// Earthworks on a heightfield (gan_heightmaps_amd/earthworks.py): cut river channels and grade roadbeds into the
// ground.  Two steps, each one launch.
//
// 1. The nearest mark -- an exact, bounded Euclidean feature transform, in integers.  A cell c of the uint32 plane ``marks`` is
//    marked iff marks[c] >= threshold (the paint kernel's convention).  For the cell (y, x) and the reach R in [0, 32]:
//      nearest[y, x] = i W + j of the marked cell (i, j) of the plane with |i - y| <= R, |j - x| <= R and
//                      d2 = (i - y)^2 + (j - x)^2 <= R^2 that minimises (d2, i, j) lexicographically, -1 if there is none;
//      dist2[y, x]   = that d2, or -1.
//    Only cells of the plane count: its edge ends the search, and no cell beyond a row's width is read.  Two forms, the same bits:
//      plain : one thread per cell scans its (2R + 1)^2 window of global memory in row-major order and keeps a candidate only on a
//              strictly smaller d2 -- the first of equal d2 in row-major order has the least (i, j);
//      tiled : a 256-thread block owns a 32 x 32 tile.  It stages the marks of its (32 + 2R)^2 window as bytes in LDS (0 outside the
//              plane).  A column pass finds, per window column and tile row, the signed row offset dy of the nearest mark of that
//              column within R rows, the upper one on equal |dy|.  A row pass minimises (dx^2 + dy^2, dy, dx) over the 2R + 1
//              columns of a cell.  Why this equals the plain form: within one column dx is fixed, so the column's least under
//              (d2, i) is its least under (|dy|, i) -- what the column pass keeps -- and the window's least under (d2, i, j) is the
//              representative of its own column; a column has a mark within d2 <= R^2 iff its representative is.  A tile whose
//              window holds no mark writes -1 and runs neither pass.
//    LDS: (32 + 2R)^2 bytes of marks and 32 (32 + 2R) bytes of column offsets, 12288 bytes at R = 32.  The MI355X has 160 KiB of
//    LDS per CU and room for 32 waves, eight blocks of this kernel: 8 x 12 KiB = 96 KiB, so the LDS never limits the occupancy.
//
// 2. The shaping -- float32, each operation rounded on its own (no contraction), no sqrt and no division on the device: positions
//    enter through the host's table of (keep, take) pairs indexed by d2 = 0 .. R^2 alone.
//      untouched (out = h, the same bits): nearest < 0, or take[d2] == 0 (and a nearest or dist2 outside its range);
//      otherwise v = (keep[d2] h) + (take[d2] target[nearest]);  mode 0: out = v;  1 (cut): out = v if v < h else h;
//      2 (fill): out = v if v > h else h.
//    ``target`` is read at marked cells alone (at nearest[c]); elsewhere it may hold anything.  keep = 0 and take = 1 give the
//    target's bits exactly.
#include "common.h"
#include "relax.h"

// the shaping's two products and its sum are rounded one by one (tests/earthworks_ref.py restates them)
#pragma clang fp contract(off)

namespace {

constexpr int EW_TILE = GHM_EARTHWORKS_TILE;
constexpr int EW_MAX_REACH = GHM_EARTHWORKS_MAX_REACH;
constexpr int EW_NONE = GHM_EARTHWORKS_NONE;
constexpr int EW_NO_DY = 127;                          // a window column without a mark within R rows of a tile row

struct EwNear {
    const unsigned* marks;
    int *nearest, *dist2;
    int H, W, pm, pn, pd, R;
    unsigned threshold;
};

// ---- the nearest mark, plain -----------------------------------------------------------------------------------------------
__device__ __forceinline__ void ew_plain_cell(const EwNear& a, int y, int x) {
    const int i0 = max(0, y - a.R), i1 = min(a.H - 1, y + a.R), j0 = max(0, x - a.R), j1 = min(a.W - 1, x + a.R);
    int best = a.R * a.R + 1, at = EW_NONE;
    for (int i = i0; i <= i1; ++i) {
        const unsigned* row = a.marks + (long)i * a.pm;
        const int dy2 = (i - y) * (i - y);
        for (int j = j0; j <= j1; ++j) {
            const int d2 = dy2 + (j - x) * (j - x);
            if (d2 < best && row[j] >= a.threshold) {
                best = d2;
                at = i * a.W + j;
            }
        }
    }
    a.nearest[(long)y * a.pn + x] = at;
    a.dist2[(long)y * a.pd + x] = at == EW_NONE ? EW_NONE : best;
}

__global__ __launch_bounds__(256) void ew_plain_kernel(const EwNear a) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (y < a.H && x < a.W) ew_plain_cell(a, y, x);
}

// ---- the nearest mark, tiled: the phases of a block, thread t of 256; a barrier lies between two phases ------------------------
// the window of the tile at (ty, tx) has n = 32 + 2R rows and columns and starts at (ty - R, tx - R)
__device__ __forceinline__ int ew_stage(const EwNear& a, unsigned char* win, int ty, int tx, int t) {
    const int n = EW_TILE + 2 * a.R;
    int any = 0;
    for (int i = t; i < n * n; i += 256) {
        const int lr = i / n, lc = i - lr * n;
        const int r = ty - a.R + lr, c = tx - a.R + lc;
        const int m = (r >= 0 && r < a.H && c >= 0 && c < a.W) ? a.marks[(long)r * a.pm + c] >= a.threshold : 0;
        win[i] = (unsigned char)m;
        any |= m;
    }
    return any;
}

// col[lc * 32 + tr]: the dy in [-R, R] of the nearest mark of window column lc to tile row tr, the upper on a tie, or EW_NO_DY
__device__ __forceinline__ void ew_columns(const EwNear& a, const unsigned char* win, signed char* col, int t) {
    const int n = EW_TILE + 2 * a.R;
    for (int i = t; i < n * EW_TILE; i += 256) {
        const int lc = i / EW_TILE, tr = i - lc * EW_TILE;
        const int centre = tr + a.R;
        int found = EW_NO_DY;
        for (int d = 0; d <= a.R; ++d) {
            if (win[(centre - d) * n + lc]) {
                found = -d;
                break;
            }
            if (win[(centre + d) * n + lc]) {
                found = d;
                break;
            }
        }
        col[i] = (signed char)found;
    }
}

__device__ __forceinline__ void ew_rows(const EwNear& a, const signed char* col, int ty, int tx, int t) {
    const int tc = t & 31, x = tx + tc;
    for (int tr = t >> 5; tr < EW_TILE; tr += 8) {
        const int y = ty + tr;
        if (y >= a.H || x >= a.W) continue;
        int best = a.R * a.R + 1, bdy = 0, bdx = 0;
        for (int k = 0; k <= 2 * a.R; ++k) {
            const int dy = col[(tc + k) * EW_TILE + tr];
            if (dy == EW_NO_DY) continue;
            const int dx = k - a.R, d2 = dx * dx + dy * dy;
            if (d2 < best || (d2 == best && dy < bdy)) {     // dx ascends: on equal (d2, dy) the first stays
                best = d2;
                bdy = dy;
                bdx = dx;
            }
        }
        const bool hit = best <= a.R * a.R;
        a.nearest[(long)y * a.pn + x] = hit ? (y + bdy) * a.W + (x + bdx) : EW_NONE;
        a.dist2[(long)y * a.pd + x] = hit ? best : EW_NONE;
    }
}

__device__ __forceinline__ void ew_none(const EwNear& a, int ty, int tx, int t) {
    const int x = tx + (t & 31);
    for (int tr = t >> 5; tr < EW_TILE; tr += 8) {
        const int y = ty + tr;
        if (y >= a.H || x >= a.W) continue;
        a.nearest[(long)y * a.pn + x] = EW_NONE;
        a.dist2[(long)y * a.pd + x] = EW_NONE;
    }
}

__host__ __device__ constexpr int ew_window_bytes(int R) { return ((EW_TILE + 2 * R) * (EW_TILE + 2 * R) + 15) / 16 * 16; }

__global__ __launch_bounds__(256) void ew_tiled_kernel(const EwNear a) {
    extern __shared__ unsigned char ew_lds[];
    unsigned char* win = ew_lds;
    signed char* col = (signed char*)(ew_lds + ew_window_bytes(a.R));
    const int t = threadIdx.x, ty = blockIdx.y * EW_TILE, tx = blockIdx.x * EW_TILE;
    const int any = __syncthreads_or(ew_stage(a, win, ty, tx, t));
#ifndef GHM_EARTHWORKS_NO_SKIP /* a tuning build measures what the skip is worth (GHM_BUILD_DEFINES, csrc/build.py): the same bits */
    if (!any) {
        ew_none(a, ty, tx, t);
        return;
    }
#endif
    ew_columns(a, win, col, t);
    __syncthreads();
    ew_rows(a, col, ty, tx, t);
}

// ---- the shaping -----------------------------------------------------------------------------------------------------------
struct EwShape {
    const float *h, *target, *table;
    const int *nearest, *dist2;
    float* out;
    int H, W, ph, pn, pd, pt, po, R, mode;
};

__device__ __forceinline__ void ew_shape_cell(const EwShape& a, int y, int x) {
    const float h = a.h[(long)y * a.ph + x];
    const int at = a.nearest[(long)y * a.pn + x], d2 = a.dist2[(long)y * a.pd + x];
    float out = h;
    if (at >= 0 && at < a.H * a.W && d2 >= 0 && d2 <= a.R * a.R) {
        const float keep = a.table[2 * d2], take = a.table[2 * d2 + 1];
        if (take != 0.0f) {
            const int i = at / a.W, j = at - i * a.W;
            const float kh = keep * h;
            const float tt = take * a.target[(long)i * a.pt + j];
            const float v = kh + tt;
            out = a.mode == 0 ? v : a.mode == 1 ? (v < h ? v : h) : (v > h ? v : h);
        }
    }
    a.out[(long)y * a.po + x] = out;
}

__global__ __launch_bounds__(256) void ew_shape_kernel(const EwShape a) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (y < a.H && x < a.W) ew_shape_cell(a, y, x);
}

}  // namespace

extern "C" {

int64_t ghm_earthworks_lds_bytes(int32_t reach) {
    if (reach < 0 || reach > EW_MAX_REACH) return -1;
    return (int64_t)ew_window_bytes(reach) + (int64_t)EW_TILE * (EW_TILE + 2 * reach);
}

int ghm_earthworks_nearest(ghm_ctx* ctx, const uint32_t* marks, int32_t m_pitch, int32_t H, int32_t W, uint32_t threshold,
                           int32_t reach, int32_t tiled, int32_t* nearest, int32_t n_pitch, int32_t* dist2, int32_t d_pitch) {
    GHM_CHECK(ctx && marks && nearest && dist2, "ghm_earthworks_nearest: null pointer");
    if (int rc = hyd_check_plane("ghm_earthworks_nearest", H, W, m_pitch, "marks")) return rc;
    if (int rc = hyd_check_plane("ghm_earthworks_nearest", H, W, n_pitch, "nearest")) return rc;
    if (int rc = hyd_check_plane("ghm_earthworks_nearest", H, W, d_pitch, "dist2")) return rc;
    GHM_CHECK(reach >= 0 && reach <= EW_MAX_REACH, "ghm_earthworks_nearest: reach=%d (0 .. %d)", reach, EW_MAX_REACH);
    GHM_CHECK(threshold >= 1u, "ghm_earthworks_nearest: threshold=0 would mark every cell (>= 1)");
    EwNear a;
    a.marks = marks;
    a.nearest = nearest;
    a.dist2 = dist2;
    a.H = H;
    a.W = W;
    a.pm = m_pitch;
    a.pn = n_pitch;
    a.pd = d_pitch;
    a.R = reach;
    a.threshold = threshold;
    if (tiled)
        hipLaunchKernelGGL(ew_tiled_kernel, dim3(ceil_div(W, EW_TILE), ceil_div(H, EW_TILE)), dim3(256),
                           (size_t)ghm_earthworks_lds_bytes(reach), ctx->stream, a);
    else
        hipLaunchKernelGGL(ew_plain_kernel, dim3(ceil_div(W, 64), ceil_div(H, 4)), dim3(64, 4), 0, ctx->stream, a);
    GHM_LAUNCH_CHECK();
    return 0;
}

int ghm_earthworks_shape(ghm_ctx* ctx, const float* h, int32_t h_pitch, const int32_t* nearest, int32_t n_pitch, const int32_t* dist2,
                         int32_t d_pitch, const float* target, int32_t t_pitch, const float* table, int32_t reach, int32_t mode,
                         int32_t H, int32_t W, float* out, int32_t o_pitch) {
    GHM_CHECK(ctx && h && nearest && dist2 && target && table && out, "ghm_earthworks_shape: null pointer");
    if (int rc = hyd_check_plane("ghm_earthworks_shape", H, W, h_pitch, "h")) return rc;
    if (int rc = hyd_check_plane("ghm_earthworks_shape", H, W, n_pitch, "nearest")) return rc;
    if (int rc = hyd_check_plane("ghm_earthworks_shape", H, W, d_pitch, "dist2")) return rc;
    if (int rc = hyd_check_plane("ghm_earthworks_shape", H, W, t_pitch, "target")) return rc;
    if (int rc = hyd_check_plane("ghm_earthworks_shape", H, W, o_pitch, "out")) return rc;
    GHM_CHECK(reach >= 0 && reach <= EW_MAX_REACH, "ghm_earthworks_shape: reach=%d (0 .. %d)", reach, EW_MAX_REACH);
    GHM_CHECK(mode >= 0 && mode <= 2, "ghm_earthworks_shape: mode=%d (0 both, 1 cut, 2 fill)", mode);
    EwShape a;
    a.h = h;
    a.target = target;
    a.table = table;
    a.nearest = nearest;
    a.dist2 = dist2;
    a.out = out;
    a.H = H;
    a.W = W;
    a.ph = h_pitch;
    a.pn = n_pitch;
    a.pd = d_pitch;
    a.pt = t_pitch;
    a.po = o_pitch;
    a.R = reach;
    a.mode = mode;
    hipLaunchKernelGGL(ew_shape_kernel, dim3(ceil_div(W, 64), ceil_div(H, 4)), dim3(64, 4), 0, ctx->stream, a);
    GHM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
