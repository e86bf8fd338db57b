// The device code of csrc/mesh.hip compiled for the host (tests/test_mesh_host.py): HIP's qualifiers and the few built-ins
// the kernels use are defined away, a "launch" is a loop over blocks and threads.  MESH_DEVICE_INC is the part of the file
// before its extern "C" entry points.  Kernels with barriers are run phase by phase: every thread of a block runs a phase
// before any runs the next.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ghm.h"
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
struct Dim3 {
    unsigned x, y, z;
};
static Dim3 threadIdx, blockIdx;
static inline void __syncthreads() {}
using std::max;
using std::min;
#include MESH_DEVICE_INC

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

static const float NaN = std::numeric_limits<float>::quiet_NaN();

// ghm_mesh_errors' launches; the fused kernel phase by phase
static void errors(MeshErr k, int fused) {
    int s0 = 0;
    if (fused) {
        s0 = std::min(k.k, MESH_FUSED);
        const int nby = (k.rows + MESH_BLOCK - 1) / MESH_BLOCK, nbx = (k.cols + MESH_BLOCK - 1) / MESH_BLOCK;
        std::vector<float> lh(MESH_WIN * MESH_WIN), le(MESH_WIN * MESH_WIN);
        for (int b = 0; b < nby * nbx; ++b) {
            std::fill(lh.begin(), lh.end(), NaN);
            std::fill(le.begin(), le.end(), NaN);
            const int wy0 = b / nbx * MESH_BLOCK - MESH_APRON, wx0 = b % nbx * MESH_BLOCK - MESH_APRON;
            for (int t = 0; t < 256; ++t) mesh_fused_stage(k, lh.data(), le.data(), wy0, wx0, t);
            for (int s = 0; s < s0; ++s)
                for (int centre = 0; centre < 2; ++centre)
                    for (int t = 0; t < 256; ++t) mesh_fused_level(k, lh.data(), le.data(), wy0, wx0, s, centre, t);
            for (int t = 0; t < 256; ++t) mesh_fused_store(k, le.data(), wy0, wx0, s0, t);
        }
    }
    auto launch = [&](long total, auto fn) {
        for (long b = 0; b < (total + 255) / 256; ++b)
            for (int t = 0; t < 256; ++t) {
                blockIdx.x = (unsigned)b, threadIdx.x = (unsigned)t;
                fn();
            }
    };
    for (int s = s0; s < k.k; ++s) {
        const long ny = (k.rows - 1) >> s, nx = (k.cols - 1) >> s;
        launch((ny + 1) * (nx / 2 + 1), [&] { mesh_level_kernel(k, s, 0); });
        launch((ny / 2) * (nx / 2), [&] { mesh_level_kernel(k, s, 1); });
    }
    launch((long)(((k.rows - 1) >> k.k) + 1) * (((k.cols - 1) >> k.k) + 1), [&] { mesh_corners_kernel(k); });
}

// mesh rows cols pitch err_pitch k y0 x0 h w tol in out
// in:  src float32 [rows, pitch]
// out: the plain form's error plane [rows, err_pitch], the fused form's (cells beyond cols keep NaN), then of the mesh of the
//      rectangle at the tolerance: V, F (int64), the index plane int32 [(h + 1)(w + 1)], grid int32 [V, 2], heights float32 [V],
//      triangles uint32 [F, 3]
static int mesh_main(int argc, char** argv) {
    if (argc != 14) return 2;
    MeshErr k;
    k.rows = atoi(argv[2]), k.cols = atoi(argv[3]), k.pitch = atoi(argv[4]), k.err_pitch = atoi(argv[5]), k.k = atoi(argv[6]);
    const int y0 = atoi(argv[7]), x0 = atoi(argv[8]), h = atoi(argv[9]), w = atoi(argv[10]);
    const float tol = (float)atof(argv[11]);
    const int T = 1 << k.k;
    if (k.k < 1 || k.k > GHM_MESH_MAX_TILE_LOG2 || k.rows <= T || k.cols <= T || (k.rows - 1) % T || (k.cols - 1) % T ||
        k.pitch < k.cols || k.err_pitch < k.cols)
        return 2;
    if (y0 < 0 || x0 < 0 || h < T || w < T || y0 % T || x0 % T || h % T || w % T || y0 + h > k.rows - 1 || x0 + w > k.cols - 1)
        return 2;
    std::vector<char> in;
    if (!read_all(argv[12], in) || in.size() != (size_t)k.rows * k.pitch * 4) return 3;
    k.src = (const float*)in.data();
    FILE* fo = fopen(argv[13], "wb");
    if (!fo) return 4;
    std::vector<float> err[2];
    for (int fused = 0; fused < 2; ++fused) {
        err[fused].assign((size_t)k.rows * k.err_pitch, NaN);
        k.err = err[fused].data();
        errors(k, fused);
        fwrite(err[fused].data(), 4, err[fused].size(), fo);
    }
    // ghm_mesh_extract's launches
    MeshExt e;
    e.src = k.src, e.err = err[1].data(), e.pitch = k.pitch, e.err_pitch = k.err_pitch, e.k = k.k;
    e.y0 = y0, e.x0 = x0, e.h = h, e.w = w, e.tol = tol;
    const long nv = (long)(h + 1) * (w + 1);
    e.nblocks = (nv + 255) / 256;
    std::vector<int64_t> sums(2 * (e.nblocks + 1), -1);
    e.sums = sums.data();
    int sm[256], sg[16], own[256], mask[256];
    static int tri[256][4][6];
    for (long b = 0; b < e.nblocks; ++b) {                                // mesh_count_kernel
        for (int t = 0; t < 256; ++t) sm[t] = mesh_ext_own(e, b * 256 + t, tri[t], mask[t]);
        for (int t = 0; t < 256; ++t) mesh_ext_groups(sm, sg, t);
        const int a = mesh_ext_before(sm, sg, 256);
        sums[2 * b] = a & 0xffff, sums[2 * b + 1] = a >> 16;
    }
    {                                                                     // mesh_scan_kernel
        int64_t sv[256], sf[256];
        for (int t = 0; t < 256; ++t) mesh_scan_chunks(sums.data(), e.nblocks, sv, sf, t);
        for (int t = 0; t < 256; ++t) mesh_scan_write(sums.data(), e.nblocks, sv, sf, t);
    }
    const int64_t V = sums[2 * e.nblocks], F = sums[2 * e.nblocks + 1];
    std::vector<int32_t> index((size_t)nv, -7), grid((size_t)2 * V + 1, -7);
    std::vector<float> heights((size_t)V + 1, NaN);
    std::vector<uint32_t> tris((size_t)3 * F + 1, 0xABABABABu);
    e.index = index.data(), e.grid = grid.data(), e.heights = heights.data(), e.tris = tris.data();
    for (int pass = 0; pass < 2; ++pass)                                  // mesh_extract_kernel, twice
        for (long b = 0; b < e.nblocks; ++b) {
            for (int t = 0; t < 256; ++t) sm[t] = own[t] = mesh_ext_own(e, b * 256 + t, tri[t], mask[t]);
            for (int t = 0; t < 256; ++t) mesh_ext_groups(sm, sg, t);
            for (int t = 0; t < 256; ++t) mesh_ext_write(e, b, t, own[t], mesh_ext_before(sm, sg, t), tri[t], mask[t], pass);
        }
    // the cells behind the arrays' ends are untouched
    if (grid[2 * V] != -7 || !(heights[V] != heights[V]) || tris[3 * F] != 0xABABABABu) return 5;
    fwrite(&V, 8, 1, fo);
    fwrite(&F, 8, 1, fo);
    fwrite(index.data(), 4, (size_t)nv, fo);
    fwrite(grid.data(), 4, (size_t)2 * V, fo);
    fwrite(heights.data(), 4, (size_t)V, fo);
    fwrite(tris.data(), 4, (size_t)3 * F, fo);
    fclose(fo);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "mesh") return mesh_main(argc, argv);
    return 2;
}
