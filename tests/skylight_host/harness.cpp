// The device code of csrc/skylight.hip and csrc/render.hip compiled for the host (tests/test_skylight_host.py): HIP's
// qualifiers and the few built-ins the kernels use are defined away, a "launch" is a loop over blocks and threads.
// SKY_DEVICE_INC and RENDER_DEVICE_INC are the parts of the two files before their extern "C" entry points.  The tiled form
// of the bake is run phase by phase: every thread of a block stages, then every thread computes.
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
#define __shared__ static
#define HIP_DYNAMIC_SHARED(type, name) static type name[GHM_SKYLIGHT_MAX_LDS / sizeof(type)];
struct Dim3 {
    int x, y, z;
};
static Dim3 threadIdx, blockIdx;
static inline void __syncthreads() {}
static inline int __clz(int v) { return v == 0 ? 32 : __builtin_clz((unsigned)v); }
static inline float __fdiv_rn(float a, float b) { return a / b; }
using std::max;
using std::min;
#include RENDER_DEVICE_INC
#include SKY_DEVICE_INC

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

// bake rows cols pitch y0 x0 h w out_pitch directions steps reach height_scale strength out_u8 in out
// in:  src float32 [rows, pitch], table [directions, steps] of ghm_skylight_sample
// out: the plain form's [h, out_pitch], then the tiled form's (float32 or uint8; cells beyond w keep NaN / 0xAB)
static int bake_main(int argc, char** argv) {
    if (argc != 18) return 2;
    SkyArgs k;
    k.rows = atoi(argv[2]), k.cols = atoi(argv[3]), k.pitch = atoi(argv[4]);
    k.y0 = atoi(argv[5]), k.x0 = atoi(argv[6]), k.h = atoi(argv[7]), k.w = atoi(argv[8]);
    k.out_pitch = atoi(argv[9]);
    k.directions = atoi(argv[10]), k.steps = atoi(argv[11]), k.reach = atoi(argv[12]);
    k.hs = (float)atof(argv[13]), k.strength = (float)atof(argv[14]);
    k.out_u8 = atoi(argv[15]);
    std::vector<char> in;
    const size_t nsrc = (size_t)k.rows * k.pitch * 4, ntab = (size_t)k.directions * k.steps * sizeof(ghm_skylight_sample);
    if (!read_all(argv[16], in) || in.size() != nsrc + ntab) return 3;
    k.src = (const float*)in.data();
    k.table = (const ghm_skylight_sample*)(in.data() + nsrc);
    FILE* fo = fopen(argv[17], "wb");
    if (!fo) return 4;
    const size_t cell = k.out_u8 ? 1 : 4, nout = (size_t)k.h * k.out_pitch;
    const int WW = sky_window(k.reach);
    for (int tiled = 0; tiled < 2; ++tiled) {
        std::vector<char> out(nout * cell);
        if (k.out_u8)
            memset(out.data(), 0xAB, out.size());
        else
            std::fill((float*)out.data(), (float*)out.data() + nout, std::numeric_limits<float>::quiet_NaN());
        k.out = out.data();
        if (!tiled) {
            for (int by = 0; by < (k.h + 3) / 4; ++by)
                for (int bx = 0; bx < (k.w + 63) / 64; ++bx)
                    for (int ty = 0; ty < 4; ++ty)
                        for (int tx = 0; tx < 64; ++tx) {
                            blockIdx.x = bx, blockIdx.y = by, threadIdx.x = tx, threadIdx.y = ty;
                            sky_plain_kernel(k);
                        }
        } else {
            if ((size_t)WW * WW * 4 > GHM_SKYLIGHT_MAX_LDS) return 5;
            std::vector<float> lds((size_t)WW * WW);
            for (int by = 0; by < (k.h + SKY_TILE - 1) / SKY_TILE; ++by)
                for (int bx = 0; bx < (k.w + SKY_TILE - 1) / SKY_TILE; ++bx) {
                    std::fill(lds.begin(), lds.end(), std::numeric_limits<float>::quiet_NaN());
                    for (int t = 0; t < 256; ++t) sky_stage(k, lds.data(), by * SKY_TILE, bx * SKY_TILE, t);
                    for (int t = 0; t < 256; ++t) sky_compute(k, lds.data(), by * SKY_TILE, bx * SKY_TILE, t);
                }
        }
        fwrite(out.data(), 1, out.size(), fo);
    }
    fclose(fo);
    return 0;
}

// view H W Hi Wi step max_dist py px pz yaw pitch fov height_scale sun_az sun_el softness ambient haze shadows in out
// in:  hm [H, W], tex [3, H, W], sky [H, W] float32
// out: image [3, Hi, Wi] of ren_view_kernel, then of ren_view_sky_kernel with the plane, float32 (accel on)
static int view_main(int argc, char** argv) {
    if (argc != 23) return 2;
    char** a = argv + 1;
    const int H = atoi(a[1]), W = atoi(a[2]), Hi = atoi(a[3]), Wi = atoi(a[4]);
    const float step = (float)atof(a[5]), max_dist = (float)atof(a[6]);
    const float pos[3] = {(float)atof(a[7]), (float)atof(a[8]), (float)atof(a[9])};
    const double yaw = atof(a[10]), pitch = atof(a[11]), fov = atof(a[12]);
    const double az = atof(a[14]), el = atof(a[15]);
    std::vector<char> in;
    const size_t n = (size_t)H * W;
    if (!read_all(a[20], in) || in.size() != 5 * n * 4) return 3;
    const float *hm = (const float*)in.data(), *tex = hm + n, *sky = hm + 4 * n;

    RView v = {};
    const int64_t ne = ren_layout(H, W, v.off);
    const int top = ren_levels(H, W);
    std::vector<float> mip((size_t)ne);
    auto launch1 = [&](long total, auto fn) {
        for (long b = 0; b < (total + 255) / 256; ++b)
            for (int t = 0; t < 256; ++t) {
                blockIdx.x = (int)b;
                threadIdx.x = t;
                fn();
            }
    };
    launch1((long)H * W, [&] { ren_mip0_kernel(hm, H, W, mip.data()); });
    for (int l = 1; l <= top; ++l) {
        const int sh = (H + (1 << (l - 1)) - 1) >> (l - 1), sw = (W + (1 << (l - 1)) - 1) >> (l - 1);
        const int dh = (H + (1 << l) - 1) >> l, dw = (W + (1 << l) - 1) >> l;
        launch1((long)dh * dw, [&] { ren_mip_kernel(mip.data() + v.off[l - 1], sh, sw, mip.data() + v.off[l], dh, dw); });
    }
    // ghm_render_view's host part
    const double cy = cos(yaw), sy = sin(yaw), cp = cos(pitch), sp = sin(pitch);
    const double f = 0.5 * Hi / tan(0.5 * fov);
    const double fw[3] = {cp * cy, cp * sy, sp}, rt[3] = {sy, -cy, 0.0}, up[3] = {-sp * cy, -sp * sy, cp};
    const double sun[3] = {cos(el) * cos(az), cos(el) * sin(az), sin(el)};
    const float hor[3] = {0.80f, 0.86f, 0.92f}, zen[3] = {0.30f, 0.50f, 0.85f};
    for (int c = 0; c < 3; ++c) {
        v.o[c] = pos[c];
        v.F[c] = (float)(f * fw[c]);
        v.R[c] = (float)rt[c];
        v.U[c] = (float)up[c];
        v.sun[c] = (float)sun[c];
        v.horizon[c] = hor[c];
        v.zenith[c] = zen[c];
    }
    v.hs = (float)atof(a[13]);
    v.step = step;
    v.max_dist = max_dist;
    v.softness = (float)atof(a[16]);
    v.ambient = (float)atof(a[17]);
    v.haze = (float)atof(a[18]);
    v.H = H;
    v.W = W;
    v.Hi = Hi;
    v.Wi = Wi;
    v.K = (int)floor((double)max_dist / (double)step);
    v.top = top;
    v.shadows = atoi(a[19]);
    v.accel = 1;
    FILE* fo = fopen(a[21], "wb");
    if (!fo) return 4;
    for (int with_sky = 0; with_sky < 2; ++with_sky) {
        std::vector<float> img((size_t)3 * Hi * Wi, -1.0f);
        for (int by = 0; by < (Hi + 15) / 16; ++by)
            for (int bx = 0; bx < (Wi + 15) / 16; ++bx)
                for (int t = 0; t < 256; ++t) {
                    blockIdx.x = bx;
                    blockIdx.y = by;
                    threadIdx.x = t;
                    if (with_sky)
                        ren_view_sky_kernel<8, 8>(v, hm, tex, mip.data(), sky, img.data(), nullptr);
                    else
                        ren_view_kernel<8, 8>(v, hm, tex, mip.data(), img.data(), nullptr);
                }
        fwrite(img.data(), 4, img.size(), fo);
    }
    fclose(fo);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "bake") return bake_main(argc, argv);
    if (mode == "view") return view_main(argc, argv);
    return 2;
}
