// The device code of csrc/render.hip compiled for the host (tests/test_render_host.py): HIP's qualifiers and the few
// built-ins the kernels use are defined away, a "launch" is a loop over blocks and threads.  RENDER_DEVICE_INC is the part
// of render.hip before its extern "C" entry points.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct Dim3 {
    int x, y, z;
};
static Dim3 threadIdx, blockIdx;
static inline void __syncthreads() {}
static inline int __clz(int v) { return v == 0 ? 32 : __builtin_clz((unsigned)v); }
using std::max;
using std::min;
#include RENDER_DEVICE_INC

// argv: H W Hi Wi step max_dist py px pz yaw pitch fov height_scale sun_az sun_el softness ambient haze shadows in out
// in:  hm [H, W], tex [3, H, W] float32;  out: for accel = 0 then 1: image [3, Hi, Wi], depth [Hi, Wi] float32
int main(int argc, char** argv) {
    if (argc != 22) return 2;
    const int H = atoi(argv[1]), W = atoi(argv[2]), Hi = atoi(argv[3]), Wi = atoi(argv[4]);
    const float step = (float)atof(argv[5]), max_dist = (float)atof(argv[6]);
    const float pos[3] = {(float)atof(argv[7]), (float)atof(argv[8]), (float)atof(argv[9])};
    const double yaw = atof(argv[10]), pitch = atof(argv[11]), fov = atof(argv[12]);
    const double az = atof(argv[14]), el = atof(argv[15]);
    std::vector<float> hm((size_t)H * W), tex((size_t)3 * H * W);
    FILE* fi = fopen(argv[20], "rb");
    if (!fi || fread(hm.data(), 4, hm.size(), fi) != hm.size() || fread(tex.data(), 4, tex.size(), fi) != tex.size()) return 3;
    fclose(fi);

    RView v = {};
    const int64_t n = ren_layout(H, W, v.off);
    const int top = ren_levels(H, W);
    std::vector<float> mip((size_t)n);
    auto launch1 = [&](long total, auto fn) {
        for (long b = 0; b < (total + 255) / 256; ++b)
            for (int t = 0; t < 256; ++t) {
                blockIdx.x = (int)b;
                threadIdx.x = t;
                fn();
            }
    };
    launch1((long)H * W, [&] { ren_mip0_kernel(hm.data(), H, W, mip.data()); });
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
    v.hs = (float)atof(argv[13]);
    v.step = step;
    v.max_dist = max_dist;
    v.softness = (float)atof(argv[16]);
    v.ambient = (float)atof(argv[17]);
    v.haze = (float)atof(argv[18]);
    v.H = H;
    v.W = W;
    v.Hi = Hi;
    v.Wi = Wi;
    v.K = (int)floor((double)max_dist / (double)step);
    v.top = top;
    v.shadows = atoi(argv[19]);
    FILE* fo = fopen(argv[21], "wb");
    if (!fo) return 4;
    for (int accel = 0; accel < 2; ++accel) {
        v.accel = accel;
        std::vector<float> img((size_t)3 * Hi * Wi, -1.0f), dep((size_t)Hi * Wi, -1.0f);
        for (int by = 0; by < (Hi + 15) / 16; ++by)
            for (int bx = 0; bx < (Wi + 15) / 16; ++bx)
                for (int t = 0; t < 256; ++t) {
                    blockIdx.x = bx;
                    blockIdx.y = by;
                    threadIdx.x = t;
                    ren_view_kernel<8, 8>(v, hm.data(), tex.data(), mip.data(), img.data(), dep.data());
                }
        fwrite(img.data(), 4, img.size(), fo);
        fwrite(dep.data(), 4, dep.size(), fo);
    }
    fclose(fo);
    return 0;
}
