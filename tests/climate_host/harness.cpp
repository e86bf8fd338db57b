// The transport kernels of csrc/climate.hip compiled for the host (tests/test_climate_host.py): HIP's qualifiers are defined away, a
// block is a set of host threads, one per lane, __syncthreads is a barrier between them and __shared__ memory is a static array, so
// the staged form's three waves that move tiles and the one that runs the recurrence overlap here as they do on the device.  Blocks
// run one after the other.  CLIMATE_DEVICE_INC is the part of the file in front of its launch macro.  The heights come in rows of
// W + 3 cells, raw goes out in rows of W + 3 cells that start as 0xAB bytes, and both buffers have exactly that size, so that an index
// past one is an error of its own under the sanitizers.
//   harness H W wind form sea_q hum_q evap_q base_q up_q rec_q IN OUT
#include <pthread.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ghm.h"
#define __host__
#define __device__
#define __global__
#define __shared__ static
#define __constant__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
struct Dim3 {
    unsigned x, y, z;
};
static thread_local Dim3 threadIdx;
static Dim3 blockIdx;
static pthread_barrier_t g_barrier;
#define __syncthreads() pthread_barrier_wait(&g_barrier)
using std::max;
using std::min;
static inline void hyd_raise(int, int*) {}
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) {
    const unsigned long long old = *p;
    *p = old + v;
    return old;
}
#include CLIMATE_DEVICE_INC

struct Lane {
    void (*kernel)(const Transport);
    const Transport* k;
    unsigned x;
};

static void* run_lane(void* p) {
    const Lane* lane = (const Lane*)p;
    threadIdx.x = lane->x;
    threadIdx.y = threadIdx.z = 0;
    lane->kernel(*lane->k);
    return nullptr;
}

static int launch(void (*kernel)(const Transport), const Transport& k, unsigned grid, unsigned block) {
    std::vector<pthread_t> threads(block);
    std::vector<Lane> lanes(block);
    for (unsigned b = 0; b < grid; ++b) {
        blockIdx.x = b;
        blockIdx.y = blockIdx.z = 0;
        if (pthread_barrier_init(&g_barrier, nullptr, block)) return 4;
        for (unsigned t = 0; t < block; ++t) {
            lanes[t] = {kernel, &k, t};
            if (pthread_create(&threads[t], nullptr, run_lane, &lanes[t])) return 5;
        }
        for (unsigned t = 0; t < block; ++t) pthread_join(threads[t], nullptr);
        pthread_barrier_destroy(&g_barrier);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 13) return 2;
    const int H = atoi(argv[1]), W = atoi(argv[2]), wind = atoi(argv[3]), form = atoi(argv[4]);
    if (H < 1 || W < 1 || wind < 0 || wind > 7) return 2;
    std::vector<int> zq((size_t)H * (W + 3));
    std::vector<unsigned> raw((size_t)H * (W + 3), 0xABABABABu);
    FILE* f = fopen(argv[11], "rb");
    if (!f || fread(zq.data(), sizeof(int), zq.size(), f) != zq.size()) return 3;
    fclose(f);
    Transport k;
    k.zq = zq.data();
    k.raw = raw.data();
    k.H = H;
    k.W = W;
    k.pz = k.pr = W + 3;
    k.flipy = CLM_DY[wind] > 0;
    k.flipx = CLM_DX[wind] > 0;
    k.sea_q = atoi(argv[5]);
    k.hum_q = (unsigned)atoi(argv[6]);
    k.evap_q = (unsigned)atoi(argv[7]);
    k.base_q = (unsigned)atoi(argv[8]);
    k.up_q = (unsigned)atoi(argv[9]);
    k.rec_q = (unsigned)atoi(argv[10]);
    const int kind = CLM_DY[wind] == 0 ? 0 : CLM_DX[wind] == 0 ? 1 : 2;
    const long lines = kind == 0 ? H : kind == 1 ? W : (long)H + W - 1;
    const unsigned grid = (unsigned)((lines + CLM_LINES - 1) / CLM_LINES);
    void (*const line[3])(const Transport) = {clm_line_kernel<0>, clm_line_kernel<1>, clm_line_kernel<2>};
    void (*const staged[3])(const Transport) = {clm_staged_kernel<0>, clm_staged_kernel<1>, clm_staged_kernel<2>};
    if (int rc = form ? launch(staged[kind], k, grid, 256) : launch(line[kind], k, grid, CLM_LINES)) return rc;
    f = fopen(argv[12], "wb");
    if (!f || fwrite(raw.data(), sizeof(unsigned), raw.size(), f) != raw.size()) return 3;
    fclose(f);
    return 0;
}
