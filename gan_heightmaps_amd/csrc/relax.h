// What the monotone relaxations share (hydrology.hip; route.hip): the one device word a block raises
// when it changed a cell, the checks of a plane, and the host loop that issues sweeps in groups and reads that word once per
// group.  The names are those of their first user.  Internal: included by those two files, by scatter.hip, whose
// thinning is a relaxation of the same kind, and by earthworks.hip for the checks of a plane, after common.h.
#pragma once
#include "common.h"

namespace {

// one store per block that changed anything; every thread of the block arrives here
__device__ __forceinline__ void hyd_raise(int changed, int* word) {
    const int any = __syncthreads_or(changed);
    if (any && threadIdx.x == 0 && threadIdx.y == 0) *word = 1;
}

int hyd_check_plane(const char* who, int H, int W, int pitch, const char* what) {
    GHM_CHECK(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31) && H <= 4 * 65535,
              "%s: a plane of %d x %d is out of range (H W < 2^31, H <= 262140)", who, H, W);
    GHM_CHECK(pitch >= W && (int64_t)H * pitch < ((int64_t)1 << 31), "%s: the pitch of %s, %d, is out of range for %d x %d", who,
              what, pitch, H, W);
    return 0;
}

int hyd_sync_ok(ghm_ctx* ctx, const char* who) {
    GHM_CHECK(ctx != nullptr, "%s: null context", who);
    GHM_CHECK(!ctx->rec && !ctx->capturing, "%s waits for the device: it cannot be recorded or captured", who);
    return 0;
}

int hyd_read_word(ghm_ctx* ctx, const int* word, int* value) {
    GHM_LAUNCH_CHECK();
    GHM_HIP(hipMemcpyAsync(value, word, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GHM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// groups of sweeps until one group changes nothing; sweep(i) issues sweep number i.  last_alone: sweep number ``cap`` goes out in
// a group of its own, for a relaxation whose sweep ``cap`` is the first that is sure to change nothing -- in a group with
// earlier sweeps it would be reported as a change, and the cap would refuse a plane that did converge
template <class Sweep>
int hyd_relax(ghm_ctx* ctx, const char* who, int* word, int group, int64_t cap, Sweep sweep, int64_t* sweeps, int32_t* changed,
              bool last_alone = false) {
    int64_t done = 0;
    int any = 0;
    for (;;) {
        GHM_CHECK(done < cap, "%s: no fixed point within the hard cap of %lld sweeps", who, (long long)cap);
        GHM_HIP(hipMemsetAsync(word, 0, sizeof(int), ctx->stream));
        const int64_t left = cap - done - (last_alone && cap - done > 1 ? 1 : 0);
        const int64_t n = left < group ? left : group;
        for (int64_t i = 0; i < n; ++i) sweep(done + i);
        int w = 0;
        if (int rc = hyd_read_word(ctx, word, &w)) return rc;
        done += n;
        if (!w) break;
        any = 1;
    }
    if (sweeps) *sweeps = done;
    if (changed) *changed = any;
    return 0;
}

}  // namespace
