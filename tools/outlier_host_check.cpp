// Host-only driver of the argument checks and workspace arithmetic of hpl_outlier_filter, for a sanitizer build: no device is
// needed, every call returns before a launch (a refusal, or N = 0).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/outlier_host_check.cpp hplflownet_amd/csrc/outlier_filter.hip -o /tmp/outlier_host_check && /tmp/outlier_host_check
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/hpl_bcl.h"

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links outlier_filter.hip alone)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace hpl

static int failures = 0;

static void expect(bool ok, const char *what) {
    if (!ok) {
        ++failures;
        printf("FAILED: %s (last error: %s)\n", what, hpl::g_err);
    }
}

struct Call {
    uintptr_t pc = 0x10000, keep = 0x20000, keep_idx = 0x30000, mean_dist = 0x40000, count = 0x50000, nbr_d2 = 0x60000,
              thresh = 0x70000, stats = 0x80000, ws = 0x100000;
    int64_t pc_ld = 100, ws_bytes = (int64_t)1 << 24;
    int batch = 1, mode = 0, k = 16, min_neighbors = 0;
    float radius = 1.f, std_ratio = 2.f;
    int64_t prefix[66] = {0, 100};
    bool null_prefix = false;
    static Call radius_mode() {
        Call c;
        c.mode = 1; c.min_neighbors = 2; c.mean_dist = c.nbr_d2 = 0; c.k = 0;
        return c;
    }
    int run() const {
        return hpl_outlier_filter((const float *)pc, pc_ld, batch, null_prefix ? nullptr : prefix, mode, k, radius, std_ratio,
                                  min_neighbors, (uint8_t *)keep, (int32_t *)keep_idx, (float *)mean_dist, (int32_t *)count,
                                  (float *)nbr_d2, (float *)thresh, (int32_t *)stats, (void *)ws, ws_bytes, nullptr);
    }
};

int main() {
    // workspace arithmetic: in range, monotone in the count and the batch, hpl_normals' grid and two words a point, -1 outside
    const int64_t ns[] = {0, 1, 3, 255, 256, 257, 1023, 1024, 1025, 8192, 8193, 100191, 131072, 450000, (int64_t)1 << 27};
    for (int b : {1, 2, 16, 63, 64}) {
        int64_t prev = 0;
        for (int64_t n : ns) {
            const int64_t v = hpl_outlier_filter_workspace_bytes(b, n);
            expect(v > 0 && v % 256 == 0 && v >= prev, "workspace bytes monotone in the count");
            expect(v >= hpl_outlier_filter_workspace_bytes(1, n), "workspace bytes monotone in the batch");
            expect(v >= 56 * n + 32 * (n / 1024 + b), "workspace bytes hold keys, records, mean, count and the partials");
            prev = v;
        }
    }
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    expect(hpl_outlier_filter_workspace_bytes(0, 1) == -1 && hpl_outlier_filter_workspace_bytes(65, 1) == -1 &&
               hpl_outlier_filter_workspace_bytes(-1, 1) == -1 && hpl_outlier_filter_workspace_bytes(1, -1) == -1 &&
               hpl_outlier_filter_workspace_bytes(1, big) == -1 && hpl_outlier_filter_workspace_bytes(1, (int64_t)1 << 60) == -1 &&
               hpl_outlier_filter_workspace_bytes(64, big - 1) > 0,
           "workspace bytes out of range");

    // refusals, each before any launch, each naming the op
    auto refuse = [](Call c, const char *what) {
        hpl::g_err[0] = 0;
        expect(c.run() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_outlier_filter", 18) == 0, what);
    };
    { Call c; c.batch = 0; refuse(c, "batch 0"); }
    { Call c; c.batch = 65; refuse(c, "batch 65"); }
    { Call c; c.batch = -1; refuse(c, "batch -1"); }
    { Call c; c.mode = 2; refuse(c, "mode 2"); }
    { Call c; c.mode = -1; refuse(c, "mode -1"); }
    { Call c; c.k = 0; refuse(c, "k 0"); }
    { Call c; c.k = 33; refuse(c, "k 33"); }
    { Call c; c.k = -1; refuse(c, "k -1"); }
    for (int mode = 0; mode < 2; ++mode) {
        const Call base = mode ? Call::radius_mode() : Call();
        { Call c = base; c.radius = 0.f; refuse(c, "radius 0"); }
        { Call c = base; c.radius = -1.f; refuse(c, "negative radius"); }
        { Call c = base; c.radius = INFINITY; refuse(c, "infinite radius"); }
        { Call c = base; c.radius = NAN; refuse(c, "NaN radius"); }
        { Call c = base; c.null_prefix = true; refuse(c, "null prefix"); }
        { Call c = base; c.prefix[0] = 1; refuse(c, "prefix from 1"); }
        { Call c = base; c.batch = 2; c.prefix[1] = 60; c.prefix[2] = 50; refuse(c, "prefix decreases"); }
        { Call c = base; c.pc_ld = 99; refuse(c, "pc_ld"); }
        { Call c = base; c.pc = 0; refuse(c, "null pc"); }
        { Call c = base; c.thresh = 0; refuse(c, "null thresh"); }
        { Call c = base; c.stats = 0; refuse(c, "null stats"); }
        { Call c = base; c.ws = 0; refuse(c, "null workspace"); }
        { Call c = base; c.pc += 2; refuse(c, "misaligned pc"); }
        { Call c = base; c.keep_idx += 1; refuse(c, "misaligned keep_idx"); }
        { Call c = base; c.count += 2; refuse(c, "misaligned count"); }
        { Call c = base; c.thresh += 3; refuse(c, "misaligned thresh"); }
        { Call c = base; c.stats += 1; refuse(c, "misaligned stats"); }
        { Call c = base; c.ws += 128; refuse(c, "misaligned workspace"); }
        { Call c = base; c.ws_bytes = 0; refuse(c, "no workspace"); }
        { Call c = base; c.ws_bytes = hpl_outlier_filter_workspace_bytes(1, 100) - 1; refuse(c, "short workspace"); }
        { Call c = base; c.prefix[1] = big; c.pc_ld = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50; refuse(c, "N >= 2^31 / 3"); }
        { Call c = base; c.prefix[1] = (int64_t)1 << 60; c.pc_ld = (int64_t)1 << 60; c.ws_bytes = (int64_t)1 << 62; refuse(c, "N = 2^60"); }
        // an output inside the input, the workspace or another output
        { Call c = base; c.keep = c.pc; refuse(c, "keep on pc"); }
        { Call c = base; c.keep = c.pc + 1199; refuse(c, "keep on the last byte of pc"); }
        { Call c = base; c.keep = c.pc - 99; refuse(c, "the last byte of keep on pc"); }
        { Call c = base; c.keep_idx = c.pc + 400; refuse(c, "keep_idx in pc"); }
        { Call c = base; c.count = c.pc - 396; refuse(c, "the last element of count on pc"); }
        { Call c = base; c.thresh = c.pc + 1196; refuse(c, "thresh on the last element of pc"); }
        { Call c = base; c.stats = c.pc - 12; refuse(c, "the last element of stats on pc"); }
        { Call c = base; c.keep = c.ws; refuse(c, "keep on the workspace"); }
        { Call c = base; c.keep_idx = c.ws + 256; refuse(c, "keep_idx in the workspace"); }
        { Call c = base; c.count = c.ws - 396; refuse(c, "the last element of count on the workspace"); }
        { Call c = base; c.thresh = c.ws + (uintptr_t)hpl_outlier_filter_workspace_bytes(1, 100) - 4; refuse(c, "thresh on the workspace's last word"); }
        { Call c = base; c.stats = c.ws + 1024; refuse(c, "stats in the workspace"); }
        { Call c = base; c.keep = c.keep_idx + 399; refuse(c, "keep on the last byte of keep_idx"); }
        { Call c = base; c.count = c.keep_idx; refuse(c, "count on keep_idx"); }
        { Call c = base; c.stats = c.thresh + 12; refuse(c, "stats on the last element of thresh"); }
        { Call c = base; c.thresh = c.count + 396; refuse(c, "thresh on the last element of count"); }
        { Call c = base; c.stats = c.keep + 96; refuse(c, "stats on the last bytes of keep"); }
    }
    { Call c; c.std_ratio = -1e-6f; refuse(c, "negative std_ratio"); }
    { Call c; c.std_ratio = INFINITY; refuse(c, "infinite std_ratio"); }
    { Call c; c.std_ratio = NAN; refuse(c, "NaN std_ratio"); }
    { Call c; c.mean_dist += 2; refuse(c, "misaligned mean_dist"); }
    { Call c; c.nbr_d2 += 1; refuse(c, "misaligned nbr_d2"); }
    { Call c; c.mean_dist = c.pc + 800; refuse(c, "mean_dist in pc"); }
    { Call c; c.nbr_d2 = c.pc - 4 * 1599; refuse(c, "the last element of nbr_d2 on pc"); }
    { Call c; c.mean_dist = c.ws + 512; refuse(c, "mean_dist in the workspace"); }
    { Call c; c.nbr_d2 = c.ws - 4; refuse(c, "nbr_d2 over the workspace"); }
    { Call c; c.nbr_d2 = c.mean_dist + 396; refuse(c, "nbr_d2 on the last element of mean_dist"); }
    { Call c; c.mean_dist = c.count; refuse(c, "mean_dist on count"); }
    { Call c; c.prefix[1] = (int64_t)1 << 27; c.pc_ld = (int64_t)1 << 27; c.ws = (uintptr_t)1 << 50; c.ws_bytes = (int64_t)1 << 50;
      refuse(c, "N k = 2^31 with nbr_d2"); }
    { Call c = Call::radius_mode(); c.min_neighbors = 0; refuse(c, "min_neighbors 0"); }
    { Call c = Call::radius_mode(); c.min_neighbors = -7; refuse(c, "min_neighbors -7"); }
    { Call c = Call::radius_mode(); c.mean_dist = 0x40000; refuse(c, "mean_dist in the radius mode"); }
    { Call c = Call::radius_mode(); c.nbr_d2 = 0x60000; refuse(c, "nbr_d2 in the radius mode"); }
    // optional arrays left out, an exact workspace, arrays that merely touch and empty batches are accepted: N = 0 returns
    // before any launch
    { Call c; c.prefix[1] = 0; expect(c.run() == HPL_OK, "N = 0"); }
    { Call c; c.prefix[1] = 0; c.ws_bytes = hpl_outlier_filter_workspace_bytes(1, 0); expect(c.run() == HPL_OK, "N = 0, exact workspace"); }
    { Call c; c.prefix[1] = 0; c.pc_ld = 0; c.keep = c.keep_idx = c.mean_dist = c.count = c.nbr_d2 = 0; c.k = 1; c.radius = 1e-30f;
      c.std_ratio = 0.f; expect(c.run() == HPL_OK, "N = 0, no optional array"); }
    { Call c; c.prefix[1] = 0; c.keep = c.pc; c.nbr_d2 = c.ws; c.count = c.keep_idx; expect(c.run() == HPL_OK, "N = 0: nothing to overlap"); }
    { Call c; c.batch = 64; for (int b = 0; b <= 64; ++b) c.prefix[b] = 0; c.k = 32; c.radius = 1e30f;
      expect(c.run() == HPL_OK, "64 empty clouds"); }
    { Call c = Call::radius_mode(); c.prefix[1] = 0; c.min_neighbors = INT32_MAX; c.std_ratio = NAN;
      expect(c.run() == HPL_OK, "radius mode, N = 0: the largest min_neighbors; std_ratio is not read"); }
    { Call c; c.prefix[1] = 0; c.min_neighbors = -1; expect(c.run() == HPL_OK, "statistical mode, N = 0: min_neighbors is not read"); }
    { Call c; c.prefix[1] = (int64_t)1 << 26; c.pc_ld = (int64_t)1 << 26; c.k = 32; c.nbr_d2 = 0; c.ws = (uintptr_t)1 << 50;
      c.ws_bytes = hpl_outlier_filter_workspace_bytes(1, (int64_t)1 << 26) - 1; refuse(c, "2^26 points: a workspace one byte short"); }
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
