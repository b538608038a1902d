// Host-only driver of the argument checks and workspace arithmetic of hpl_object_fit and hpl_object_fit_workspace_bytes, for a
// sanitizer build: no device is needed, every call returns before a launch (a refusal, or N = 0).  Build and run from the
// repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/object_fit_host_check.cpp hplflownet_amd/csrc/object_fit.hip -o /tmp/object_fit_host_check && /tmp/object_fit_host_check
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/hpl_bcl.h"

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links object_fit.hip alone)
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
    uintptr_t pc = 0x10000, flow = 0x20000, weight = 0, labels = 0x30000, Rt = 0x40000, stats = 0x50000, residual = 0x60000,
              refined = 0x70000, ws = 0x100000;
    int64_t pc_ld = 100, sc = 1, sp = 3, ws_bytes = (int64_t)1 << 24;
    int batch = 1, max_objects = 16, iters = 4;
    float tau = 0.1f;
    int64_t prefix[66] = {0, 100};
    bool null_prefix = false;
    int run() const {
        return hpl_object_fit((const float *)pc, pc_ld, (const float *)flow, sc, sp, (const float *)weight, (const int32_t *)labels,
                              batch, null_prefix ? nullptr : prefix, max_objects, iters, tau, (float *)Rt, (float *)stats,
                              (float *)residual, (float *)refined, (void *)ws, ws_bytes, nullptr);
    }
};

int main() {
    // workspace arithmetic: in range, 256-aligned, monotone in the batch, the count and the table, -1 outside
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    const int64_t ns[] = {0, 1, 3, 255, 256, 257, 1023, 1024, 1025, 8192, 8193, 24001, 131072, 262145, 450000, (int64_t)1 << 27, big - 1};
    for (int b : {1, 2, 16, 63, 64})
        for (int m : {1, 2, 12, 256, 4095, 4096}) {
            int64_t prev = 0;
            for (int64_t n : ns) {
                const int64_t v = hpl_object_fit_workspace_bytes(b, n, m);
                expect(v > 0 && v % 256 == 0 && v >= prev, "workspace bytes monotone in the count");
                // keys, values, records and a slot of 16 doubles per span and per (pair, object)
                expect(v >= 48 * n + 128 * (n / 1024 + (int64_t)b * m + 1), "workspace bytes: the arrays and the slots");
                if (b < 64) expect(hpl_object_fit_workspace_bytes(b + 1, n, m) >= v, "monotone in batch");
                if (m < 4096) expect(hpl_object_fit_workspace_bytes(b, n, m + 1) >= v, "monotone in max_objects");
                prev = v;
            }
        }
    expect(hpl_object_fit_workspace_bytes(0, 1, 1) == -1 && hpl_object_fit_workspace_bytes(65, 1, 1) == -1 &&
               hpl_object_fit_workspace_bytes(-1, 1, 1) == -1 && hpl_object_fit_workspace_bytes(1, -1, 1) == -1 &&
               hpl_object_fit_workspace_bytes(1, big, 1) == -1 && hpl_object_fit_workspace_bytes(1, (int64_t)1 << 60, 1) == -1 &&
               hpl_object_fit_workspace_bytes(1, 1, 0) == -1 && hpl_object_fit_workspace_bytes(1, 1, -1) == -1 &&
               hpl_object_fit_workspace_bytes(1, 1, 4097) == -1 && hpl_object_fit_workspace_bytes(64, big - 1, 4096) > 0,
           "workspace bytes out of range");

    // refusals, each before any launch, each naming the op
    auto refuse = [](Call c, const char *what) {
        hpl::g_err[0] = 0;
        expect(c.run() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_object_fit:", 15) == 0, what);
    };
    { Call c; c.batch = 0; refuse(c, "batch 0"); }
    { Call c; c.batch = 65; refuse(c, "batch 65"); }
    { Call c; c.batch = -1; refuse(c, "batch -1"); }
    { Call c; c.max_objects = 0; refuse(c, "max_objects 0"); }
    { Call c; c.max_objects = -3; refuse(c, "max_objects -3"); }
    { Call c; c.max_objects = 4097; refuse(c, "max_objects 4097"); }
    { Call c; c.iters = -1; refuse(c, "iters -1"); }
    { Call c; c.iters = 17; refuse(c, "iters 17"); }
    { Call c; c.tau = 0.f; refuse(c, "tau 0"); }
    { Call c; c.tau = -0.1f; refuse(c, "tau < 0"); }
    { Call c; c.tau = INFINITY; refuse(c, "tau inf"); }
    { Call c; c.tau = NAN; refuse(c, "tau NaN"); }
    { Call c; c.null_prefix = true; refuse(c, "null prefix"); }
    { Call c; c.prefix[0] = 1; refuse(c, "prefix from 1"); }
    { Call c; c.batch = 2; c.prefix[1] = 60; c.prefix[2] = 50; refuse(c, "prefix decreases"); }
    { Call c; c.pc_ld = 99; refuse(c, "pc_ld"); }
    { Call c; c.sc = 0; refuse(c, "flow_sc 0"); }
    { Call c; c.sp = 0; refuse(c, "flow_sp 0"); }
    { Call c; c.sc = -1; refuse(c, "flow_sc -1"); }
    { Call c; c.sc = 50; c.sp = 1; refuse(c, "rows that overlap"); }
    { Call c; c.sc = 1; c.sp = 2; refuse(c, "points that overlap"); }
    { Call c; c.pc = 0; refuse(c, "null pc"); }
    { Call c; c.flow = 0; refuse(c, "null flow"); }
    { Call c; c.labels = 0; refuse(c, "null labels"); }
    { Call c; c.Rt = 0; refuse(c, "null obj_Rt"); }
    { Call c; c.stats = 0; refuse(c, "null obj_stats"); }
    { Call c; c.ws = 0; refuse(c, "null workspace"); }
    { Call c; c.pc += 2; refuse(c, "misaligned pc"); }
    { Call c; c.flow += 1; refuse(c, "misaligned flow"); }
    { Call c; c.weight = 0x80001; refuse(c, "misaligned weight"); }
    { Call c; c.labels += 2; refuse(c, "misaligned labels"); }
    { Call c; c.Rt += 3; refuse(c, "misaligned obj_Rt"); }
    { Call c; c.stats += 2; refuse(c, "misaligned obj_stats"); }
    { Call c; c.residual += 1; refuse(c, "misaligned residual"); }
    { Call c; c.refined += 2; refuse(c, "misaligned refined"); }
    { Call c; c.ws += 128; refuse(c, "misaligned workspace"); }
    { Call c; c.ws_bytes = 0; refuse(c, "no workspace"); }
    { Call c; c.ws_bytes = hpl_object_fit_workspace_bytes(1, 100, 16) - 1; refuse(c, "short workspace"); }
    { Call c; c.max_objects = 4096; c.ws_bytes = hpl_object_fit_workspace_bytes(1, 100, 4095) - 1; refuse(c, "a smaller table's workspace"); }
    { Call c; c.prefix[1] = big; c.pc_ld = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50; refuse(c, "N >= 2^31 / 3"); }
    { Call c; c.prefix[1] = (int64_t)1 << 60; c.pc_ld = (int64_t)1 << 60; c.ws_bytes = (int64_t)1 << 62; refuse(c, "N = 2^60"); }
    // optional arrays left out and empty batches are accepted: N = 0 returns before any launch
    { Call c; c.prefix[1] = 0; expect(c.run() == HPL_OK, "N = 0"); }
    { Call c; c.prefix[1] = 0; c.pc_ld = 0; c.residual = c.refined = 0; c.iters = 0; c.max_objects = 4096; c.sc = 7; c.sp = 1;
      expect(c.run() == HPL_OK, "N = 0, no in-place array, the largest table"); }
    { Call c; c.batch = 64; for (int b = 0; b <= 64; ++b) c.prefix[b] = 0; c.weight = 0x80000; c.iters = 16;
      expect(c.run() == HPL_OK, "64 empty pairs"); }
    { Call c; c.ws_bytes = hpl_object_fit_workspace_bytes(1, 0, 16); c.prefix[1] = 0; expect(c.run() == HPL_OK, "N = 0, the exact workspace"); }
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
