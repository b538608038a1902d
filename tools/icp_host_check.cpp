// Host-only driver of hpl_icp's argument checks and workspace arithmetic, for a sanitizer build: no device is needed, every
// call returns before a launch (a refusal, or N = 0).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/icp_host_check.cpp hplflownet_amd/csrc/icp.hip -o /tmp/icp_host_check && /tmp/icp_host_check
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/hpl_bcl.h"

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links icp.hip alone)
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
    uintptr_t src = 0x10000, dst = 0x20000, weight = 0x30000, init = 0x40000, Rt = 0x50000, stats = 0x60000, match = 0x70000,
              dist2 = 0x80000, flow = 0x90000, ws = 0x100000;
    int64_t src_ld = 100, dst_ld = 80, ws_bytes = (int64_t)1 << 24;
    int batch = 1, iters = 30;
    float max_dist = 1.f, tau = 0.3f, tol_rot = 0.f, tol_trans = 0.f;
    int64_t sprefix[66] = {0, 100}, dprefix[66] = {0, 80};
    bool null_sprefix = false, null_dprefix = false;
    int run() const {
        return hpl_icp((const float *)src, src_ld, (const float *)dst, dst_ld, (const float *)weight, (const float *)init, batch,
                       null_sprefix ? nullptr : sprefix, null_dprefix ? nullptr : dprefix, iters, max_dist, tau, tol_rot, tol_trans,
                       (float *)Rt, (float *)stats, (int32_t *)match, (float *)dist2, (float *)flow, (void *)ws, ws_bytes, nullptr);
    }
};

int main() {
    // workspace arithmetic: in range, monotone in each argument, -1 outside
    const int64_t ns[] = {0, 1, 3, 255, 256, 257, 1024, 1025, 8192, 8193, 100191, 131072, 450000, (int64_t)1 << 27};
    for (int b : {1, 2, 16, 64})
        for (int64_t m : ns) {
            int64_t prev = 0;
            for (int64_t n : ns) {
                const int64_t v = hpl_icp_workspace_bytes(b, n, m);
                expect(v > 0 && v % 256 == 0 && v >= prev, "workspace bytes monotone in the src count");
                expect(hpl_icp_workspace_bytes(b, m, n) >= hpl_icp_workspace_bytes(b, m, n > 0 ? n - 1 : 0),
                       "workspace bytes monotone in the dst count");
                if (b < 64) expect(hpl_icp_workspace_bytes(b + 1, n, m) >= v, "monotone in batch");
                prev = v;
            }
        }
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    expect(hpl_icp_workspace_bytes(0, 1, 1) == -1 && hpl_icp_workspace_bytes(65, 1, 1) == -1 &&
               hpl_icp_workspace_bytes(-1, 1, 1) == -1 && hpl_icp_workspace_bytes(1, -1, 1) == -1 &&
               hpl_icp_workspace_bytes(1, 1, -1) == -1 && hpl_icp_workspace_bytes(1, big, 1) == -1 &&
               hpl_icp_workspace_bytes(1, 1, big) == -1 && hpl_icp_workspace_bytes(1, (int64_t)1 << 60, 1) == -1 &&
               hpl_icp_workspace_bytes(1, 1, (int64_t)1 << 60) == -1 && hpl_icp_workspace_bytes(64, big - 1, big - 1) > 0,
           "workspace bytes out of range");

    // refusals, each before any launch, each naming the op
    auto refuse = [](Call c, const char *what) {
        hpl::g_err[0] = 0;
        expect(c.run() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_icp", 7) == 0, what);
    };
    { Call c; c.batch = 0; refuse(c, "batch 0"); }
    { Call c; c.batch = 65; refuse(c, "batch 65"); }
    { Call c; c.batch = -1; refuse(c, "batch -1"); }
    { Call c; c.iters = -1; refuse(c, "iters -1"); }
    { Call c; c.iters = 65; refuse(c, "iters 65"); }
    { Call c; c.max_dist = 0.f; refuse(c, "max_dist 0"); }
    { Call c; c.max_dist = -1.f; refuse(c, "negative max_dist"); }
    { Call c; c.max_dist = INFINITY; refuse(c, "infinite max_dist"); }
    { Call c; c.max_dist = NAN; refuse(c, "NaN max_dist"); }
    { Call c; c.tau = 0.f; refuse(c, "tau 0"); }
    { Call c; c.tau = -1.f; refuse(c, "negative tau"); }
    { Call c; c.tau = INFINITY; refuse(c, "infinite tau"); }
    { Call c; c.tau = NAN; refuse(c, "NaN tau"); }
    { Call c; c.tol_rot = -1e-6f; refuse(c, "negative tol_rot"); }
    { Call c; c.tol_trans = -1e-6f; refuse(c, "negative tol_trans"); }
    { Call c; c.tol_rot = NAN; refuse(c, "NaN tol_rot"); }
    { Call c; c.tol_trans = NAN; refuse(c, "NaN tol_trans"); }
    { Call c; c.null_sprefix = true; refuse(c, "null src prefix"); }
    { Call c; c.null_dprefix = true; refuse(c, "null dst prefix"); }
    { Call c; c.sprefix[0] = 1; refuse(c, "src prefix from 1"); }
    { Call c; c.dprefix[0] = 1; refuse(c, "dst prefix from 1"); }
    { Call c; c.batch = 2; c.sprefix[1] = 60; c.sprefix[2] = 50; c.dprefix[2] = 80; refuse(c, "src prefix decreases"); }
    { Call c; c.batch = 2; c.sprefix[2] = 100; c.dprefix[1] = 50; c.dprefix[2] = 40; refuse(c, "dst prefix decreases"); }
    { Call c; c.src_ld = 99; refuse(c, "src_ld"); }
    { Call c; c.dst_ld = 79; refuse(c, "dst_ld"); }
    { Call c; c.src = 0; refuse(c, "null src"); }
    { Call c; c.dst = 0; refuse(c, "null dst with points"); }
    { Call c; c.Rt = 0; refuse(c, "null Rt"); }
    { Call c; c.stats = 0; refuse(c, "null stats"); }
    { Call c; c.ws = 0; refuse(c, "null workspace"); }
    { Call c; c.src += 2; refuse(c, "misaligned src"); }
    { Call c; c.dst += 1; refuse(c, "misaligned dst"); }
    { Call c; c.weight += 3; refuse(c, "misaligned weight"); }
    { Call c; c.init += 2; refuse(c, "misaligned init"); }
    { Call c; c.Rt += 1; refuse(c, "misaligned Rt"); }
    { Call c; c.stats += 2; refuse(c, "misaligned stats"); }
    { Call c; c.match += 1; refuse(c, "misaligned match"); }
    { Call c; c.dist2 += 2; refuse(c, "misaligned dist2"); }
    { Call c; c.flow += 3; refuse(c, "misaligned flow"); }
    { Call c; c.ws += 128; refuse(c, "misaligned workspace"); }
    { Call c; c.ws_bytes = 0; refuse(c, "no workspace"); }
    { Call c; c.ws_bytes = hpl_icp_workspace_bytes(1, 100, 80) - 1; refuse(c, "short workspace"); }
    { Call c; c.sprefix[1] = big; c.src_ld = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50; refuse(c, "N >= 2^31 / 3"); }
    { Call c; c.dprefix[1] = big; c.dst_ld = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50; refuse(c, "M >= 2^31 / 3"); }
    { Call c; c.sprefix[1] = (int64_t)1 << 60; c.src_ld = (int64_t)1 << 60; c.ws_bytes = (int64_t)1 << 62; refuse(c, "N = 2^60"); }
    { Call c; c.dprefix[1] = (int64_t)1 << 60; c.dst_ld = (int64_t)1 << 60; c.ws_bytes = (int64_t)1 << 62; refuse(c, "M = 2^60"); }
    // optional arrays left out, an exact workspace and empty batches are accepted: N = 0 returns before any launch
    { Call c; c.sprefix[1] = 0; expect(c.run() == HPL_OK, "N = 0"); }
    { Call c; c.sprefix[1] = 0; c.ws_bytes = hpl_icp_workspace_bytes(1, 0, 80); expect(c.run() == HPL_OK, "N = 0, exact workspace"); }
    { Call c; c.sprefix[1] = 0; c.dprefix[1] = 0; c.src_ld = c.dst_ld = 0; c.dst = c.weight = c.init = c.match = c.dist2 = c.flow = 0;
      c.iters = 0; c.max_dist = 1e-30f; c.tau = 1e30f; c.tol_rot = INFINITY; expect(c.run() == HPL_OK, "N = M = 0, no optional array"); }
    { Call c; c.batch = 64; for (int b = 0; b <= 64; ++b) { c.sprefix[b] = 0; c.dprefix[b] = b; } c.iters = 64;
      expect(c.run() == HPL_OK, "64 empty src clouds"); }
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
