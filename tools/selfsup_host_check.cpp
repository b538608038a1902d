// Host-only driver of hpl_selfsup_loss's argument checks and workspace arithmetic, for a sanitizer build: no device is needed,
// every call returns before a launch (a refusal, or N1 = 0).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/selfsup_host_check.cpp hplflownet_amd/csrc/selfsup_loss.hip -o /tmp/selfsup_host_check && /tmp/selfsup_host_check
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/hpl_bcl.h"

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links selfsup_loss.hip alone)
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
    uintptr_t pc1 = 0x10000, flow = 0x20000, pc2 = 0x30000, loss = 0x40000, dflow = 0x50000, ws = 0x100000;
    int64_t ld1 = 100, sc = 1, sp = 3, ld2 = 100, ws_bytes = (int64_t)1 << 24;
    int batch = 1, k = 8;
    float wc = 1.f, wsm = 1.f;
    int64_t p1[66] = {0, 100}, p2[66] = {0, 100};
    bool null_p1 = false, null_p2 = false;
    int run() const {
        return hpl_selfsup_loss((const float *)pc1, ld1, (const float *)flow, sc, sp, (const float *)pc2, ld2, batch,
                                null_p1 ? nullptr : p1, null_p2 ? nullptr : p2, k, wc, wsm, (float *)loss, (float *)dflow, nullptr,
                                nullptr, nullptr, (void *)ws, ws_bytes, nullptr);
    }
};

int main() {
    // workspace arithmetic: in range, monotone, -1 outside
    const int64_t ns[] = {0, 1, 3, 255, 256, 257, 1024, 1025, 8192, 8193, 131072, 450000, (int64_t)1 << 27};
    for (int b : {1, 2, 16, 64})
        for (int k = 0; k <= 8; ++k) {
            int64_t prev1 = 0, prev2 = 0;
            for (int64_t n : ns) {
                const int64_t v1 = hpl_selfsup_loss_workspace_bytes(b, n, 1000, k), v2 = hpl_selfsup_loss_workspace_bytes(b, 1000, n, k);
                expect(v1 > 0 && v1 % 256 == 0 && v1 >= prev1 && v2 > 0 && v2 >= prev2, "workspace bytes monotone in the counts");
                if (k < 8) expect(hpl_selfsup_loss_workspace_bytes(b, n, n, k + 1) >= hpl_selfsup_loss_workspace_bytes(b, n, n, k), "monotone in k");
                if (b < 64) expect(hpl_selfsup_loss_workspace_bytes(b + 1, n, n, k) >= hpl_selfsup_loss_workspace_bytes(b, n, n, k), "monotone in batch");
                prev1 = v1;
                prev2 = v2;
            }
        }
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    expect(hpl_selfsup_loss_workspace_bytes(0, 1, 1, 1) == -1 && hpl_selfsup_loss_workspace_bytes(65, 1, 1, 1) == -1 &&
               hpl_selfsup_loss_workspace_bytes(1, -1, 1, 1) == -1 && hpl_selfsup_loss_workspace_bytes(1, 1, -1, 1) == -1 &&
               hpl_selfsup_loss_workspace_bytes(1, 1, 1, 9) == -1 && hpl_selfsup_loss_workspace_bytes(1, 1, 1, -1) == -1 &&
               hpl_selfsup_loss_workspace_bytes(1, big, 1, 1) == -1 && hpl_selfsup_loss_workspace_bytes(1, 1, big, 1) == -1 &&
               hpl_selfsup_loss_workspace_bytes(1, (int64_t)1 << 29, 1, 4) == -1 && hpl_selfsup_loss_workspace_bytes(1, big - 1, big - 1, 1) > 0,
           "workspace bytes out of range");

    // refusals, each before any launch
    auto refuse = [](Call c, const char *what) { expect(c.run() == HPL_EINVAL, what); };
    { Call c; c.batch = 0; refuse(c, "batch 0"); }
    { Call c; c.batch = 65; refuse(c, "batch 65"); }
    { Call c; c.k = -1; refuse(c, "k -1"); }
    { Call c; c.k = 9; refuse(c, "k 9"); }
    { Call c; c.k = 0; refuse(c, "k 0 with w_smooth"); }
    { Call c; c.wc = -1.f; refuse(c, "negative weight"); }
    { Call c; c.wsm = INFINITY; refuse(c, "infinite weight"); }
    { Call c; c.wc = NAN; refuse(c, "NaN weight"); }
    { Call c; c.wsm = NAN; refuse(c, "NaN weight"); }
    { Call c; c.p1[0] = 1; refuse(c, "prefix1 from 1"); }
    { Call c; c.p2[0] = 1; refuse(c, "prefix2 from 1"); }
    { Call c; c.batch = 2; c.p1[1] = 60; c.p1[2] = 50; c.p2[1] = 50; c.p2[2] = 100; refuse(c, "prefix1 decreases"); }
    { Call c; c.batch = 2; c.p2[1] = 60; c.p2[2] = 50; c.p1[1] = 50; c.p1[2] = 100; refuse(c, "prefix2 decreases"); }
    { Call c; c.ld1 = 99; refuse(c, "ld1"); }
    { Call c; c.ld2 = 99; refuse(c, "ld2"); }
    { Call c; c.sc = 0; refuse(c, "sc 0"); }
    { Call c; c.sp = 0; refuse(c, "sp 0"); }
    { Call c; c.sc = 50; c.sp = 1; refuse(c, "rows overlap"); }
    { Call c; c.sc = 1; c.sp = 2; refuse(c, "points overlap"); }
    { Call c; c.pc1 = 0; refuse(c, "null pc1"); }
    { Call c; c.flow = 0; refuse(c, "null flow"); }
    { Call c; c.pc2 = 0; refuse(c, "null pc2"); }
    { Call c; c.loss = 0; refuse(c, "null loss"); }
    { Call c; c.ws = 0; refuse(c, "null workspace"); }
    { Call c; c.null_p1 = true; refuse(c, "null prefix1"); }
    { Call c; c.null_p2 = true; refuse(c, "null prefix2"); }
    { Call c; c.pc1 += 2; refuse(c, "misaligned pc1"); }
    { Call c; c.dflow += 1; refuse(c, "misaligned dflow"); }
    { Call c; c.ws += 128; refuse(c, "misaligned workspace"); }
    { Call c; c.ws_bytes = 0; refuse(c, "no workspace"); }
    { Call c; c.ws_bytes = hpl_selfsup_loss_workspace_bytes(1, 100, 100, 8) - 1; refuse(c, "short workspace"); }
    { Call c; c.p1[1] = big; c.ld1 = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50; refuse(c, "N1 >= 2^31 / 3"); }
    { Call c; c.p2[1] = big; c.ld2 = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50; refuse(c, "N2 >= 2^31 / 3"); }
    { Call c; c.p1[1] = (int64_t)1 << 60; c.ld1 = (int64_t)1 << 60; c.ws_bytes = (int64_t)1 << 62; refuse(c, "N1 = 2^60"); }
    { Call c; c.p1[1] = (int64_t)1 << 29; c.ld1 = (int64_t)1 << 29; c.k = 4; c.ws_bytes = (int64_t)1 << 50; refuse(c, "k N1 >= 2^31"); }
    { Call c; c.dflow = c.pc1 + 4; refuse(c, "dflow in pc1"); }
    { Call c; c.dflow = c.flow; refuse(c, "dflow on flow"); }
    { Call c; c.dflow = c.pc2 + 8; refuse(c, "dflow in pc2"); }
    // accepted arguments with N1 = 0 return HPL_OK before any launch
    { Call c; c.p1[1] = 0; c.ld1 = 0; expect(c.run() == HPL_OK, "N1 = 0"); }
    { Call c; c.p1[1] = 0; c.ld1 = 0; c.p2[1] = 0; c.ld2 = 0; c.pc2 = 0; expect(c.run() == HPL_OK, "N1 = N2 = 0, no pc2"); }
    { Call c; c.batch = 64; for (int b = 0; b <= 64; ++b) { c.p1[b] = 0; c.p2[b] = 3 * b; } c.ld1 = 0; c.ld2 = 192; c.k = 0; c.wsm = 0.f; c.dflow = 0;
      expect(c.run() == HPL_OK, "64 empty pairs"); }
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
