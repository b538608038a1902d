// Host-only driver of the argument checks and workspace arithmetic of hpl_fps and hpl_fps_workspace_bytes, for a sanitizer
// build: no device is needed, every call returns before a launch (a refusal, or N = 0).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/fps_host_check.cpp hplflownet_amd/csrc/fps.hip -o /tmp/fps_host_check && /tmp/fps_host_check
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/hpl_bcl.h"

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links fps.hip alone)
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
    uintptr_t pc = 0x10000, attr = 0x20000, out_pc = 0x30000, out_attr = 0x40000, idx = 0x50000, dist = 0x60000, cover = 0x70000,
              stats = 0x80000, ws = 0x100000;
    int64_t pc_ld = 100, attr_ld = 100, out_ld = 10, oattr_ld = 10, ws_bytes = (int64_t)1 << 24, m = 10;
    int batch = 1, channels = 3, path = HPL_FPS_AUTO;
    int64_t prefix[66] = {0, 100};
    int32_t start[64] = {0};
    bool null_prefix = false, null_start = true;
    int run() const {
        return hpl_fps((const float *)pc, pc_ld, (const float *)attr, attr_ld, channels, batch, null_prefix ? nullptr : prefix,
                       null_start ? nullptr : start, m, path, (int32_t *)idx, (float *)dist, (float *)out_pc, out_ld,
                       (float *)out_attr, oattr_ld, (float *)cover, (int32_t *)stats, (void *)ws, ws_bytes, nullptr);
    }
};

int main() {
    const int cap = hpl_fps_resident_capacity();
    expect(cap >= 8192 && cap % 64 == 0, "the resident capacity");
    // workspace arithmetic: in range, monotone in the batch and the count, -1 outside
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    const int64_t ns[] = {0, 1, 3, 255, 256, 257, 1024, 1025, 8192, 8193, 100191, 131072, 262144, 262145, 450000, (int64_t)1 << 27, big - 1};
    for (int b : {1, 2, 16, 64})
        for (int c = 0; c <= 8; c += 4)
            for (int64_t m : {(int64_t)1, (int64_t)8192, (big - 1) / 64}) {
                int64_t prev = 0;
                for (int64_t n : ns) {
                    const int64_t v = hpl_fps_workspace_bytes(b, n, m, c);
                    expect(v >= 0 && v % 256 == 0 && v >= prev, "workspace bytes monotone in the count");
                    expect(v >= 4 * n && v <= 4 * n + (n / 1024 + 65) * 16 + 3 * 256, "workspace bytes: D and the candidates");
                    if (b < 64) expect(hpl_fps_workspace_bytes(b + 1, n, m, c) >= v, "monotone in batch");
                    prev = v;
                }
            }
    expect(hpl_fps_workspace_bytes(0, 1, 1, 0) == -1 && hpl_fps_workspace_bytes(65, 1, 1, 0) == -1 &&
               hpl_fps_workspace_bytes(-1, 1, 1, 0) == -1 && hpl_fps_workspace_bytes(1, -1, 1, 0) == -1 &&
               hpl_fps_workspace_bytes(1, 1, 1, 9) == -1 && hpl_fps_workspace_bytes(1, 1, 1, -1) == -1 &&
               hpl_fps_workspace_bytes(1, big, 1, 0) == -1 && hpl_fps_workspace_bytes(1, (int64_t)1 << 60, 1, 0) == -1 &&
               hpl_fps_workspace_bytes(1, 1, 0, 0) == -1 && hpl_fps_workspace_bytes(1, 1, -1, 0) == -1 &&
               hpl_fps_workspace_bytes(1, 1, big, 0) == -1 && hpl_fps_workspace_bytes(64, 1, big / 64 + 1, 0) == -1 &&
               hpl_fps_workspace_bytes(2, 1, (int64_t)1 << 62, 0) == -1 && hpl_fps_workspace_bytes(1, big - 1, big - 1, 8) > 0,
           "workspace bytes out of range");

    // refusals, each before any launch, each naming the op
    auto refuse = [](Call c, const char *what) {
        hpl::g_err[0] = 0;
        expect(c.run() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_fps:", 8) == 0, what);
    };
    { Call c; c.batch = 0; refuse(c, "batch 0"); }
    { Call c; c.batch = 65; refuse(c, "batch 65"); }
    { Call c; c.batch = -1; refuse(c, "batch -1"); }
    { Call c; c.channels = -1; refuse(c, "channels -1"); }
    { Call c; c.channels = 9; refuse(c, "channels 9"); }
    { Call c; c.attr = 0; refuse(c, "null attr with channels"); }
    { Call c; c.path = 3; refuse(c, "path 3"); }
    { Call c; c.path = -1; refuse(c, "path -1"); }
    { Call c; c.m = 0; refuse(c, "m 0"); }
    { Call c; c.m = -5; refuse(c, "m -5"); }
    { Call c; c.m = big; c.out_ld = c.oattr_ld = (int64_t)1 << 40; refuse(c, "m = 2^31 / 3"); }
    { Call c; c.m = (int64_t)1 << 62; c.out_ld = c.oattr_ld = (int64_t)1 << 62; refuse(c, "m = 2^62"); }
    { Call c; c.batch = 64; for (int b = 1; b <= 64; ++b) c.prefix[b] = 100; c.m = big / 64 + 1; c.out_ld = c.oattr_ld = (int64_t)1 << 40;
      refuse(c, "batch * m >= 2^31 / 3"); }
    { Call c; c.null_prefix = true; refuse(c, "null prefix"); }
    { Call c; c.prefix[0] = 1; refuse(c, "prefix from 1"); }
    { Call c; c.batch = 2; c.prefix[1] = 60; c.prefix[2] = 50; c.out_ld = c.oattr_ld = 20; refuse(c, "prefix decreases"); }
    { Call c; c.null_start = false; c.start[0] = 100; refuse(c, "start past its cloud"); }
    { Call c; c.null_start = false; c.start[0] = -1; refuse(c, "negative start"); }
    { Call c; c.batch = 2; c.prefix[1] = 60; c.prefix[2] = 100; c.out_ld = c.oattr_ld = 20; c.null_start = false; c.start[0] = 59;
      c.start[1] = 40; refuse(c, "start past the second cloud"); }
    { Call c; c.pc_ld = 99; refuse(c, "pc_ld"); }
    { Call c; c.attr_ld = 99; refuse(c, "attr_ld"); }
    { Call c; c.out_ld = 9; refuse(c, "out_ld"); }
    { Call c; c.oattr_ld = 9; refuse(c, "out_attr_ld"); }
    { Call c; c.pc = 0; refuse(c, "null pc"); }
    { Call c; c.idx = 0; refuse(c, "null idx"); }
    { Call c; c.dist = 0; refuse(c, "null dist"); }
    { Call c; c.out_pc = 0; refuse(c, "null out_pc"); }
    { Call c; c.stats = 0; refuse(c, "null stats"); }
    { Call c; c.ws = 0; refuse(c, "null workspace"); }
    { Call c; c.pc += 2; refuse(c, "misaligned pc"); }
    { Call c; c.attr += 1; refuse(c, "misaligned attr"); }
    { Call c; c.out_pc += 3; refuse(c, "misaligned out_pc"); }
    { Call c; c.out_attr += 2; refuse(c, "misaligned out_attr"); }
    { Call c; c.idx += 1; refuse(c, "misaligned idx"); }
    { Call c; c.dist += 2; refuse(c, "misaligned dist"); }
    { Call c; c.cover += 1; refuse(c, "misaligned cover"); }
    { Call c; c.stats += 2; refuse(c, "misaligned stats"); }
    { Call c; c.ws += 128; refuse(c, "misaligned workspace"); }
    { Call c; c.ws_bytes = 0; refuse(c, "no workspace"); }
    { Call c; c.ws_bytes = hpl_fps_workspace_bytes(1, 100, 10, 3) - 1; refuse(c, "short workspace"); }
    { Call c; c.prefix[1] = big; c.pc_ld = c.attr_ld = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50; refuse(c, "N >= 2^31 / 3"); }
    { Call c; c.prefix[1] = (int64_t)1 << 60; c.pc_ld = c.attr_ld = (int64_t)1 << 60; c.ws_bytes = (int64_t)1 << 62; refuse(c, "N = 2^60"); }
    { Call c; c.out_pc = c.pc; refuse(c, "out_pc on pc"); }
    { Call c; c.out_pc = c.pc + 4 * 299; refuse(c, "out_pc on pc's last element"); }
    { Call c; c.out_pc = c.attr - 4 * 29; refuse(c, "out_pc's last element on attr"); }
    { Call c; c.out_attr = c.attr + 4; refuse(c, "out_attr in attr"); }
    { Call c; c.out_attr = c.pc + 400; refuse(c, "out_attr in pc"); }
    { Call c; c.idx = c.pc + 800; refuse(c, "idx in pc"); }
    { Call c; c.dist = c.attr; refuse(c, "dist on attr"); }
    { Call c; c.cover = c.pc + 4 * 299; refuse(c, "cover on pc's last element"); }
    { Call c; c.stats = c.attr + 4 * 299; refuse(c, "stats on attr's last element"); }
    { Call c; c.path = HPL_FPS_RESIDENT; c.prefix[1] = cap + 1; c.pc_ld = c.attr_ld = cap + 1; refuse(c, "resident above the capacity"); }
    { Call c; c.path = HPL_FPS_RESIDENT; c.batch = 2; c.prefix[1] = 5; c.prefix[2] = cap + 6; c.pc_ld = c.attr_ld = cap + 6;
      c.out_ld = c.oattr_ld = 20; refuse(c, "resident, the second cloud above the capacity"); }
    // arrays that only touch, optional outputs left out and empty batches are accepted: N = 0 returns before any launch
    { Call c; c.prefix[1] = 0; expect(c.run() == HPL_OK, "N = 0"); }
    { Call c; c.prefix[1] = 0; c.pc_ld = c.attr_ld = 0; c.out_attr = c.cover = 0; c.path = HPL_FPS_ROUNDS; c.null_start = false;
      c.start[0] = 77; expect(c.run() == HPL_OK, "N = 0, no optional output, the start of an empty cloud"); }
    { Call c; c.prefix[1] = 0; c.channels = 0; c.attr = 0; c.out_attr = 0; c.m = big - 1; c.out_ld = big - 1;
      expect(c.run() == HPL_OK, "N = 0, no channels, the largest m"); }
    { Call c; c.batch = 64; for (int b = 0; b <= 64; ++b) c.prefix[b] = 0; c.channels = 8; c.out_ld = c.oattr_ld = 640;
      c.path = HPL_FPS_RESIDENT; expect(c.run() == HPL_OK, "64 empty clouds"); }
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
