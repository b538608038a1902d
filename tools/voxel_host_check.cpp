// Host-only driver of hpl_voxel_downsample's argument checks and workspace arithmetic, for a sanitizer build: no device is
// needed, every call returns before a launch (a refusal, or N = 0).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/voxel_host_check.cpp hplflownet_amd/csrc/voxel_grid.hip -o /tmp/voxel_host_check && /tmp/voxel_host_check
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/hpl_bcl.h"

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links voxel_grid.hip alone)
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
    uintptr_t pc = 0x10000, attr = 0x20000, out_pc = 0x30000, out_attr = 0x40000, count = 0x50000, rep = 0x60000,
              voxel_of = 0x70000, stats = 0x80000, ws = 0x100000;
    int64_t pc_ld = 100, attr_ld = 100, out_ld = 100, oattr_ld = 100, ws_bytes = (int64_t)1 << 24;
    int batch = 1, channels = 3, mode = HPL_VOXEL_CENTROID;
    float voxel = 0.1f, origin[3] = {0.f, 0.f, 0.f};
    int64_t prefix[66] = {0, 100};
    bool null_prefix = false, null_origin = false;
    int run() const {
        return hpl_voxel_downsample((const float *)pc, pc_ld, (const float *)attr, attr_ld, channels, batch,
                                    null_prefix ? nullptr : prefix, voxel, null_origin ? nullptr : origin, mode, (float *)out_pc,
                                    out_ld, (float *)out_attr, oattr_ld, (int32_t *)count, (int32_t *)rep, (int32_t *)voxel_of,
                                    (int32_t *)stats, (void *)ws, ws_bytes, nullptr);
    }
};

int main() {
    // workspace arithmetic: in range, monotone, -1 outside
    const int64_t ns[] = {0, 1, 3, 255, 256, 257, 1024, 1025, 8192, 8193, 100191, 131072, 450000, (int64_t)1 << 27};
    for (int b : {1, 2, 16, 64})
        for (int c = 0; c <= 8; ++c) {
            int64_t prev = 0;
            for (int64_t n : ns) {
                const int64_t v = hpl_voxel_downsample_workspace_bytes(b, n, c);
                expect(v >= 0 && v % 256 == 0 && v >= prev, "workspace bytes monotone in the count");
                if (c < 8) expect(hpl_voxel_downsample_workspace_bytes(b, n, c + 1) >= v, "monotone in channels");
                if (b < 64) expect(hpl_voxel_downsample_workspace_bytes(b + 1, n, c) >= v, "monotone in batch");
                prev = v;
            }
        }
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    expect(hpl_voxel_downsample_workspace_bytes(0, 1, 0) == -1 && hpl_voxel_downsample_workspace_bytes(65, 1, 0) == -1 &&
               hpl_voxel_downsample_workspace_bytes(-1, 1, 0) == -1 && hpl_voxel_downsample_workspace_bytes(1, -1, 0) == -1 &&
               hpl_voxel_downsample_workspace_bytes(1, 1, 9) == -1 && hpl_voxel_downsample_workspace_bytes(1, 1, -1) == -1 &&
               hpl_voxel_downsample_workspace_bytes(1, big, 0) == -1 && hpl_voxel_downsample_workspace_bytes(1, (int64_t)1 << 60, 0) == -1 &&
               hpl_voxel_downsample_workspace_bytes(1, big - 1, 8) > 0,
           "workspace bytes out of range");

    // refusals, each before any launch, each naming the op
    auto refuse = [](Call c, const char *what) {
        hpl::g_err[0] = 0;
        expect(c.run() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_voxel_downsample", 20) == 0, what);
    };
    { Call c; c.batch = 0; refuse(c, "batch 0"); }
    { Call c; c.batch = 65; refuse(c, "batch 65"); }
    { Call c; c.batch = -1; refuse(c, "batch -1"); }
    { Call c; c.channels = -1; refuse(c, "channels -1"); }
    { Call c; c.channels = 9; refuse(c, "channels 9"); }
    { Call c; c.attr = 0; refuse(c, "null attr with channels"); }
    { Call c; c.mode = 2; refuse(c, "mode 2"); }
    { Call c; c.mode = -1; refuse(c, "mode -1"); }
    { Call c; c.voxel = 0.f; refuse(c, "voxel 0"); }
    { Call c; c.voxel = -1.f; refuse(c, "negative voxel"); }
    { Call c; c.voxel = INFINITY; refuse(c, "infinite voxel"); }
    { Call c; c.voxel = NAN; refuse(c, "NaN voxel"); }
    { Call c; c.origin[0] = NAN; refuse(c, "NaN origin"); }
    { Call c; c.origin[1] = INFINITY; refuse(c, "infinite origin"); }
    { Call c; c.origin[2] = -INFINITY; refuse(c, "infinite origin"); }
    { Call c; c.null_origin = true; refuse(c, "null origin"); }
    { Call c; c.null_prefix = true; refuse(c, "null prefix"); }
    { Call c; c.prefix[0] = 1; refuse(c, "prefix from 1"); }
    { Call c; c.batch = 2; c.prefix[1] = 60; c.prefix[2] = 50; refuse(c, "prefix decreases"); }
    { Call c; c.pc_ld = 99; refuse(c, "pc_ld"); }
    { Call c; c.attr_ld = 99; refuse(c, "attr_ld"); }
    { Call c; c.out_ld = 99; refuse(c, "out_ld"); }
    { Call c; c.oattr_ld = 99; refuse(c, "out_attr_ld"); }
    { Call c; c.pc = 0; refuse(c, "null pc"); }
    { Call c; c.out_pc = 0; refuse(c, "null out_pc"); }
    { Call c; c.stats = 0; refuse(c, "null stats"); }
    { Call c; c.ws = 0; refuse(c, "null workspace"); }
    { Call c; c.pc += 2; refuse(c, "misaligned pc"); }
    { Call c; c.attr += 1; refuse(c, "misaligned attr"); }
    { Call c; c.out_pc += 3; refuse(c, "misaligned out_pc"); }
    { Call c; c.out_attr += 2; refuse(c, "misaligned out_attr"); }
    { Call c; c.count += 1; refuse(c, "misaligned count"); }
    { Call c; c.rep += 2; refuse(c, "misaligned rep"); }
    { Call c; c.voxel_of += 1; refuse(c, "misaligned voxel_of"); }
    { Call c; c.stats += 2; refuse(c, "misaligned stats"); }
    { Call c; c.ws += 128; refuse(c, "misaligned workspace"); }
    { Call c; c.ws_bytes = 0; refuse(c, "no workspace"); }
    { Call c; c.ws_bytes = hpl_voxel_downsample_workspace_bytes(1, 100, 3) - 1; refuse(c, "short workspace"); }
    { Call c; c.prefix[1] = big; c.pc_ld = c.attr_ld = c.out_ld = c.oattr_ld = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50;
      refuse(c, "N >= 2^31 / 3"); }
    { Call c; c.prefix[1] = (int64_t)1 << 60; c.pc_ld = c.attr_ld = c.out_ld = c.oattr_ld = (int64_t)1 << 60; c.ws_bytes = (int64_t)1 << 62;
      refuse(c, "N = 2^60"); }
    { Call c; c.out_pc = c.pc; refuse(c, "out_pc on pc"); }
    { Call c; c.out_pc = c.pc + 4 * 299; refuse(c, "out_pc on pc's last element"); }
    { Call c; c.out_pc = c.attr - 4 * 299; refuse(c, "out_pc's last element on attr"); }
    { Call c; c.out_attr = c.attr + 4; refuse(c, "out_attr in attr"); }
    { Call c; c.out_attr = c.pc + 400; refuse(c, "out_attr in pc"); }
    { Call c; c.count = c.pc + 800; refuse(c, "count in pc"); }
    { Call c; c.rep = c.attr; refuse(c, "rep on attr"); }
    { Call c; c.voxel_of = c.pc + 4 * 299; refuse(c, "voxel_of on pc's last element"); }
    { Call c; c.stats = c.attr + 4 * 299; refuse(c, "stats on attr's last element"); }
    // arrays that only touch, optional outputs left out and empty batches are accepted: N = 0 returns before any launch
    { Call c; c.prefix[1] = 0; expect(c.run() == HPL_OK, "N = 0"); }
    { Call c; c.prefix[1] = 0; c.pc_ld = c.attr_ld = c.out_ld = c.oattr_ld = 0; c.out_attr = c.count = c.rep = c.voxel_of = 0;
      c.mode = HPL_VOXEL_NEAREST; c.voxel = 1e-30f; c.origin[0] = 1e30f; expect(c.run() == HPL_OK, "N = 0, no optional output"); }
    { Call c; c.prefix[1] = 0; c.channels = 0; c.attr = 0; c.out_attr = 0; expect(c.run() == HPL_OK, "N = 0, no channels"); }
    { Call c; c.batch = 64; for (int b = 0; b <= 64; ++b) c.prefix[b] = 0; c.channels = 8; expect(c.run() == HPL_OK, "64 empty clouds"); }
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
