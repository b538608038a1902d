// Host-only driver of the argument checks of hpl_render_maps / hpl_maps_to_kitti and their workspace arithmetic, for a
// sanitizer build: no device is needed, every call returns before a launch (a refusal, or nothing to do).
// Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/render_host_check.cpp hplflownet_amd/csrc/render.hip -o /tmp/render_host_check && /tmp/render_host_check
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/hpl_bcl.h"

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links render.hip alone)
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
    // 50 points, 10 x 10 pixels, 2 channels; hpl_render_maps reads pc and attr, hpl_maps_to_kitti pc (as pc1) and pc2
    uintptr_t pc = 0x100000, attr = 0x110000, pc2 = 0x120000, pixel_of = 0x200000, winner = 0x210000, depth = 0x220000,
              attr_map = 0x230000, visible = 0x240000, stats = 0x250000, disp1 = 0x300000, disp2 = 0x310000, flow = 0x320000,
              ws = 0x700000;
    int64_t pc_ld = 50, attr_ld = 50, pc2_ld = 50, attr_map_ld = 100, ws_bytes = (int64_t)1 << 20;
    int batch = 1, channels = 2, footprint = 0;
    float rel_tol = 0.02f, abs_tol = 0.f, near_z = 1e-3f, baseline = 0.54f;
    int64_t prefix[66] = {0, 50}, pprefix[66] = {0, 100};
    int32_t height[66] = {10}, width[66] = {10};
    float camera[64 * 6] = {-721.5f, 609.5f, 172.8f, 44.8f, 0.2f, 0.0027f};
    float P[64 * 12] = {721.5f, 0.f, 609.5f, 44.8f, 0.f, 721.5f, 172.8f, 0.2f, 0.f, 0.f, 1.f, 0.0027f};
    bool null_prefix = false, null_height = false, null_width = false, null_pprefix = false, null_camera = false, null_P = false;
    int maps() const {
        return hpl_render_maps((const float *)pc, pc_ld, (const float *)attr, attr_ld, channels, batch, null_prefix ? nullptr : prefix,
                               null_camera ? nullptr : camera, null_height ? nullptr : height, null_width ? nullptr : width,
                               null_pprefix ? nullptr : pprefix, footprint, rel_tol, abs_tol, near_z, (int32_t *)pixel_of,
                               (int32_t *)winner, (float *)depth, (float *)attr_map, attr_map_ld, (uint8_t *)visible, (int32_t *)stats,
                               (void *)ws, ws_bytes, nullptr);
    }
    int kitti() const {
        return hpl_maps_to_kitti((const float *)pc, pc_ld, (const float *)pc2, pc2_ld, batch, null_prefix ? nullptr : prefix,
                                 null_height ? nullptr : height, null_width ? nullptr : width, null_pprefix ? nullptr : pprefix,
                                 null_P ? nullptr : P, baseline, footprint, (uint16_t *)disp1, (uint16_t *)disp2, (uint16_t *)flow,
                                 (void *)ws, ws_bytes, nullptr);
    }
};

static void refuse_maps(const Call &c, const char *what) {
    hpl::g_err[0] = 0;
    expect(c.maps() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_render_maps", 15) == 0, what);
}
static void refuse_kitti(const Call &c, const char *what) {
    hpl::g_err[0] = 0;
    expect(c.kitti() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_maps_to_kitti", 17) == 0, what);
}
static void refuse(const Call &c, const char *what) {
    refuse_maps(c, what);
    refuse_kitti(c, what);
}

int main() {
    // workspace arithmetic: 8 bytes a pixel in 256-byte pieces, monotone, -1 outside
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    const int64_t ms[] = {0, 1, 31, 32, 33, 1025, 465750, 16 * 465750, (int64_t)1 << 29, big - 1};
    for (int b : {1, 2, 64}) {
        int64_t prev = 0;
        for (int64_t m : ms) {
            const int64_t v = hpl_render_workspace_bytes(b, m);
            expect(v >= 8 * m && v < 8 * m + 256 && v % 256 == 0 && v >= prev, "workspace bytes");
            prev = v;
        }
    }
    expect(hpl_render_workspace_bytes(0, 1) == -1 && hpl_render_workspace_bytes(65, 1) == -1 && hpl_render_workspace_bytes(-1, 1) == -1 &&
               hpl_render_workspace_bytes(1, -1) == -1 && hpl_render_workspace_bytes(1, big) == -1 &&
               hpl_render_workspace_bytes(1, (int64_t)1 << 60) == -1,
           "workspace bytes out of range");

    // refusals of both entries, each before any launch, each naming the op
    { Call c; c.batch = 0; refuse(c, "batch 0"); }
    { Call c; c.batch = 65; refuse(c, "batch 65"); }
    { Call c; c.batch = -1; refuse(c, "batch -1"); }
    { Call c; c.null_prefix = true; refuse(c, "null prefix"); }
    { Call c; c.null_height = true; refuse(c, "null height"); }
    { Call c; c.null_width = true; refuse(c, "null width"); }
    { Call c; c.null_pprefix = true; refuse(c, "null pixel prefix"); }
    { Call c; c.pc = 0; refuse(c, "null cloud"); }
    { Call c; c.ws = 0; refuse(c, "null workspace"); }
    { Call c; c.prefix[0] = 1; c.prefix[1] = 51; refuse(c, "prefix from 1"); }
    { Call c; c.batch = 2; c.prefix[1] = 60; c.prefix[2] = 50; c.pprefix[2] = 100; refuse(c, "prefix decreases"); }
    { Call c; c.height[0] = c.width[0] = -10; refuse(c, "negative sizes"); }
    { Call c; c.pprefix[0] = 1; c.pprefix[1] = 101; refuse(c, "pixel prefix from 1"); }
    { Call c; c.pprefix[1] = 99; refuse(c, "pixel prefix below height * width"); }
    { Call c; c.width[0] = 11; refuse(c, "pixel prefix above height * width"); }
    { Call c; c.batch = 2; c.prefix[2] = 50; c.height[1] = 0; c.width[1] = 5; c.pprefix[2] = 90; refuse(c, "pixel prefix decreases"); }
    { Call c; c.footprint = -1; refuse(c, "footprint -1"); }
    { Call c; c.footprint = 5; refuse(c, "footprint 5"); }
    { Call c; c.pc_ld = 49; refuse(c, "row stride below N"); }
    { Call c; c.pc_ld = ((int64_t)1 << 40) + 1; refuse(c, "row stride above 2^40"); }
    { Call c; c.pc_ld = (int64_t)1 << 62; refuse(c, "row stride 2^62"); }
    { Call c; c.pc += 2; refuse(c, "misaligned cloud"); }
    { Call c; c.ws += 128; refuse(c, "misaligned workspace"); }
    { Call c; c.ws_bytes = 0; refuse(c, "no workspace"); }
    { Call c; c.ws_bytes = hpl_render_workspace_bytes(1, 100) - 1; refuse(c, "short workspace"); }
    { Call c; c.prefix[1] = big; c.pc_ld = c.attr_ld = c.pc2_ld = big; refuse(c, "N >= 2^31 / 3"); }
    { Call c; c.height[0] = 1; c.width[0] = (int32_t)big; c.pprefix[1] = big; c.attr_map_ld = big; c.ws_bytes = (int64_t)1 << 40;
      refuse(c, "M >= 2^31 / 3"); }
    { Call c; c.height[0] = c.width[0] = INT32_MAX; c.pprefix[1] = (int64_t)INT32_MAX * INT32_MAX; c.attr_map_ld = (int64_t)1 << 39;
      c.ws_bytes = (int64_t)1 << 62; refuse(c, "M = (2^31 - 1)^2"); }
    { Call c; c.ws = c.pc; c.pc += 256; refuse(c, "the workspace on the cloud"); }
    // hpl_render_maps alone
    { Call c; c.null_camera = true; refuse_maps(c, "null camera"); }
    { Call c; c.pixel_of = 0; refuse_maps(c, "null pixel_of"); }
    { Call c; c.winner = 0; refuse_maps(c, "null winner"); }
    { Call c; c.depth = 0; refuse_maps(c, "null depth"); }
    { Call c; c.visible = 0; refuse_maps(c, "null visible"); }
    { Call c; c.stats = 0; refuse_maps(c, "null stats"); }
    { Call c; c.attr = 0; refuse_maps(c, "null attr with channels"); }
    { Call c; c.channels = -1; refuse_maps(c, "channels -1"); }
    { Call c; c.channels = 9; refuse_maps(c, "channels 9"); }
    { Call c; c.attr_ld = 49; refuse_maps(c, "attr_ld"); }
    { Call c; c.attr_map_ld = 99; refuse_maps(c, "attr_map_ld"); }
    { Call c; c.attr_map_ld = (int64_t)1 << 41; refuse_maps(c, "attr_map_ld above 2^40"); }
    { Call c; c.attr += 1; refuse_maps(c, "misaligned attr"); }
    { Call c; c.winner += 2; refuse_maps(c, "misaligned winner"); }
    { Call c; c.stats += 3; refuse_maps(c, "misaligned stats"); }
    for (float f : {0.f, INFINITY, -INFINITY, NAN}) { Call c; c.camera[0] = f; refuse_maps(c, "f zero or not finite"); }
    { Call c; c.batch = 2; c.prefix[1] = 20; c.prefix[2] = 50; c.height[0] = 5; c.height[1] = 10; c.width[1] = 5; c.pprefix[1] = 50;
      c.pprefix[2] = 100; for (int k = 1; k < 6; ++k) c.camera[6 + k] = c.camera[k];
      refuse_maps(c, "f == 0 in the second camera"); }
    for (float t : {-1e-6f, INFINITY, NAN}) {
        { Call c; c.rel_tol = t; refuse_maps(c, "rel_tol"); }
        { Call c; c.abs_tol = t; refuse_maps(c, "abs_tol"); }
    }
    for (float z : {0.f, -1.f, INFINITY, NAN}) { Call c; c.near_z = z; refuse_maps(c, "near"); }
    { Call c; c.pixel_of = c.pc; refuse_maps(c, "pixel_of on pc"); }
    { Call c; c.winner = c.pc + 4 * 149; refuse_maps(c, "winner on pc's last element"); }
    { Call c; c.depth = c.attr + 4 * 99; refuse_maps(c, "depth on attr's last element"); }
    { Call c; c.visible = c.pc + 5; refuse_maps(c, "visible inside pc"); }
    { Call c; c.attr_map = c.attr - 4 * 199; refuse_maps(c, "attr_map's last element on attr"); }
    { Call c; c.winner = c.pixel_of + 4 * 49; refuse_maps(c, "winner on pixel_of's last element"); }
    { Call c; c.stats = c.visible + 48; refuse_maps(c, "stats on visible's last bytes"); }
    { Call c; c.ws = c.attr_map + 256; refuse_maps(c, "the workspace inside attr_map"); }
    // hpl_maps_to_kitti alone
    { Call c; c.null_P = true; refuse_kitti(c, "null P"); }
    { Call c; c.pc2 = 0; refuse_kitti(c, "null pc2"); }
    { Call c; c.disp1 = 0; refuse_kitti(c, "null disp1"); }
    { Call c; c.disp2 = 0; refuse_kitti(c, "null disp2"); }
    { Call c; c.flow = 0; refuse_kitti(c, "null flow"); }
    { Call c; c.pc2_ld = 49; refuse_kitti(c, "pc2_ld"); }
    { Call c; c.pc2 += 1; refuse_kitti(c, "misaligned pc2"); }
    { Call c; c.disp1 += 1; refuse_kitti(c, "odd disp1"); }
    { Call c; c.disp2 += 1; refuse_kitti(c, "odd disp2"); }
    { Call c; c.flow += 1; refuse_kitti(c, "odd flow"); }
    for (int k : {1, 4, 8, 9}) { Call c; c.P[k] = 0.5f; refuse_kitti(c, "P01 / P10 / P20 / P21 != 0"); }
    { Call c; c.P[5] = 700.f; refuse_kitti(c, "P00 != P11"); }
    for (float f : {0.f, INFINITY, NAN}) { Call c; c.P[0] = c.P[5] = f; refuse_kitti(c, "P00 zero or not finite"); }
    { Call c; c.baseline = NAN; refuse_kitti(c, "NaN baseline"); }
    { Call c; c.baseline = INFINITY; refuse_kitti(c, "infinite baseline"); }
    { Call c; c.disp1 = c.pc; refuse_kitti(c, "disp1 on pc1"); }
    { Call c; c.flow = c.pc2 + 4 * 149; refuse_kitti(c, "flow on pc2's last element"); }
    { Call c; c.disp2 = c.disp1 + 198; refuse_kitti(c, "disp2 on disp1's last pixel"); }
    { Call c; c.ws = c.flow + 512; refuse_kitti(c, "the workspace inside flow"); }
    // accepted: nothing to do returns before any launch; arrays of no elements may be null
    { Call c; c.prefix[1] = 0; c.height[0] = 0; c.pprefix[1] = 0; c.pc_ld = c.attr_ld = c.pc2_ld = c.attr_map_ld = 0; c.ws_bytes = 0;
      expect(c.maps() == HPL_OK && c.kitti() == HPL_OK, "N = 0 and M = 0");
      c.pc = c.attr = c.pc2 = c.pixel_of = c.winner = c.depth = c.attr_map = c.visible = c.disp1 = c.disp2 = c.flow = 0;
      expect(c.maps() == HPL_OK && c.kitti() == HPL_OK, "N = 0 and M = 0, null arrays"); }
    { Call c; c.height[0] = 0; c.pprefix[1] = 0; expect(c.kitti() == HPL_OK, "maps_to_kitti: points, no pixel"); }
    { Call c; c.batch = 64;
      for (int b = 0; b < 64; ++b) {
          c.prefix[b + 1] = 0; c.height[b] = 0; c.width[b] = b; c.pprefix[b + 1] = 0;
          for (int k = 0; k < 6; ++k) c.camera[6 * b + k] = c.camera[k];
          for (int k = 0; k < 12; ++k) c.P[12 * b + k] = c.P[k];
      }
      expect(c.maps() == HPL_OK && c.kitti() == HPL_OK, "64 empty clouds and frames"); }
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
