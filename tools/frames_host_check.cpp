// Host-only driver of the argument checks of hpl_frames_from_kitti / hpl_frames_from_ft3d, their workspace arithmetic and
// hpl_png_unfilter, for a sanitizer build: no device is needed, every frames call returns before a launch (a refusal, or N = 0).
// Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/frames_host_check.cpp hplflownet_amd/csrc/frames.hip -o /tmp/frames_host_check && /tmp/frames_host_check
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/hpl_bcl.h"

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links frames.hip alone)
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
    // KITTI reads in0 .. in2 (disp1, disp2, flow), FlyingThings3D in0 .. in4 (disp, dchange, flow, occ1, occ2)
    uintptr_t in0 = 0x100000, in1 = 0x110000, in2 = 0x120000, in3 = 0x130000, in4 = 0x140000, out1 = 0x300000, out2 = 0x400000,
              pixel = 0x500000, counts = 0x600000, ws = 0x700000;
    int64_t ld1 = 100, ld2 = 100, ws_bytes = (int64_t)1 << 20;
    int batch = 1, use_near = 1;
    float baseline = 0.54f, near_z = -35.f;
    int32_t height[66] = {10}, width[66] = {10};
    int64_t prefix[66] = {0, 100};
    float P[64 * 12] = {721.5f, 0.f, 609.5f, 44.8f, 0.f, 721.5f, 172.8f, 0.2f, 0.f, 0.f, 1.f, 0.0027f};
    bool null_height = false, null_width = false, null_prefix = false, null_P = false;
    int kitti() const {
        return hpl_frames_from_kitti((const uint16_t *)in0, (const uint16_t *)in1, (const uint16_t *)in2, batch,
                                     null_height ? nullptr : height, null_width ? nullptr : width, null_prefix ? nullptr : prefix,
                                     null_P ? nullptr : P, baseline, (float *)out1, ld1, (float *)out2, ld2, (int32_t *)pixel,
                                     (int32_t *)counts, (void *)ws, ws_bytes, nullptr);
    }
    int ft3d() const {
        return hpl_frames_from_ft3d((const float *)in0, (const float *)in1, (const float *)in2, (const uint8_t *)in3,
                                    (const uint8_t *)in4, batch, null_height ? nullptr : height, null_width ? nullptr : width,
                                    null_prefix ? nullptr : prefix, -1050.f, 479.5f, 269.5f, use_near, near_z, (float *)out1, ld1,
                                    (float *)out2, ld2, (int32_t *)pixel, (int32_t *)counts, (void *)ws, ws_bytes, nullptr);
    }
};

static void refuse_kitti(const Call &c, const char *what) {
    hpl::g_err[0] = 0;
    expect(c.kitti() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_frames_from_kitti", 21) == 0, what);
}
static void refuse_ft3d(const Call &c, const char *what) {
    hpl::g_err[0] = 0;
    expect(c.ft3d() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_frames_from_ft3d", 20) == 0, what);
}
static void refuse(const Call &c, const char *what) {
    refuse_kitti(c, what);
    refuse_ft3d(c, what);
}

static void unfilter_checks() {
    // every filter on a 3-byte pixel: rows of 1 + 9 bytes, made by the forward filters from known pixels
    const int bpp = 3, n = 9, H = 6;
    std::vector<uint8_t> px((size_t)H * n);
    for (size_t i = 0; i < px.size(); ++i) px[i] = (uint8_t)(i * 37 + (i / n) * 11 + 200);
    std::vector<uint8_t> rows((size_t)H * (n + 1));
    for (int y = 0; y < H; ++y) {
        const int f = y % 5;
        rows[(size_t)y * (n + 1)] = (uint8_t)f;
        for (int x = 0; x < n; ++x) {
            const int a = x >= bpp ? px[(size_t)y * n + x - bpp] : 0, b = y > 0 ? px[(size_t)(y - 1) * n + x] : 0,
                      c = (y > 0 && x >= bpp) ? px[(size_t)(y - 1) * n + x - bpp] : 0;
            const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
            const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
            const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? (a + b) / 2 : paeth;
            rows[(size_t)y * (n + 1) + 1 + x] = (uint8_t)(px[(size_t)y * n + x] - pred);
        }
    }
    std::vector<uint8_t> work = rows;
    expect(hpl_png_unfilter(work.data(), H, n + 1, bpp) == HPL_OK, "unfilter: all filters");
    bool same = true;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < n; ++x) same = same && work[(size_t)y * (n + 1) + 1 + x] == px[(size_t)y * n + x];
    expect(same, "unfilter: the pixels come back");
    // each filter on the first row alone (no row above), one byte a pixel, a row of one byte
    for (int f = 0; f <= 4; ++f) {
        uint8_t row[5] = {(uint8_t)f, 10, 20, 30, 250};
        expect(hpl_png_unfilter(row, 1, 5, 1) == HPL_OK, "unfilter: first row");
        uint8_t one[2] = {(uint8_t)f, 77};
        expect(hpl_png_unfilter(one, 1, 2, 8) == HPL_OK && one[1] == 77, "unfilter: one byte, bpp 8");
        uint8_t none[1] = {(uint8_t)f};
        expect(hpl_png_unfilter(none, 1, 1, 1) == HPL_OK, "unfilter: a row without data");
    }
    work = rows;
    work[(size_t)2 * (n + 1)] = 5;
    hpl::g_err[0] = 0;
    expect(hpl_png_unfilter(work.data(), H, n + 1, bpp) == HPL_EINVAL && strncmp(hpl::g_err, "hpl_png_unfilter", 16) == 0, "unfilter: filter byte 5");
    work[(size_t)2 * (n + 1)] = 255;
    expect(hpl_png_unfilter(work.data(), H, n + 1, bpp) == HPL_EINVAL, "unfilter: filter byte 255");
    expect(hpl_png_unfilter(nullptr, 0, 10, 3) == HPL_OK && hpl_png_unfilter(work.data(), 0, 1, 1) == HPL_OK, "unfilter: zero rows");
    expect(hpl_png_unfilter(nullptr, 1, 10, 3) == HPL_EINVAL && hpl_png_unfilter(work.data(), -1, 10, 3) == HPL_EINVAL &&
               hpl_png_unfilter(work.data(), 1, 0, 3) == HPL_EINVAL && hpl_png_unfilter(work.data(), 1, 10, 0) == HPL_EINVAL &&
               hpl_png_unfilter(work.data(), 1, 10, 9) == HPL_EINVAL,
           "unfilter: arguments out of range");
}

int main() {
    // workspace arithmetic: in range, monotone, -1 outside
    const int64_t ns[] = {0, 1, 3, 1023, 1024, 1025, 8192, 465750, 518400, 16 * 518400, (int64_t)1 << 29};
    for (int b : {1, 2, 16, 63}) {
        int64_t prev = 0;
        for (int64_t n : ns) {
            const int64_t v = hpl_frames_workspace_bytes(b, n);
            expect(v > 0 && v % 256 == 0 && v >= prev, "workspace bytes monotone in the count");
            expect(hpl_frames_workspace_bytes(b + 1, n) >= v, "monotone in batch");
            prev = v;
        }
    }
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    expect(hpl_frames_workspace_bytes(0, 1) == -1 && hpl_frames_workspace_bytes(65, 1) == -1 && hpl_frames_workspace_bytes(-1, 1) == -1 &&
               hpl_frames_workspace_bytes(1, -1) == -1 && hpl_frames_workspace_bytes(1, big) == -1 &&
               hpl_frames_workspace_bytes(1, (int64_t)1 << 60) == -1 && hpl_frames_workspace_bytes(1, big - 1) > 0,
           "workspace bytes out of range");

    // refusals of both entries, each before any launch, each naming the op
    { Call c; c.batch = 0; refuse(c, "batch 0"); }
    { Call c; c.batch = 65; refuse(c, "batch 65"); }
    { Call c; c.batch = -1; refuse(c, "batch -1"); }
    { Call c; c.null_height = true; refuse(c, "null height"); }
    { Call c; c.null_width = true; refuse(c, "null width"); }
    { Call c; c.null_prefix = true; refuse(c, "null prefix"); }
    { Call c; c.in0 = 0; refuse(c, "null first input"); }
    { Call c; c.in1 = 0; refuse(c, "null second input"); }
    { Call c; c.in2 = 0; refuse(c, "null flow"); }
    { Call c; c.out1 = 0; refuse(c, "null out_pc1"); }
    { Call c; c.out2 = 0; refuse(c, "null out_pc2"); }
    { Call c; c.counts = 0; refuse(c, "null counts"); }
    { Call c; c.ws = 0; refuse(c, "null workspace"); }
    { Call c; c.height[0] = -10; c.width[0] = -10; refuse(c, "negative sizes"); }
    { Call c; c.prefix[0] = 1; c.prefix[1] = 101; refuse(c, "prefix from 1"); }
    { Call c; c.prefix[1] = 99; refuse(c, "prefix below height * width"); }
    { Call c; c.width[0] = 11; refuse(c, "prefix above height * width"); }
    { Call c; c.batch = 2; c.height[1] = 0; c.width[1] = 5; c.prefix[2] = 90; refuse(c, "prefix decreases"); }
    { Call c; c.ld1 = 99; refuse(c, "out1_ld"); }
    { Call c; c.ld2 = 99; refuse(c, "out2_ld"); }
    { Call c; c.out1 += 2; refuse(c, "misaligned out_pc1"); }
    { Call c; c.out2 += 1; refuse(c, "misaligned out_pc2"); }
    { Call c; c.pixel += 2; refuse(c, "misaligned pixel"); }
    { Call c; c.counts += 3; refuse(c, "misaligned counts"); }
    { Call c; c.ws += 2; refuse(c, "misaligned workspace"); }
    { Call c; c.ws_bytes = 0; refuse(c, "no workspace"); }
    { Call c; c.ws_bytes = hpl_frames_workspace_bytes(1, 100) - 1; refuse(c, "short workspace"); }
    { Call c; c.height[0] = 1; c.width[0] = (int32_t)big; c.prefix[1] = big; c.ld1 = c.ld2 = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 40;
      refuse(c, "N >= 2^31 / 3"); }
    { Call c; c.height[0] = c.width[0] = INT32_MAX; c.prefix[1] = (int64_t)INT32_MAX * INT32_MAX; c.ld1 = c.ld2 = (int64_t)1 << 62;
      c.ws_bytes = (int64_t)1 << 62; refuse(c, "N = (2^31 - 1)^2"); }
    { Call c; c.out1 = c.in2; refuse(c, "out_pc1 on the flow"); }
    { Call c; c.out2 = c.in1; refuse(c, "out_pc2 on the second input"); }
    { Call c; c.pixel = c.in2; refuse(c, "pixel on the flow"); }
    { Call c; c.counts = c.in0; refuse(c, "counts on the first input"); }
    { Call c; c.out1 = c.in2 - 4 * 299; refuse(c, "out_pc1's last element on the flow"); }
    { Call c; c.in2 = c.out1 + 4 * 299; refuse(c, "the flow on out_pc1's last element"); }
    { Call c; c.ld1 = (int64_t)1 << 62; refuse(c, "out1_ld = 2^62 with a valid N"); }
    { Call c; c.ld2 = ((int64_t)1 << 40) + 1; refuse(c, "out2_ld above 2^40"); }
    { Call c; c.out2 = c.out1; refuse(c, "out_pc2 on out_pc1"); }
    { Call c; c.out2 = c.out1 + 4 * 299; refuse(c, "out_pc2 on out_pc1's last element"); }
    { Call c; c.pixel = c.out1 + 4 * 150; refuse(c, "pixel inside out_pc1"); }
    { Call c; c.counts = c.out2 + 4 * 299; refuse(c, "counts on out_pc2's last element"); }
    { Call c; c.counts = c.pixel + 4 * 99; refuse(c, "counts on pixel's last element"); }
    { Call c; c.ws = c.out1 + 4 * 200; refuse(c, "the workspace inside out_pc1"); }
    { Call c; c.ws = c.counts; refuse(c, "the workspace on counts"); }
    { Call c; c.height[0] = 0; c.prefix[1] = 0; c.ld1 = c.ld2 = (int64_t)1 << 40; c.out2 = c.out1; c.pixel = c.out1;
      expect(c.kitti() == HPL_OK && c.ft3d() == HPL_OK, "N = 0: nothing is written, nothing overlaps"); }
    // KITTI alone
    { Call c; c.null_P = true; refuse_kitti(c, "null P"); }
    { Call c; c.in0 += 1; refuse_kitti(c, "odd disp1"); }
    { Call c; c.in1 += 1; refuse_kitti(c, "odd disp2"); }
    { Call c; c.in2 += 1; refuse_kitti(c, "odd flow"); }
    { Call c; c.out1 = c.in0 + 196; refuse_kitti(c, "out_pc1 on disp1's last pixels"); }
    for (int k : {1, 4, 8, 9}) { Call c; c.P[k] = 0.5f; refuse_kitti(c, "P01 / P10 / P20 / P21 != 0"); }
    { Call c; c.P[5] = 700.f; refuse_kitti(c, "P00 != P11"); }
    { Call c; c.P[0] = c.P[5] = 0.f; refuse_kitti(c, "P00 == 0"); }
    { Call c; c.P[0] = c.P[5] = INFINITY; refuse_kitti(c, "infinite P00"); }
    { Call c; c.P[0] = c.P[5] = NAN; refuse_kitti(c, "NaN P00"); }
    { Call c; c.baseline = NAN; refuse_kitti(c, "NaN baseline"); }
    { Call c; c.batch = 2; c.height[0] = 5; c.height[1] = 10; c.width[1] = 5; c.prefix[1] = 50; c.prefix[2] = 100;
      for (int k = 0; k < 12; ++k) c.P[12 + k] = c.P[k];
      c.P[12 + 1] = 2.f; refuse_kitti(c, "P01 != 0 in the second frame"); }
    // FlyingThings3D alone
    { Call c; c.in3 = 0; refuse_ft3d(c, "null occ1"); }
    { Call c; c.in4 = 0; refuse_ft3d(c, "null occ2"); }
    { Call c; c.in0 += 2; refuse_ft3d(c, "misaligned disp"); }
    { Call c; c.in1 += 1; refuse_ft3d(c, "misaligned dchange"); }
    { Call c; c.in2 += 2; refuse_ft3d(c, "misaligned flow"); }
    { Call c; c.pixel = c.in3 + 96; refuse_ft3d(c, "pixel on occ1's last pixels"); }
    { Call c; c.in4 = c.counts + 3; refuse_ft3d(c, "occ2 on counts"); }
    { Call c; c.use_near = 2; refuse_ft3d(c, "use_near 2"); }
    { Call c; c.use_near = -1; refuse_ft3d(c, "use_near -1"); }
    { Call c; c.near_z = NAN; refuse_ft3d(c, "NaN near"); }
    // accepted: N = 0 returns before any launch; odd mask addresses, a NULL pixel, a NaN cut that is not in use
    { Call c; c.height[0] = 0; c.prefix[1] = 0; c.ld1 = c.ld2 = 0; expect(c.kitti() == HPL_OK && c.ft3d() == HPL_OK, "N = 0"); }
    { Call c; c.height[0] = 0; c.prefix[1] = 0; c.pixel = 0; c.in3 += 1; c.in4 += 3; c.use_near = 0; c.near_z = NAN;
      expect(c.ft3d() == HPL_OK, "N = 0, odd masks, no pixel"); }
    { Call c; c.width[0] = 0; c.prefix[1] = 0; c.in0 += 2; c.in1 += 6; c.in2 += 2; c.pixel = 0; expect(c.kitti() == HPL_OK, "N = 0, 2-byte aligned planes"); }
    { Call c; c.batch = 64; for (int b = 0; b < 64; ++b) { c.height[b] = 0; c.width[b] = b; c.prefix[b + 1] = 0; for (int k = 0; k < 12; ++k) c.P[12 * b + k] = c.P[k]; }
      expect(c.kitti() == HPL_OK && c.ft3d() == HPL_OK, "64 empty frames"); }
    unfilter_checks();
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
