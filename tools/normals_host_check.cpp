// Host-only driver of the argument checks and workspace arithmetic of hpl_normals and hpl_icp_plane, for a sanitizer build: no device is needed, every
// call returns before a launch (a refusal, or N = 0).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/normals_host_check.cpp hplflownet_amd/csrc/normals.hip hplflownet_amd/csrc/icp_plane.hip -o /tmp/normals_host_check && /tmp/normals_host_check
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/hpl_bcl.h"

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links normals.hip and icp_plane.hip alone)
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
    uintptr_t pc = 0x10000, normal = 0x20000, curvature = 0x30000, count = 0x40000, nbr = 0x50000, nbr_d2 = 0x60000, ws = 0x100000;
    int64_t pc_ld = 100, normal_ld = 100, ws_bytes = (int64_t)1 << 24;
    int batch = 1, k = 16;
    float radius = 1.f;
    int64_t prefix[66] = {0, 100};
    float view[3 * 64] = {};
    bool null_prefix = false, null_view = true;
    int run() const {
        return hpl_normals((const float *)pc, pc_ld, batch, null_prefix ? nullptr : prefix, k, radius, null_view ? nullptr : view,
                           (float *)normal, normal_ld, (float *)curvature, (int32_t *)count, (int32_t *)nbr, (float *)nbr_d2,
                           (void *)ws, ws_bytes, nullptr);
    }
};

struct PlaneCall {
    uintptr_t src = 0x10000, dst = 0x20000, nrm = 0x28000, weight = 0x30000, init = 0x40000, Rt = 0x50000, stats = 0x60000,
              match = 0x70000, dist2 = 0x80000, flow = 0x90000, ws = 0x100000;
    int64_t src_ld = 100, dst_ld = 80, nrm_ld = 80, ws_bytes = (int64_t)1 << 24;
    int batch = 1, iters = 30;
    float max_dist = 1.f, tau = 0.3f, tol_rot = 0.f, tol_trans = 0.f;
    int64_t sprefix[66] = {0, 100}, dprefix[66] = {0, 80};
    bool null_sprefix = false, null_dprefix = false;
    int run() const {
        return hpl_icp_plane((const float *)src, src_ld, (const float *)dst, dst_ld, (const float *)nrm, nrm_ld, (const float *)weight,
                             (const float *)init, batch, null_sprefix ? nullptr : sprefix, null_dprefix ? nullptr : dprefix, iters,
                             max_dist, tau, tol_rot, tol_trans, (float *)Rt, (float *)stats, (int32_t *)match, (float *)dist2,
                             (float *)flow, (void *)ws, ws_bytes, nullptr);
    }
};

static void check_icp_plane() {
    const int64_t ns[] = {0, 1, 3, 255, 1024, 1025, 8192, 8193, 100191, 450000, (int64_t)1 << 27};
    for (int b : {1, 2, 16, 64})
        for (int64_t m : ns) {
            int64_t prev = 0;
            for (int64_t n : ns) {
                const int64_t v = hpl_icp_plane_workspace_bytes(b, n, m);
                expect(v > 0 && v % 256 == 0 && v >= prev, "icp_plane: workspace bytes monotone in the src count");
                expect(hpl_icp_plane_workspace_bytes(b, m, n) >= hpl_icp_plane_workspace_bytes(b, m, n > 0 ? n - 1 : 0),
                       "icp_plane: workspace bytes monotone in the dst count");
                if (b < 64) expect(hpl_icp_plane_workspace_bytes(b + 1, n, m) >= v, "icp_plane: monotone in batch");
                prev = v;
            }
        }
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    expect(hpl_icp_plane_workspace_bytes(0, 1, 1) == -1 && hpl_icp_plane_workspace_bytes(65, 1, 1) == -1 &&
               hpl_icp_plane_workspace_bytes(1, -1, 1) == -1 && hpl_icp_plane_workspace_bytes(1, 1, -1) == -1 &&
               hpl_icp_plane_workspace_bytes(1, big, 1) == -1 && hpl_icp_plane_workspace_bytes(1, 1, big) == -1 &&
               hpl_icp_plane_workspace_bytes(64, big - 1, big - 1) > 0,
           "icp_plane: workspace bytes out of range");
    auto refuse = [](PlaneCall c, const char *what) {
        hpl::g_err[0] = 0;
        expect(c.run() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_icp_plane", 13) == 0, what);
    };
    { PlaneCall c; c.batch = 0; refuse(c, "icp_plane: batch 0"); }
    { PlaneCall c; c.batch = 65; refuse(c, "icp_plane: batch 65"); }
    { PlaneCall c; c.iters = -1; refuse(c, "icp_plane: iters -1"); }
    { PlaneCall c; c.iters = 65; refuse(c, "icp_plane: iters 65"); }
    { PlaneCall c; c.max_dist = 0.f; refuse(c, "icp_plane: max_dist 0"); }
    { PlaneCall c; c.max_dist = NAN; refuse(c, "icp_plane: NaN max_dist"); }
    { PlaneCall c; c.max_dist = INFINITY; refuse(c, "icp_plane: infinite max_dist"); }
    { PlaneCall c; c.tau = 0.f; refuse(c, "icp_plane: tau 0"); }
    { PlaneCall c; c.tau = NAN; refuse(c, "icp_plane: NaN tau"); }
    { PlaneCall c; c.tol_rot = -1e-6f; refuse(c, "icp_plane: negative tol_rot"); }
    { PlaneCall c; c.tol_trans = NAN; refuse(c, "icp_plane: NaN tol_trans"); }
    { PlaneCall c; c.null_sprefix = true; refuse(c, "icp_plane: null src prefix"); }
    { PlaneCall c; c.null_dprefix = true; refuse(c, "icp_plane: null dst prefix"); }
    { PlaneCall c; c.sprefix[0] = 1; refuse(c, "icp_plane: src prefix from 1"); }
    { PlaneCall c; c.batch = 2; c.sprefix[2] = 100; c.dprefix[1] = 50; c.dprefix[2] = 40; refuse(c, "icp_plane: dst prefix decreases"); }
    { PlaneCall c; c.src_ld = 99; refuse(c, "icp_plane: src_ld"); }
    { PlaneCall c; c.dst_ld = 79; refuse(c, "icp_plane: dst_ld"); }
    { PlaneCall c; c.nrm_ld = 79; refuse(c, "icp_plane: dnormal_ld"); }
    { PlaneCall c; c.src = 0; refuse(c, "icp_plane: null src"); }
    { PlaneCall c; c.dst = 0; refuse(c, "icp_plane: null dst with points"); }
    { PlaneCall c; c.nrm = 0; refuse(c, "icp_plane: null dst_normal with points"); }
    { PlaneCall c; c.Rt = 0; refuse(c, "icp_plane: null Rt"); }
    { PlaneCall c; c.stats = 0; refuse(c, "icp_plane: null stats"); }
    { PlaneCall c; c.ws = 0; refuse(c, "icp_plane: null workspace"); }
    { PlaneCall c; c.nrm += 2; refuse(c, "icp_plane: misaligned dst_normal"); }
    { PlaneCall c; c.src += 1; refuse(c, "icp_plane: misaligned src"); }
    { PlaneCall c; c.flow += 3; refuse(c, "icp_plane: misaligned flow"); }
    { PlaneCall c; c.ws += 128; refuse(c, "icp_plane: misaligned workspace"); }
    { PlaneCall c; c.ws_bytes = hpl_icp_plane_workspace_bytes(1, 100, 80) - 1; refuse(c, "icp_plane: short workspace"); }
    { PlaneCall c; c.sprefix[1] = big; c.src_ld = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50; refuse(c, "icp_plane: N >= 2^31 / 3"); }
    { PlaneCall c; c.dprefix[1] = big; c.dst_ld = c.nrm_ld = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50; refuse(c, "icp_plane: M >= 2^31 / 3"); }
    { PlaneCall c; c.sprefix[1] = 0; expect(c.run() == HPL_OK, "icp_plane: N = 0"); }
    { PlaneCall c; c.sprefix[1] = 0; c.dprefix[1] = 0; c.src_ld = c.dst_ld = c.nrm_ld = 0; c.dst = c.nrm = c.weight = c.init = c.match = c.dist2 = c.flow = 0;
      c.iters = 0; expect(c.run() == HPL_OK, "icp_plane: N = M = 0, no optional array"); }
}

int main() {
    check_icp_plane();
    // workspace arithmetic: in range, monotone in the count, the same for every batch, -1 outside
    const int64_t ns[] = {0, 1, 3, 255, 256, 257, 1024, 1025, 8192, 8193, 100191, 131072, 450000, (int64_t)1 << 27};
    for (int b : {1, 2, 16, 64}) {
        int64_t prev = 0;
        for (int64_t n : ns) {
            const int64_t v = hpl_normals_workspace_bytes(b, n);
            expect(v > 0 && v % 256 == 0 && v >= prev, "workspace bytes monotone in the count");
            expect(v == hpl_normals_workspace_bytes(1, n), "workspace bytes do not depend on the batch");
            expect(v >= 48 * n, "workspace bytes hold two keys and two records per point");
            prev = v;
        }
    }
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    expect(hpl_normals_workspace_bytes(0, 1) == -1 && hpl_normals_workspace_bytes(65, 1) == -1 &&
               hpl_normals_workspace_bytes(-1, 1) == -1 && hpl_normals_workspace_bytes(1, -1) == -1 &&
               hpl_normals_workspace_bytes(1, big) == -1 && hpl_normals_workspace_bytes(1, (int64_t)1 << 60) == -1 &&
               hpl_normals_workspace_bytes(64, big - 1) > 0,
           "workspace bytes out of range");

    // refusals, each before any launch, each naming the op
    auto refuse = [](Call c, const char *what) {
        hpl::g_err[0] = 0;
        expect(c.run() == HPL_EINVAL && strncmp(hpl::g_err, "hpl_normals", 11) == 0, what);
    };
    { Call c; c.batch = 0; refuse(c, "batch 0"); }
    { Call c; c.batch = 65; refuse(c, "batch 65"); }
    { Call c; c.batch = -1; refuse(c, "batch -1"); }
    { Call c; c.k = 2; refuse(c, "k 2"); }
    { Call c; c.k = 33; refuse(c, "k 33"); }
    { Call c; c.k = -1; refuse(c, "k -1"); }
    { Call c; c.radius = 0.f; refuse(c, "radius 0"); }
    { Call c; c.radius = -1.f; refuse(c, "negative radius"); }
    { Call c; c.radius = INFINITY; refuse(c, "infinite radius"); }
    { Call c; c.radius = NAN; refuse(c, "NaN radius"); }
    { Call c; c.null_view = false; c.view[1] = NAN; refuse(c, "NaN viewpoint"); }
    { Call c; c.null_view = false; c.view[2] = -INFINITY; refuse(c, "infinite viewpoint"); }
    { Call c; c.null_view = false; c.batch = 64; for (int b = 0; b <= 64; ++b) c.prefix[b] = b < 64 ? 0 : 100; c.view[191] = NAN;
      refuse(c, "NaN viewpoint of the last cloud"); }
    { Call c; c.null_prefix = true; refuse(c, "null prefix"); }
    { Call c; c.prefix[0] = 1; refuse(c, "prefix from 1"); }
    { Call c; c.batch = 2; c.prefix[1] = 60; c.prefix[2] = 50; refuse(c, "prefix decreases"); }
    { Call c; c.pc_ld = 99; refuse(c, "pc_ld"); }
    { Call c; c.normal_ld = 99; refuse(c, "normal_ld"); }
    { Call c; c.pc = 0; refuse(c, "null pc"); }
    { Call c; c.normal = 0; refuse(c, "null normal"); }
    { Call c; c.ws = 0; refuse(c, "null workspace"); }
    { Call c; c.pc += 2; refuse(c, "misaligned pc"); }
    { Call c; c.normal += 1; refuse(c, "misaligned normal"); }
    { Call c; c.curvature += 3; refuse(c, "misaligned curvature"); }
    { Call c; c.count += 2; refuse(c, "misaligned count"); }
    { Call c; c.nbr += 1; refuse(c, "misaligned nbr"); }
    { Call c; c.nbr_d2 += 2; refuse(c, "misaligned nbr_d2"); }
    { Call c; c.ws += 128; refuse(c, "misaligned workspace"); }
    { Call c; c.ws_bytes = 0; refuse(c, "no workspace"); }
    { Call c; c.ws_bytes = hpl_normals_workspace_bytes(1, 100) - 1; refuse(c, "short workspace"); }
    { Call c; c.prefix[1] = big; c.pc_ld = c.normal_ld = (int64_t)1 << 31; c.ws_bytes = (int64_t)1 << 50; refuse(c, "N >= 2^31 / 3"); }
    { Call c; c.prefix[1] = (int64_t)1 << 60; c.pc_ld = c.normal_ld = (int64_t)1 << 60; c.ws_bytes = (int64_t)1 << 62; refuse(c, "N = 2^60"); }
    { Call c; c.prefix[1] = (int64_t)1 << 27; c.pc_ld = c.normal_ld = (int64_t)1 << 27; c.ws = (uintptr_t)1 << 50; c.ws_bytes = (int64_t)1 << 50;
      c.nbr_d2 = 0; refuse(c, "N k = 2^31 with nbr"); }
    { Call c; c.prefix[1] = (int64_t)1 << 27; c.pc_ld = c.normal_ld = (int64_t)1 << 27; c.ws = (uintptr_t)1 << 50; c.ws_bytes = (int64_t)1 << 50;
      c.nbr = 0; c.k = 32; refuse(c, "N k = 2^32 with nbr_d2"); }
    // an output inside the input or the workspace
    { Call c; c.normal = c.pc; refuse(c, "normal on pc"); }
    { Call c; c.normal = c.pc + 4 * 299; refuse(c, "normal on the last element of pc"); }
    { Call c; c.normal = c.pc - 4 * 299; refuse(c, "the last element of normal on pc"); }
    { Call c; c.curvature = c.pc + 400; refuse(c, "curvature in pc"); }
    { Call c; c.count = c.pc + 800; refuse(c, "count in pc"); }
    { Call c; c.nbr = c.pc - 4 * 1599; refuse(c, "the last element of nbr on pc"); }
    { Call c; c.nbr_d2 = c.pc + 1196; refuse(c, "nbr_d2 on the last element of pc"); }
    { Call c; c.normal = c.ws; refuse(c, "normal on the workspace"); }
    { Call c; c.curvature = c.ws + 256; refuse(c, "curvature in the workspace"); }
    { Call c; c.count = c.ws - 396; refuse(c, "the last element of count on the workspace"); }
    { Call c; c.nbr = c.ws + 1024; refuse(c, "nbr in the workspace"); }
    { Call c; c.nbr_d2 = c.ws + (uintptr_t)hpl_normals_workspace_bytes(1, 100) - 4; refuse(c, "nbr_d2 on the workspace's last word"); }
    // optional arrays left out, an exact workspace, arrays that merely touch and empty batches are accepted: N = 0 returns
    // before any launch
    { Call c; c.prefix[1] = 0; expect(c.run() == HPL_OK, "N = 0"); }
    { Call c; c.prefix[1] = 0; c.ws_bytes = hpl_normals_workspace_bytes(1, 0); expect(c.run() == HPL_OK, "N = 0, exact workspace"); }
    { Call c; c.prefix[1] = 0; c.pc_ld = c.normal_ld = 0; c.curvature = c.count = c.nbr = c.nbr_d2 = 0; c.k = 3; c.radius = 1e-30f;
      expect(c.run() == HPL_OK, "N = 0, no optional array"); }
    { Call c; c.prefix[1] = 0; c.normal = c.pc; c.nbr = c.ws; expect(c.run() == HPL_OK, "N = 0: nothing to overlap"); }
    { Call c; c.batch = 64; for (int b = 0; b <= 64; ++b) c.prefix[b] = 0; c.null_view = false; c.k = 32; c.radius = 1e30f;
      expect(c.run() == HPL_OK, "64 empty clouds with viewpoints"); }
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
