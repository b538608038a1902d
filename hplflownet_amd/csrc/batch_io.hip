// batch_io.hip -- batched inference around the native forward (include/hpl_bcl.h hpl_plan_run_batch).  A batch of B pairs is
// one pair of clouds whose rows are pair-major (csrc/lattice_fused.hip); the forward program runs on it unchanged.  Its point
// load reads a (3, n) matrix per cloud, so the (B, 3, N) clouds are laid out as (3, B x N) in the workspace's tail first:
// one launch over 3 x B x (N1 + N2) floats.  The flow it writes, an [B x N1][3] matrix, IS the (B, N1, 3) output.
#include "common.h"

using namespace hpl;

namespace {

// (B, 3, np) -> (3, B * np), both clouds in one launch
__global__ void k_pair_major(const float *__restrict__ pc1, int64_t np1, const float *__restrict__ pc2, int64_t np2, int batch,
                             float *__restrict__ dst1, float *__restrict__ dst2) {
    const int64_t n1 = batch * np1 * 3, total = n1 + batch * np2 * 3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const bool two = i >= n1;
        const int64_t j = two ? i - n1 : i, np = two ? np2 : np1, rows = batch * np;
        const int64_t k = j / rows, r = j - k * rows, b = r / np, p = r - b * np;      // dst[k][r], r = b * np + p
        (two ? dst2 : dst1)[j] = (two ? pc2 : pc1)[(b * 3 + k) * np + p];
    }
}

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" int64_t hpl_plan_batch_extra_bytes(const hpl_level_tables *levels, int n_levels) {
    if (!levels || n_levels < 1) return -1;
    return align256(3 * levels[0].n0 * 4) + align256(3 * levels[0].n1 * 4) + 256;
}

extern "C" int hpl_plan_run_batch(hpl_plan *plan, const hpl_level_tables *levels, int n_levels, int batch, const float *pc1,
                                  const float *pc2, float *out, void *workspace, int64_t workspace_bytes, hplStream stream) {
    HPL_REQUIRE(plan && levels && n_levels >= 1 && pc1 && pc2 && out && workspace, "hpl_plan_run_batch: null argument");
    HPL_REQUIRE(batch >= 1 && batch <= 64, "hpl_plan_run_batch: %d pairs (1 .. 64)", batch);
    if (batch == 1) return hpl_plan_run(plan, levels, n_levels, pc1, pc2, out, workspace, workspace_bytes, stream);
    const int64_t n0 = levels[0].n0, n1 = levels[0].n1;
    HPL_REQUIRE(n0 % batch == 0 && n1 % batch == 0, "hpl_plan_run_batch: the lattice's %lld / %lld points are not %d equal pairs",
                (long long)n0, (long long)n1, batch);
    const int64_t need = hpl_plan_workspace_bytes(plan, levels, n_levels);
    const int64_t extra = hpl_plan_batch_extra_bytes(levels, n_levels);
    HPL_REQUIRE(need > 0 && workspace_bytes >= need + extra, "hpl_plan_run_batch: workspace of %lld bytes, needs %lld + %lld",
                (long long)workspace_bytes, (long long)need, (long long)extra);
    // the staged clouds sit behind everything the forward uses (its layout is carved from the start of the workspace)
    const uintptr_t tail = (reinterpret_cast<uintptr_t>(workspace) + workspace_bytes - (extra - 256)) / 256 * 256;
    float *s1 = reinterpret_cast<float *>(tail);
    float *s2 = reinterpret_cast<float *>(tail + align256(3 * n0 * 4));
    const int64_t total = 3 * (n0 + n1);
    k_pair_major<<<(unsigned)imin(cdiv(total, 256), 2048), 256, 0, to_stream(stream)>>>(pc1, n0 / batch, pc2, n1 / batch, batch, s1, s2);
    HPL_CHECK_LAUNCH("hpl_plan_run_batch (pair-major clouds)");
    return hpl_plan_run(plan, levels, n_levels, s1, s2, out, workspace, need, stream);
}
