// batch_io.hip -- batched inference and training around the native program (include/hpl_bcl.h hpl_plan_run_batch,
// hpl_batch_stage).  A batch of B pairs is
// one pair of clouds whose rows are pair-major (csrc/lattice_fused.hip); the forward program runs on it unchanged.  Its point
// load reads a (3, n) matrix per cloud, so the (B, 3, N) clouds are laid out as (3, B x N) in the workspace's tail first:
// one launch over 3 x B x (N1 + N2) floats.  The flow it writes, an [B x N1][3] matrix, IS the (B, N1, 3) output.
// A ragged batch (pairs of their own point counts, hpl_ragged_stage) is staged the same way from B per-pair clouds.
#include "common.h"

#include <string.h>

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

// (B, 3, np_a) -> (3, B * np_a) for up to three arrays a in one launch; V = float4 moves four consecutive points of a row
// (every np_a % 4 == 0, every pointer 16-byte aligned), np_a counted in V.  Grid-stride, lanes walk the destination in order.
template <typename V>
__global__ void __launch_bounds__(256) k_batch_stage(const V *__restrict__ s0, const V *__restrict__ s1, const V *__restrict__ s2,
                                                     int64_t np0, int64_t np1, int64_t np2, int batch, V *__restrict__ d0,
                                                     V *__restrict__ d1, V *__restrict__ d2) {
    const int64_t t0 = 3 * batch * np0, t1 = t0 + 3 * batch * np1, total = t1 + (s2 ? 3 * batch * np2 : 0);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int a = i < t0 ? 0 : (i < t1 ? 1 : 2);
        const int64_t j = i - (a == 0 ? 0 : (a == 1 ? t0 : t1)), np = a == 0 ? np0 : (a == 1 ? np1 : np2), rows = batch * np;
        const int64_t k = j / rows, r = j - k * rows, b = r / np, p = r - b * np;      // dst[k][r], r = b * np + p
        const V *src = a == 0 ? s0 : (a == 1 ? s1 : s2);
        V *dst = a == 0 ? d0 : (a == 1 ? d1 : d2);
        dst[j] = src[(b * 3 + k) * np + p];
    }
}

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// ragged staging: B per-pair (3, ld_b) clouds -> one (3, sum n_b) matrix per side, for up to three sides (clouds 1, 2, target
// flow).  The descriptors travel in the kernel arguments (3 x 64 x 16 bytes + the prefixes): no table, no copy, no host sync.
constexpr int RAGGED_SIDES = 3;
constexpr int RAGGED_MAX = 64;
struct RaggedSide {
    const void *src[RAGGED_MAX];    // pair b's coordinate rows, row k at src[b] + k * ld[b] (elements of V)
    int32_t ld[RAGGED_MAX];
    int32_t off[RAGGED_MAX + 1];    // prefixes of the pairs' counts (elements of V); off[batch] = the side's total
    void *dst;                      // (3, off[batch])
    int32_t total;                  // 3 x off[batch]
    int32_t pad_;
};
struct RaggedArgs {
    RaggedSide side[RAGGED_SIDES];
    int32_t batch, n_sides;
};

// Grid-stride over the destination elements of every side in order; an element's pair by a branch-free search of the
// side's prefixes (the lanes of a wave inside one pair -- all but the waves across a boundary -- read the same words).
template <typename V>
__global__ void __launch_bounds__(256) k_ragged_stage(const RaggedArgs a) {
    int64_t t0 = 0;
    for (int si = 0; si < a.n_sides; ++si) {
        const RaggedSide &S = a.side[si];
        const int rows = S.off[a.batch];
        const int64_t step = (int64_t)gridDim.x * 256;
        int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x - t0;      // (one grid-stride walk over the sides in order)
        if (i < 0) i += (-i + step - 1) / step * step;
        for (; i < S.total; i += step) {
            const int j = (int)i, k = j / rows, r = j - k * rows;
            int b = 0;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) b = (b + s < a.batch && S.off[b + s] <= r) ? b + s : b;
            const V *src = reinterpret_cast<const V *>(S.src[b]);
            reinterpret_cast<V *>(S.dst)[j] = src[(int64_t)k * S.ld[b] + (r - S.off[b])];
        }
        t0 += S.total;
    }
}

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

extern "C" int hpl_batch_stage(int batch, int64_t n1, int64_t n2, const float *pc1, const float *pc2, const float *sf, float *dst1,
                               float *dst2, float *dst_sf, hplStream stream) {
    HPL_REQUIRE(pc1 && pc2 && dst1 && dst2 && (!sf || dst_sf), "hpl_batch_stage: null argument");
    HPL_REQUIRE(batch >= 1 && batch <= 64 && n1 >= 1 && n2 >= 1, "hpl_batch_stage: %d pairs of %lld / %lld points (1 .. 64 pairs)",
                batch, (long long)n1, (long long)n2);
    const int64_t total = 3 * batch * (n1 + n2 + (sf ? n1 : 0));
    const bool vec = n1 % 4 == 0 && n2 % 4 == 0 && aligned16(pc1) && aligned16(pc2) && aligned16(dst1) && aligned16(dst2) &&
                     (!sf || (aligned16(sf) && aligned16(dst_sf)));
    hipStream_t s = to_stream(stream);
    if (vec) {
        const int grid = (int)imin(cdiv(total / 4, 256), 2048);
        k_batch_stage<float4><<<grid, 256, 0, s>>>(reinterpret_cast<const float4 *>(pc1), reinterpret_cast<const float4 *>(pc2),
                                                   reinterpret_cast<const float4 *>(sf), n1 / 4, n2 / 4, n1 / 4, batch,
                                                   reinterpret_cast<float4 *>(dst1), reinterpret_cast<float4 *>(dst2),
                                                   reinterpret_cast<float4 *>(dst_sf));
    } else {
        const int grid = (int)imin(cdiv(total, 256), 2048);
        k_batch_stage<float><<<grid, 256, 0, s>>>(pc1, pc2, sf, n1, n2, n1, batch, dst1, dst2, dst_sf);
    }
    HPL_CHECK_LAUNCH("hpl_batch_stage");
    return HPL_OK;
}

extern "C" int hpl_ragged_stage(int batch, const float *const *pc1, const int64_t *n1, const int64_t *ld1, const float *const *pc2,
                                const int64_t *n2, const int64_t *ld2, const float *const *sf, const int64_t *ldsf, float *dst1,
                                float *dst2, float *dst_sf, hplStream stream) {
    HPL_REQUIRE(pc1 && n1 && ld1 && pc2 && n2 && ld2 && dst1 && dst2 && (!sf || (ldsf && dst_sf)), "hpl_ragged_stage: null argument");
    HPL_REQUIRE(batch >= 1 && batch <= RAGGED_MAX, "hpl_ragged_stage: %d pairs (1 .. %d)", batch, RAGGED_MAX);
    const float *const *src[RAGGED_SIDES] = {pc1, pc2, sf};
    const int64_t *cnt[RAGGED_SIDES] = {n1, n2, n1}, *ld[RAGGED_SIDES] = {ld1, ld2, ldsf};
    float *dst[RAGGED_SIDES] = {dst1, dst2, dst_sf};
    const int sides = sf ? 3 : 2;
    // 16-byte accesses when every count, stride and pointer allows them (float4 = 4 consecutive points of a row)
    bool vec = aligned16(dst1) && aligned16(dst2) && (!sf || aligned16(dst_sf));
    int64_t total = 0;
    for (int si = 0; si < sides; ++si) {
        int64_t t = 0;
        for (int b = 0; b < batch; ++b) {
            HPL_REQUIRE(src[si][b], "hpl_ragged_stage: no cloud for pair %d", b);
            HPL_REQUIRE(cnt[si][b] >= 1 && ld[si][b] >= cnt[si][b], "hpl_ragged_stage: pair %d has %lld points, row stride %lld", b,
                        (long long)cnt[si][b], (long long)ld[si][b]);
            t += cnt[si][b];
            HPL_REQUIRE(3 * t < INT32_MAX && 3 * ld[si][b] < INT32_MAX, "hpl_ragged_stage: more than 2^31 elements");
            vec = vec && cnt[si][b] % 4 == 0 && ld[si][b] % 4 == 0 && aligned16(src[si][b]);
        }
        total += 3 * t;
    }
    RaggedArgs a;
    memset(&a, 0, sizeof(a));
    a.batch = batch;
    a.n_sides = sides;
    const int w = vec ? 4 : 1;
    for (int si = 0; si < sides; ++si) {
        RaggedSide &S = a.side[si];
        S.off[0] = 0;
        for (int b = 0; b < batch; ++b) {
            S.src[b] = src[si][b];
            S.ld[b] = (int32_t)(ld[si][b] / w);
            S.off[b + 1] = S.off[b] + (int32_t)(cnt[si][b] / w);
        }
        S.dst = dst[si];
        S.total = 3 * S.off[batch];
    }
    hipStream_t s = to_stream(stream);
    const int grid = (int)imin(cdiv(total / w, 256), 2048);
    if (vec) k_ragged_stage<float4><<<grid, 256, 0, s>>>(a);
    else k_ragged_stage<float><<<grid, 256, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_ragged_stage");
    return HPL_OK;
}
