// icp.hip -- rigid registration of a cloud pair from the clouds alone (hpl_icp): point-to-point ICP with
// Geman-McClure weights, the nearest neighbours taken exactly within a radius on a sorted uniform grid over dst.
//
// The definition of a match is the all-pairs one of include/hpl_bcl.h; the grid only finds the candidates.  The cell edge is
// 1.001 max_dist and a point's cell floor(x / (1.001 max_dist)) is taken in float64, so a dst point within max_dist of a query
// (even by the rounded float32 d2, which can exceed the real one by a few 2^-24) lies in the query's cell or in an adjacent
// one: 27 cells hold every acceptable match, and a nearest point that is not acceptable is no match whichever it is.
//
//   k_icp_keys     a lane per dst point: the 64-bit key (pair, cell x, y, z) of grid_common.h (a point that takes
//                  no part carries the largest key) and its 16-byte (x, y, z, index) record; the first lanes set the pairs' state
//   rocPRIM        ONE stable radix sort of (key, record) per call
//   k_icp_round    per round: workgroups of 256 lanes, each inside one pair and over 1024 consecutive src points (rigid_fit's
//                  split).  A lane moves its point by the round's float32 motion, reads the 27 cells around the query as 9 runs
//                  of three z-adjacent cells (two binary searches each, all 18 in lockstep), keeps the smallest d2 (ties: the
//                  smaller dst index) and adds its 16 float64 terms; one LDS tree per workgroup into the partials
//   k_icp_solve    per round: a workgroup per pair folds the partials in rigid_fit's order, lane 0 solves (rigid_solve.h),
//                  rounds (R, t) to float32, compares with the motion the round started from and stores it
//   k_icp_finish   the match under the final motion: match, dist2, flow, and per workgroup the float64 sum of r2 and the count
//   k_icp_fold     a workgroup per pair: Rt and stats
//
// A finished or failed pair's workgroups return at once.  No floating-point atomic, no read-back, no lane waits for another;
// every loop is bounded by a cell population or a search depth.  The bits depend on the pair alone.
#include "icp_common.h"

namespace {

__global__ void __launch_bounds__(ICP_BLOCK) k_icp_round(const IcpArgs a) {
    __shared__ double red[RIGID_SUMS][ICP_BLOCK];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = group_of(a.bprefix, a.batch, blk);
    const State *st = a.state + b;
    if (st->status == 0 || st->done != 0) return;            // (uniform over the workgroup)
    const int p0 = a.sprefix[b], p1 = a.sprefix[b + 1];
    const int64_t base = (int64_t)p0 + (int64_t)(blk - a.bprefix[b]) * ICP_SPAN;
    double piv[3], R[12];
    pivot_of(a, p0, piv);
#pragma unroll
    for (int k = 0; k < 12; ++k) R[k] = (double)st->m[k];
    double acc[RIGID_SUMS];
#pragma unroll
    for (int k = 0; k < RIGID_SUMS; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int j = 0; j < ICP_PER_LANE; ++j) {
        const int64_t i = base + j * ICP_BLOCK + t;
        if (i >= p1) continue;
        const SrcPoint s = match_point(a, b, i, R);
        if (!(s.w > 0.f) || s.match < 0) continue;
        const double g = 1.0 + residual2(s) * a.itau2;
        const double u = (double)s.w / (g * g);              // Geman-McClure
        double dp[3], dq[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { dp[k] = s.p[k] - piv[k]; dq[k] = s.q[k] - piv[k]; }
        acc[0] += u;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double up = u * dp[k];
            acc[1 + k] += up;
            acc[4 + k] += u * dq[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[7 + 3 * k + c] += up * dq[c];
        }
    }
    block_tree_sum(red, acc, t);
    if (t < RIGID_SUMS) a.partials[(int64_t)blk * RIGID_SUMS + t] = red[t][0];
}

__global__ void __launch_bounds__(ICP_BLOCK) k_icp_solve(const IcpArgs a) {
    __shared__ double run[ICP_RUNS][RIGID_SUMS];
    __shared__ double tot[RIGID_SUMS];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    State *st = a.state + b;
    if (st->status == 0 || st->done != 0) return;            // a finished pair's state is left alone
    fold_partials<RIGID_SUMS, ICP_RUNS, ICP_BLOCK>(a.partials, a.bprefix[b], a.bprefix[b + 1] - a.bprefix[b], run, tot, t);
    if (t != 0) return;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < RIGID_SUMS; ++i) ok = ok && isfinite(tot[i]);
    ok = ok && tot[0] > 0.0;
    float m[12];
    if (ok) {
        double piv[3], R[12], angle, tn;
        pivot_of(a, a.sprefix[b], piv);
        rigid_from_sums(tot, piv, R, angle, tn);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            m[i] = (float)R[i];                              // what the round hands on is what a caller reads from Rt
            ok = ok && isfinite(m[i]);
        }
    }
    st->rounds = st->rounds + 1;
    if (!ok) {                                               // the motion stays the one the round started from
        st->status = 0;
        return;
    }
    bool still = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        still = still && fabs((double)m[i] - (double)st->m[i]) <= (double)(i < 9 ? a.tol_rot : a.tol_trans);
        st->m[i] = m[i];
    }
    st->done = still ? 1 : 0;
}

// workspace: state | partials | key | sorted key | records | sorted records | rocPRIM temporaries
struct Layout {                  // byte offsets
    int64_t state, partials, key, skey, rec, srec, bytes;
    Layout(int batch, int64_t n, int64_t m) {
        Carver c;
        state = c.take((int64_t)batch * (int64_t)sizeof(State));
        partials = c.take((cdiv(n, ICP_SPAN) + batch) * RIGID_SUMS * (int64_t)sizeof(double));
        key = c.take(m * 8);
        skey = c.take(m * 8);
        rec = c.take(m * (int64_t)sizeof(GridRec));
        srec = c.take(m * (int64_t)sizeof(GridRec));
        bytes = c.bytes;
    }
};

int64_t workspace_bytes(int batch, int64_t n, int64_t m) { return Layout(batch, n, m).bytes + temp_room(m); }

}  // namespace

extern "C" int64_t hpl_icp_workspace_bytes(int batch, int64_t n_src, int64_t n_dst) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || n_src < 0 || n_src >= CLOUD_MAX_POINTS || n_dst < 0 || n_dst >= CLOUD_MAX_POINTS)
        return -1;
    return workspace_bytes(batch, n_src, n_dst);
}

extern "C" int hpl_icp(const float *src, int64_t src_ld, const float *dst, int64_t dst_ld, const float *weight, const float *init,
                       int batch, const int64_t *src_prefix, const int64_t *dst_prefix, int iters, float max_dist, float tau,
                       float tol_rot, float tol_trans, float *Rt, float *stats, int32_t *match, float *dist2, float *flow,
                       void *workspace, int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_icp";
    HPL_REQUIRE(src && Rt && stats && src_prefix && dst_prefix && workspace, "hpl_icp: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(iters >= 0 && iters <= ICP_MAX_ITERS, "hpl_icp: iters = %d (0 .. %d)", iters, ICP_MAX_ITERS);
    HPL_REQUIRE(max_dist > 0.f && isfinite(max_dist), "hpl_icp: max_dist must be finite and > 0");
    HPL_REQUIRE(tau > 0.f && isfinite(tau), "hpl_icp: tau must be finite and > 0");
    HPL_REQUIRE(tol_rot >= 0.f && tol_trans >= 0.f, "hpl_icp: tol_rot and tol_trans must be >= 0");      // (NaN fails)
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix of src", "pair", src_prefix, batch));
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix of dst", "pair", dst_prefix, batch));
    const int64_t N = src_prefix[batch], M = dst_prefix[batch];
    HPL_REQUIRE(dst || M == 0, "hpl_icp: null pointer");
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_CLOUD_CHECK(check_points(op, M));
    HPL_CLOUD_CHECK(check_row_stride(op, src_ld, N));
    HPL_CLOUD_CHECK(check_row_stride(op, dst_ld, M));
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, workspace_bytes(batch, N, M)));
    HPL_CLOUD_CHECK(check_aligned4(op, {src, dst, weight, init, Rt, stats, match, dist2, flow}));
    if (N == 0) return HPL_OK;

    const Layout L(batch, N, M);
    void *const temp = carved<char>(workspace, L.bytes);
    IcpArgs a{};
    a.src = src; a.src_ld = src_ld; a.dst = dst; a.dst_ld = dst_ld; a.weight = weight; a.init = init;
    a.state = carved<State>(workspace, L.state);
    a.partials = carved<double>(workspace, L.partials);
    a.key = carved<u64>(workspace, L.key); a.skey = carved<u64>(workspace, L.skey);
    a.rec = carved<GridRec>(workspace, L.rec); a.srec = carved<GridRec>(workspace, L.srec);
    a.Rt = Rt; a.stats = stats; a.match = match; a.dist2 = dist2; a.flow = flow;
    a.inv_cell = 1.0 / (GRID_CELL_MARGIN * (double)max_dist);
    a.itau2 = 1.0 / ((double)tau * (double)tau);
    a.md2 = max_dist * max_dist;                 // rounded once to float32, as the acceptance states
    a.tol_rot = tol_rot; a.tol_trans = tol_trans;
    a.m = (int32_t)M; a.batch = batch;
    const int64_t blocks = narrow_prefix(src_prefix, batch, ICP_SPAN, a.sprefix, a.bprefix);
    narrow_prefix(dst_prefix, batch, ICP_BLOCK, a.dprefix, nullptr);

    hipStream_t s = to_stream(stream);
    k_icp_keys<<<(unsigned)imax(cdiv(M, ICP_BLOCK), (int64_t)1), ICP_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_icp (keys)");
    if (M > 0) {
        size_t tb = (size_t)temp_room(M);
        const hipError_t e = rocprim::radix_sort_pairs(temp, tb, (const u64 *)a.key, a.skey, (const GridRec *)a.rec, a.srec, (size_t)M,
                                                       0u, 64u, s);      // (the largest key, of the points left out, has every bit set)
        if (e != hipSuccess) { set_error("hpl_icp: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    }
    for (int k = 0; k < iters; ++k) {
        k_icp_round<<<(unsigned)blocks, ICP_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_icp (round)");
        k_icp_solve<<<batch, ICP_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_icp (solve)");
    }
    k_icp_finish<<<(unsigned)blocks, ICP_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_icp (finish)");
    k_icp_fold<<<batch, ICP_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_icp (fold)");
    return HPL_OK;
}
