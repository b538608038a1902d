// icp_plane.hip -- rigid registration of a cloud pair by robust point-to-PLANE ICP (hpl_icp_plane): hpl_icp
// (icp.hip) with the residual taken along the matched dst point's normal.  The grid, the keys, the match, the
// finish and the fold are icp.hip's own (icp_common.h); the round and its solve differ.
//
//   k_icpp_round   per round: icp.hip's split (workgroups of 256 lanes over 1024 consecutive src points of one pair).  A lane
//                  matches its moved point, reads the match's normal, and adds its 28 float64 terms -- W, the 21 upper entries
//                  of H = sum u J J^T and g = sum u r J with J = ((y - c) x n, n) --; one LDS tree per workgroup
//                  (28 x 256 doubles, 57 344 bytes) into the partials
//   k_icpp_solve   per round: a workgroup per pair folds the partials, lane 0 takes the eigen-decomposition of H by cyclic
//                  Jacobi, the minimum-norm step x = -H^+ g over the eigenvalues above 1e-10 of the largest, the rotation
//                  exp([omega]x) by Rodrigues' formula, and hands on the new motion rounded to float32
//
// A direction the geometry does not observe (sliding along a single plane) gets no update and does not fail the pair.
// R is a product of one rotation per round, each product rounded to float32: after T rounds R^T R differs from I by at most
// about 6 T 2^-24 per entry (three products of entries <= 1, each entry off by 2^-25, per round, and their first-order sum); it
// is not re-projected.  No floating-point atomic, no read-back, no lane waits for another.
#include "icp_common.h"

namespace {

constexpr int ICPP_SUMS = 28;                        // W, H (21, row-major upper), g (6)
constexpr int ICPP_RUNS = ICP_BLOCK / 32;            // strided runs of the solve kernel's sum: 32 lanes a run >= 28 sums
constexpr int ICPP_SWEEPS = 16;                      // cyclic Jacobi sweeps of the 6 x 6 H at most
constexpr double ICPP_RANK = 1e-10;                  // an eigenvalue takes part above this share of the largest

__global__ void __launch_bounds__(ICP_BLOCK) k_icpp_round(const IcpArgs a) {
    __shared__ double red[ICPP_SUMS][ICP_BLOCK];
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
    double acc[ICPP_SUMS];
#pragma unroll
    for (int k = 0; k < ICPP_SUMS; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int j = 0; j < ICP_PER_LANE; ++j) {
        const int64_t i = base + j * ICP_BLOCK + t;
        if (i >= p1) continue;
        const SrcPoint s = match_point(a, b, i, R);
        if (!(s.w > 0.f) || s.match < 0) continue;
        const float nx = a.dnormal[s.match], ny = a.dnormal[a.dnormal_ld + s.match], nz = a.dnormal[2 * a.dnormal_ld + s.match];
        if (!(isfinite(nx) && isfinite(ny) && isfinite(nz)) || (nx == 0.f && ny == 0.f && nz == 0.f)) continue;     // u = 0
        double J[6], e[3];
        J[3] = (double)nx; J[4] = (double)ny; J[5] = (double)nz;
        double r = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r = r + (s.y[k] - s.q[k]) * J[3 + k];
            e[k] = s.y[k] - piv[k];
        }
        J[0] = e[1] * J[5] - e[2] * J[4];                    // (y - c) x n
        J[1] = e[2] * J[3] - e[0] * J[5];
        J[2] = e[0] * J[4] - e[1] * J[3];
        const double g = 1.0 + (r * r) * a.itau2;
        const double u = (double)s.w / (g * g);              // Geman-McClure
        acc[0] += u;
        int at = 1;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const double uj = u * J[p];
#pragma unroll
            for (int q = p; q < 6; ++q) acc[at++] += uj * J[q];
            acc[22 + p] += uj * r;
        }
    }
    block_tree_sum(red, acc, t);
    if (t < ICPP_SUMS) a.partials[(int64_t)blk * ICPP_SUMS + t] = red[t][0];
}

__global__ void __launch_bounds__(ICP_BLOCK) k_icpp_solve(const IcpArgs a) {
    __shared__ double run[ICPP_RUNS][ICPP_SUMS];
    __shared__ double tot[ICPP_SUMS];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    State *st = a.state + b;
    if (st->status == 0 || st->done != 0) return;            // a finished pair's state is left alone
    fold_partials<ICPP_SUMS, ICPP_RUNS, ICP_BLOCK>(a.partials, a.bprefix[b], a.bprefix[b + 1] - a.bprefix[b], run, tot, t);
    if (t != 0) return;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < ICPP_SUMS; ++i) ok = ok && isfinite(tot[i]);
    ok = ok && tot[0] > 0.0;
    float m[12];
    if (ok) {
        double H[6][6], V[6][6], g[6];
        int at = 1;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
#pragma unroll
            for (int q = p; q < 6; ++q) { H[p][q] = tot[at]; H[q][p] = tot[at]; ++at; }
            g[p] = tot[22 + p];
        }
        jacobi_eigen(H, V, ICPP_SWEEPS);
        double lmax = H[0][0];
#pragma unroll
        for (int i = 1; i < 6; ++i) lmax = fmax(lmax, H[i][i]);
        ok = lmax > 0.0;                                     // (NaN fails)
        double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (H[i][i] > ICPP_RANK * lmax) {
                double vg = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) vg += V[k][i] * g[k];
                const double f = vg / H[i][i];
#pragma unroll
                for (int k = 0; k < 6; ++k) x[k] -= V[k][i] * f;
            }
        }
        // E = exp([omega]x) = I + sin(theta) / theta K + (1 - cos(theta)) / theta^2 K^2
        const double th = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
        const double K[3][3] = {{0.0, -x[2], x[1]}, {x[2], 0.0, -x[0]}, {-x[1], x[0], 0.0}};
        double E[3][3];
        const double fa = th < 1e-12 ? 1.0 : sin(th) / th, fb = th < 1e-12 ? 0.0 : (1.0 - cos(th)) / (th * th);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double k2 = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) k2 += K[i][k] * K[k][j];
                E[i][j] = (i == j ? 1.0 : 0.0) + fa * K[i][j] + fb * k2;
            }
        double piv[3], R0[12];
        pivot_of(a, a.sprefix[b], piv);
#pragma unroll
        for (int i = 0; i < 12; ++i) R0[i] = (double)st->m[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) m[3 * i + j] = (float)((E[i][0] * R0[j] + E[i][1] * R0[3 + j]) + E[i][2] * R0[6 + j]);
            m[9 + i] = (float)((((E[i][0] * (R0[9] - piv[0]) + E[i][1] * (R0[10] - piv[1])) + E[i][2] * (R0[11] - piv[2])) + piv[i]) + x[3 + i]);
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) ok = ok && isfinite(m[i]);      // what the round hands on is what a caller reads from Rt
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
        partials = c.take((cdiv(n, ICP_SPAN) + batch) * ICPP_SUMS * (int64_t)sizeof(double));
        key = c.take(m * 8);
        skey = c.take(m * 8);
        rec = c.take(m * (int64_t)sizeof(GridRec));
        srec = c.take(m * (int64_t)sizeof(GridRec));
        bytes = c.bytes;
    }
};

int64_t workspace_bytes(int batch, int64_t n, int64_t m) { return Layout(batch, n, m).bytes + temp_room(m); }

}  // namespace

extern "C" int64_t hpl_icp_plane_workspace_bytes(int batch, int64_t n_src, int64_t n_dst) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || n_src < 0 || n_src >= CLOUD_MAX_POINTS || n_dst < 0 || n_dst >= CLOUD_MAX_POINTS)
        return -1;
    return workspace_bytes(batch, n_src, n_dst);
}

extern "C" int hpl_icp_plane(const float *src, int64_t src_ld, const float *dst, int64_t dst_ld, const float *dst_normal,
                             int64_t dnormal_ld, const float *weight, const float *init, int batch, const int64_t *src_prefix,
                             const int64_t *dst_prefix, int iters, float max_dist, float tau, float tol_rot, float tol_trans,
                             float *Rt, float *stats, int32_t *match, float *dist2, float *flow, void *workspace,
                             int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_icp_plane";
    HPL_REQUIRE(src && Rt && stats && src_prefix && dst_prefix && workspace, "hpl_icp_plane: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(iters >= 0 && iters <= ICP_MAX_ITERS, "hpl_icp_plane: iters = %d (0 .. %d)", iters, ICP_MAX_ITERS);
    HPL_REQUIRE(max_dist > 0.f && isfinite(max_dist), "hpl_icp_plane: max_dist must be finite and > 0");
    HPL_REQUIRE(tau > 0.f && isfinite(tau), "hpl_icp_plane: tau must be finite and > 0");
    HPL_REQUIRE(tol_rot >= 0.f && tol_trans >= 0.f, "hpl_icp_plane: tol_rot and tol_trans must be >= 0");      // (NaN fails)
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix of src", "pair", src_prefix, batch));
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix of dst", "pair", dst_prefix, batch));
    const int64_t N = src_prefix[batch], M = dst_prefix[batch];
    HPL_REQUIRE((dst && dst_normal) || M == 0, "hpl_icp_plane: null pointer (dst and dst_normal of %lld points)", (long long)M);
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_CLOUD_CHECK(check_points(op, M));
    HPL_CLOUD_CHECK(check_row_stride(op, src_ld, N));
    HPL_CLOUD_CHECK(check_row_stride(op, dst_ld, M));
    HPL_CLOUD_CHECK(check_row_stride(op, dnormal_ld, M));
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, workspace_bytes(batch, N, M)));
    HPL_CLOUD_CHECK(check_aligned4(op, {src, dst, dst_normal, weight, init, Rt, stats, match, dist2, flow}));
    if (N == 0) return HPL_OK;

    const Layout L(batch, N, M);
    void *const temp = carved<char>(workspace, L.bytes);
    IcpArgs a{};
    a.src = src; a.src_ld = src_ld; a.dst = dst; a.dst_ld = dst_ld; a.weight = weight; a.init = init;
    a.dnormal = dst_normal; a.dnormal_ld = dnormal_ld;
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
    HPL_CHECK_LAUNCH("hpl_icp_plane (keys)");
    if (M > 0) {
        size_t tb = (size_t)temp_room(M);
        const hipError_t e = rocprim::radix_sort_pairs(temp, tb, (const u64 *)a.key, a.skey, (const GridRec *)a.rec, a.srec, (size_t)M,
                                                       0u, 64u, s);      // (the largest key, of the points left out, has every bit set)
        if (e != hipSuccess) { set_error("hpl_icp_plane: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    }
    for (int k = 0; k < iters; ++k) {
        k_icpp_round<<<(unsigned)blocks, ICP_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_icp_plane (round)");
        k_icpp_solve<<<batch, ICP_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_icp_plane (solve)");
    }
    k_icp_finish<<<(unsigned)blocks, ICP_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_icp_plane (finish)");
    k_icp_fold<<<batch, ICP_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_icp_plane (fold)");
    return HPL_OK;
}
