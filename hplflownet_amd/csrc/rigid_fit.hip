// rigid_fit.hip -- the rigid motion (R, t) that explains most of a pair's flow, robustly, and the flow refined by it
// (hpl_rigid_fit): ego-motion from a scene-flow field without a host round trip.
//
// Per round two launches.  k_rigid_reduce: workgroups of 256 lanes, each inside ONE pair (the host gives the pairs' first
// workgroups in the kernel arguments beside the point prefix) and over a span of 1024 consecutive points of it, lane l taking
// points l, l + 256, l + 512, l + 768 of the span (coalesced dword loads: a pair may start at any index of any row stride, so
// no wider load is aligned in general).  A point's weight of the round comes from the previous round's (R, t), read from the
// workspace: reweight and reduce are one pass.  16 float64 sums per workgroup -- W, sum u dp, sum u dq, sum u dp dq^T about the
// pair's first point -- go through a fixed LDS tree into the workspace.  k_rigid_solve: one workgroup per pair adds the
// partials in a fixed order (16 strided runs in index order, then the runs in order) and lane 0 solves: Horn's unit quaternion,
// the dominant eigenvector of the symmetric 4x4 matrix of H by cyclic Jacobi sweeps in float64.  A quaternion is a proper
// rotation whatever the cloud: there is no determinant to fix.  k_rigid_apply writes residual, refined and the inlier share
// (integer counts: their order does not matter).  2 (iters + 1) + 1 launches, no copy, no read-back, no floating-point atomic:
// the bits depend on the pair alone, not on its place in a batch or on what else the device runs.
//
// The arithmetic is part of the interface (include/hpl_bcl.h; tests/rigid_oracle.py restates it in numpy with an SVD).
#include "cloud_common.h"
#include "rigid_solve.h"        // horn_quaternion, rigid_from_sums: shared with icp.hip

#include <math.h>

using namespace hpl;

namespace {

constexpr int RF_MAX_ITERS = 16;
constexpr int RF_BLOCK = 256;
constexpr int RF_PER_LANE = 4;
constexpr int RF_SPAN = RF_BLOCK * RF_PER_LANE;      // points per workgroup
constexpr int RF_SUMS = 16;                          // W, Sp[3], Sq[3], Spq[9]
constexpr int RF_STATE = 16;                         // doubles per pair: R[9], t[3], status, angle (deg), |t|, {inliers, done}
constexpr int RF_RUNS = RF_BLOCK / RF_SUMS;          // strided runs of the solve kernel's sum

struct RigidArgs {
    const float *pc;
    int64_t pc_ld;
    const float *flow;
    int64_t fsc, fsp;
    const float *weight;
    double *state;              // [batch][RF_STATE]
    double *partials;           // [workgroups][RF_SUMS]
    float *Rt, *stats, *residual, *refined;
    double tau;
    int32_t batch, round, last;
    int32_t pprefix[CLOUD_MAX_BATCH + 1];      // points of pairs 0 .. b-1 (N < 2^31 / 3)
    int32_t bprefix[CLOUD_MAX_BATCH + 1];      // workgroups of pairs 0 .. b-1
};

struct Point {
    double p[3], q[3];
    float f[3];
    float w;                     // the effective base weight: 0 for a weight that is not in (0, inf) and for a non-finite point
};

__device__ __forceinline__ Point load_point(const RigidArgs &a, int64_t i) {
    Point pt;
    const float x = a.pc[i], y = a.pc[a.pc_ld + i], z = a.pc[2 * a.pc_ld + i];
    const float *f = a.flow + i * a.fsp;
    pt.f[0] = f[0];
    pt.f[1] = f[a.fsc];
    pt.f[2] = f[2 * a.fsc];
    const float w = a.weight ? a.weight[i] : 1.f;
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(pt.f[0]) && isfinite(pt.f[1]) && isfinite(pt.f[2]);
    pt.w = (ok && w > 0.f && w < INFINITY) ? w : 0.f;
    pt.p[0] = (double)x; pt.p[1] = (double)y; pt.p[2] = (double)z;
#pragma unroll
    for (int k = 0; k < 3; ++k) pt.q[k] = pt.p[k] + (double)pt.f[k];
    return pt;
}

// |R p + t - q|^2 and, in m, R p + t - p
__device__ __forceinline__ double residual2(const double *R, const Point &pt, double *m) {
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double y = ((R[3 * k] * pt.p[0] + R[3 * k + 1] * pt.p[1]) + R[3 * k + 2] * pt.p[2]) + R[9 + k];
        const double d = y - pt.q[k];
        m[k] = y - pt.p[k];
        r2 = r2 + d * d;
    }
    return r2;
}

__global__ void __launch_bounds__(RF_BLOCK) k_rigid_reduce(const RigidArgs a) {
    __shared__ double red[RF_SUMS][RF_BLOCK];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = group_of(a.bprefix, a.batch, blk);
    const int p0 = a.pprefix[b], p1 = a.pprefix[b + 1];
    const int64_t base = (int64_t)p0 + (int64_t)(blk - a.bprefix[b]) * RF_SPAN;
    double piv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = a.pc[k * a.pc_ld + p0];
        piv[k] = isfinite(v) ? (double)v : 0.0;
    }
    double R[12];
    if (a.round > 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) R[k] = a.state[(int64_t)b * RF_STATE + k];
    }
    const double itau2 = 1.0 / (a.tau * a.tau);
    double acc[RF_SUMS];
#pragma unroll
    for (int k = 0; k < RF_SUMS; ++k) acc[k] = 0.0;
#pragma unroll
    for (int j = 0; j < RF_PER_LANE; ++j) {
        const int64_t i = base + j * RF_BLOCK + t;
        if (i >= p1) continue;
        const Point pt = load_point(a, i);
        if (!(pt.w > 0.f)) continue;
        double u = (double)pt.w;
        if (a.round > 0) {
            double m[3];
            const double s = 1.0 + residual2(R, pt, m) * itau2;
            u = u / (s * s);                     // Geman-McClure
        }
        double dp[3], dq[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { dp[k] = pt.p[k] - piv[k]; dq[k] = pt.q[k] - piv[k]; }
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
    if (t < RF_SUMS) a.partials[(int64_t)blk * RF_SUMS + t] = red[t][0];
}

__global__ void __launch_bounds__(RF_BLOCK) k_rigid_solve(const RigidArgs a) {
    __shared__ double run[RF_RUNS][RF_SUMS];
    __shared__ double tot[RF_SUMS];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    fold_partials<RF_SUMS, RF_RUNS, RF_BLOCK>(a.partials, a.bprefix[b], a.bprefix[b + 1] - a.bprefix[b], run, tot, t);
    if (t != 0) return;

    double *st = a.state + (int64_t)b * RF_STATE;
    const int p0 = a.pprefix[b], n = a.pprefix[b + 1] - p0;
    bool ok = n >= 3 && (a.round == 0 || st[12] != 0.0);     // a pair that failed at an earlier round stays failed
    const double W = tot[0];
#pragma unroll
    for (int i = 0; i < RF_SUMS; ++i) ok = ok && isfinite(tot[i]);
    ok = ok && W > 0.0;
    double R[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    double angle = 0.0, tn = 0.0;
    if (ok) {
        double piv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float v = a.pc[i * a.pc_ld + p0];
            piv[i] = isfinite(v) ? (double)v : 0.0;
        }
        rigid_from_sums(tot, piv, R, angle, tn);
#pragma unroll
        for (int i = 0; i < 12; ++i) ok = ok && isfinite(R[i]);
        if (!ok) {
            const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 12; ++i) R[i] = I[i];
            angle = tn = 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) st[i] = R[i];
    st[12] = ok ? 1.0 : 0.0;
    st[13] = angle;
    st[14] = tn;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(st + 15);       // the apply kernel's inlier count and finished workgroups
    cnt[0] = 0u;
    cnt[1] = 0u;
    if (a.last) {
#pragma unroll
        for (int i = 0; i < 12; ++i) a.Rt[(int64_t)b * 12 + i] = (float)R[i];
        float *o = a.stats + (int64_t)b * 4;
        o[0] = ok ? 1.f : 0.f;
        o[1] = 0.f;              // (k_rigid_apply's last workgroup of the pair writes the share of a fitted pair)
        o[2] = (float)angle;
        o[3] = (float)tn;
    }
}

__global__ void __launch_bounds__(RF_BLOCK) k_rigid_apply(const RigidArgs a) {
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = group_of(a.bprefix, a.batch, blk);
    const int p0 = a.pprefix[b], p1 = a.pprefix[b + 1];
    const int64_t base = (int64_t)p0 + (int64_t)(blk - a.bprefix[b]) * RF_SPAN;
    double *st = a.state + (int64_t)b * RF_STATE;
    double R[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) R[k] = st[k];
    const bool fitted = st[12] != 0.0;
    int inl = 0;
#pragma unroll
    for (int j = 0; j < RF_PER_LANE; ++j) {
        const int64_t i = base + j * RF_BLOCK + t;
        bool inlier = false;
        if (i < p1) {
            const Point pt = load_point(a, i);
            double m[3];
            // (a pair without a fit has R = I, t = 0: its residual is |f|)
            const double r = sqrt(residual2(R, pt, m));
            inlier = fitted && pt.w > 0.f && r <= a.tau;
            if (a.residual) a.residual[i] = (float)r;
            if (a.refined) {
                float *o = a.refined + i * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) o[k] = inlier ? (float)m[k] : pt.f[k];
            }
        }
        inl += __syncthreads_count(inlier ? 1 : 0);
    }
    if (t == 0 && fitted) {
        uint32_t *cnt = reinterpret_cast<uint32_t *>(st + 15);
        atomicAdd(&cnt[0], (uint32_t)inl);
        __threadfence();
        const uint32_t nb = (uint32_t)(a.bprefix[b + 1] - a.bprefix[b]);
        if (atomicAdd(&cnt[1], 1u) == nb - 1u) {             // the pair's last workgroup: every count is in
            __threadfence();
            const uint32_t total = atomicAdd(&cnt[0], 0u);
            a.stats[(int64_t)b * 4 + 1] = (float)((double)total / (double)(p1 - p0));
        }
    }
}

int64_t workspace_bytes(int batch, int64_t n_total) {
    return (int64_t)sizeof(double) * ((int64_t)batch * RF_STATE + (cdiv(n_total, RF_SPAN) + batch) * RF_SUMS);
}

}  // namespace

extern "C" int64_t hpl_rigid_fit_workspace_bytes(int batch, int64_t n_total) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || n_total < 0 || n_total >= CLOUD_MAX_POINTS) return -1;
    return workspace_bytes(batch, n_total);
}

extern "C" int hpl_rigid_fit(const float *pc, int64_t pc_ld, const float *flow, int64_t flow_sc, int64_t flow_sp,
                             const float *weight, int batch, const int64_t *prefix, int iters, float tau, float *Rt, float *stats,
                             float *residual, float *refined, void *workspace, int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_rigid_fit";
    HPL_REQUIRE(pc && flow && Rt && stats && prefix && workspace, "hpl_rigid_fit: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(iters >= 0 && iters <= RF_MAX_ITERS, "hpl_rigid_fit: iters = %d (0 .. %d)", iters, RF_MAX_ITERS);
    HPL_REQUIRE(tau > 0.f && isfinite(tau), "hpl_rigid_fit: tau must be finite and > 0");
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix", "pair", prefix, batch));
    const int64_t N = prefix[batch];
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_CLOUD_CHECK(check_row_stride(op, pc_ld, N));
    HPL_CLOUD_CHECK(check_flow_strides(op, flow_sc, flow_sp, N));
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 8, workspace_bytes_, workspace_bytes(batch, N)));
    HPL_CLOUD_CHECK(check_aligned4(op, {pc, flow, weight, Rt, stats, residual, refined}));
    if (N == 0) return HPL_OK;
    RigidArgs a{};
    const int64_t blocks = narrow_prefix(prefix, batch, RF_SPAN, a.pprefix, a.bprefix);
    a.pc = pc; a.pc_ld = pc_ld; a.flow = flow; a.fsc = flow_sc; a.fsp = flow_sp; a.weight = weight;
    a.state = static_cast<double *>(workspace);
    a.partials = a.state + (int64_t)batch * RF_STATE;
    a.Rt = Rt; a.stats = stats; a.residual = residual; a.refined = refined;
    a.tau = (double)tau;
    a.batch = batch;
    hipStream_t s = to_stream(stream);
    for (int k = 0; k <= iters; ++k) {
        a.round = k;
        a.last = k == iters;
        k_rigid_reduce<<<(unsigned)blocks, RF_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_rigid_fit (reduce)");
        k_rigid_solve<<<batch, RF_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_rigid_fit (solve)");
    }
    k_rigid_apply<<<(unsigned)blocks, RF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_rigid_fit (apply)");
    return HPL_OK;
}
