// icp_common.h -- what icp.hip (point-to-point) and icp_plane.hip (point-to-plane) share: the
// per-pair state, the keys kernel, the exact match of a moved src point within max_dist (match_point), the residual, the
// pivot, the finish, the fold and the room of the sort.  The grid itself (key, cell, record) is grid_common.h's
// (DESIGN.md §31).  IcpArgs carries the two fields of the normals (unused by icp.hip).  Header only; everything has internal
// linkage.
#pragma once
#include "grid_common.h"
#include "rigid_solve.h"

#include <limits.h>
#include <math.h>

using namespace hpl;

namespace {

constexpr int ICP_MAX_ITERS = 64;
constexpr int ICP_BLOCK = 256;
constexpr int ICP_PER_LANE = 4;
constexpr int ICP_SPAN = ICP_BLOCK * ICP_PER_LANE;   // src points per workgroup
constexpr int ICP_RUNS = ICP_BLOCK / RIGID_SUMS;
constexpr int ICP_AHEAD = 4;                         // records of a run loaded before they are compared

struct State {                  // per pair, 64 bytes
    float m[12];                // the current motion: R row-major, then t
    int32_t status;             // 1; 0 for a pair that cannot be fitted or whose round failed
    int32_t done;               // the last round moved nothing beyond the tolerances
    int32_t rounds;             // rounds run
    int32_t pad;
};

struct IcpArgs {
    const float *src;
    int64_t src_ld;
    const float *dst;
    int64_t dst_ld;
    const float *weight;
    const float *init;
    const float *dnormal;       // (3, M) SoA normals of dst (icp_plane.hip only)
    int64_t dnormal_ld;
    State *state;
    double *partials;           // [src workgroups][16]; the finish reuses it as [src workgroups][2]
    u64 *key, *skey;
    GridRec *rec, *srec;        // i: the packed dst index
    float *Rt, *stats, *dist2, *flow;
    int32_t *match;
    double inv_cell, itau2;
    float md2, tol_rot, tol_trans;
    int32_t m, batch;
    int32_t sprefix[CLOUD_MAX_BATCH + 1];      // src points of pairs 0 .. b-1
    int32_t dprefix[CLOUD_MAX_BATCH + 1];      // dst points of pairs 0 .. b-1
    int32_t bprefix[CLOUD_MAX_BATCH + 1];      // src workgroups of pairs 0 .. b-1
};

__global__ void __launch_bounds__(ICP_BLOCK) k_icp_keys(const IcpArgs a) {
    const int64_t j64 = (int64_t)blockIdx.x * ICP_BLOCK + threadIdx.x;
    if (blockIdx.x == 0 && (int)threadIdx.x < a.batch) {
        const int b = (int)threadIdx.x;
        State st;
#pragma unroll
        for (int k = 0; k < 12; ++k) st.m[k] = a.init ? a.init[b * 12 + k] : ((k < 9 && k % 4 == 0) ? 1.f : 0.f);
        st.status = (a.sprefix[b + 1] - a.sprefix[b] >= 3 && a.dprefix[b + 1] > a.dprefix[b]) ? 1 : 0;
        st.done = 0;
        st.rounds = 0;
        st.pad = 0;
        a.state[b] = st;
    }
    if (j64 >= a.m) return;
    const int j = (int)j64;
    grid_store(a, a.dprefix, j, a.dst[j], a.dst[a.dst_ld + j], a.dst[2 * a.dst_ld + j]);
}

struct SrcPoint {
    double p[3], y[3];           // the point and the moved point, float64
    double q[3];                 // the matched dst point
    float w;                     // the effective base weight
    float d2;                    // the match's float32 d2 (+inf: none)
    int32_t match;               // packed dst index (-1: none)
};

// Point i of pair b under the motion R (12 doubles widened from float32): its weight, the moved point and its match.
__device__ __forceinline__ SrcPoint match_point(const IcpArgs &a, int b, int64_t i, const double *R) {
    SrcPoint s;
    const float px = a.src[i], py = a.src[a.src_ld + i], pz = a.src[2 * a.src_ld + i];
    const float w = a.weight ? a.weight[i] : 1.f;
    const bool ok = isfinite(px) && isfinite(py) && isfinite(pz);
    s.w = (ok && w > 0.f && w < INFINITY) ? w : 0.f;
    s.p[0] = (double)px; s.p[1] = (double)py; s.p[2] = (double)pz;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.y[k] = ((R[3 * k] * s.p[0] + R[3 * k + 1] * s.p[1]) + R[3 * k + 2] * s.p[2]) + R[9 + k];
    const float qx = (float)s.y[0], qy = (float)s.y[1], qz = (float)s.y[2];
    float best = INFINITY;
    int bi = INT_MAX;
    float bx = 0.f, by = 0.f, bz = 0.f;          // the best candidate so far
    int c[3];
    if (a.m > 0 && grid_cell_of(a.inv_cell, qx, qy, qz, c)) {
        // The 9 runs [lo, hi): lower_bound of the run's first key and of the key behind its last, all 18 searches in lockstep.
        // The step sizes depend on m alone, so the 18 loads of a step are independent: a point waits for log2(m) loads in a
        // row, not for 18 times as many, and the scans below know their ends without reading a key.  (k_normals has the same
        // text: one function for both changed the code of both, k_normals<32> was slower through it and the ICP kernels were
        // not timed, DESIGN.md §31, rule R.)
        u64 klo[9], khi[9];
        int lo[9], hi[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            klo[k] = grid_key(b, c[0] + k / 3 - 1, c[1] + k % 3 - 1, c[2] - 1);
            khi[k] = grid_key(b, c[0] + k / 3 - 1, c[1] + k % 3 - 1, c[2] + 1) + 1;
            lo[k] = hi[k] = 0;
        }
        int n = a.m;                             // the answer lies in [lo, lo + n]
        while (n > 1) {
            const int half = n >> 1;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                lo[k] = a.skey[lo[k] + half - 1] < klo[k] ? lo[k] + half : lo[k];
                hi[k] = a.skey[hi[k] + half - 1] < khi[k] ? hi[k] + half : hi[k];
            }
            n -= half;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            lo[k] += a.skey[lo[k]] < klo[k] ? 1 : 0;
            hi[k] += a.skey[hi[k]] < khi[k] ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            for (int t = lo[k]; t < hi[k]; t += ICP_AHEAD) {
                GridRec r[ICP_AHEAD];            // independent loads, in flight together; those past the run repeat its last
#pragma unroll
                for (int v = 0; v < ICP_AHEAD; ++v) r[v] = a.srec[min(t + v, hi[k] - 1)];
#pragma unroll
                for (int v = 0; v < ICP_AHEAD; ++v) {
                    const float ex = qx - r[v].x, ey = qy - r[v].y, ez = qz - r[v].z;
                    const float d2 = (ex * ex + ey * ey) + ez * ez;
                    // the cells are not in index order: the tie rule is here (a repeated record changes nothing)
                    if (d2 < best || (d2 == best && r[v].i < bi)) {
                        best = d2;
                        bi = r[v].i;
                        bx = r[v].x; by = r[v].y; bz = r[v].z;
                    }
                }
            }
        }
    }
    s.q[0] = (double)bx; s.q[1] = (double)by; s.q[2] = (double)bz;
    const bool hit = bi != INT_MAX && best <= a.md2;
    s.match = hit ? bi : -1;
    s.d2 = hit ? best : INFINITY;
    return s;
}

__device__ __forceinline__ double residual2(const SrcPoint &s) {
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double d = s.y[k] - s.q[k];
        r2 = r2 + d * d;
    }
    return r2;
}

__device__ __forceinline__ void pivot_of(const IcpArgs &a, int p0, double *piv) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = a.src[k * a.src_ld + p0];
        piv[k] = isfinite(v) ? (double)v : 0.0;
    }
}

__global__ void __launch_bounds__(ICP_BLOCK) k_icp_finish(const IcpArgs a) {
    __shared__ double red[2][ICP_BLOCK];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = group_of(a.bprefix, a.batch, blk);
    const int p0 = a.sprefix[b], p1 = a.sprefix[b + 1];
    const int64_t base = (int64_t)p0 + (int64_t)(blk - a.bprefix[b]) * ICP_SPAN;
    double R[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) R[k] = (double)a.state[b].m[k];
    double acc[2] = {0.0, 0.0};
#pragma unroll 1
    for (int j = 0; j < ICP_PER_LANE; ++j) {
        const int64_t i = base + j * ICP_BLOCK + t;
        if (i >= p1) continue;
        const SrcPoint s = match_point(a, b, i, R);
        if (a.match) a.match[i] = s.match;
        if (a.dist2) a.dist2[i] = s.d2;
        if (a.flow) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.flow[i * 3 + k] = (float)(s.y[k] - s.p[k]);
        }
        if (s.w > 0.f && s.match >= 0) {
            acc[0] += residual2(s);
            acc[1] += 1.0;
        }
    }
    block_tree_sum(red, acc, t);
    if (t < 2) a.partials[(int64_t)blk * 2 + t] = red[t][0];
}

__global__ void __launch_bounds__(ICP_BLOCK) k_icp_fold(const IcpArgs a) {
    __shared__ double run[ICP_RUNS][2];
    __shared__ double tot[2];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    fold_partials<2, ICP_RUNS, ICP_BLOCK>(a.partials, a.bprefix[b], a.bprefix[b + 1] - a.bprefix[b], run, tot, t);
    if (t != 0) return;
    const State st = a.state[b];
    const int n = a.sprefix[b + 1] - a.sprefix[b];
    double R[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        a.Rt[(int64_t)b * 12 + i] = st.m[i];
        R[i] = (double)st.m[i];
    }
    // the angle of the float32 motion: atan2(|axial vector|, trace - 1), both twice the sine and the cosine
    const double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
    const double angle = atan2(sqrt((vx * vx + vy * vy) + vz * vz), ((R[0] + R[4]) + R[8]) - 1.0) * (180.0 / 3.14159265358979323846);
    const double tn = sqrt((R[9] * R[9] + R[10] * R[10]) + R[11] * R[11]);
    float *o = a.stats + (int64_t)b * 6;
    o[0] = st.status ? 1.f : 0.f;
    o[1] = n > 0 ? (float)(tot[1] / (double)n) : 0.f;
    o[2] = tot[1] > 0.0 ? (float)sqrt(tot[0] / tot[1]) : 0.f;
    o[3] = (float)angle;
    o[4] = (float)tn;
    o[5] = (float)st.rounds;
}

// the room of the one sort of (key, record)
inline int64_t temp_room(int64_t n) {
    return room_next_pow2(n, [](int64_t c) { return radix_temp_bytes<u64, GridRec>(c, 64u); });
}

}  // namespace
