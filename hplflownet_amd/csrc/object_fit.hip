// object_fit.hip -- a rigid fit per labelled object (hpl_object_fit): hpl_rigid_fit's arithmetic over segments
// that a label per point gives, not a host prefix.  The per-object motions of a piecewise-rigid scene without a read-back.
//
//   k_of_keys      a lane a point: the 32-bit key pair * (max_objects + 1) + (label in range ? label : max_objects), the point
//                  index as the value
//   rocPRIM        ONE stable radix sort of (key, index) over the bits in use: an object's members as a run, ascending index
//   k_of_gather    a lane a sorted member of a listed object: (p, effective base weight, f, index) as one 32-byte record, so
//                  that the rounds read coalesced
//   k_of_fit       one workgroup of 256 lanes per (pair, object) slot; it finds its run by two binary searches, and an empty
//                  slot writes its (I, 0, 0) row and leaves.  ALL iters + 1 rounds in this launch: per round the workgroup walks
//                  its spans of 1024 members -- lane l taking members l, l + 256, l + 512, l + 768 --, each span's 16 float64
//                  sums go through block_tree_sum into the object's own slots of the workspace, fold_partials adds the slots,
//                  lane 0 solves (rigid_solve.h) and (R, t) goes back through LDS.  A last walk writes residual and refined by
//                  original index and counts the inliers (an integer).
//
// That is hpl_rigid_fit's order of every sum on the members as one pair, so the bits are its bits.  No object needs another
// workgroup: no grid-wide dependency, no atomic at all, and rigid_fit's 2 (iters + 1) + 1 dependent launches are one.
#include "grid_common.h"        // radix_temp_bytes, room_next_pow2
#include "rigid_solve.h"

#include <math.h>

using namespace hpl;

namespace {

constexpr int OF_MAX_ITERS = 16;
constexpr int OF_MAX_OBJECTS = 4096;
constexpr int OF_BLOCK = 256;
constexpr int OF_PER_LANE = 4;
constexpr int OF_SPAN = OF_BLOCK * OF_PER_LANE;      // members per span: hpl_rigid_fit's workgroup
constexpr int OF_SUMS = RIGID_SUMS;
constexpr int OF_RUNS = OF_BLOCK / OF_SUMS;

struct __attribute__((aligned(16))) ObjRec {
    float x, y, z, w;           // w: the effective base weight, 0 for a weight that is not in (0, inf) and for a non-finite point
    float fx, fy, fz;
    int32_t i;                  // the packed index
};

struct ObjArgs {
    const float *pc;
    int64_t pc_ld;
    const float *flow;
    int64_t fsc, fsp;
    const float *weight;
    const int32_t *labels;
    uint32_t *key, *skey;
    int32_t *val, *sval;
    ObjRec *rec;
    double *partials;           // [slots][OF_SUMS]
    float *Rt, *stats, *residual, *refined;
    double tau;
    int32_t n, batch, max_objects, iters;
    int32_t pprefix[CLOUD_MAX_BATCH + 1];
};

__global__ void __launch_bounds__(OF_BLOCK) k_of_keys(const ObjArgs a) {
    const int i = (int)(blockIdx.x * OF_BLOCK + threadIdx.x);
    if (i >= a.n) return;
    const int b = group_of(a.pprefix, a.batch, i);
    const int32_t l = a.labels[i];
    a.key[i] = (uint32_t)(b * (a.max_objects + 1) + ((l >= 0 && l < a.max_objects) ? l : a.max_objects));
    a.val[i] = i;
}

__global__ void __launch_bounds__(OF_BLOCK) k_of_gather(const ObjArgs a) {
    const int j = (int)(blockIdx.x * OF_BLOCK + threadIdx.x);
    if (j >= a.n) return;
    if ((int)(a.skey[j] % (uint32_t)(a.max_objects + 1)) == a.max_objects) return;       // a member of no object
    const int64_t i = a.sval[j];
    ObjRec r;
    r.x = a.pc[i]; r.y = a.pc[a.pc_ld + i]; r.z = a.pc[2 * a.pc_ld + i];
    const float *f = a.flow + i * a.fsp;
    r.fx = f[0]; r.fy = f[a.fsc]; r.fz = f[2 * a.fsc];
    const float w = a.weight ? a.weight[i] : 1.f;
    const bool ok = isfinite(r.x) && isfinite(r.y) && isfinite(r.z) && isfinite(r.fx) && isfinite(r.fy) && isfinite(r.fz);
    r.w = (ok && w > 0.f && w < INFINITY) ? w : 0.f;
    r.i = (int32_t)i;
    a.rec[j] = r;
}

struct Member {
    double p[3], q[3];
    float w;
    int32_t i;
};

__device__ __forceinline__ Member load_member(const ObjRec *rec) {
    const ObjRec r = *rec;
    Member m;
    m.p[0] = (double)r.x; m.p[1] = (double)r.y; m.p[2] = (double)r.z;
    m.q[0] = m.p[0] + (double)r.fx; m.q[1] = m.p[1] + (double)r.fy; m.q[2] = m.p[2] + (double)r.fz;
    m.w = r.w;
    m.i = r.i;
    return m;
}

// |R p + t - q|^2 and, in m, R p + t - p (hpl_rigid_fit's, operation for operation)
__device__ __forceinline__ double residual2(const double *R, const Member &pt, double *m) {
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

__global__ void __launch_bounds__(OF_BLOCK) k_of_fit(const ObjArgs a) {
    __shared__ double red[OF_SUMS][OF_BLOCK];
    __shared__ double run[OF_RUNS][OF_SUMS];
    __shared__ double tot[OF_SUMS];
    __shared__ double sol[12];
    const int g = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = g / a.max_objects, o = g - b * a.max_objects;
    const uint32_t key = (uint32_t)(b * (a.max_objects + 1) + o);
    const int lo = lower_bound<uint32_t>(a.skey, a.n, key), hi = lower_bound<uint32_t>(a.skey, a.n, key + 1u);
    const int n = hi - lo;
    float *const oRt = a.Rt + (int64_t)g * 12, *const ost = a.stats + (int64_t)g * 4;
    if (n == 0) {
        if (t < 12) oRt[t] = (t == 0 || t == 4 || t == 8) ? 1.f : 0.f;
        if (t < 4) ost[t] = 0.f;
        return;
    }
    const ObjRec *const rec = a.rec + lo;
    const int spans = (n + OF_SPAN - 1) / OF_SPAN;
    const int slot0 = lo / OF_SPAN + g;          // the object's slots: no other object's
    double piv[3];
    {
        const float v[3] = {rec[0].x, rec[0].y, rec[0].z};
#pragma unroll
        for (int k = 0; k < 3; ++k) piv[k] = isfinite(v[k]) ? (double)v[k] : 0.0;
    }
    const double itau2 = 1.0 / (a.tau * a.tau);
    double R[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    bool ok = n >= 3;                            // (lane 0's: an object that failed at an earlier round stays failed)
    double angle = 0.0, tn = 0.0;

    for (int round = 0; round <= a.iters; ++round) {
        for (int s = 0; s < spans; ++s) {
            double acc[OF_SUMS];
#pragma unroll
            for (int k = 0; k < OF_SUMS; ++k) acc[k] = 0.0;
#pragma unroll
            for (int j = 0; j < OF_PER_LANE; ++j) {
                const int m = s * OF_SPAN + j * OF_BLOCK + t;
                if (m >= n) continue;
                const Member pt = load_member(rec + m);
                if (!(pt.w > 0.f)) continue;
                double u = (double)pt.w;
                if (round > 0) {
                    double mv[3];
                    const double sc = 1.0 + residual2(R, pt, mv) * itau2;
                    u = u / (sc * sc);           // Geman-McClure
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
            if (t < OF_SUMS) a.partials[(int64_t)(slot0 + s) * OF_SUMS + t] = red[t][0];
            __syncthreads();                     // red is free again, and the slot is written for the fold
        }
        fold_partials<OF_SUMS, OF_RUNS, OF_BLOCK>(a.partials, slot0, spans, run, tot, t);
        if (t == 0) {
            const double W = tot[0];
#pragma unroll
            for (int i = 0; i < OF_SUMS; ++i) ok = ok && isfinite(tot[i]);
            ok = ok && W > 0.0;
            double S[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
            angle = tn = 0.0;
            if (ok) {
                rigid_from_sums(tot, piv, S, angle, tn);
#pragma unroll
                for (int i = 0; i < 12; ++i) ok = ok && isfinite(S[i]);
                if (!ok) {
                    const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
#pragma unroll
                    for (int i = 0; i < 12; ++i) S[i] = I[i];
                    angle = tn = 0.0;
                }
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) sol[i] = S[i];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 12; ++k) R[k] = sol[k];
        // (the next round's fold_partials ends on a barrier before lane 0 writes sol again)
    }

    __shared__ int fitted_s;
    if (t == 0) fitted_s = ok ? 1 : 0;
    __syncthreads();
    const bool fitted = fitted_s != 0;
    int inl = 0;
    for (int s = 0; s < spans; ++s) {
#pragma unroll
        for (int j = 0; j < OF_PER_LANE; ++j) {
            const int m = s * OF_SPAN + j * OF_BLOCK + t;
            bool inlier = false;
            if (m < n) {
                const Member pt = load_member(rec + m);
                double mv[3];
                // (an object without a fit has R = I, t = 0: its residual is |f|)
                const double r = sqrt(residual2(R, pt, mv));
                inlier = fitted && pt.w > 0.f && r <= a.tau;
                if (a.residual) a.residual[pt.i] = (float)r;
                if (a.refined && inlier) {
                    float *out = a.refined + (int64_t)pt.i * 3;
#pragma unroll
                    for (int k = 0; k < 3; ++k) out[k] = (float)mv[k];
                }
            }
            inl += __syncthreads_count(inlier ? 1 : 0);
        }
    }
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) oRt[i] = (float)R[i];
        ost[0] = ok ? 1.f : 0.f;
        ost[1] = ok ? (float)((double)inl / (double)n) : 0.f;
        ost[2] = (float)angle;
        ost[3] = (float)tn;
    }
}

inline unsigned key_bits(int batch, int max_objects) { return (unsigned)count_bits((int64_t)batch * (max_objects + 1)); }

inline int64_t slots(int batch, int64_t n, int max_objects) { return n / OF_SPAN + (int64_t)batch * max_objects + 1; }

// the sort's room: rocPRIM does not promise that it grows with the key bits either, so the widest key is kept room for too
inline int64_t temp_room(int64_t n, unsigned bits) {
    return room_next_pow2(n, [bits](int64_t c) {
        const size_t s = radix_temp_bytes<uint32_t, int32_t>(c, bits), w = radix_temp_bytes<uint32_t, int32_t>(c, 32u);
        return s > w ? s : w;
    });
}

// workspace: key | sorted key | val | sorted val | records | partial sums | rocPRIM temporaries
struct Layout {                  // byte offsets
    int64_t key, skey, val, sval, rec, partials, bytes;
    Layout(int batch, int64_t n, int max_objects) {
        Carver c;
        key = c.take(n * 4);
        skey = c.take(n * 4);
        val = c.take(n * 4);
        sval = c.take(n * 4);
        rec = c.take(n * (int64_t)sizeof(ObjRec));
        partials = c.take(slots(batch, n, max_objects) * OF_SUMS * (int64_t)sizeof(double));
        bytes = c.bytes;
    }
};

int64_t workspace_bytes(int batch, int64_t n, int max_objects) {
    return Layout(batch, n, max_objects).bytes + temp_room(n, key_bits(batch, max_objects));
}

}  // namespace

extern "C" int64_t hpl_object_fit_workspace_bytes(int batch, int64_t n_total, int max_objects) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || n_total < 0 || n_total >= CLOUD_MAX_POINTS || max_objects < 1 ||
        max_objects > OF_MAX_OBJECTS)
        return -1;
    return workspace_bytes(batch, n_total, max_objects);
}

extern "C" int hpl_object_fit(const float *pc, int64_t pc_ld, const float *flow, int64_t flow_sc, int64_t flow_sp,
                              const float *weight, const int32_t *labels, int batch, const int64_t *prefix, int max_objects,
                              int iters, float tau, float *obj_Rt, float *obj_stats, float *residual, float *refined,
                              void *workspace, int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_object_fit";
    HPL_REQUIRE(pc && flow && labels && obj_Rt && obj_stats && prefix && workspace, "hpl_object_fit: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(max_objects >= 1 && max_objects <= OF_MAX_OBJECTS, "hpl_object_fit: max_objects = %d (1 .. %d)", max_objects,
                OF_MAX_OBJECTS);
    HPL_REQUIRE(iters >= 0 && iters <= OF_MAX_ITERS, "hpl_object_fit: iters = %d (0 .. %d)", iters, OF_MAX_ITERS);
    HPL_REQUIRE(tau > 0.f && isfinite(tau), "hpl_object_fit: tau must be finite and > 0");
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix", "pair", prefix, batch));
    const int64_t N = prefix[batch];
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_CLOUD_CHECK(check_row_stride(op, pc_ld, N));
    HPL_CLOUD_CHECK(check_flow_strides(op, flow_sc, flow_sp, N));
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, workspace_bytes(batch, N, max_objects)));
    HPL_CLOUD_CHECK(check_aligned4(op, {pc, flow, weight, labels, obj_Rt, obj_stats, residual, refined}));
    if (N == 0) return HPL_OK;

    const Layout L(batch, N, max_objects);
    void *const temp = carved<char>(workspace, L.bytes);
    ObjArgs a{};
    a.pc = pc; a.pc_ld = pc_ld; a.flow = flow; a.fsc = flow_sc; a.fsp = flow_sp; a.weight = weight; a.labels = labels;
    a.key = carved<uint32_t>(workspace, L.key); a.skey = carved<uint32_t>(workspace, L.skey);
    a.val = carved<int32_t>(workspace, L.val); a.sval = carved<int32_t>(workspace, L.sval);
    a.rec = carved<ObjRec>(workspace, L.rec);
    a.partials = carved<double>(workspace, L.partials);
    a.Rt = obj_Rt; a.stats = obj_stats; a.residual = residual; a.refined = refined;
    a.tau = (double)tau;
    a.n = (int32_t)N; a.batch = batch; a.max_objects = max_objects; a.iters = iters;
    narrow_prefix(prefix, batch, OF_BLOCK, a.pprefix, nullptr);

    hipStream_t s = to_stream(stream);
    const unsigned grid = (unsigned)cdiv(N, OF_BLOCK), bits = key_bits(batch, max_objects);
    k_of_keys<<<grid, OF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_object_fit (keys)");
    size_t tb = (size_t)temp_room(N, bits);
    const hipError_t e = rocprim::radix_sort_pairs(temp, tb, (const uint32_t *)a.key, a.skey, (const int32_t *)a.val, a.sval,
                                                   (size_t)N, 0u, bits, s);
    if (e != hipSuccess) { set_error("hpl_object_fit: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    k_of_gather<<<grid, OF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_object_fit (gather)");
    k_of_fit<<<(unsigned)(batch * max_objects), OF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_object_fit (fit)");
    return HPL_OK;
}
