// selfsup_loss.hip -- the self-supervised loss of the point-based flow networks and its gradient (hpl_selfsup_loss, DESIGN.md
// §20): Chamfer distance between the warped cloud p = pc1 + flow and pc2 in both directions, plus the smoothness of the flow
// over pc1's k-nearest-neighbour graph -- without a flow label, a host round trip or a floating-point atomic.
//
//   k_ss_nearest<0>  a lane per warped point p_i: its nearest q (a), the float32 d2 into a float64 partial per workgroup
//   k_ss_nearest<1>  a lane per q_j: its nearest warped point (b), the partial, and the key (b, or N1: none) of the sort
//   k_ss_graph<K>    a lane per x_i: its K nearest x of other indices (N), k_i, the smoothness term, the K keys of the sort
//   rocPRIM          two stable radix sorts by target: {j : b(j) = i} and {m : i in N(m)} as runs, sources ascending
//   k_ss_grad        a lane per point: its own terms, then its two runs in ascending source order.  A run of more than
//                    SS_SHORT entries is taken by the whole wave: 64 lanes load 64 terms at once, the float64 additions
//                    keep the documented order (lane values handed round by index), so a run of a whole cloud costs the
//                    wave its additions, not its loads
//   k_ss_fold        a workgroup per pair: the partials in a fixed order, the four loss components rounded once
//
// The searches follow k_knn_interp: one lane per query, 256 queries per workgroup, every workgroup inside ONE pair, the
// pair's reference points through LDS in tiles of 16-byte records that all lanes read at the same address.  The warped points
// are formed on the fly (x + f, one float32 addition per component) wherever they are a query or a reference.  The sizes of
// all launches are host numbers (N1, N2, batch, k); nothing is read back and no lane waits for another.  Every sum has one
// order and every workgroup lies at a fixed offset of its pair: a pair's outputs are the same bits alone, anywhere in a batch
// and beside other work.
//
// The arithmetic is part of the interface (include/hpl_bcl.h; tests/selfsup_oracle.py restates it in numpy).
#include "grid_common.h"

#include <math.h>

using namespace hpl;

namespace {

constexpr int SS_MAX_K = 8;
constexpr int SS_BLOCK = 256;
constexpr int SS_TILE = 1024;            // records per LDS tile: 16 KiB
constexpr int SS_SHORT = 16;             // a longer incoming run is summed by its wave together

struct SsArgs {
    const float *pc1;
    int64_t ld1;
    const float *flow;
    int64_t fsc, fsp;
    const float *pc2;
    int64_t ld2;
    float wc, ws;
    int32_t batch, k, n1, n2, grad;
    float *loss, *dflow;
    int32_t *nn12_out, *nn21_out, *nbr_out;
    double *part12, *part21, *partS;     // per workgroup of the N1 / N2 / N1 launches
    int32_t *nn12, *nn21, *nbr, *kcnt;   // (N1), (N2), (k, N1), (N1)
    uint32_t *key2, *skey2, *keyg, *skeyg;
    int32_t *val2, *sval2, *valg, *svalg;
    int32_t p1[CLOUD_MAX_BATCH + 1], p2[CLOUD_MAX_BATCH + 1];     // points of pairs 0 .. b-1
    int32_t b1[CLOUD_MAX_BATCH + 1], b2[CLOUD_MAX_BATCH + 1];     // workgroups of pairs 0 .. b-1 of a launch over N1 / N2
};

__device__ __forceinline__ void load_flow(const SsArgs &a, int64_t i, float (&f)[3]) {
    const float *p = a.flow + i * a.fsp;
    f[0] = p[0];
    f[1] = p[a.fsc];
    f[2] = p[2 * a.fsc];
}

// The K nearest of ref[r0 .. r1) to (qx, qy, qz), index `self` left out: hpl_knn_interp's arithmetic and tie rule.  WARP: the
// references are pc1 + flow.  An idle lane carries a NaN query and never enters the insertion.
template <int K, bool WARP>
__device__ __forceinline__ void search(const SsArgs &a, float4 *tile, const float *ref, int64_t ld, int r0, int r1, float qx,
                                       float qy, float qz, int self, bool wave_on, float (&d)[K], int (&id)[K]) {
#pragma unroll
    for (int s = 0; s < K; ++s) { d[s] = INFINITY; id[s] = -1; }
    for (int t0 = r0; t0 < r1; t0 += SS_TILE) {
        const int n = min(SS_TILE, r1 - t0);
        __syncthreads();         // the previous tile has been read
        for (int j = threadIdx.x; j < n; j += SS_BLOCK) {
            float x = ref[t0 + j], y = ref[ld + t0 + j], z = ref[2 * ld + t0 + j];
            if (WARP) {
                float f[3];
                load_flow(a, t0 + j, f);
                x = x + f[0]; y = y + f[1]; z = z + f[2];
            }
            tile[j] = make_float4(x, y, z, 0.f);
        }
        __syncthreads();
        if (wave_on) {
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const float4 p = tile[j];
                const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                const int cand = t0 + j;
                if (d2 < d[K - 1] && cand != self) {
#pragma unroll
                    for (int s = K - 1; s >= 0; --s) {       // entry s-1 is still the old one when entry s takes it
                        const bool below = s > 0 && d2 < d[s > 0 ? s - 1 : 0];
                        const bool here = d2 < d[s];
                        id[s] = below ? id[s > 0 ? s - 1 : 0] : (here ? cand : id[s]);
                        d[s] = below ? d[s > 0 ? s - 1 : 0] : (here ? d2 : d[s]);
                    }
                }
            }
        }
    }
}

// the workgroup's sum of v in a fixed tree, on lane 0
__device__ __forceinline__ double block_sum(double (&red)[1][SS_BLOCK], double v) {
    const double acc[1] = {v};
    __syncthreads();             // (red may still be read from an earlier sum)
    block_tree_sum(red, acc, (int)threadIdx.x);
    return red[0][0];
}

// DIR 0: queries p_i among pc2.  DIR 1: queries q_j among the warped points.
template <int DIR>
__global__ void __launch_bounds__(SS_BLOCK) k_ss_nearest(const SsArgs a) {
    __shared__ float4 tile[SS_TILE];
    __shared__ double red[1][SS_BLOCK];
    const int blk = (int)blockIdx.x;
    const int32_t *qp = DIR == 0 ? a.p1 : a.p2, *rp = DIR == 0 ? a.p2 : a.p1, *bp = DIR == 0 ? a.b1 : a.b2;
    const int b = group_of(bp, a.batch, blk);
    const int64_t qi = (int64_t)qp[b] + (int64_t)(blk - bp[b]) * SS_BLOCK + threadIdx.x;
    const bool active = qi < (int64_t)qp[b + 1];
    float qx = nanf(""), qy = 0.f, qz = 0.f;
    if (active) {
        if (DIR == 0) {
            float f[3];
            load_flow(a, qi, f);
            qx = a.pc1[qi] + f[0];
            qy = a.pc1[a.ld1 + qi] + f[1];
            qz = a.pc1[2 * a.ld1 + qi] + f[2];
        } else {
            qx = a.pc2[qi];
            qy = a.pc2[a.ld2 + qi];
            qz = a.pc2[2 * a.ld2 + qi];
        }
    }
    float d[1];
    int id[1];
    const bool wave_on = __ballot(active) != 0;
    if (DIR == 0) search<1, false>(a, tile, a.pc2, a.ld2, rp[b], rp[b + 1], qx, qy, qz, -1, wave_on, d, id);
    else search<1, true>(a, tile, a.pc1, a.ld1, rp[b], rp[b + 1], qx, qy, qz, -1, wave_on, d, id);
    if (active) {
        if (DIR == 0) {
            a.nn12[qi] = id[0];
            if (a.nn12_out) a.nn12_out[qi] = id[0];
        } else {
            a.nn21[qi] = id[0];
            if (a.nn21_out) a.nn21_out[qi] = id[0];
            if (a.grad) {
                a.key2[qi] = id[0] >= 0 ? (uint32_t)id[0] : (uint32_t)a.n1;
                a.val2[qi] = (int32_t)qi;
            }
        }
    }
    const double s = block_sum(red, (active && id[0] >= 0) ? (double)d[0] : 0.0);
    if (threadIdx.x == 0) (DIR == 0 ? a.part12 : a.part21)[blk] = s;
}

template <int K>
__global__ void __launch_bounds__(SS_BLOCK) k_ss_graph(const SsArgs a) {
    __shared__ float4 tile[SS_TILE];
    __shared__ double red[1][SS_BLOCK];
    const int blk = (int)blockIdx.x;
    const int b = group_of(a.b1, a.batch, blk);
    const int64_t qi = (int64_t)a.p1[b] + (int64_t)(blk - a.b1[b]) * SS_BLOCK + threadIdx.x;
    const bool active = qi < (int64_t)a.p1[b + 1];
    float qx = nanf(""), qy = 0.f, qz = 0.f;
    if (active) {
        qx = a.pc1[qi];
        qy = a.pc1[a.ld1 + qi];
        qz = a.pc1[2 * a.ld1 + qi];
    }
    float d[K];
    int id[K];
    const bool wave_on = __ballot(active) != 0;
    search<K, false>(a, tile, a.pc1, a.ld1, a.p1[b], a.p1[b + 1], qx, qy, qz, active ? (int)qi : -1, wave_on, d, id);
    double term = 0.0;
    if (active) {
        float f[3];
        load_flow(a, qi, f);
        int ki = 0;
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            a.nbr[(int64_t)r * a.n1 + qi] = id[r];
            if (a.nbr_out) a.nbr_out[(int64_t)r * a.n1 + qi] = id[r];
            if (a.grad) {
                a.keyg[qi * K + r] = id[r] >= 0 ? (uint32_t)id[r] : (uint32_t)a.n1;
                a.valg[qi * K + r] = (int32_t)qi;
            }
            if (id[r] >= 0) {
                float g[3];
                load_flow(a, id[r], g);
                const double ex = (double)f[0] - (double)g[0], ey = (double)f[1] - (double)g[1], ez = (double)f[2] - (double)g[2];
                s = s + ((ex * ex + ey * ey) + ez * ez);
                ++ki;
            }
        }
        a.kcnt[qi] = ki;
        term = ki > 0 ? s / (double)ki : 0.0;
    }
    const double s = block_sum(red, term);
    if (threadIdx.x == 0) a.partS[blk] = s;
}

// One entry of an incoming run.  KIND 0: q_j picked p_i: p_i - q_j.  KIND 1: x_m lists x_i: (f_i - f_m) / k_m.
template <int KIND>
__device__ __forceinline__ void incoming_term(const SsArgs &a, int pos, const float (&v)[3], double (&t)[3]) {
    if (KIND == 0) {
        const int j = a.sval2[pos];
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = (double)v[c] - (double)a.pc2[c * a.ld2 + j];
    } else {
        const int m = a.svalg[pos];
        float g[3];
        load_flow(a, m, g);
        const double w = 1.0 / (double)a.kcnt[m];
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = ((double)v[c] - (double)g[c]) * w;
    }
}

// acc = the sum of the lane's run [lo, lo + len) from 0 in ascending order.  Every lane of the wave calls it (an idle lane with
// len = 0): a run above SS_SHORT is loaded 64 entries at a time by the whole wave and added in the same order.
template <int KIND>
__device__ __forceinline__ void incoming_sum(const SsArgs &a, int lo, int len, const float (&v)[3], double (&acc)[3]) {
    const int lane = (int)(threadIdx.x & 63);
    acc[0] = acc[1] = acc[2] = 0.0;
    if (len <= SS_SHORT) {
        for (int e = 0; e < len; ++e) {
            double t[3];
            incoming_term<KIND>(a, lo + e, v, t);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + t[c];
        }
    }
    u64 todo = __ballot(len > SS_SHORT);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int lo_b = __shfl(lo, src), len_b = __shfl(len, src);
        float vb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) vb[c] = __shfl(v[c], src);
        double s[3] = {0.0, 0.0, 0.0};
        for (int c0 = 0; c0 < len_b; c0 += 64) {
            double t[3] = {0.0, 0.0, 0.0};
            if (c0 + lane < len_b) incoming_term<KIND>(a, lo_b + c0 + lane, vb, t);
            const int n = min(64, len_b - c0);
            for (int l = 0; l < n; ++l) {
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c] = s[c] + __shfl(t[c], l);
            }
        }
        if (lane == src) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = s[c];
        }
    }
}

__global__ void __launch_bounds__(SS_BLOCK) k_ss_grad(const SsArgs a) {
    const int blk = (int)blockIdx.x;
    const int b = group_of(a.b1, a.batch, blk);
    const int64_t i64 = (int64_t)a.p1[b] + (int64_t)(blk - a.b1[b]) * SS_BLOCK + threadIdx.x;
    const bool active = i64 < (int64_t)a.p1[b + 1];
    const int i = (int)i64;
    const int n1p = a.p1[b + 1] - a.p1[b], n2p = a.p2[b + 1] - a.p2[b];
    float f[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
    double own[3] = {0.0, 0.0, 0.0};
    int lo2 = 0, len2 = 0, log = 0, leng = 0;
    if (active) {
        load_flow(a, i, f);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = a.pc1[c * a.ld1 + i] + f[c];
        const int j = a.nn12[i];
        if (j >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) own[c] = (double)p[c] - (double)a.pc2[c * a.ld2 + j];
        }
        if (n2p > 0) {
            lo2 = lower_bound(a.skey2, a.n2, (uint32_t)i);
            len2 = lower_bound(a.skey2, a.n2, (uint32_t)i + 1u) - lo2;
        }
    }
    double A[3];
    incoming_sum<0>(a, lo2, len2, p, A);
    double B[3] = {0.0, 0.0, 0.0}, C[3] = {0.0, 0.0, 0.0};
    int ki = 0;
    if (a.k > 0) {               // (uniform)
        if (active) {
            for (int r = 0; r < a.k; ++r) {
                const int n = a.nbr[(int64_t)r * a.n1 + i];
                if (n < 0) continue;
                float g[3];
                load_flow(a, n, g);
#pragma unroll
                for (int c = 0; c < 3; ++c) B[c] = B[c] + ((double)f[c] - (double)g[c]);
                ++ki;
            }
            log = lower_bound(a.skeyg, a.n1 * a.k, (uint32_t)i);
            leng = lower_bound(a.skeyg, a.n1 * a.k, (uint32_t)i + 1u) - log;
        }
        incoming_sum<1>(a, log, leng, f, C);
    }
    if (!active) return;
    const double s1 = 2.0 / (double)n1p, s2 = n2p > 0 ? 2.0 / (double)n2p : 0.0;
    float *o = a.dflow + i64 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double g = (double)a.wc * (s1 * own[c] + s2 * A[c]);
        if (a.k > 0) g = g + (double)a.ws * (s1 * ((ki > 0 ? B[c] / (double)ki : 0.0) + C[c]));
        o[c] = (float)g;
    }
}

__global__ void __launch_bounds__(SS_BLOCK) k_ss_fold(const SsArgs a) {
    __shared__ double red[1][SS_BLOCK];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int n1p = a.p1[b + 1] - a.p1[b], n2p = a.p2[b + 1] - a.p2[b];
    const int nb1 = a.b1[b + 1] - a.b1[b], nb2 = a.b2[b + 1] - a.b2[b];
    double s12 = 0.0, s21 = 0.0, sS = 0.0;
    for (int j = t; j < nb1; j += SS_BLOCK) s12 = s12 + a.part12[a.b1[b] + j];
    for (int j = t; j < nb2; j += SS_BLOCK) s21 = s21 + a.part21[a.b2[b] + j];
    if (a.k > 0)
        for (int j = t; j < nb1; j += SS_BLOCK) sS = sS + a.partS[a.b1[b] + j];
    s12 = block_sum(red, s12);
    s21 = block_sum(red, s21);
    sS = block_sum(red, sS);
    if (t != 0) return;
    const bool both = n1p > 0 && n2p > 0;
    const double C12 = both ? s12 / (double)n1p : 0.0, C21 = both ? s21 / (double)n2p : 0.0;
    const double S = (n1p > 0 && a.k > 0) ? sS / (double)n1p : 0.0;
    double L = (double)a.wc * (C12 + C21);
    if (a.k > 0) L = L + (double)a.ws * S;
    float *o = a.loss + (int64_t)b * 4;
    o[0] = (float)L;
    o[1] = (float)C12;
    o[2] = (float)C21;
    o[3] = (float)S;
}

// the room of one sort of n (key, index) pairs (grid_common.h)
inline int64_t temp_room(int64_t n) {
    return room_all_pow2(n, [](int64_t c) { return radix_temp_bytes<uint32_t, int32_t>(c, 32u); });
}

// workspace: the three partial arrays | nn12 | nn21 | nbr | k_i | the two sorts' keys and values, unsorted and sorted | rocPRIM
struct Layout {                  // byte offsets
    int64_t part12, part21, partS, nn12, nn21, nbr, kcnt, key2, skey2, val2, sval2, keyg, skeyg, valg, svalg, bytes;
    Layout(int batch, int64_t n1, int64_t n2, int k) {
        Carver c;
        const int64_t w1 = cdiv(n1, SS_BLOCK) + batch, w2 = cdiv(n2, SS_BLOCK) + batch, e = n1 * k;
        part12 = c.take(w1 * 8);
        part21 = c.take(w2 * 8);
        partS = c.take(w1 * 8);
        nn12 = c.take(n1 * 4);
        nn21 = c.take(n2 * 4);
        nbr = c.take(e * 4);
        kcnt = c.take(n1 * 4);
        key2 = c.take(n2 * 4);
        skey2 = c.take(n2 * 4);
        val2 = c.take(n2 * 4);
        sval2 = c.take(n2 * 4);
        keyg = c.take(e * 4);
        skeyg = c.take(e * 4);
        valg = c.take(e * 4);
        svalg = c.take(e * 4);
        bytes = c.bytes;
    }
};

bool in_range(int batch, int64_t n1, int64_t n2, int k) {
    return batch >= 1 && batch <= CLOUD_MAX_BATCH && k >= 0 && k <= SS_MAX_K && n1 >= 0 && n1 < CLOUD_MAX_POINTS && n2 >= 0 &&
           n2 < CLOUD_MAX_POINTS && n1 * k < ((int64_t)1 << 31);
}

// the two sorts share the room: enough for either
inline int64_t sort_room(int64_t n1, int64_t n2, int k) { return imax(temp_room(n2), temp_room(n1 * k)); }

int64_t workspace_bytes(int batch, int64_t n1, int64_t n2, int k) {
    return Layout(batch, n1, n2, k).bytes + sort_room(n1, n2, k);
}

inline bool overlaps(const void *p, int64_t pn, const void *q, int64_t qn) {      // element counts of 4 bytes each
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return pn > 0 && qn > 0 && a < b + 4u * (uintptr_t)qn && b < a + 4u * (uintptr_t)pn;
}

template <int K>
void launch_graph(const SsArgs &a, unsigned blocks, hipStream_t s) {
    k_ss_graph<K><<<blocks, SS_BLOCK, 0, s>>>(a);
}

}  // namespace

extern "C" int64_t hpl_selfsup_loss_workspace_bytes(int batch, int64_t n1_total, int64_t n2_total, int k) {
    if (!in_range(batch, n1_total, n2_total, k)) return -1;
    return workspace_bytes(batch, n1_total, n2_total, k);
}

extern "C" int hpl_selfsup_loss(const float *pc1, int64_t pc1_ld, const float *flow, int64_t flow_sc, int64_t flow_sp,
                                const float *pc2, int64_t pc2_ld, int batch, const int64_t *prefix1, const int64_t *prefix2, int k,
                                float w_chamfer, float w_smooth, float *loss, float *dflow, int32_t *nn12, int32_t *nn21,
                                int32_t *nbr, void *workspace, int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_selfsup_loss";
    HPL_REQUIRE(pc1 && flow && prefix1 && prefix2 && loss && workspace, "hpl_selfsup_loss: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(k >= 0 && k <= SS_MAX_K, "hpl_selfsup_loss: k = %d (0 .. %d)", k, SS_MAX_K);
    HPL_REQUIRE(w_chamfer >= 0.f && isfinite(w_chamfer) && w_smooth >= 0.f && isfinite(w_smooth),
                "hpl_selfsup_loss: the weights must be finite and >= 0");
    HPL_REQUIRE(k >= 1 || w_smooth == 0.f, "hpl_selfsup_loss: k = 0 goes with w_smooth = 0");
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix of pc1", "pair", prefix1, batch));
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix of pc2", "pair", prefix2, batch));
    const int64_t N1 = prefix1[batch], N2 = prefix2[batch];
    HPL_REQUIRE(pc2 || N2 == 0, "hpl_selfsup_loss: null pointer (pc2 of %lld points)", (long long)N2);
    HPL_REQUIRE(in_range(batch, N1, N2, k),
                "hpl_selfsup_loss: %lld / %lld points, k = %d pass the 32-bit element limit (counts < 2^31 / 3, k N1 < 2^31)",
                (long long)N1, (long long)N2, k);
    HPL_CLOUD_CHECK(check_row_stride(op, pc1_ld, N1));
    HPL_CLOUD_CHECK(check_row_stride(op, pc2_ld, N2));
    HPL_CLOUD_CHECK(check_flow_strides(op, flow_sc, flow_sp, N1));
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, workspace_bytes(batch, N1, N2, k)));
    HPL_CLOUD_CHECK(check_aligned4(op, {pc1, flow, pc2, loss, dflow, nn12, nn21, nbr}));
    if (dflow && N1 > 0) {
        const int64_t fext = (N1 - 1) * flow_sp + 2 * flow_sc + 1;
        HPL_REQUIRE(!overlaps(dflow, 3 * N1, pc1, 2 * pc1_ld + N1) && !overlaps(dflow, 3 * N1, flow, fext) &&
                        !overlaps(dflow, 3 * N1, pc2, 2 * pc2_ld + N2),
                    "hpl_selfsup_loss: dflow overlaps an input");
    }
    if (N1 == 0) return HPL_OK;

    const Layout L(batch, N1, N2, k);
    void *const temp = carved<char>(workspace, L.bytes);
    SsArgs a{};
    const int64_t blocks1 = narrow_prefix(prefix1, batch, SS_BLOCK, a.p1, a.b1);
    const int64_t blocks2 = narrow_prefix(prefix2, batch, SS_BLOCK, a.p2, a.b2);
    a.pc1 = pc1; a.ld1 = pc1_ld; a.flow = flow; a.fsc = flow_sc; a.fsp = flow_sp; a.pc2 = pc2; a.ld2 = pc2_ld;
    a.wc = w_chamfer; a.ws = w_smooth;
    a.batch = batch; a.k = k; a.n1 = (int32_t)N1; a.n2 = (int32_t)N2; a.grad = dflow ? 1 : 0;
    a.loss = loss; a.dflow = dflow; a.nn12_out = nn12; a.nn21_out = nn21; a.nbr_out = nbr;
    a.part12 = carved<double>(workspace, L.part12);
    a.part21 = carved<double>(workspace, L.part21);
    a.partS = carved<double>(workspace, L.partS);
    a.nn12 = carved<int32_t>(workspace, L.nn12);
    a.nn21 = carved<int32_t>(workspace, L.nn21);
    a.nbr = carved<int32_t>(workspace, L.nbr);
    a.kcnt = carved<int32_t>(workspace, L.kcnt);
    a.key2 = carved<uint32_t>(workspace, L.key2);
    a.skey2 = carved<uint32_t>(workspace, L.skey2);
    a.val2 = carved<int32_t>(workspace, L.val2);
    a.sval2 = carved<int32_t>(workspace, L.sval2);
    a.keyg = carved<uint32_t>(workspace, L.keyg);
    a.skeyg = carved<uint32_t>(workspace, L.skeyg);
    a.valg = carved<int32_t>(workspace, L.valg);
    a.svalg = carved<int32_t>(workspace, L.svalg);

    hipStream_t s = to_stream(stream);
    k_ss_nearest<0><<<(unsigned)blocks1, SS_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_selfsup_loss (nearest 1 -> 2)");
    if (blocks2 > 0) {
        k_ss_nearest<1><<<(unsigned)blocks2, SS_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_selfsup_loss (nearest 2 -> 1)");
    }
    switch (k) {
        case 0: break;
        case 1: launch_graph<1>(a, (unsigned)blocks1, s); break;
        case 2: launch_graph<2>(a, (unsigned)blocks1, s); break;
        case 3: launch_graph<3>(a, (unsigned)blocks1, s); break;
        case 4: launch_graph<4>(a, (unsigned)blocks1, s); break;
        case 5: launch_graph<5>(a, (unsigned)blocks1, s); break;
        case 6: launch_graph<6>(a, (unsigned)blocks1, s); break;
        case 7: launch_graph<7>(a, (unsigned)blocks1, s); break;
        default: launch_graph<8>(a, (unsigned)blocks1, s); break;
    }
    HPL_CHECK_LAUNCH("hpl_selfsup_loss (graph)");
    k_ss_fold<<<batch, SS_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_selfsup_loss (fold)");
    if (!dflow) return HPL_OK;

    const unsigned bits = (unsigned)count_bits(N1);
    size_t tb = (size_t)sort_room(N1, N2, k);
    if (N2 > 0) {
        const hipError_t e = rocprim::radix_sort_pairs(temp, tb, (const uint32_t *)a.key2, a.skey2, (const int32_t *)a.val2, a.sval2,
                                                       (size_t)N2, 0u, bits, s);
        if (e != hipSuccess) { set_error("hpl_selfsup_loss: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    }
    if (k > 0) {
        tb = (size_t)sort_room(N1, N2, k);
        const hipError_t e = rocprim::radix_sort_pairs(temp, tb, (const uint32_t *)a.keyg, a.skeyg, (const int32_t *)a.valg, a.svalg,
                                                       (size_t)(N1 * k), 0u, bits, s);
        if (e != hipSuccess) { set_error("hpl_selfsup_loss: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    }
    k_ss_grad<<<(unsigned)blocks1, SS_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_selfsup_loss (gradient)");
    return HPL_OK;
}
