// knn_interp.hip -- exact k nearest neighbours of query points among a pair's reference points, and the inverse-distance
// interpolation of per-point values from them (hpl_knn_interp): the feature propagation that fills the dense queries the
// level-0 lattice does not cover.  Brute force: N is the sampled cloud (8 192 per pair in the protocol).
//
// One lane per query, 256 queries per workgroup, every workgroup inside ONE pair (the host gives the pairs' first workgroups in
// the kernel arguments beside the two prefixes), so the tile loop is uniform over the workgroup.  The pair's points go through
// LDS in tiles of 16-byte (x, y, z, 0) records; all lanes read the same record at the same time, a uniform-address LDS read
// that broadcasts.  The running top-k is 2 k registers per lane (k is a template parameter, the insertion is unrolled).
//
// The arithmetic is part of the interface (include/hpl_bcl.h, tests/knn_oracle.py restates it in numpy): float32
// d2 = (dx * dx + dy * dy) + dz * dz with dx = q.x - p.x, no contraction (the library builds with -ffp-contract=off);
// candidates in index order, an entry replaced only by a strictly smaller d2, so ties go to the smaller index.
#include "cloud_common.h"

#include <limits.h>
#include <math.h>

using namespace hpl;

namespace {

constexpr int KNN_MAX_K = 8;
constexpr int KNN_MAX_C = 16;
constexpr int KNN_BLOCK = 256;
constexpr int KNN_TILE = 1024;          // records per LDS tile: 16 KiB

struct KnnArgs {
    const float *ref;
    int64_t ref_ld;
    const float *val;
    const float *q;
    int64_t q_ld;
    int32_t *idx;
    float *dist2;
    float *out;
    const float *cov;
    int64_t Q;
    int32_t C, batch;
    float eps;
    int32_t rprefix[CLOUD_MAX_BATCH + 1];   // points of pairs 0 .. b-1 (N < 2^31)
    int32_t qprefix[CLOUD_MAX_BATCH + 1];   // queries of pairs 0 .. b-1 (Q < 2^31)
    int32_t bprefix[CLOUD_MAX_BATCH + 1];   // workgroups of pairs 0 .. b-1
};

template <int K>
__global__ void __launch_bounds__(KNN_BLOCK) k_knn_interp(const KnnArgs a) {
    __shared__ float4 tile[KNN_TILE];
    const int blk = (int)blockIdx.x;
    const int b = group_of(a.bprefix, a.batch, blk);
    const int p0 = a.rprefix[b], p1 = a.rprefix[b + 1];
    const int64_t qi = (int64_t)a.qprefix[b] + (int64_t)(blk - a.bprefix[b]) * KNN_BLOCK + threadIdx.x;
    bool active = qi < (int64_t)a.qprefix[b + 1];
    float c = 0.f;
    if (active && a.cov) {
        c = a.cov[qi];
        active = c != 1.f;       // a fully covered query is neither searched nor written
    }
    if (!__syncthreads_or(active ? 1 : 0)) return;
    // an idle lane carries a NaN query: its d2 is NaN, never smaller than anything, so it never enters the insertion
    float qx = nanf(""), qy = 0.f, qz = 0.f;
    if (active) {
        qx = a.q[qi];
        qy = a.q[a.q_ld + qi];
        qz = a.q[2 * a.q_ld + qi];
    }
    float d[K];
    int id[K];
#pragma unroll
    for (int s = 0; s < K; ++s) { d[s] = INFINITY; id[s] = -1; }
    const bool wave_on = __ballot(active) != 0;

    for (int t0 = p0; t0 < p1; t0 += KNN_TILE) {
        const int n = min(KNN_TILE, p1 - t0);
        __syncthreads();         // the previous tile has been read
        for (int j = threadIdx.x; j < n; j += KNN_BLOCK)
            tile[j] = make_float4(a.ref[t0 + j], a.ref[a.ref_ld + t0 + j], a.ref[2 * a.ref_ld + t0 + j], 0.f);
        __syncthreads();
        if (wave_on) {
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const float4 p = tile[j];
                const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < d[K - 1]) {
                    const int cand = t0 + j;
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
    if (!active) return;

    if (a.idx) {
#pragma unroll
        for (int s = 0; s < K; ++s) a.idx[(int64_t)s * a.Q + qi] = id[s];
    }
    if (a.dist2) {
#pragma unroll
        for (int s = 0; s < K; ++s) a.dist2[(int64_t)s * a.Q + qi] = d[s];
    }
    const int C = a.C;
    float *o = a.out + qi * C;
    const bool hit = d[0] == 0.f;           // the nearest point IS the query: its row, bit for bit
    // (a query whose every d2 overflowed to +inf has no neighbour: wsum = 0 and the interpolation is 0 / 0 = NaN, as documented)
    float w[K];
    float wsum = 0.f;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        w[s] = id[s] >= 0 ? 1.f / (d[s] + a.eps) : 0.f;
        wsum = wsum + w[s];
    }
    for (int ch = 0; ch < C; ++ch) {
        float r;
        if (hit) {
            r = a.val[(int64_t)id[0] * C + ch];
        } else {
            float acc = 0.f;
#pragma unroll
            for (int s = 0; s < K; ++s) {
                const float v = id[s] >= 0 ? a.val[(int64_t)id[s] * C + ch] : 0.f;
                acc = acc + w[s] * v;
            }
            r = acc / wsum;
        }
        o[ch] = a.cov ? c * o[ch] + (1.f - c) * r : r;
    }
}

template <int K>
void launch(const KnnArgs &a, unsigned blocks, hipStream_t s) {
    k_knn_interp<K><<<blocks, KNN_BLOCK, 0, s>>>(a);
}

}  // namespace

extern "C" int hpl_knn_interp(const float *ref, int64_t ref_ld, const float *val, int C, const float *q, int64_t q_ld, int k,
                              float eps, int batch, const int64_t *ref_prefix, const int64_t *q_prefix, int32_t *idx,
                              float *dist2, float *out, const float *coverage, hplStream stream) {
    const char *const op = "hpl_knn_interp";
    HPL_REQUIRE(ref && val && q && out && ref_prefix && q_prefix, "hpl_knn_interp: null pointer");
    HPL_REQUIRE(k >= 1 && k <= KNN_MAX_K, "hpl_knn_interp: k = %d (1 .. %d)", k, KNN_MAX_K);
    HPL_REQUIRE(C >= 1 && C <= KNN_MAX_C, "hpl_knn_interp: %d value channels (1 .. %d)", C, KNN_MAX_C);
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(eps >= 0.f && isfinite(eps), "hpl_knn_interp: eps must be finite and >= 0");
    HPL_CLOUD_CHECK(check_prefix(op, "the point prefix", "pair", ref_prefix, batch));
    HPL_CLOUD_CHECK(check_prefix(op, "the query prefix", "pair", q_prefix, batch));
    const int64_t N = ref_prefix[batch], Q = q_prefix[batch];
    const int64_t lim = (int64_t)1 << 31;       // (N, Q below it first: the products cannot overflow)
    HPL_REQUIRE(N < lim && Q < lim && N * C < lim && Q * C < lim && (int64_t)k * Q < lim,
                "hpl_knn_interp: %lld points, %lld queries, %d channels, k = %d pass the 32-bit element limit", (long long)N,
                (long long)Q, C, k);
    HPL_REQUIRE(ref_ld >= N && q_ld >= Q, "hpl_knn_interp: row strides %lld / %lld below %lld points / %lld queries",
                (long long)ref_ld, (long long)q_ld, (long long)N, (long long)Q);
    for (int b = 0; b < batch; ++b)
        HPL_REQUIRE(ref_prefix[b + 1] > ref_prefix[b] || q_prefix[b + 1] == q_prefix[b],
                    "hpl_knn_interp: pair %d has queries and no points", b);
    HPL_CLOUD_CHECK(check_aligned4(op, {ref, val, q, out, idx, dist2, coverage}));
    if (Q == 0) return HPL_OK;
    KnnArgs a{};
    narrow_prefix(ref_prefix, batch, KNN_BLOCK, a.rprefix, nullptr);
    const int64_t blocks = narrow_prefix(q_prefix, batch, KNN_BLOCK, a.qprefix, a.bprefix);
    a.ref = ref; a.ref_ld = ref_ld; a.val = val; a.q = q; a.q_ld = q_ld;
    a.idx = idx; a.dist2 = dist2; a.out = out; a.cov = coverage;
    a.Q = Q; a.C = C; a.batch = batch; a.eps = eps;
    hipStream_t s = to_stream(stream);
    switch (k) {
        case 1: launch<1>(a, (unsigned)blocks, s); break;
        case 2: launch<2>(a, (unsigned)blocks, s); break;
        case 3: launch<3>(a, (unsigned)blocks, s); break;
        case 4: launch<4>(a, (unsigned)blocks, s); break;
        case 5: launch<5>(a, (unsigned)blocks, s); break;
        case 6: launch<6>(a, (unsigned)blocks, s); break;
        case 7: launch<7>(a, (unsigned)blocks, s); break;
        default: launch<8>(a, (unsigned)blocks, s); break;
    }
    HPL_CHECK_LAUNCH("hpl_knn_interp");
    return HPL_OK;
}
