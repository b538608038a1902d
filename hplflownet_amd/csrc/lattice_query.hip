// lattice_query.hip -- where arbitrary query points fall in level 0 of cloud 1 of a finished lattice (hpl_lattice_query):
// the forward's output at a pc1 point depends on that point only through its level-0 barycentric slice of the last Up layer
// (models/HPLFlowNet.py:418-430), so the flow at any point inside pc1's simplices is that slice at the point's own simplex,
// then the per-point head.  One lane per query: the keys stage of the builders (lat::lattice_point, the same float
// statements, hence a pc1 point's own bits), then four probes of the table the build left -- no insertion, no new vertex.
//
// Aliasing.  The builders pack a key over the level's per-coordinate key range WITHOUT a range check (key2int,
// transforms.py:70-86), which the neighbour tables reproduce on purpose.  A query key outside that range could alias a real
// vertex; it is missing here before any probe.  A batch packs over the query's PAIR's range below the pair digit, so a query
// of pair b never reaches a vertex of another pair.
#include "lattice_common.h"

#include <limits.h>

using namespace hpl;
using namespace hpl::lat;

namespace {

constexpr int QUERY_MAX_BATCH = 64;

struct QueryArgs {
    const float *q;
    int64_t Q;
    const int4 *slots;           // fused table, or
    const int64_t *keys;         // the staged table's keys / ids
    const int32_t *ids;
    uint64_t mask;
    const int32_t *mm, *pmm;
    int32_t batch, pair_shift, renorm;
    float scale;
    float *bary;
    int32_t *off;
    float *cov;
    int64_t prefix[QUERY_MAX_BATCH + 1];
};

__device__ __forceinline__ int query_pair(const QueryArgs &a, int64_t i) {
    int b = 0;                   // the last pair whose first query is <= i (prefix[0] = 0)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) b = (b + s < a.batch && a.prefix[b + s] <= i) ? b + s : b;
    return b;
}

// lattice_fused.hip pair_range: keys in a pair's range; 0 if they do not fit below the pair digit
__device__ __forceinline__ int64_t pair_range(const int32_t *__restrict__ mm, int shift) {
    double rd = 1.0;
    int64_t R = 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t r = (int64_t)mm[4 + i] - mm[i] + 1;
        rd *= (double)r;
        R *= r;
    }
    return rd < 0.999999 * (double)(1ll << shift) ? R : 0;
}

__device__ __forceinline__ int32_t probe_slots(const int4 *__restrict__ ts, uint64_t mask, int64_t packed) {
    uint64_t s = mix64((uint64_t)packed) & mask;
    while (true) {
        const int4 v = ts[s];
        const int64_t k = (int64_t)(((uint64_t)(uint32_t)v.y << 32) | (uint32_t)v.x);
        if (k == packed) return v.w;
        if (k == EMPTY) return -1;
        s = (s + 1) & mask;
    }
}

__global__ void __launch_bounds__(256) k_lattice_query(const QueryArgs a, const Elev E) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.Q) return;
    alignas(16) int32_t keys[16];
    alignas(16) float w[4];
    float emg[4];
    lattice_point(a.q[i], a.q[a.Q + i], a.q[2 * a.Q + i], 0, 1, a.scale, E, keys, w, emg, 4);
    const int pr = a.batch > 1 ? query_pair(a, i) : 0;
    const int32_t *mm = a.batch > 1 ? a.pmm + pr * 8 : a.mm;
    int lo[4], hi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { lo[j] = mm[j]; hi[j] = mm[4 + j]; }
    const int64_t R = a.batch > 1 ? pair_range(mm, a.pair_shift) : 1;
    int32_t id[4];
    bool full = true;
    float cov = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {       // vertex r: coordinates keys[x * 4 + r] (the builders' (4, N, 4) layout at N = 1)
        int k[4];
        bool in = R > 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            k[x] = keys[x * 4 + r];
            in = in && k[x] >= lo[x] && k[x] <= hi[x];
        }
        int32_t v = -1;
        if (in) {
            const int64_t local = pack_key(k, mm);
            const int64_t packed = a.batch > 1 ? (((int64_t)pr << a.pair_shift) | local) : local;
            v = a.slots ? probe_slots(a.slots, a.mask, packed) : lookup(a.keys, a.ids, a.mask, packed);
        }
        id[r] = v;
        if (v >= 0) cov += w[r];
        else if (w[r] != 0.f) full = false;
    }
    if (full) cov = 1.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float wr = id[r] >= 0 ? w[r] : 0.f;
        if (a.renorm && !full && cov > 0.f) wr = wr / cov;
        a.bary[r * a.Q + i] = wr;
        a.off[r * a.Q + i] = id[r] >= 0 ? id[r] : 0;
    }
    a.cov[i] = cov;
}

}  // namespace

extern "C" int hpl_lattice_query(const hpl_query_info *info, const float *q, int64_t Q, const int64_t *pair_prefix,
                                 int renormalize, float *bary, int32_t *off, float *coverage, hplStream stream) {
    HPL_REQUIRE(info && q && bary && off && coverage, "hpl_lattice_query: null pointer");
    HPL_REQUIRE(Q >= 1 && Q < INT32_MAX, "hpl_lattice_query: %lld queries (1 .. 2^31 - 2)", (long long)Q);
    HPL_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(bary) | reinterpret_cast<uintptr_t>(off) |
                  reinterpret_cast<uintptr_t>(coverage)) & 3u) == 0, "hpl_lattice_query: arrays must be 4-byte aligned");
    HPL_REQUIRE((info->slots != nullptr) != (info->keys != nullptr && info->ids != nullptr) && info->mm && info->H0 >= 1,
                "hpl_lattice_query: the info names no table (hpl_lattice_query_info of a finished build)");
    HPL_REQUIRE(info->batch >= 1 && info->batch <= QUERY_MAX_BATCH, "hpl_lattice_query: batch %d (1 .. %d)", info->batch,
                QUERY_MAX_BATCH);
    HPL_REQUIRE(info->batch == 1 || (info->pmm && info->slots && info->pair_shift > 0 && info->pair_shift < 63),
                "hpl_lattice_query: a batch needs its per-pair key ranges");
    QueryArgs a{};
    a.q = q; a.Q = Q;
    a.slots = reinterpret_cast<const int4 *>(info->slots);
    a.keys = info->keys; a.ids = info->ids; a.mask = info->mask;
    a.mm = info->mm; a.pmm = info->pmm;
    a.batch = info->batch; a.pair_shift = info->pair_shift; a.renorm = renormalize ? 1 : 0;
    a.scale = info->scale;
    a.bary = bary; a.off = off; a.cov = coverage;
    if (info->batch > 1) {
        HPL_REQUIRE(pair_prefix, "hpl_lattice_query: a batch of %d pairs needs the queries' pair prefix", info->batch);
        HPL_REQUIRE(pair_prefix[0] == 0 && pair_prefix[info->batch] == Q, "hpl_lattice_query: the pair prefix must run from 0 to Q");
        for (int b = 0; b < info->batch; ++b) {
            HPL_REQUIRE(pair_prefix[b + 1] >= pair_prefix[b], "hpl_lattice_query: the pair prefix decreases at pair %d", b);
            a.prefix[b] = pair_prefix[b];
        }
        a.prefix[info->batch] = Q;
    } else {
        HPL_REQUIRE(!pair_prefix || (pair_prefix[0] == 0 && pair_prefix[1] == Q), "hpl_lattice_query: the pair prefix must run from 0 to Q");
    }
    const Elev E = make_elev();
    k_lattice_query<<<(unsigned)cdiv(Q, 256), 256, 0, to_stream(stream)>>>(a, E);
    HPL_CHECK_LAUNCH("hpl_lattice_query");
    return HPL_OK;
}
