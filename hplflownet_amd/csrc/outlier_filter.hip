// outlier_filter.hip -- the stray points of packed ragged clouds, removed on the device (hpl_outlier_filter):
// the statistical filter (mean distance to the k nearest neighbours against the cloud's mu + std_ratio sigma) and the radius
// filter (at least min_neighbors within a radius), both exact on a sorted uniform grid over the cloud itself.
//
// The definition is the all-pairs one of include/hpl_bcl.h (tests/outlier_oracle.py restates it in numpy without a grid); the
// grid only finds the candidates.  Key, cell, record and sort room are grid_common.h's, taken as hpl_normals takes them: cell
// edge 1.001 radius, the cell of a point in float64.
//
//   k_outlier_keys       a lane per point: key (all ones: the point takes no part) and (x, y, z, index) record
//   rocPRIM              ONE stable radix sort of (key, record) per call
//   k_outlier_search<K>  a lane per SORTED record, writing to the record's original index: the 27 cells around the point as 9
//                        runs (18 binary searches in lockstep, the rolled walk with a 4-deep look-ahead: k_normals' search,
//                        restated here -- DESIGN.md §31, rule R).  K = 8, 16, 32: the K smallest d2 of the OTHER points in
//                        registers, values only (compile-time indices, one gate d2 < worst), then the float64 sum of their
//                        roots in list order.  K = 0: the count alone (radius mode).
//   k_outlier_sum1       statistical: per workgroup (inside ONE cloud, 1024 points) the partial (n', sum m) through one LDS tree
//   k_outlier_sum2       statistical: folds the cloud's pass-1 partials to mu (every workgroup of a cloud in the same order: the
//                        same bits), partial of (m - mu)^2
//   k_outlier_thresh     a workgroup per cloud: folds both passes to (mu, sigma, T) and publishes them as float32 (zeros in
//                        radius mode)
//   k_outlier_classify   keep = takes part and (mean_dist <= the PUBLISHED float32 T | count >= min_neighbors); per workgroup
//                        the kept and the participating counts
//   k_outlier_scan       a workgroup per cloud: the counts to offsets, and stats
//   k_outlier_emit       places every kept index (only with keep_idx)
//
// No floating-point atomic, no integer atomic either, no read-back, no lane or workgroup waits for another; every loop is bounded
// by a cell population, a search depth or a cloud's workgroups.  The bits depend on the cloud alone.
#include "grid_common.h"

#include <limits.h>
#include <math.h>

using namespace hpl;

namespace {

constexpr int OF_BLOCK = 256;
constexpr int OF_WAVES = OF_BLOCK / 64;
constexpr int OF_MAX_K = 32;
constexpr int OF_AHEAD = 4;                          // records of a run loaded before they are compared
constexpr int OF_PER_LANE = 4;
constexpr int OF_SPAN = OF_BLOCK * OF_PER_LANE;      // points per workgroup of the per-cloud launches (ground_fit's span)
constexpr int OF_RUNS = OF_BLOCK / 16;               // strided runs of a fold
constexpr int OF_STATISTICAL = 0, OF_RADIUS = 1;

struct OutlierArgs {
    const float *pc;
    int64_t pc_ld;
    uint8_t *keep;
    int32_t *keep_idx;
    float *mean;                // the caller's mean_dist or the workspace's
    int32_t *count;             // the caller's count or the workspace's
    float *nbr_d2;
    float *thresh;
    int32_t *stats;
    u64 *key, *skey;
    GridRec *rec, *srec;
    double *part1;              // [workgroups][2]: n', sum m
    double *part2;              // [workgroups]: sum (m - mu)^2
    int32_t *blockoff;          // [workgroups]: kept points per workgroup, then their exclusive sums within the cloud
    int32_t *blockpart;         // [workgroups]: participating points per workgroup
    double inv_cell, radius, std_ratio;
    float r2;
    int32_t n, batch, k, mode, min_neighbors;
    int32_t prefix[CLOUD_MAX_BATCH + 1];       // points of clouds 0 .. b-1
    int32_t bprefix[CLOUD_MAX_BATCH + 1];      // workgroups (of OF_SPAN points) of clouds 0 .. b-1
};

__global__ void __launch_bounds__(OF_BLOCK) k_outlier_keys(const OutlierArgs a) {
    const int64_t j64 = (int64_t)blockIdx.x * OF_BLOCK + threadIdx.x;
    if (j64 >= a.n) return;
    const int j = (int)j64;
    grid_store(a, a.prefix, j, a.pc[j], a.pc[a.pc_ld + j], a.pc[2 * a.pc_ld + j]);
}

template <int K>                                     // K = 0: the count alone
__global__ void __launch_bounds__(OF_BLOCK) k_outlier_search(const OutlierArgs a) {
    const int64_t s64 = (int64_t)blockIdx.x * OF_BLOCK + threadIdx.x;
    if (s64 >= a.n) return;
    const int s = (int)s64;
    const u64 key = a.skey[s];
    const GridRec me = a.srec[s];
    const int64_t i = me.i;

    constexpr int L = K > 0 ? K : 1;
    float ld[L];                                 // the list: the smallest d2 ascending; unused entries +inf
#pragma unroll
    for (int t = 0; t < L; ++t) ld[t] = INFINITY;
    int found = 0;                               // K = 0: the neighbours

    if (key != ~0ull) {
        const int b = grid_group(key);
        int c[3], lo[9], hi[9];
        grid_cell(key, c);
        // The 9 runs [lo, hi): lower_bound of the run's first key and of the key behind its last, all 18 searches in lockstep
        // (the step sizes depend on n alone, so the 18 loads of a step are independent).  The text of k_normals' search.
        {
            u64 klo[9], khi[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                klo[k] = grid_key(b, c[0] + k / 3 - 1, c[1] + k % 3 - 1, c[2] - 1);
                khi[k] = grid_key(b, c[0] + k / 3 - 1, c[1] + k % 3 - 1, c[2] + 1) + 1;
                lo[k] = hi[k] = 0;
            }
            int n = a.n;                         // the answer lies in [lo, lo + n]
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
        }
#pragma unroll 1
        for (int run = 0; run < 9; ++run) {
            const int end = pick9(hi, run);
#pragma unroll 1
            for (int t = pick9(lo, run); t < end; t += OF_AHEAD) {
                GridRec r[OF_AHEAD];             // independent loads, in flight together; those past the run repeat its last
#pragma unroll
                for (int v = 0; v < OF_AHEAD; ++v) r[v] = a.srec[min(t + v, end - 1)];
#pragma unroll
                for (int v = 0; v < OF_AHEAD; ++v) {
                    const float ex = me.x - r[v].x, ey = me.y - r[v].y, ez = me.z - r[v].z;
                    const float d2 = (ex * ex + ey * ey) + ez * ez;
                    // a repeated record and the lane's own index are no candidates; a d2 of +inf is nobody's neighbour
                    const bool cand = t + v < end && r[v].i != me.i && d2 <= a.r2;
                    if constexpr (K == 0) {
                        found += (cand && d2 < INFINITY) ? 1 : 0;
                    } else {
                        if (cand && d2 < ld[K - 1]) {            // (equal to the worst: the values stay what they are)
#pragma unroll
                            for (int q = K - 1; q > 0; --q) ld[q] = d2 < ld[q - 1] ? ld[q - 1] : (d2 < ld[q] ? d2 : ld[q]);
                            ld[0] = d2 < ld[0] ? d2 : ld[0];
                        }
                    }
                }
            }
        }
    }

    if constexpr (K == 0) {
        a.count[i] = found;
    } else {
        int cnt = 0;
#pragma unroll
        for (int t = 0; t < K; ++t) cnt += (t < a.k && ld[t] < INFINITY) ? 1 : 0;
        double S = 0.0;
#pragma unroll
        for (int t = 0; t < K; ++t)
            if (t < cnt) S += sqrt((double)ld[t]);
        const double sm = S + (double)(a.k - cnt) * a.radius;
        a.count[i] = cnt;
        a.mean[i] = key != ~0ull ? (float)(sm / (double)a.k) : INFINITY;
        if (a.nbr_d2) {
#pragma unroll
            for (int t = 0; t < K; ++t)
                if (t < a.k) a.nbr_d2[i * a.k + t] = t < cnt ? ld[t] : INFINITY;
        }
    }
}

// (n', mu) of cloud b from its pass-1 partials: the same bits in every workgroup that asks.  All lanes call it.
__device__ __forceinline__ void fold_mu(const OutlierArgs &a, int b, double (&run)[OF_RUNS][2], double (&tot)[2], int t) {
    fold_partials<2, OF_RUNS, OF_BLOCK>(a.part1, a.bprefix[b], a.bprefix[b + 1] - a.bprefix[b], run, tot, t);
}

__global__ void __launch_bounds__(OF_BLOCK) k_outlier_sum1(const OutlierArgs a) {
    __shared__ double red[2][OF_BLOCK];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = block_group(a.bprefix, a.batch, blk);
    const int p1 = a.prefix[b + 1];
    const int64_t base = (int64_t)a.prefix[b] + (int64_t)(blk - a.bprefix[b]) * OF_SPAN;
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < OF_PER_LANE; ++j) {
        const int64_t i = base + j * OF_BLOCK + t;
        if (i < p1 && a.key[i] != ~0ull) {
            acc[0] += 1.0;
            acc[1] += (double)a.mean[i];
        }
    }
    block_tree_sum(red, acc, t);
    if (t < 2) a.part1[(int64_t)blk * 2 + t] = red[t][0];
}

__global__ void __launch_bounds__(OF_BLOCK) k_outlier_sum2(const OutlierArgs a) {
    __shared__ double red[1][OF_BLOCK];
    __shared__ double run[OF_RUNS][2];
    __shared__ double tot[2];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = block_group(a.bprefix, a.batch, blk);
    fold_mu(a, b, run, tot, t);
    const double mu = tot[0] > 0.0 ? tot[1] / tot[0] : 0.0;
    const int p1 = a.prefix[b + 1];
    const int64_t base = (int64_t)a.prefix[b] + (int64_t)(blk - a.bprefix[b]) * OF_SPAN;
    double acc[1] = {0.0};
#pragma unroll
    for (int j = 0; j < OF_PER_LANE; ++j) {
        const int64_t i = base + j * OF_BLOCK + t;
        if (i < p1 && a.key[i] != ~0ull) {
            const double d = (double)a.mean[i] - mu;
            acc[0] += d * d;
        }
    }
    block_tree_sum(red, acc, t);
    if (t == 0) a.part2[blk] = red[0][0];
}

__global__ void __launch_bounds__(OF_BLOCK) k_outlier_thresh(const OutlierArgs a) {
    __shared__ double run[OF_RUNS][2];
    __shared__ double tot[2];
    __shared__ double run2[OF_RUNS][1];
    __shared__ double tot2[1];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    float *o = a.thresh + (int64_t)b * 4;
    if (a.mode != OF_STATISTICAL) {              // (uniform over the launch)
        if (t < 4) o[t] = 0.f;
        return;
    }
    fold_mu(a, b, run, tot, t);
    fold_partials<1, OF_RUNS, OF_BLOCK>(a.part2, a.bprefix[b], a.bprefix[b + 1] - a.bprefix[b], run2, tot2, t);
    if (t != 0) return;
    const double n = tot[0];
    const double mu = n > 0.0 ? tot[1] / n : 0.0;
    const double sigma = n >= 2.0 ? sqrt(tot2[0] / (n - 1.0)) : 0.0;
    const double T = mu + a.std_ratio * sigma;
    o[0] = (float)mu; o[1] = (float)sigma; o[2] = (float)T; o[3] = 0.f;
}

// takes part, and kept: from what the call published (mean_dist, thresh) or counted
__device__ __forceinline__ bool keeps(const OutlierArgs &a, int64_t i, float T, bool *part) {
    *part = a.key[i] != ~0ull;
    return *part && (a.mode == OF_STATISTICAL ? a.mean[i] <= T : a.count[i] >= a.min_neighbors);
}

__global__ void __launch_bounds__(OF_BLOCK) k_outlier_classify(const OutlierArgs a) {
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = block_group(a.bprefix, a.batch, blk);
    const int p1 = a.prefix[b + 1];
    const int64_t base = (int64_t)a.prefix[b] + (int64_t)(blk - a.bprefix[b]) * OF_SPAN;
    const float T = a.thresh[(int64_t)b * 4 + 2];
    int kept = 0, parts = 0;
#pragma unroll
    for (int j = 0; j < OF_PER_LANE; ++j) {
        const int64_t i = base + j * OF_BLOCK + t;
        bool keep = false, part = false;
        if (i < p1) {
            keep = keeps(a, i, T, &part);
            if (a.keep) a.keep[i] = keep ? 1 : 0;
        }
        kept += __syncthreads_count(keep ? 1 : 0);
        parts += __syncthreads_count(part ? 1 : 0);
    }
    if (t == 0) { a.blockoff[blk] = kept; a.blockpart[blk] = parts; }
}

__global__ void __launch_bounds__(OF_BLOCK) k_outlier_scan(const OutlierArgs a) {
    // (k_ground_scan's text with a second column, summed only: through two calls of one function it was slower -- rule R, §35)
    __shared__ int sc[OF_BLOCK], sp[OF_BLOCK];
    __shared__ int carry, carry_p;
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b0 = a.bprefix[b], nb = a.bprefix[b + 1] - b0;
    if (t == 0) { carry = 0; carry_p = 0; }
    __syncthreads();
    for (int c0 = 0; c0 < nb; c0 += OF_BLOCK) {
        const int j = c0 + t;
        const int v = j < nb ? a.blockoff[b0 + j] : 0;
        sc[t] = v;
        sp[t] = j < nb ? a.blockpart[b0 + j] : 0;
        __syncthreads();
        for (int w = 1; w < OF_BLOCK; w <<= 1) {             // inclusive sums of the chunk
            const int u = t >= w ? sc[t - w] : 0, up = t >= w ? sp[t - w] : 0;
            __syncthreads();
            sc[t] += u;
            sp[t] += up;
            __syncthreads();
        }
        const int before = carry, before_p = carry_p;
        if (j < nb) a.blockoff[b0 + j] = before + sc[t] - v;
        __syncthreads();
        if (t == OF_BLOCK - 1) { carry = before + sc[t]; carry_p = before_p + sp[t]; }
        __syncthreads();
    }
    if (t == 0) {
        const int n = a.prefix[b + 1] - a.prefix[b];
        int32_t *o = a.stats + (int64_t)b * 4;
        o[0] = carry_p; o[1] = carry; o[2] = carry_p - carry; o[3] = n - carry_p;
    }
}

__global__ void __launch_bounds__(OF_BLOCK) k_outlier_emit(const OutlierArgs a) {
    // (k_ground_emit's rank: as one function for both, each call's A/B fell outside the parent's span -- rule R)
    __shared__ int wc[OF_PER_LANE * OF_WAVES];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = block_group(a.bprefix, a.batch, blk);
    const int p0 = a.prefix[b], p1 = a.prefix[b + 1];
    const int64_t base = (int64_t)p0 + (int64_t)(blk - a.bprefix[b]) * OF_SPAN;
    const float T = a.thresh[(int64_t)b * 4 + 2];
    const int total = a.stats[(int64_t)b * 4 + 1];
    bool keep[OF_PER_LANE];
    int below[OF_PER_LANE];                      // kept points of the same wave and row in lower lanes
#pragma unroll
    for (int j = 0; j < OF_PER_LANE; ++j) {
        const int64_t i = base + j * OF_BLOCK + t;
        bool part;
        keep[j] = i < p1 && keeps(a, i, T, &part);
        const unsigned long long m = __ballot(keep[j]);
        below[j] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wc[j * OF_WAVES + wave] = __popcll(m);
    }
    __syncthreads();
    int run = a.blockoff[blk];                   // kept points of the cloud before this workgroup's
#pragma unroll
    for (int j = 0; j < OF_PER_LANE; ++j) {
        const int64_t i = base + j * OF_BLOCK + t;
#pragma unroll
        for (int w = 0; w < OF_WAVES; ++w) {
            if (w == wave && keep[j]) a.keep_idx[(int64_t)p0 + run + below[j]] = (int32_t)i;
            run += wc[j * OF_WAVES + w];
        }
        if (i < p1 && i - p0 >= total) a.keep_idx[i] = -1;   // (kept indices land below `total`, these at or above it)
    }
}

// the room of the one sort of (key, record)
inline int64_t temp_room(int64_t n) {
    return room_next_pow2(n, [](int64_t c) { return radix_temp_bytes<u64, GridRec>(c, 64u); });
}

// workspace: key | sorted key | records | sorted records | mean_dist | count | pass-1 partials | pass-2 partials | kept counts |
// participating counts | rocPRIM temporaries
struct Layout {                  // byte offsets
    int64_t key, skey, rec, srec, mean, count, part1, part2, blockoff, blockpart, bytes;
    Layout(int batch, int64_t n) {
        const int64_t blocks = cdiv(n, OF_SPAN) + batch;
        Carver c;
        key = c.take(n * 8);
        skey = c.take(n * 8);
        rec = c.take(n * (int64_t)sizeof(GridRec));
        srec = c.take(n * (int64_t)sizeof(GridRec));
        mean = c.take(n * 4);
        count = c.take(n * 4);
        part1 = c.take(blocks * 2 * (int64_t)sizeof(double));
        part2 = c.take(blocks * (int64_t)sizeof(double));
        blockoff = c.take(blocks * 4);
        blockpart = c.take(blocks * 4);
        bytes = c.bytes;
    }
};

int64_t workspace_bytes(int batch, int64_t n) { return Layout(batch, n).bytes + temp_room(n); }

inline bool overlaps(const void *p, int64_t pbytes, const void *q, int64_t qbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && pbytes > 0 && qbytes > 0 && a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}

}  // namespace

extern "C" int64_t hpl_outlier_filter_workspace_bytes(int batch, int64_t n_total) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || n_total < 0 || n_total >= CLOUD_MAX_POINTS) return -1;
    return workspace_bytes(batch, n_total);
}

extern "C" int hpl_outlier_filter(const float *pc, int64_t pc_ld, int batch, const int64_t *prefix, int mode, int k, float radius,
                                  float std_ratio, int min_neighbors, uint8_t *keep, int32_t *keep_idx, float *mean_dist,
                                  int32_t *count, float *nbr_d2, float *thresh, int32_t *stats, void *workspace,
                                  int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_outlier_filter";
    HPL_REQUIRE(pc && prefix && thresh && stats && workspace, "hpl_outlier_filter: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(mode == OF_STATISTICAL || mode == OF_RADIUS, "hpl_outlier_filter: mode = %d (0 statistical, 1 radius)", mode);
    HPL_REQUIRE(radius > 0.f && isfinite(radius), "hpl_outlier_filter: radius must be finite and > 0");
    if (mode == OF_STATISTICAL) {
        HPL_REQUIRE(k >= 1 && k <= OF_MAX_K, "hpl_outlier_filter: k = %d (1 .. %d)", k, OF_MAX_K);
        HPL_REQUIRE(std_ratio >= 0.f && isfinite(std_ratio), "hpl_outlier_filter: std_ratio must be finite and >= 0");
    } else {
        HPL_REQUIRE(min_neighbors >= 1, "hpl_outlier_filter: min_neighbors = %d (>= 1)", min_neighbors);
        HPL_REQUIRE(!mean_dist && !nbr_d2, "hpl_outlier_filter: the radius mode has no mean_dist and no nbr_d2");
    }
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix", "cloud", prefix, batch));
    const int64_t N = prefix[batch];
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_REQUIRE(!nbr_d2 || N * k < ((int64_t)1 << 31), "hpl_outlier_filter: %lld points of %d neighbours pass the 32-bit element limit (N k < 2^31)",
                (long long)N, k);
    HPL_CLOUD_CHECK(check_row_stride(op, pc_ld, N));
    const int64_t need = workspace_bytes(batch, N);
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, need));
    HPL_CLOUD_CHECK(check_aligned4(op, {pc, keep_idx, mean_dist, count, nbr_d2, thresh, stats}));
    {
        constexpr int OUTS = 7;
        const void *const outs[OUTS] = {keep, keep_idx, mean_dist, count, nbr_d2, thresh, stats};
        const int64_t out_bytes[OUTS] = {N, 4 * N, 4 * N, 4 * N, nbr_d2 ? 4 * N * k : 0, 16 * (int64_t)batch, 16 * (int64_t)batch};
        const int64_t pc_bytes = N > 0 ? (2 * pc_ld + N) * 4 : 0;
        for (int o = 0; o < OUTS; ++o) {
            HPL_REQUIRE(!overlaps(outs[o], out_bytes[o], pc, pc_bytes), "hpl_outlier_filter: an output overlaps the input");
            HPL_REQUIRE(!overlaps(outs[o], out_bytes[o], workspace, need), "hpl_outlier_filter: an output overlaps the workspace");
            for (int p = 0; p < o; ++p)
                HPL_REQUIRE(!overlaps(outs[o], out_bytes[o], outs[p], out_bytes[p]), "hpl_outlier_filter: two outputs overlap");
        }
    }
    if (N == 0) return HPL_OK;

    const Layout L(batch, N);
    void *const temp = carved<char>(workspace, L.bytes);
    OutlierArgs a{};
    const int64_t cblocks = narrow_prefix(prefix, batch, OF_SPAN, a.prefix, a.bprefix);
    a.pc = pc; a.pc_ld = pc_ld;
    a.keep = keep; a.keep_idx = keep_idx; a.nbr_d2 = nbr_d2; a.thresh = thresh; a.stats = stats;
    a.mean = mean_dist ? mean_dist : carved<float>(workspace, L.mean);
    a.count = count ? count : carved<int32_t>(workspace, L.count);
    a.key = carved<u64>(workspace, L.key); a.skey = carved<u64>(workspace, L.skey);
    a.rec = carved<GridRec>(workspace, L.rec); a.srec = carved<GridRec>(workspace, L.srec);
    a.part1 = carved<double>(workspace, L.part1); a.part2 = carved<double>(workspace, L.part2);
    a.blockoff = carved<int32_t>(workspace, L.blockoff); a.blockpart = carved<int32_t>(workspace, L.blockpart);
    a.inv_cell = 1.0 / (GRID_CELL_MARGIN * (double)radius);
    a.radius = (double)radius;
    a.std_ratio = (double)std_ratio;
    a.r2 = radius * radius;                      // rounded once to float32
    a.n = (int32_t)N; a.batch = batch; a.k = k; a.mode = mode; a.min_neighbors = min_neighbors;

    hipStream_t s = to_stream(stream);
    const unsigned blocks = (unsigned)cdiv(N, OF_BLOCK);
    k_outlier_keys<<<blocks, OF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_outlier_filter (keys)");
    size_t tb = (size_t)temp_room(N);
    const hipError_t e = rocprim::radix_sort_pairs(temp, tb, (const u64 *)a.key, a.skey, (const GridRec *)a.rec, a.srec, (size_t)N, 0u,
                                                   64u, s);      // (the largest key, of the points left out, has every bit set)
    if (e != hipSuccess) { set_error("hpl_outlier_filter: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    if (mode == OF_RADIUS) k_outlier_search<0><<<blocks, OF_BLOCK, 0, s>>>(a);
    else if (k <= 8) k_outlier_search<8><<<blocks, OF_BLOCK, 0, s>>>(a);
    else if (k <= 16) k_outlier_search<16><<<blocks, OF_BLOCK, 0, s>>>(a);
    else k_outlier_search<32><<<blocks, OF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_outlier_filter (search)");
    if (mode == OF_STATISTICAL) {
        k_outlier_sum1<<<(unsigned)cblocks, OF_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_outlier_filter (sum 1)");
        k_outlier_sum2<<<(unsigned)cblocks, OF_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_outlier_filter (sum 2)");
    }
    k_outlier_thresh<<<batch, OF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_outlier_filter (thresh)");
    k_outlier_classify<<<(unsigned)cblocks, OF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_outlier_filter (classify)");
    k_outlier_scan<<<batch, OF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_outlier_filter (scan)");
    if (keep_idx) {
        k_outlier_emit<<<(unsigned)cblocks, OF_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_outlier_filter (emit)");
    }
    return HPL_OK;
}
