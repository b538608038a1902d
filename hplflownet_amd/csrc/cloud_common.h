// cloud_common.h -- what the ops over packed ragged batches of point clouds share: the limits, the search
// from a workgroup to its group, the entry points' argument checks, the workspace carver, the fixed-order float64 sums and the
// cyclic Jacobi eigen-solver.  Included by knn_interp, rigid_fit (and rigid_solve.h), pair_loss, fps, ground_fit, frames and
// render, and through grid_common.h (§31) by the ops on a sorted grid.  Header only.  Every rule here is a promise about bits
// or about a 32-bit limit: it is stated once.
#pragma once
#include "common.h"

#include <initializer_list>
#include <math.h>

namespace hpl {

constexpr int CLOUD_MAX_BATCH = 64;
constexpr int64_t CLOUD_MAX_POINTS = (((int64_t)1 << 31) + 2) / 3;  // N >= 2^31 / 3 is refused: 3 N elements pass 32 bits

// The group of item x: the last b with prefix[b] <= x, prefix[0 .. batch] from 0 and not decreasing, batch <= 64.  Over a
// workgroup prefix it is the last pair whose first workgroup is <= x (empty pairs own no workgroup); over a point prefix the
// last pair that starts at or before x (empty pairs start where the next one does).
__host__ __device__ __forceinline__ int group_of(const int32_t *prefix, int batch, int x) {
    int b = 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) b = (b + s < batch && prefix[b + s] <= x) ? b + s : b;
    return b;
}

// The group of workgroup blk over a workgroup prefix, in a scalar register: every lane computes the same b, and what is
// indexed by it afterwards (the prefixes, a camera, a plane) arrives by scalar loads.
__device__ __forceinline__ int block_group(const int32_t *bprefix, int batch, int blk) {
    return __builtin_amdgcn_readfirstlane(group_of(bprefix, batch, blk));
}

// ---------------------------------------------------------------------------------------------- the entry points' checks
// Each returns HPL_EINVAL with an error text that begins with the op's name, or HPL_OK.
#define HPL_CLOUD_CHECK(call)                   \
    do {                                        \
        const int rc__ = (call);                \
        if (rc__ != HPL_OK) return rc__;        \
    } while (0)

inline int check_batch(const char *op, int batch) {
    HPL_REQUIRE(batch >= 1 && batch <= CLOUD_MAX_BATCH, "%s: batch %d (1 .. %d)", op, batch, CLOUD_MAX_BATCH);
    return HPL_OK;
}

// what: "the prefix", "the prefix of pc1", ...; unit: "pair" or "cloud"
inline int check_prefix(const char *op, const char *what, const char *unit, const int64_t *prefix, int batch) {
    HPL_REQUIRE(prefix[0] == 0, "%s: %s must start at 0", op, what);
    for (int b = 0; b < batch; ++b) HPL_REQUIRE(prefix[b + 1] >= prefix[b], "%s: %s decreases at %s %d", op, what, unit, b);
    return HPL_OK;
}

inline int check_points(const char *op, int64_t n) {
    HPL_REQUIRE(n < CLOUD_MAX_POINTS, "%s: %lld points pass the 32-bit element limit (N < 2^31 / 3)", op, (long long)n);
    return HPL_OK;
}

inline int check_row_stride(const char *op, int64_t ld, int64_t n) {
    HPL_REQUIRE(ld >= n, "%s: row stride %lld below %lld points", op, (long long)ld, (long long)n);
    return HPL_OK;
}

// a flow of n points read at flow[c * sc + i * sp]: (3, N) rows or [N, 3] points of any strides that keep the elements apart
inline int check_flow_strides(const char *op, int64_t sc, int64_t sp, int64_t n) {
    HPL_REQUIRE(sc >= 1 && sp >= 1 && (sp != 1 || sc >= n) && (sc != 1 || sp >= 3 || n <= 1),
                "%s: flow strides %lld (component) / %lld (point) overlap for %lld points", op, (long long)sc, (long long)sp,
                (long long)n);
    return HPL_OK;
}

inline int check_aligned4(const char *op, std::initializer_list<const void *> arrays) {     // (a null pointer passes)
    uintptr_t bits = 0;
    for (const void *p : arrays) bits |= reinterpret_cast<uintptr_t>(p);
    HPL_REQUIRE((bits & 3u) == 0, "%s: arrays must be 4-byte aligned", op);
    return HPL_OK;
}

inline int check_workspace(const char *op, const void *workspace, int align, int64_t have, int64_t need) {
    HPL_REQUIRE(have >= need, "%s: workspace of %lld bytes, needs %lld", op, (long long)have, (long long)need);
    HPL_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & (uintptr_t)(align - 1)) == 0, "%s: the workspace must be %d-byte aligned",
                op, align);
    return HPL_OK;
}

// pprefix[0 .. batch] = the prefix in 32 bits and, with bprefix, bprefix[b] = the workgroups of groups 0 .. b-1 at `span` items
// per workgroup, every workgroup inside one group.  -> the workgroups of all groups.
inline int64_t narrow_prefix(const int64_t *prefix, int batch, int span, int32_t *pprefix, int32_t *bprefix) {
    int64_t blocks = 0;
    for (int b = 0; b <= batch; ++b) {
        pprefix[b] = (int32_t)prefix[b];
        if (bprefix) bprefix[b] = (int32_t)blocks;
        if (b < batch) blocks += cdiv(prefix[b + 1] - prefix[b], span);
    }
    return blocks;
}

// ---------------------------------------------------------------------------------------------- workspaces
inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

inline int count_bits(int64_t n) {               // the bits of the keys 0 .. n
    int bits = 1;
    while (((int64_t)1 << bits) <= n) ++bits;
    return bits;
}

// Carves a workspace into 256-byte aligned pieces as byte offsets (a size query has no base address to offset).
struct Carver {
    int64_t bytes = 0;
    int64_t take(int64_t nbytes) {
        const int64_t at = bytes;
        bytes += align256(nbytes);
        return at;
    }
};

template <class T>
inline T *carved(void *workspace, int64_t offset) { return reinterpret_cast<T *>(static_cast<char *>(workspace) + offset); }

// ---------------------------------------------------------------------------------------------- device helpers
// the first index of the ascending keys[0 .. n) whose key is not below k
template <class Key>
__host__ __device__ __forceinline__ int lower_bound(const Key *keys, int n, Key k) {
    int lo = 0, len = n;
    while (len > 0) {
        const int half = len >> 1;
        const bool right = keys[lo + half] < k;
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo;
}

// red[k][0] = the workgroup's sum of acc[k], every k through one LDS tree of a fixed order.  All BLOCK lanes call it.
template <int SUMS, int BLOCK>
__device__ __forceinline__ void block_tree_sum(double (&red)[SUMS][BLOCK], const double (&acc)[SUMS], int t) {
#pragma unroll
    for (int k = 0; k < SUMS; ++k) red[k][t] = acc[k];
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int k = 0; k < SUMS; ++k) red[k][t] += red[k][t + w];
        }
        __syncthreads();
    }
}

// tot[k] = the sum over j = 0 .. nb-1 of partials[(b0 + j) * SUMS + k] in a fixed order: RUNS strided runs in index order,
// then the runs in order.  A run is taken by BLOCK / RUNS >= SUMS lanes, one per sum (the others idle).
template <int SUMS, int RUNS, int BLOCK>
__device__ __forceinline__ void fold_partials(const double *partials, int b0, int nb, double (&run)[RUNS][SUMS],
                                              double (&tot)[SUMS], int t) {
    constexpr int LANES = BLOCK / RUNS;
    static_assert(SUMS <= LANES, "a run needs a lane per sum");
    const int g = t / LANES, k = t % LANES;
    if (k < SUMS) {
        double s = 0.0;
#pragma unroll 4
        for (int j = g; j < nb; j += RUNS) s += partials[(int64_t)(b0 + j) * SUMS + k];
        run[g][k] = s;
    }
    __syncthreads();
    if (t < SUMS) {
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < RUNS; ++r) v += run[r][t];
        tot[t] = v;
    }
    __syncthreads();
}

// One rotation of the cyclic Jacobi sweep of the symmetric N x N A (eigenvectors accumulate in the columns of V).
template <int N, int P, int Q>
__host__ __device__ __forceinline__ void jacobi_rotate(double (&A)[N][N], double (&V)[N][N]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));     // (theta = +-inf: 0)
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
    for (int k = 0; k < N; ++k) {                // A <- A J
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {                // A <- J^T A
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
    A[P][Q] = 0.0;
    A[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// the rotations (P, Q), (P, Q + 1), ... of one sweep, in lexicographic order
template <int N, int P, int Q>
__host__ __device__ __forceinline__ void jacobi_sweep_from(double (&A)[N][N], double (&V)[N][N]) {
    jacobi_rotate<N, P, Q>(A, V);
    if constexpr (Q + 1 < N) jacobi_sweep_from<N, P, Q + 1>(A, V);
    else if constexpr (P + 2 < N) jacobi_sweep_from<N, P + 1, P + 2>(A, V);
}

// Eigenvalues (the diagonal of A afterwards) and eigenvectors (the columns of V) of the symmetric A, by at most `sweeps`
// cyclic Jacobi sweeps in float64; a sweep starts only while the off-diagonal weight is above 1e-32 of the whole.  Which
// eigenpair the caller wants, and its tie rule, is the caller's.
template <int N>
__host__ __device__ __forceinline__ void jacobi_eigen(double (&A)[N][N], double (&V)[N][N], int sweeps) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < sweeps; ++sweep) {
        double off = 0.0, all = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                all += A[i][j] * A[i][j];
                if (i != j) off += A[i][j] * A[i][j];
            }
        if (!(off > 1e-32 * all)) break;         // (also a zero or non-finite matrix)
        jacobi_sweep_from<N, 0, 1>(A, V);
    }
}

}  // namespace hpl
