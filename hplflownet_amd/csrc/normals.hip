// normals.hip -- surface normals of packed ragged clouds (hpl_normals): per point its k nearest neighbours
// within a radius, taken exactly on a sorted uniform grid over the cloud itself, and the eigenvector of the smallest
// eigenvalue of their float64 scatter matrix, oriented towards a viewpoint.
//
// The definition of a neighbourhood is the all-pairs one of include/hpl_bcl.h; the grid only finds the candidates.  The cell
// edge is 1.001 radius and a point's cell floor(x / (1.001 radius)) is taken in float64 (the key, the cell and the record are
// grid_common.h's), so a point within radius of another (even by the rounded float32 d2) lies in
// its cell or an adjacent one.
//
//   k_normals_keys  a lane per point: the 64-bit key (cloud, cell x, y, z) -- a point that takes no part carries the largest
//                   key -- and its 16-byte (x, y, z, index) record
//   rocPRIM         ONE stable radix sort of (key, record) per call
//   k_normals<K>    a lane per SORTED record: the lanes of a wave sit in the same or adjacent cells, so they read the same
//                   runs and leave their loops together.  The 27 cells around the point as 9 runs of three z-adjacent cells
//                   (two binary searches each, all 18 in lockstep); the K best (d2, index) pairs in registers -- every list
//                   access has a compile-time index, an insertion is one unrolled pass behind a single compare with the
//                   worst entry --; the k points read again by index for the float64 mean and scatter sums in list order;
//                   cyclic Jacobi on the lane; everything written to the record's original index.
//
// No floating-point atomic, no read-back, no lane waits for another; every loop is bounded by a cell population or a search
// depth.  The bits depend on the cloud alone.
#include "grid_common.h"

#include <limits.h>
#include <math.h>

using namespace hpl;

namespace {

constexpr int NR_BLOCK = 256;
constexpr int NR_MIN_K = 3;
constexpr int NR_MAX_K = 32;
constexpr int NR_AHEAD = 4;                          // records of a run loaded before they are compared
constexpr int NR_SWEEPS = 12;                        // ground_fit.hip's GF_SWEEPS

struct NormalsArgs {
    const float *pc;
    int64_t pc_ld;
    float *normal;
    int64_t normal_ld;
    float *curvature;
    int32_t *count, *nbr;
    float *nbr_d2;
    u64 *key, *skey;
    GridRec *rec, *srec;
    double inv_cell;
    float r2;
    int32_t n, batch, k;
    int32_t prefix[CLOUD_MAX_BATCH + 1];
    float view[CLOUD_MAX_BATCH][3];
};

__global__ void __launch_bounds__(NR_BLOCK) k_normals_keys(const NormalsArgs a) {
    const int64_t j64 = (int64_t)blockIdx.x * NR_BLOCK + threadIdx.x;
    if (j64 >= a.n) return;
    const int j = (int)j64;
    grid_store(a, a.prefix, j, a.pc[j], a.pc[a.pc_ld + j], a.pc[2 * a.pc_ld + j]);
}

template <int K>
__global__ void __launch_bounds__(NR_BLOCK) k_normals(const NormalsArgs a) {
    const int64_t s64 = (int64_t)blockIdx.x * NR_BLOCK + threadIdx.x;
    if (s64 >= a.n) return;
    const int s = (int)s64;
    const u64 key = a.skey[s];
    const GridRec me = a.srec[s];
    const int64_t i = me.i;

    float ld[K];                                 // the list: ascending (d2, index); unused entries (+inf, INT_MAX)
    int lj[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { ld[t] = INFINITY; lj[t] = INT_MAX; }

    if (key != ~0ull) {
        const int b = grid_group(key);
        int c[3], lo[9], hi[9];
        grid_cell(key, c);
        // The 9 runs [lo, hi): lower_bound of the run's first key and of the key behind its last, all 18 searches in lockstep
        // (the step sizes depend on n alone, so the 18 loads of a step are independent).  match_point of icp_common.h has the
        // same text: through one function for both, k_normals<32> was 0.4 % slower (rule R).
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
            for (int t = pick9(lo, run); t < end; t += NR_AHEAD) {
                GridRec r[NR_AHEAD];             // independent loads, in flight together; those past the run repeat its last
#pragma unroll
                for (int v = 0; v < NR_AHEAD; ++v) r[v] = a.srec[min(t + v, end - 1)];
#pragma unroll
                for (int v = 0; v < NR_AHEAD; ++v) {
                    const float ex = me.x - r[v].x, ey = me.y - r[v].y, ez = me.z - r[v].z;
                    const float d2 = (ex * ex + ey * ey) + ez * ez;
                    const int j = r[v].i;
                    // the cells are not in index order: the tie rule is here.  A repeated record is no candidate.
                    if (t + v < end && d2 <= a.r2 && (d2 < ld[K - 1] || (d2 == ld[K - 1] && j < lj[K - 1]))) {
                        bool before[K];          // the candidate comes before entry q
#pragma unroll
                        for (int q = 0; q < K; ++q) before[q] = d2 < ld[q] || (d2 == ld[q] && j < lj[q]);
#pragma unroll
                        for (int q = K - 1; q > 0; --q) {
                            ld[q] = before[q - 1] ? ld[q - 1] : (before[q] ? d2 : ld[q]);
                            lj[q] = before[q - 1] ? lj[q - 1] : (before[q] ? j : lj[q]);
                        }
                        ld[0] = before[0] ? d2 : ld[0];
                        lj[0] = before[0] ? j : lj[0];
                    }
                }
            }
        }
    }

    int cnt = 0;
#pragma unroll
    for (int t = 0; t < K; ++t) cnt += (t < a.k && lj[t] != INT_MAX) ? 1 : 0;
    if (a.count) a.count[i] = cnt;
    if (a.nbr) {
#pragma unroll
        for (int t = 0; t < K; ++t)
            if (t < a.k) a.nbr[i * a.k + t] = t < cnt ? lj[t] : -1;
    }
    if (a.nbr_d2) {
#pragma unroll
        for (int t = 0; t < K; ++t)
            if (t < a.k) a.nbr_d2[i * a.k + t] = t < cnt ? ld[t] : INFINITY;
    }

    float out[4] = {0.f, 0.f, 0.f, 0.f};         // the normal and the curvature
    if (cnt >= 3) {
        double m[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < K; ++t) {
            if (t < cnt) {
#pragma unroll
                for (int c = 0; c < 3; ++c) m[c] += (double)a.pc[c * a.pc_ld + lj[t]];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = m[c] / (double)cnt;
        double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};            // xx, xy, xz, yy, yz, zz
#pragma unroll
        for (int t = 0; t < K; ++t) {
            if (t < cnt) {
                double d[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) d[c] = (double)a.pc[c * a.pc_ld + lj[t]] - m[c];
                C[0] += d[0] * d[0]; C[1] += d[0] * d[1]; C[2] += d[0] * d[2];
                C[3] += d[1] * d[1]; C[4] += d[1] * d[2]; C[5] += d[2] * d[2];
            }
        }
        double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}}, V[3][3];
        jacobi_eigen(A, V, NR_SWEEPS);
        const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
        const bool one = l1 < l0, two = l2 < (one ? l1 : l0);    // ties to the smaller column
        const double lmin = two ? l2 : (one ? l1 : l0), lmax = fmax(fmax(l0, l1), l2);
        double nv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) nv[c] = two ? V[c][2] : (one ? V[c][1] : V[c][0]);
        if (isfinite(l0) && isfinite(l1) && isfinite(l2) && lmax > 0.0) {
            const double len = sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) nv[c] = nv[c] / len;
            const int b = grid_group(key);
            const double sx = nv[0] * ((double)a.view[b][0] - (double)me.x), sy = nv[1] * ((double)a.view[b][1] - (double)me.y),
                         sz = nv[2] * ((double)a.view[b][2] - (double)me.z);
            const double sd = (sx + sy) + sz;
            const double lead = nv[0] != 0.0 ? nv[0] : (nv[1] != 0.0 ? nv[1] : nv[2]);
            const bool flip = sd < 0.0 || (sd == 0.0 && lead < 0.0);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = (float)(flip ? -nv[c] : nv[c]);
            out[3] = (float)(fmax(lmin, 0.0) / ((l0 + l1) + l2));
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.normal[c * a.normal_ld + i] = out[c];
    if (a.curvature) a.curvature[i] = out[3];
}

// the room of the one sort of (key, record)
inline int64_t temp_room(int64_t n) {
    return room_next_pow2(n, [](int64_t c) { return radix_temp_bytes<u64, GridRec>(c, 64u); });
}

// workspace: key | sorted key | records | sorted records | rocPRIM temporaries
struct Layout {                  // byte offsets
    int64_t key, skey, rec, srec, bytes;
    explicit Layout(int64_t n) {
        Carver c;
        key = c.take(n * 8);
        skey = c.take(n * 8);
        rec = c.take(n * (int64_t)sizeof(GridRec));
        srec = c.take(n * (int64_t)sizeof(GridRec));
        bytes = c.bytes;
    }
};

int64_t workspace_bytes(int64_t n) { return Layout(n).bytes + temp_room(n); }

inline bool overlaps(const void *p, int64_t pbytes, const void *q, int64_t qbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && pbytes > 0 && qbytes > 0 && a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}

inline int64_t extent(int rows, int64_t ld, int64_t n) { return n > 0 ? ((rows - 1) * ld + n) * 4 : 0; }      // bytes

}  // namespace

extern "C" int64_t hpl_normals_workspace_bytes(int batch, int64_t n_total) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || n_total < 0 || n_total >= CLOUD_MAX_POINTS) return -1;
    return workspace_bytes(n_total);
}

extern "C" int hpl_normals(const float *pc, int64_t pc_ld, int batch, const int64_t *prefix, int k, float radius,
                           const float *viewpoint, float *normal, int64_t normal_ld, float *curvature, int32_t *count,
                           int32_t *nbr, float *nbr_d2, void *workspace, int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_normals";
    HPL_REQUIRE(pc && normal && prefix && workspace, "hpl_normals: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(k >= NR_MIN_K && k <= NR_MAX_K, "hpl_normals: k = %d (%d .. %d)", k, NR_MIN_K, NR_MAX_K);
    HPL_REQUIRE(radius > 0.f && isfinite(radius), "hpl_normals: radius must be finite and > 0");
    if (viewpoint)
        for (int b = 0; b < 3 * batch; ++b) HPL_REQUIRE(isfinite(viewpoint[b]), "hpl_normals: the viewpoint of cloud %d is not finite", b / 3);
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix", "cloud", prefix, batch));
    const int64_t N = prefix[batch];
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_REQUIRE(!(nbr || nbr_d2) || N * k < ((int64_t)1 << 31), "hpl_normals: %lld points of %d neighbours pass the 32-bit element limit (N k < 2^31)",
                (long long)N, k);
    HPL_CLOUD_CHECK(check_row_stride(op, pc_ld, N));
    HPL_CLOUD_CHECK(check_row_stride(op, normal_ld, N));
    const int64_t need = workspace_bytes(N);
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, need));
    HPL_CLOUD_CHECK(check_aligned4(op, {pc, normal, curvature, count, nbr, nbr_d2}));
    {
        const void *const outs[5] = {normal, curvature, count, nbr, nbr_d2};
        const int64_t out_bytes[5] = {extent(3, normal_ld, N), 4 * N, 4 * N, 4 * N * k, 4 * N * k};
        for (int o = 0; o < 5; ++o) {
            HPL_REQUIRE(!overlaps(outs[o], out_bytes[o], pc, extent(3, pc_ld, N)), "hpl_normals: an output overlaps the input");
            HPL_REQUIRE(!overlaps(outs[o], out_bytes[o], workspace, need), "hpl_normals: an output overlaps the workspace");
        }
    }
    if (N == 0) return HPL_OK;

    const Layout L(N);
    void *const temp = carved<char>(workspace, L.bytes);
    NormalsArgs a{};
    a.pc = pc; a.pc_ld = pc_ld; a.normal = normal; a.normal_ld = normal_ld; a.curvature = curvature;
    a.count = count; a.nbr = nbr; a.nbr_d2 = nbr_d2;
    a.key = carved<u64>(workspace, L.key); a.skey = carved<u64>(workspace, L.skey);
    a.rec = carved<GridRec>(workspace, L.rec); a.srec = carved<GridRec>(workspace, L.srec);
    a.inv_cell = 1.0 / (GRID_CELL_MARGIN * (double)radius);
    a.r2 = radius * radius;                      // rounded once to float32, as the acceptance states
    a.n = (int32_t)N; a.batch = batch; a.k = k;
    narrow_prefix(prefix, batch, NR_BLOCK, a.prefix, nullptr);
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < 3; ++c) a.view[b][c] = viewpoint ? viewpoint[3 * b + c] : 0.f;

    hipStream_t s = to_stream(stream);
    const unsigned blocks = (unsigned)cdiv(N, NR_BLOCK);
    k_normals_keys<<<blocks, NR_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_normals (keys)");
    size_t tb = (size_t)temp_room(N);
    const hipError_t e = rocprim::radix_sort_pairs(temp, tb, (const u64 *)a.key, a.skey, (const GridRec *)a.rec, a.srec, (size_t)N, 0u,
                                                   64u, s);      // (the largest key, of the points left out, has every bit set)
    if (e != hipSuccess) { set_error("hpl_normals: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    if (k <= 8) k_normals<8><<<blocks, NR_BLOCK, 0, s>>>(a);
    else if (k <= 16) k_normals<16><<<blocks, NR_BLOCK, 0, s>>>(a);
    else k_normals<32><<<blocks, NR_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_normals (search)");
    return HPL_OK;
}
