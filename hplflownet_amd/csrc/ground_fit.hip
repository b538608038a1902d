// ground_fit.hip -- the ground plane of each cloud of a packed ragged batch, fitted robustly on the device, every point
// classified by its signed height over it, and the non-ground indices compacted (hpl_ground_fit).
//
// k_ground_hyp: one lane per (cloud, hypothesis) draws three points of the cloud (Philox4x32-10, counter (h, call, purpose
// PHILOX_GROUND): a function of h, the cloud's size, seed and call alone) and writes the candidate plane's record -- first
// point a, unnormalised normal m, (tau tau) q -- into the workspace, and zeroes the hypothesis' count.
// k_ground_vote, the hot kernel (N x hyps plane tests): workgroups of 256 lanes, each inside ONE cloud, over a span of 1024
// consecutive points of it (lane l keeps points l, l + 256, l + 512, l + 768 in registers as float64) and a slab of 64
// hypotheses.  A hypothesis' record is wave-uniform: it is read through a uniform index, so it arrives by scalar loads and
// the test's operands come from scalar registers; no LDS traffic in the loop.  A (wave, hypothesis) count is
// __popcll(__ballot()) over the 64-bit mask, kept by the lane whose number is the hypothesis' place in the slab; the four
// waves' counts meet in LDS and leave the workgroup as ONE integer atomic add per hypothesis (64 consecutive words per
// instruction).  Integer counts commute: the totals do not depend on the order of arrival.
// k_ground_pick: one workgroup per cloud takes the most-voted hypothesis (the smallest h among equals) and normalises it.
// Per refinement round k_ground_reduce / k_ground_solve, structured as k_rigid_reduce / k_rigid_solve: ten float64 sums over
// the plane's inliers about the pivot a, one partial per workgroup through a fixed LDS tree, then a fixed-order fold and the
// eigenvector of the scatter matrix' smallest eigenvalue by cyclic Jacobi on one lane.
// k_ground_classify writes height / ground and counts the kept points per workgroup, k_ground_scan turns a cloud's counts into
// offsets (one workgroup per cloud, chunks of 256 in order) and k_ground_emit places every kept index: count / scan / emit,
// nobody waits for anybody.  6 + 2 refine launches (5 + 2 refine without keep_idx), no copy, no read-back,
// no floating-point atomic: the bits depend on the cloud alone, not on its place in a batch or on what else the device runs.
//
// The arithmetic is part of the interface (include/hpl_bcl.h; tests/ground_oracle.py restates it in numpy).
#include "cloud_common.h"
#include "philox.h"

#include <math.h>

using namespace hpl;

namespace {

constexpr int GF_MAX_HYPS = 1024;
constexpr int GF_MAX_REFINE = 8;
constexpr int GF_BLOCK = 256;
constexpr int GF_WAVES = GF_BLOCK / 64;
constexpr int GF_PER_LANE = 4;
constexpr int GF_SPAN = GF_BLOCK * GF_PER_LANE;      // S: points per workgroup
constexpr int GF_SLAB = 64;                          // Hc: hypotheses per vote workgroup, one per lane of a wave
constexpr int GF_REC = 8;                            // doubles per hypothesis: a[3], m[3], (tau tau) q or -1, q or -1
constexpr int GF_SUMS = 10;                          // count, sum dp[3], sum dp dp^T (xx, xy, xz, yy, yz, zz)
constexpr int GF_RUNS = GF_BLOCK / 16;               // strided runs of the solve kernel's sum
constexpr int GF_STATE = 16;                         // doubles per cloud: n[3], d, a[3], status, refinement over
constexpr int GF_SWEEPS = 12;

struct GroundArgs {
    const float *pc;
    int64_t pc_ld;
    double *hyp;                // [batch][hyps][GF_REC]
    double *state;              // [batch][GF_STATE]
    double *partials;           // [workgroups][GF_SUMS]
    int32_t *cnt;               // [batch][hyps]
    int32_t *blockoff;          // [workgroups]: kept points per workgroup, then their exclusive sums within the cloud
    float *plane, *height;
    int32_t *stats, *votes, *keep_idx;
    uint8_t *ground;
    double up[3], gate;         // gate = (min_cos min_cos) uu
    double tau, tau2, cut;
    uint32_t seed_lo, seed_hi, call_lo, call_hi;
    int32_t batch, hyps, last;
    int32_t pprefix[CLOUD_MAX_BATCH + 1];      // points of clouds 0 .. b-1 (N < 2^31 / 3)
    int32_t bprefix[CLOUD_MAX_BATCH + 1];      // workgroups of clouds 0 .. b-1
};

__device__ __forceinline__ bool load_point(const GroundArgs &a, int64_t i, double *p) {
    const float x = a.pc[i], y = a.pc[a.pc_ld + i], z = a.pc[2 * a.pc_ld + i];
    p[0] = (double)x; p[1] = (double)y; p[2] = (double)z;
    return isfinite(x) && isfinite(y) && isfinite(z);
}

__device__ __forceinline__ double dot3(const double *u, const double *v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__global__ void __launch_bounds__(GF_BLOCK) k_ground_hyp(const GroundArgs a) {
    const int b = (int)blockIdx.y, h = (int)(blockIdx.x * GF_BLOCK + threadIdx.x);
    if (h >= a.hyps) return;
    const int p0 = a.pprefix[b], n = a.pprefix[b + 1] - p0;
    double pa[3] = {0, 0, 0}, m[3] = {0, 0, 0}, q = -1.0;
    bool ok = n >= 3;
    if (ok) {
        const u4 r = philox4x32_10(u4{(uint32_t)h, a.call_lo, a.call_hi, PHILOX_GROUND}, a.seed_lo, a.seed_hi);
        const uint32_t w[3] = {r.x, r.y, r.z};
        double p[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) ok = load_point(a, (int64_t)p0 + (int64_t)(((uint64_t)w[k] * (uint64_t)n) >> 32), p[k]) && ok;
        double u[3], v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { pa[k] = p[0][k]; u[k] = p[1][k] - pa[k]; v[k] = p[2][k] - pa[k]; }
        m[0] = u[1] * v[2] - u[2] * v[1];
        m[1] = u[2] * v[0] - u[0] * v[2];
        m[2] = u[0] * v[1] - u[1] * v[0];
        q = dot3(m, m);
        double c = dot3(m, a.up);
        if (c < 0.0) { m[0] = -m[0]; m[1] = -m[1]; m[2] = -m[2]; c = -c; }
        ok = ok && q > 0.0 && isfinite(q) && c * c >= a.gate * q;
    }
    double *rec = a.hyp + ((int64_t)b * a.hyps + h) * GF_REC;
#pragma unroll
    for (int k = 0; k < 3; ++k) { rec[k] = ok ? pa[k] : 0.0; rec[3 + k] = ok ? m[k] : 0.0; }
    rec[6] = ok ? a.tau2 * q : -1.0;             // (s s <= -1 never holds: an invalid hypothesis collects no vote)
    rec[7] = ok ? q : -1.0;
    a.cnt[(int64_t)b * a.hyps + h] = 0;
}

__global__ void __launch_bounds__(GF_BLOCK) k_ground_vote(const GroundArgs a) {
    __shared__ int wcnt[GF_WAVES][GF_SLAB];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = block_group(a.bprefix, a.batch, blk);
    const int p0 = a.pprefix[b], p1 = a.pprefix[b + 1];
    const int64_t base = (int64_t)p0 + (int64_t)(blk - a.bprefix[b]) * GF_SPAN;
    double x[GF_PER_LANE], y[GF_PER_LANE], z[GF_PER_LANE];
    bool ok[GF_PER_LANE];
#pragma unroll
    for (int j = 0; j < GF_PER_LANE; ++j) {
        const int64_t i = base + j * GF_BLOCK + t;
        double p[3] = {0, 0, 0};
        ok[j] = i < p1 && load_point(a, i, p);
        x[j] = p[0]; y[j] = p[1]; z[j] = p[2];
    }
    const int h0 = (int)blockIdx.y * GF_SLAB;
    const int hn = (int)imin(GF_SLAB, a.hyps - h0);
    const double *rec = a.hyp + ((int64_t)b * a.hyps + h0) * GF_REC;
    int acc = 0;
    for (int h = 0; h < hn; ++h) {               // (rec, h are wave-uniform: scalar loads, scalar operands)
        const double ax = rec[h * GF_REC], ay = rec[h * GF_REC + 1], az = rec[h * GF_REC + 2];
        const double mx = rec[h * GF_REC + 3], my = rec[h * GF_REC + 4], mz = rec[h * GF_REC + 5];
        const double thr = rec[h * GF_REC + 6];
        int c = 0;
#pragma unroll
        for (int j = 0; j < GF_PER_LANE; ++j) {
            const double s = (mx * (x[j] - ax) + my * (y[j] - ay)) + mz * (z[j] - az);
            c += __popcll(__ballot(ok[j] && s * s <= thr));
        }
        acc = lane == h ? c : acc;
    }
    wcnt[wave][lane] = acc;
    __syncthreads();
    if (t < hn) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < GF_WAVES; ++w) v += wcnt[w][t];
        if (v) atomicAdd(&a.cnt[(int64_t)b * a.hyps + h0 + t], v);
    }
}

// The plane of the state as float32, once: what the classification reads back.
__device__ __forceinline__ void publish_plane(const GroundArgs &a, int b, const double *st) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.plane[(int64_t)b * 4 + k] = st[7] != 0.0 ? (float)st[k] : 0.f;
}

__global__ void __launch_bounds__(GF_BLOCK) k_ground_pick(const GroundArgs a) {
    __shared__ int bv[GF_BLOCK], bh[GF_BLOCK];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int n = a.pprefix[b + 1] - a.pprefix[b];
    int v = -1, hb = GF_MAX_HYPS;                // most votes, the smallest h among equals; (-1, MAX): no valid hypothesis
    for (int h = t; h < a.hyps; h += GF_BLOCK) {
        const bool valid = a.hyp[((int64_t)b * a.hyps + h) * GF_REC + 7] > 0.0;
        const int c = valid ? a.cnt[(int64_t)b * a.hyps + h] : -1;
        if (a.votes) a.votes[(int64_t)b * a.hyps + h] = c;
        if (c > v) { v = c; hb = h; }
    }
    bv[t] = v; bh[t] = hb;
    __syncthreads();
    for (int w = GF_BLOCK / 2; w > 0; w >>= 1) {
        if (t < w && (bv[t + w] > bv[t] || (bv[t + w] == bv[t] && bh[t + w] < bh[t]))) { bv[t] = bv[t + w]; bh[t] = bh[t + w]; }
        __syncthreads();
    }
    if (t != 0) return;
    double *st = a.state + (int64_t)b * GF_STATE;
    const bool ok = bv[0] >= 0;
#pragma unroll
    for (int k = 0; k < GF_STATE; ++k) st[k] = 0.0;
    if (ok) {
        const double *rec = a.hyp + ((int64_t)b * a.hyps + bh[0]) * GF_REC;
        const double r = sqrt(rec[7]);
        double nn[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { nn[k] = rec[3 + k] / r; st[k] = nn[k]; st[4 + k] = rec[k]; }
        st[3] = -dot3(nn, rec);
        st[7] = 1.0;
    }
    int32_t *o = a.stats + (int64_t)b * 4;
    o[0] = ok ? 1 : 0;
    o[1] = ok ? bh[0] : -1;
    o[2] = ok ? bv[0] : 0;
    o[3] = n;                    // (k_ground_scan writes the kept count)
    if (a.last) publish_plane(a, b, st);
}

__global__ void __launch_bounds__(GF_BLOCK) k_ground_reduce(const GroundArgs a) {
    __shared__ double red[GF_SUMS][GF_BLOCK];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = block_group(a.bprefix, a.batch, blk);
    const int p1 = a.pprefix[b + 1];
    const int64_t base = (int64_t)a.pprefix[b] + (int64_t)(blk - a.bprefix[b]) * GF_SPAN;
    const double *st = a.state + (int64_t)b * GF_STATE;
    const bool live = st[7] != 0.0 && st[8] == 0.0;
    const double nn[3] = {st[0], st[1], st[2]}, d = st[3], piv[3] = {st[4], st[5], st[6]};
    double acc[GF_SUMS];
#pragma unroll
    for (int k = 0; k < GF_SUMS; ++k) acc[k] = 0.0;
#pragma unroll
    for (int j = 0; j < GF_PER_LANE; ++j) {
        const int64_t i = base + j * GF_BLOCK + t;
        if (!live || i >= p1) continue;
        double p[3];
        if (!load_point(a, i, p)) continue;
        if (!(fabs(dot3(nn, p) + d) <= a.tau)) continue;
        const double dx = p[0] - piv[0], dy = p[1] - piv[1], dz = p[2] - piv[2];
        acc[0] += 1.0;
        acc[1] += dx; acc[2] += dy; acc[3] += dz;
        acc[4] += dx * dx; acc[5] += dx * dy; acc[6] += dx * dz;
        acc[7] += dy * dy; acc[8] += dy * dz; acc[9] += dz * dz;
    }
    block_tree_sum(red, acc, t);
    if (t < GF_SUMS) a.partials[(int64_t)blk * GF_SUMS + t] = red[t][0];
}

__global__ void __launch_bounds__(GF_BLOCK) k_ground_solve(const GroundArgs a) {
    __shared__ double run[GF_RUNS][GF_SUMS];
    __shared__ double tot[GF_SUMS];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    fold_partials<GF_SUMS, GF_RUNS, GF_BLOCK>(a.partials, a.bprefix[b], a.bprefix[b + 1] - a.bprefix[b], run, tot, t);
    if (t != 0) return;

    double *st = a.state + (int64_t)b * GF_STATE;
    if (st[7] != 0.0 && st[8] == 0.0) {
        const double W = tot[0];
        bool ok = W >= 3.0;
#pragma unroll
        for (int i = 0; i < GF_SUMS; ++i) ok = ok && isfinite(tot[i]);
        double nn[3] = {0, 0, 0}, d = 0.0;
        if (ok) {
            const double mu[3] = {tot[1] / W, tot[2] / W, tot[3] / W};
            double A[3][3], V[3][3];
            A[0][0] = tot[4] - (W * mu[0]) * mu[0];
            A[0][1] = A[1][0] = tot[5] - (W * mu[0]) * mu[1];
            A[0][2] = A[2][0] = tot[6] - (W * mu[0]) * mu[2];
            A[1][1] = tot[7] - (W * mu[1]) * mu[1];
            A[1][2] = A[2][1] = tot[8] - (W * mu[1]) * mu[2];
            A[2][2] = tot[9] - (W * mu[2]) * mu[2];
            jacobi_eigen(A, V, GF_SWEEPS);
            int best = 0;                                // the smallest eigenvalue; ties go to the smaller index
            double least = A[0][0];
#pragma unroll
            for (int i = 1; i < 3; ++i) {
                best = A[i][i] < least ? i : best;
                least = A[i][i] < least ? A[i][i] : least;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) nn[i] = best == 0 ? V[i][0] : best == 1 ? V[i][1] : V[i][2];
            const double r = sqrt(dot3(nn, nn));
#pragma unroll
            for (int i = 0; i < 3; ++i) nn[i] = nn[i] / r;
            double c = dot3(nn, a.up);
            if (c < 0.0) { nn[0] = -nn[0]; nn[1] = -nn[1]; nn[2] = -nn[2]; c = -c; }
            const double q = dot3(nn, nn);
            const double ctr[3] = {st[4] + mu[0], st[5] + mu[1], st[6] + mu[2]};
            d = -dot3(nn, ctr);
            ok = isfinite(nn[0]) && isfinite(nn[1]) && isfinite(nn[2]) && isfinite(d) && c * c >= a.gate * q;
        }
        if (ok) {
            st[0] = nn[0]; st[1] = nn[1]; st[2] = nn[2]; st[3] = d;
        } else {
            st[8] = 1.0;         // this round ends the refinement: the plane it started from stays
        }
    }
    if (a.last) publish_plane(a, b, st);
}

// valid, and the float64 height of point i over the float32 plane pl
__device__ __forceinline__ bool height_of(const GroundArgs &a, int64_t i, const double *pl, double *h) {
    double p[3];
    const bool valid = load_point(a, i, p);
    *h = dot3(pl, p) + pl[3];
    return valid;
}

__global__ void __launch_bounds__(GF_BLOCK) k_ground_classify(const GroundArgs a) {
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = block_group(a.bprefix, a.batch, blk);
    const int p1 = a.pprefix[b + 1];
    const int64_t base = (int64_t)a.pprefix[b] + (int64_t)(blk - a.bprefix[b]) * GF_SPAN;
    const bool fitted = a.stats[(int64_t)b * 4] != 0;
    double pl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pl[k] = (double)a.plane[(int64_t)b * 4 + k];
    int kept = 0;
#pragma unroll
    for (int j = 0; j < GF_PER_LANE; ++j) {
        const int64_t i = base + j * GF_BLOCK + t;
        bool keep = false;
        if (i < p1) {
            double h;
            const bool valid = height_of(a, i, pl, &h);
            const bool gr = fitted && valid && h <= a.cut;
            keep = !gr;
            if (a.height) a.height[i] = !fitted ? 0.f : valid ? (float)h : NAN;
            if (a.ground) a.ground[i] = gr ? 1 : 0;
        }
        kept += __syncthreads_count(keep ? 1 : 0);
    }
    if (t == 0) a.blockoff[blk] = kept;
}

__global__ void __launch_bounds__(GF_BLOCK) k_ground_scan(const GroundArgs a) {
    // (k_frames_scan and k_outlier_scan have this text too: as one function it was refused for both by rule R)
    __shared__ int sc[GF_BLOCK];
    __shared__ int carry;
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b0 = a.bprefix[b], nb = a.bprefix[b + 1] - b0;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < nb; c0 += GF_BLOCK) {
        const int j = c0 + t;
        const int v = j < nb ? a.blockoff[b0 + j] : 0;
        sc[t] = v;
        __syncthreads();
        for (int w = 1; w < GF_BLOCK; w <<= 1) {             // inclusive sums of the chunk
            const int u = t >= w ? sc[t - w] : 0;
            __syncthreads();
            sc[t] += u;
            __syncthreads();
        }
        const int before = carry;
        if (j < nb) a.blockoff[b0 + j] = before + sc[t] - v;
        __syncthreads();
        if (t == GF_BLOCK - 1) carry = before + sc[t];
        __syncthreads();
    }
    if (t == 0) a.stats[(int64_t)b * 4 + 3] = carry;
}

__global__ void __launch_bounds__(GF_BLOCK) k_ground_emit(const GroundArgs a) {
    // (k_outlier_emit ranks the same way: as one function for both, each call's A/B fell outside the parent's span in some
    // setting -- rule R)
    __shared__ int wc[GF_PER_LANE * GF_WAVES];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = block_group(a.bprefix, a.batch, blk);
    const int p0 = a.pprefix[b], p1 = a.pprefix[b + 1];
    const int64_t base = (int64_t)p0 + (int64_t)(blk - a.bprefix[b]) * GF_SPAN;
    const bool fitted = a.stats[(int64_t)b * 4] != 0;
    const int total = a.stats[(int64_t)b * 4 + 3];
    double pl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pl[k] = (double)a.plane[(int64_t)b * 4 + k];
    bool keep[GF_PER_LANE];
    int below[GF_PER_LANE];                      // kept points of the same wave and row in lower lanes
#pragma unroll
    for (int j = 0; j < GF_PER_LANE; ++j) {
        const int64_t i = base + j * GF_BLOCK + t;
        keep[j] = false;
        if (i < p1) {
            double h;
            const bool valid = height_of(a, i, pl, &h);
            keep[j] = !(fitted && valid && h <= a.cut);
        }
        const unsigned long long m = __ballot(keep[j]);
        below[j] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wc[j * GF_WAVES + wave] = __popcll(m);
    }
    __syncthreads();
    int run = a.blockoff[blk];                   // kept points of the cloud before this workgroup's
#pragma unroll
    for (int j = 0; j < GF_PER_LANE; ++j) {
        const int64_t i = base + j * GF_BLOCK + t;
#pragma unroll
        for (int w = 0; w < GF_WAVES; ++w) {
            if (w == wave && keep[j]) a.keep_idx[(int64_t)p0 + run + below[j]] = (int32_t)i;
            run += wc[j * GF_WAVES + w];
        }
        if (i < p1 && i - p0 >= total) a.keep_idx[i] = -1;  // (kept indices land below `total`, these at or above it)
    }
}

// workspace: the hypotheses' records | the clouds' state | the reduce partials | the votes | the kept counts per workgroup
struct Layout {                  // byte offsets
    int64_t hyp, state, partials, cnt, blockoff, bytes;
    Layout(int batch, int64_t n_total, int hyps) {
        const int64_t blocks = cdiv(n_total, GF_SPAN) + batch;
        Carver c;
        hyp = c.take((int64_t)sizeof(double) * batch * hyps * GF_REC);
        state = c.take((int64_t)sizeof(double) * batch * GF_STATE);
        partials = c.take((int64_t)sizeof(double) * blocks * GF_SUMS);
        cnt = c.take((int64_t)sizeof(int32_t) * batch * hyps);
        blockoff = c.take((int64_t)sizeof(int32_t) * blocks);
        bytes = c.bytes;
    }
};

}  // namespace

extern "C" int64_t hpl_ground_fit_workspace_bytes(int batch, int64_t n_total, int hyps) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || n_total < 0 || n_total >= CLOUD_MAX_POINTS || hyps < 1 || hyps > GF_MAX_HYPS) return -1;
    return Layout(batch, n_total, hyps).bytes;
}

extern "C" int hpl_ground_fit(const float *pc, int64_t pc_ld, int batch, const int64_t *prefix, const float *up, float min_cos,
                              int hyps, float tau, int refine, float cut, uint64_t seed, uint64_t call, float *plane,
                              int32_t *stats, int32_t *votes, float *height, uint8_t *ground, int32_t *keep_idx, void *workspace,
                              int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_ground_fit";
    HPL_REQUIRE(pc && prefix && up && plane && stats && workspace, "hpl_ground_fit: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(hyps >= 1 && hyps <= GF_MAX_HYPS, "hpl_ground_fit: hyps = %d (1 .. %d)", hyps, GF_MAX_HYPS);
    HPL_REQUIRE(refine >= 0 && refine <= GF_MAX_REFINE, "hpl_ground_fit: refine = %d (0 .. %d)", refine, GF_MAX_REFINE);
    HPL_REQUIRE(tau > 0.f && isfinite(tau), "hpl_ground_fit: tau must be finite and > 0");
    HPL_REQUIRE(cut >= 0.f && isfinite(cut), "hpl_ground_fit: cut must be finite and >= 0");
    HPL_REQUIRE(min_cos > 0.f && min_cos <= 1.f, "hpl_ground_fit: min_cos must be in (0, 1]");
    const double uu = ((double)up[0] * (double)up[0] + (double)up[1] * (double)up[1]) + (double)up[2] * (double)up[2];
    HPL_REQUIRE(isfinite(up[0]) && isfinite(up[1]) && isfinite(up[2]) && uu > 0.0, "hpl_ground_fit: up must be finite and not zero");
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix", "cloud", prefix, batch));
    const int64_t N = prefix[batch];
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_CLOUD_CHECK(check_row_stride(op, pc_ld, N));
    const Layout l(batch, N, hyps);
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 8, workspace_bytes_, l.bytes));
    HPL_CLOUD_CHECK(check_aligned4(op, {pc, plane, stats, votes, height, keep_idx}));
    if (N == 0) return HPL_OK;
    GroundArgs a{};
    const int64_t blocks = narrow_prefix(prefix, batch, GF_SPAN, a.pprefix, a.bprefix);
    a.pc = pc; a.pc_ld = pc_ld;
    a.hyp = carved<double>(workspace, l.hyp);
    a.state = carved<double>(workspace, l.state);
    a.partials = carved<double>(workspace, l.partials);
    a.cnt = carved<int32_t>(workspace, l.cnt);
    a.blockoff = carved<int32_t>(workspace, l.blockoff);
    a.plane = plane; a.height = height; a.stats = stats; a.votes = votes; a.keep_idx = keep_idx; a.ground = ground;
    for (int k = 0; k < 3; ++k) a.up[k] = (double)up[k];
    a.gate = ((double)min_cos * (double)min_cos) * uu;
    a.tau = (double)tau;
    a.tau2 = a.tau * a.tau;
    a.cut = (double)cut;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.call_lo = (uint32_t)call; a.call_hi = (uint32_t)(call >> 32);
    a.batch = batch; a.hyps = hyps;
    hipStream_t s = to_stream(stream);
    k_ground_hyp<<<dim3((unsigned)cdiv(hyps, GF_BLOCK), (unsigned)batch), GF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_ground_fit (hypotheses)");
    k_ground_vote<<<dim3((unsigned)blocks, (unsigned)cdiv(hyps, GF_SLAB)), GF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_ground_fit (vote)");
    a.last = refine == 0;
    k_ground_pick<<<batch, GF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_ground_fit (pick)");
    for (int k = 1; k <= refine; ++k) {
        a.last = k == refine;
        k_ground_reduce<<<(unsigned)blocks, GF_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_ground_fit (reduce)");
        k_ground_solve<<<batch, GF_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_ground_fit (solve)");
    }
    k_ground_classify<<<(unsigned)blocks, GF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_ground_fit (classify)");
    k_ground_scan<<<batch, GF_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_ground_fit (scan)");
    if (keep_idx) {
        k_ground_emit<<<(unsigned)blocks, GF_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_ground_fit (emit)");
    }
    return HPL_OK;
}
