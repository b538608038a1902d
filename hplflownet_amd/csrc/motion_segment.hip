// motion_segment.hip -- moving objects from a flow field (hpl_motion_segment): the points a rigid fit leaves
// unexplained (residual > tau), grouped into the connected components of a fixed-radius graph over position and flow, numbered,
// and each object's size, centroid and mean flow -- without a host round trip.
//
// The definition is the all-pairs predicate of include/hpl_bcl.h; a uniform grid only finds the candidates.  The cell edge is
// 1.001 eps and a point's cell floor(x / (1.001 eps)) is taken in float64, so two points within eps of each other (even by the
// rounded float32 predicate, which can exceed the real one by a few 2^-24) lie in the same or in adjacent cells: 27 cells hold
// every partner.
//
//   k_seg_keys     a lane per point: mover or not, the 64-bit key (pair, cell x, y, z), parent[i] = i, labels -1 / -3
//   rocPRIM        stable radix sort of ALL points by key (non-movers carry the largest key and end up behind the movers): the
//                  size of every launch is a host number, nothing is read back
//   k_seg_link     a lane per sorted mover: 9 binary searches for the runs of 3 z-adjacent cells, the predicate against every
//                  earlier-indexed point of them, and for a linked pair the union of the two trees: the larger root is hooked
//                  under the smaller one by a compare-and-swap that succeeds only on a root.  A parent word only ever
//                  decreases, a failed swap hands back a smaller index to go on from: no lane waits for another, every loop
//                  is bounded by the tree depth or the cell population
//   k_seg_flatten  a lane per point: its root (the smallest index of its component), one integer atomic on the root's size
//   k_seg_flag     roots of at least min_points movers
//   rocPRIM        exclusive scan of the flags in index order: the objects' numbers (a pair's base is subtracted)
//   k_seg_label    labels, the key (object number) of the second sort, points in objects
//   rocPRIM        stable radix sort by object number: an object's points in index order
//   k_seg_objects  a workgroup per (pair, table row): float64 sums in a fixed order (lane l takes the object's points l, l + 256,
//                  ..., then an LDS tree), rounded once
//
// Integer counts do not depend on their order, the float sums have one order, the root is the smallest index: every output of
// a pair is the same bits alone, anywhere in a batch and beside other work.  The key, its limits, the counter and the room of
// the sorts are grid_common.h's.
#include "grid_common.h"

#include <math.h>
#include <rocprim/device/device_scan.hpp>

using namespace hpl;

namespace {

constexpr int MS_MAX_OBJECTS = 4096;
constexpr int MS_BLOCK = 256;

struct SegArgs {
    const float *pc;
    int64_t pc_ld;
    const float *flow;
    int64_t fsc, fsp;
    const float *residual;
    float tau, eps2, dv2;
    double inv_cell;
    int32_t n, batch, min_points, max_objects;
    u64 *key, *skey;
    int32_t *val, *sval;            // point indices: 0 .. n-1, and in key order
    int32_t *parent, *size;         // per point: parent (-1: no mover), and on a root the size of its component
    int32_t *flag, *excl;           // n + 1 each: object roots, and how many of them lie before an index
    uint32_t *okey, *sokey;         // the second sort: object number (n: none)
    int32_t *soval;
    int32_t *labels, *obj_info, *stats;
    float *obj_motion;
    int32_t pprefix[CLOUD_MAX_BATCH + 1];
};

// the pair of point i: the last one that starts at or before i
__device__ __forceinline__ int pair_of(const SegArgs &a, int i) { return group_of(a.pprefix, a.batch, i); }

__global__ void __launch_bounds__(MS_BLOCK) k_seg_keys(const SegArgs a) {
    const int64_t i0 = (int64_t)blockIdx.x * MS_BLOCK;
    const int64_t i64 = i0 + threadIdx.x;
    const bool in = i64 < a.n;
    const int i = in ? (int)i64 : a.n - 1;
    const int b = pair_of(a, i);
    const bool uniform = pair_of(a, (int)i0) == pair_of(a, (int)imin(i0 + MS_BLOCK - 1, a.n - 1));
    bool mover = false, oob = false;
    u64 key = ~0ull;
    if (in) {
        const float x = a.pc[i], y = a.pc[a.pc_ld + i], z = a.pc[2 * a.pc_ld + i];
        const float *f = a.flow + (int64_t)i * a.fsp;
        const float fx = f[0], fy = f[a.fsc], fz = f[2 * a.fsc];
        const float r = a.residual[i];
        const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(fx) && isfinite(fy) && isfinite(fz);
        if (ok && r > a.tau) {                   // (a NaN residual fails the comparison)
            const double cx = floor((double)x * a.inv_cell), cy = floor((double)y * a.inv_cell), cz = floor((double)z * a.inv_cell);
            mover = fabs(cx) <= GRID_CELL_MAX && fabs(cy) <= GRID_CELL_MAX && fabs(cz) <= GRID_CELL_MAX;
            oob = !mover;
            if (mover) key = grid_key(b, (int)cx + GRID_CELL_BIAS, (int)cy + GRID_CELL_BIAS, (int)cz + GRID_CELL_BIAS);
        }
        a.key[i] = key;
        a.val[i] = i;
        a.parent[i] = mover ? i : -1;
        a.size[i] = 0;
        a.labels[i] = oob ? -3 : -1;
    }
    count_into(a.stats, uniform, b, 0, mover ? 1 : 0);
    count_into(a.stats, uniform, b, 3, oob ? 1 : 0);
}

__device__ __forceinline__ int load_parent(const int32_t *parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree as far as this lane can see it: a stale look only ends higher up the same tree.  parent[x] < x off a root.
__device__ __forceinline__ int find_root(const int32_t *parent, int x) {
    int p = load_parent(parent, x);
    while (p != x) {
        x = p;
        p = load_parent(parent, x);
    }
    return x;
}

__device__ __forceinline__ void unite(int32_t *parent, int u, int v) {
    int ru = find_root(parent, u), rv = find_root(parent, v);
    while (ru != rv) {
        const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;                   // hi was a root and now hangs under lo
        // hi has been hooked by another lane meanwhile: old < hi is its parent.  max(ru, rv) falls with every turn.
        ru = find_root(parent, old);
        rv = lo;
    }
}

__global__ void __launch_bounds__(MS_BLOCK) k_seg_link(const SegArgs a) {
    const int64_t s64 = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (s64 >= a.n) return;
    const int s = (int)s64;
    const u64 key = a.skey[s];
    if (key == ~0ull) return;
    const int i = a.sval[s];
    const float x = a.pc[i], y = a.pc[a.pc_ld + i], z = a.pc[2 * a.pc_ld + i];
    const float *f = a.flow + (int64_t)i * a.fsp;
    const float fx = f[0], fy = f[a.fsc], fz = f[2 * a.fsc];
    int c[3];
    grid_cell(key, c);
    const int b = grid_group(key);
    for (int dx = -1; dx <= 1; ++dx) {
        for (int dy = -1; dy <= 1; ++dy) {
            const u64 klo = grid_key(b, c[0] + dx, c[1] + dy, c[2] - 1), khi = grid_key(b, c[0] + dx, c[1] + dy, c[2] + 1);
            // every link is made once, by its later-indexed end
            for (int t = lower_bound(a.skey, a.n, klo); t < a.n && a.skey[t] <= khi; ++t) {
                const int j = a.sval[t];
                if (j >= i) continue;
                const float ex = x - a.pc[j], ey = y - a.pc[a.pc_ld + j], ez = z - a.pc[2 * a.pc_ld + j];
                const float d2 = (ex * ex + ey * ey) + ez * ez;
                if (!(d2 <= a.eps2)) continue;
                const float *g = a.flow + (int64_t)j * a.fsp;
                const float gx = fx - g[0], gy = fy - g[a.fsc], gz = fz - g[2 * a.fsc];
                const float g2 = (gx * gx + gy * gy) + gz * gz;
                if (!(g2 <= a.dv2)) continue;
                unite(a.parent, i, j);
            }
        }
    }
}

__global__ void __launch_bounds__(MS_BLOCK) k_seg_flatten(const SegArgs a) {
    const int64_t i64 = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i64 >= a.n) return;
    const int i = (int)i64;
    int r = a.parent[i];                         // (the link kernel is over: plain loads see the final forest)
    if (r < 0) return;
    int p = r;
    while ((p = a.parent[r]) != r) r = p;
    a.okey[i] = (uint32_t)r;                     // the root, until k_seg_label turns it into the object number
    // lanes of one component share a root: one atomic for those that agree with the wave's first active lane
    const int r0 = __builtin_amdgcn_readfirstlane(r);
    const bool same = r == r0;
    const u64 m = __ballot(same);
    if (same) {
        if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x & 63)) == (int)(threadIdx.x & 63)) atomicAdd(&a.size[r0], __popcll(m));
    } else {
        atomicAdd(&a.size[r], 1);
    }
}

__global__ void __launch_bounds__(MS_BLOCK) k_seg_flag(const SegArgs a) {
    const int64_t i64 = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i64 > a.n) return;
    const int i = (int)i64;
    a.flag[i] = (i < a.n && a.parent[i] == i && a.size[i] >= a.min_points) ? 1 : 0;
}

__global__ void __launch_bounds__(MS_BLOCK) k_seg_label(const SegArgs a) {
    const int64_t i0 = (int64_t)blockIdx.x * MS_BLOCK;
    const int64_t i64 = i0 + threadIdx.x;
    const bool in = i64 < a.n;
    const int i = in ? (int)i64 : a.n - 1;
    const int b = pair_of(a, i);
    const bool uniform = pair_of(a, (int)i0) == pair_of(a, (int)imin(i0 + MS_BLOCK - 1, a.n - 1));
    bool member = false;
    if (in) {
        uint32_t k = (uint32_t)a.n;
        if (a.parent[i] >= 0) {
            const int r = (int)a.okey[i];
            member = a.flag[r] != 0;
            if (member) k = (uint32_t)a.excl[r];
            a.labels[i] = member ? a.excl[r] - a.excl[a.pprefix[b]] : -2;
        }
        a.okey[i] = k;
    }
    count_into(a.stats, uniform, b, 2, member ? 1 : 0);
}

__global__ void __launch_bounds__(MS_BLOCK) k_seg_objects(const SegArgs a) {
    __shared__ double red[6][MS_BLOCK];
    const int b = (int)blockIdx.x / a.max_objects, o = (int)blockIdx.x % a.max_objects, t = (int)threadIdx.x;
    const int p0 = a.pprefix[b];
    const int base = a.excl[p0], count = a.excl[a.pprefix[b + 1]] - base;
    if (o == 0 && t == 0) a.stats[b * 4 + 1] = count;
    int32_t *info = a.obj_info + ((int64_t)b * a.max_objects + o) * 2;
    float *motion = a.obj_motion + ((int64_t)b * a.max_objects + o) * 6;
    // the object's run in the second sort: its points in index order, the root first
    const int lo = lower_bound(a.sokey, o < count ? a.n : 0, (uint32_t)(base + o));
    if (o >= count || lo >= a.n) {               // an unused row (an object always has its run)
        if (t == 0) { info[0] = -1; info[1] = 0; }
        if (t < 6) motion[t] = 0.f;
        return;
    }
    const int root = a.soval[lo], m = (int)imin(a.size[root], a.n - lo);
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int j = t; j < m; j += MS_BLOCK) {
        const int i = a.soval[lo + j];
        const float *f = a.flow + (int64_t)i * a.fsp;
        acc[0] += (double)a.pc[i];
        acc[1] += (double)a.pc[a.pc_ld + i];
        acc[2] += (double)a.pc[2 * a.pc_ld + i];
        acc[3] += (double)f[0];
        acc[4] += (double)f[a.fsc];
        acc[5] += (double)f[2 * a.fsc];
    }
    block_tree_sum(red, acc, t);
    if (t == 0) { info[0] = root - p0; info[1] = m; }
    if (t < 6) motion[t] = (float)(red[t][0] / (double)m);
}

// the two sorts and the scan share the room: enough for any of them
size_t temp_bytes(int64_t n) {
    size_t sc = 0;
    (void)rocprim::exclusive_scan(nullptr, sc, (const int32_t *)nullptr, (int32_t *)nullptr, 0, (size_t)(n + 1),
                                  rocprim::plus<int32_t>(), (hipStream_t) nullptr);
    const size_t s1 = radix_temp_bytes<u64, int32_t>(n, 64u), s2 = radix_temp_bytes<uint32_t, int32_t>(n, 32u);
    const size_t m = s1 > s2 ? s1 : s2;
    return m > sc ? m : sc;
}

// workspace: key | sorted key | val | sorted val | parent | size | flag | excl | object key | sorted object key | sorted object
// val | rocPRIM temporaries
struct Layout {                  // byte offsets
    int64_t key, skey, val, sval, parent, size, flag, excl, okey, sokey, soval, bytes;
    explicit Layout(int64_t n) {
        Carver c;
        key = c.take(n * 8);
        skey = c.take(n * 8);
        val = c.take(n * 4);
        sval = c.take(n * 4);
        parent = c.take(n * 4);
        size = c.take(n * 4);
        flag = c.take((n + 1) * 4);
        excl = c.take((n + 1) * 4);
        okey = c.take(n * 4);
        sokey = c.take(n * 4);
        soval = c.take(n * 4);
        bytes = c.bytes;
    }
};

inline int64_t temp_room(int64_t n) { return room_next_pow2(n, temp_bytes); }

int64_t workspace_bytes(int64_t n) { return Layout(n).bytes + temp_room(n); }

}  // namespace

extern "C" int64_t hpl_motion_segment_workspace_bytes(int batch, int64_t n_total) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || n_total < 0 || n_total >= CLOUD_MAX_POINTS) return -1;
    return workspace_bytes(n_total);
}

extern "C" int hpl_motion_segment(const float *pc, int64_t pc_ld, const float *flow, int64_t flow_sc, int64_t flow_sp,
                                  const float *residual, int batch, const int64_t *prefix, float tau, float eps, float dv,
                                  int min_points, int max_objects, int32_t *labels, int32_t *obj_info, float *obj_motion,
                                  int32_t *stats, void *workspace, int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_motion_segment";
    HPL_REQUIRE(pc && flow && residual && prefix && labels && obj_info && obj_motion && stats && workspace,
                "hpl_motion_segment: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(tau > 0.f && isfinite(tau), "hpl_motion_segment: tau must be finite and > 0");
    HPL_REQUIRE(eps > 0.f && isfinite(eps), "hpl_motion_segment: eps must be finite and > 0");
    HPL_REQUIRE(dv > 0.f, "hpl_motion_segment: dv must be > 0 (+inf: no flow criterion)");
    HPL_REQUIRE(min_points >= 1, "hpl_motion_segment: min_points = %d (>= 1)", min_points);
    HPL_REQUIRE(max_objects >= 1 && max_objects <= MS_MAX_OBJECTS, "hpl_motion_segment: max_objects = %d (1 .. %d)", max_objects,
                MS_MAX_OBJECTS);
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix", "pair", prefix, batch));
    const int64_t N = prefix[batch];
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_CLOUD_CHECK(check_row_stride(op, pc_ld, N));
    HPL_CLOUD_CHECK(check_flow_strides(op, flow_sc, flow_sp, N));
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, workspace_bytes(N)));
    HPL_CLOUD_CHECK(check_aligned4(op, {pc, flow, residual, labels, obj_info, obj_motion, stats}));
    if (N == 0) return HPL_OK;

    const Layout L(N);
    void *const temp = carved<char>(workspace, L.bytes);
    SegArgs a{};
    a.pc = pc; a.pc_ld = pc_ld; a.flow = flow; a.fsc = flow_sc; a.fsp = flow_sp; a.residual = residual;
    a.tau = tau;
    a.eps2 = eps * eps;                          // rounded once to float32, as the predicate states
    a.dv2 = dv * dv;
    a.inv_cell = 1.0 / (GRID_CELL_MARGIN * (double)eps);
    a.n = (int32_t)N; a.batch = batch; a.min_points = min_points; a.max_objects = max_objects;
    a.key = carved<u64>(workspace, L.key); a.skey = carved<u64>(workspace, L.skey);
    a.val = carved<int32_t>(workspace, L.val); a.sval = carved<int32_t>(workspace, L.sval);
    a.parent = carved<int32_t>(workspace, L.parent); a.size = carved<int32_t>(workspace, L.size);
    a.flag = carved<int32_t>(workspace, L.flag); a.excl = carved<int32_t>(workspace, L.excl);
    a.okey = carved<uint32_t>(workspace, L.okey); a.sokey = carved<uint32_t>(workspace, L.sokey);
    a.soval = carved<int32_t>(workspace, L.soval);
    a.labels = labels; a.obj_info = obj_info; a.obj_motion = obj_motion; a.stats = stats;
    narrow_prefix(prefix, batch, MS_BLOCK, a.pprefix, nullptr);

    hipStream_t s = to_stream(stream);
    if (hipMemsetAsync(stats, 0, sizeof(int32_t) * 4 * (size_t)batch, s) != hipSuccess) {
        set_error("hpl_motion_segment: clearing the counts failed: %s", hipGetErrorString(hipGetLastError()));
        return HPL_EHIP;
    }
    const unsigned grid = (unsigned)cdiv(N, MS_BLOCK), grid1 = (unsigned)cdiv(N + 1, MS_BLOCK);
    k_seg_keys<<<grid, MS_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_motion_segment (keys)");
    size_t tb = (size_t)temp_room(N);
    hipError_t e = rocprim::radix_sort_pairs(temp, tb, (const u64 *)a.key, a.skey, (const int32_t *)a.val, a.sval, (size_t)N, 0u,
                                             64u, s);          // (the largest key, of the non-movers, has every bit set)
    if (e != hipSuccess) { set_error("hpl_motion_segment: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    k_seg_link<<<grid, MS_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_motion_segment (link)");
    k_seg_flatten<<<grid, MS_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_motion_segment (flatten)");
    k_seg_flag<<<grid1, MS_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_motion_segment (flag)");
    tb = (size_t)temp_room(N);
    e = rocprim::exclusive_scan(temp, tb, (const int32_t *)a.flag, a.excl, 0, (size_t)(N + 1), rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) { set_error("hpl_motion_segment: scan failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    k_seg_label<<<grid, MS_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_motion_segment (label)");
    tb = (size_t)temp_room(N);
    e = rocprim::radix_sort_pairs(temp, tb, (const uint32_t *)a.okey, a.sokey, (const int32_t *)a.val, a.soval, (size_t)N, 0u,
                                  (unsigned)count_bits(N), s);
    if (e != hipSuccess) { set_error("hpl_motion_segment: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    k_seg_objects<<<(unsigned)(batch * max_objects), MS_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_motion_segment (objects)");
    return HPL_OK;
}
