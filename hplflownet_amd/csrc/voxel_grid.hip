// voxel_grid.hip -- voxel-grid downsampling of a packed ragged batch of point clouds (hpl_voxel_downsample):
// one point per occupied cell of edge `voxel` -- the cell's centroid, or the member nearest to it --, with the attribute
// channels that ride along, the member count, the representative, every point's voxel and the per-cloud counts, without a
// host round trip or a floating-point atomic.
//
//   k_vx_keys     a lane per point: the float64 cell, the 64-bit key (cloud, cell x, y, z biased), an invalid point the
//                 largest key of its cloud; valid / non-finite / out-of-range counted (one integer atomic per workgroup and
//                 slot where the workgroup lies inside one cloud)
//   rocPRIM       stable radix sort of (key, index) over the bits in use: a cloud's points stay in its range, its voxels in
//                 ascending lexicographic cell order, the members of a voxel in ascending index, the invalid points last
//   k_vx_heads    a lane per sorted position: 1 on the first member of a run
//   rocPRIM       inclusive scan of the heads: a run's rank (the rank before the cloud's first position is subtracted)
//   k_vx_starts   a lane per sorted position: a head writes where its run starts, every point learns its voxel (voxel_of)
//   k_vx_reduce   a lane per packed output position: a voxel of at most VX_SHORT members is summed by its lane, a longer one
//                 by the whole wave -- 64 lanes load 64 members at once and the float64 additions are handed round in index
//                 order from scalar registers, so the documented order holds and a cloud that falls into one voxel costs the
//                 wave its additions, not its loads.  The nearest member, the outputs, and behind a cloud's voxels the tails
//
// The sizes of all launches are host numbers (N, batch); nothing is read back and no lane waits for another.  Every sum has
// one order and the voxel numbering is the cloud's own: a cloud's outputs are the same bits alone, anywhere in a batch and
// beside other work.
//
// The arithmetic is part of the interface (include/hpl_bcl.h; tests/voxel_oracle.py restates it in numpy).  The key, its
// limits, the counter and the room of the sort are grid_common.h's.
#include "grid_common.h"

#include <math.h>
#include <rocprim/device/device_scan.hpp>

using namespace hpl;

namespace {

constexpr int VX_MAX_CHANNELS = 8;
constexpr int VX_BLOCK = 256;
constexpr int VX_SHORT = 32;             // a longer run is summed by its wave together
constexpr u64 VX_CELLS_MASK = ((u64)1 << GRID_KEY_BITS) - 1;         // all ones: no cell (a biased cell is at most 2^19 - 2)

struct VxArgs {
    const float *pc;
    int64_t pc_ld;
    const float *attr;
    int64_t attr_ld;
    float *out_pc;
    int64_t out_ld;
    float *out_attr;
    int64_t oattr_ld;
    int32_t *count, *rep, *voxel_of, *stats;
    double inv, org[3];
    int32_t n, batch, channels, mode;
    u64 *key, *skey;
    int32_t *val, *sval;            // point indices: 0 .. n-1, and in key order
    int32_t *flag, *incl;           // per sorted position: the head of a run, and the heads up to and including it
    int32_t *start;                 // per packed voxel position: the sorted position of its first member
    int32_t pprefix[CLOUD_MAX_BATCH + 1];
};

__device__ __forceinline__ int cloud_of(const VxArgs &a, int i) { return group_of(a.pprefix, a.batch, i); }

__global__ void __launch_bounds__(VX_BLOCK) k_vx_keys(const VxArgs a) {
    const int64_t i0 = (int64_t)blockIdx.x * VX_BLOCK;
    const int64_t i64 = i0 + threadIdx.x;
    const bool in = i64 < a.n;
    const int i = in ? (int)i64 : a.n - 1;
    const int b = cloud_of(a, i);
    const bool uniform = cloud_of(a, (int)i0) == cloud_of(a, (int)imin(i0 + VX_BLOCK - 1, a.n - 1));
    bool valid = false, nonfinite = false, oob = false;
    if (in) {
        const float x = a.pc[i], y = a.pc[a.pc_ld + i], z = a.pc[2 * a.pc_ld + i];
        u64 key = ((u64)b << GRID_KEY_BITS) | VX_CELLS_MASK;
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            const double cx = floor(((double)x - a.org[0]) * a.inv), cy = floor(((double)y - a.org[1]) * a.inv),
                         cz = floor(((double)z - a.org[2]) * a.inv);
            valid = fabs(cx) <= GRID_CELL_MAX && fabs(cy) <= GRID_CELL_MAX && fabs(cz) <= GRID_CELL_MAX;
            oob = !valid;
            if (valid) key = grid_key(b, (int)cx + GRID_CELL_BIAS, (int)cy + GRID_CELL_BIAS, (int)cz + GRID_CELL_BIAS);
        } else {
            nonfinite = true;
        }
        a.key[i] = key;
        a.val[i] = i;
    }
    count_into(a.stats, uniform, b, 1, valid ? 1 : 0);
    count_into(a.stats, uniform, b, 2, nonfinite ? 1 : 0);
    count_into(a.stats, uniform, b, 3, oob ? 1 : 0);
}

__device__ __forceinline__ bool has_cell(u64 key) { return (key & VX_CELLS_MASK) != VX_CELLS_MASK; }

__global__ void __launch_bounds__(VX_BLOCK) k_vx_heads(const VxArgs a) {
    const int64_t s64 = (int64_t)blockIdx.x * VX_BLOCK + threadIdx.x;
    if (s64 >= a.n) return;
    const int s = (int)s64;
    const u64 key = a.skey[s];
    // (the cloud digit leads the key: a cloud's first position differs from the one before it anyway)
    a.flag[s] = (has_cell(key) && (s == 0 || a.skey[s - 1] != key)) ? 1 : 0;
}

// the heads before cloud b's range
__device__ __forceinline__ int rank_base(const VxArgs &a, int p0) { return p0 > 0 ? a.incl[p0 - 1] : 0; }

__global__ void __launch_bounds__(VX_BLOCK) k_vx_starts(const VxArgs a) {
    const int64_t s64 = (int64_t)blockIdx.x * VX_BLOCK + threadIdx.x;
    if (s64 >= a.n) return;
    const int s = (int)s64;
    const int p0 = a.pprefix[cloud_of(a, s)];
    const bool valid = has_cell(a.skey[s]);
    const int at = p0 + (a.incl[s] - 1 - rank_base(a, p0));
    if (a.flag[s]) a.start[at] = s;
    if (a.voxel_of) a.voxel_of[a.sval[s]] = valid ? at : -1;
}

__device__ __forceinline__ float d2_of(const float (&p)[3], const float (&c)[3]) {
    const float dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// what a voxel's coordinates leave behind once its sums and its representative are known
__device__ __forceinline__ void write_voxel(const VxArgs &a, int at, int len, const float (&c)[3], int rep) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.out_pc[k * a.out_ld + at] = a.mode ? a.pc[k * a.pc_ld + rep] : c[k];
    if (a.count) a.count[at] = len;
    if (a.rep) a.rep[at] = rep;
}

// value of lane l (a constant) of the wave, from a scalar register
__device__ __forceinline__ float lane_value(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// s[r] = the float64 sum of rows[r][sval[lo + e]], e = 0 .. len-1 in that order, from 0, by the whole wave: 64 members are
// loaded at once (the next 64 while these are added) and added one after the other.  A lane past the end holds +0.0, which a
// sum that started from +0.0 does not notice (it is never -0.0).  Every lane ends with the same s.
template <int R>
__device__ __forceinline__ void wave_ordered_sum(const int32_t *sval, int lo, int len, const float *const (&rows)[R], int lane,
                                                 double (&s)[R]) {
    float next[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { s[r] = 0.0; next[r] = 0.f; }
    if (lane < len) {
        const int i = sval[lo + lane];
#pragma unroll
        for (int r = 0; r < R; ++r) next[r] = rows[r][i];
    }
    for (int c0 = 0; c0 < len; c0 += 64) {
        float cur[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { cur[r] = next[r]; next[r] = 0.f; }
        if (c0 + 64 + lane < len) {
            const int i = sval[lo + c0 + 64 + lane];
#pragma unroll
            for (int r = 0; r < R; ++r) next[r] = rows[r][i];
        }
#pragma unroll
        for (int l = 0; l < 64; ++l) {
#pragma unroll
            for (int r = 0; r < R; ++r) s[r] = s[r] + (double)lane_value(cur[r], l);
        }
    }
}

__global__ void __launch_bounds__(VX_BLOCK) k_vx_reduce(const VxArgs a) {
    const int64_t j64 = (int64_t)blockIdx.x * VX_BLOCK + threadIdx.x;
    const bool in = j64 < a.n;
    const int j = in ? (int)j64 : a.n - 1;
    const int lane = (int)(threadIdx.x & 63);
    const int b = cloud_of(a, j);
    const int p0 = a.pprefix[b], p1 = a.pprefix[b + 1];
    const int V = a.incl[p1 - 1] - rank_base(a, p0);            // (the cloud of a position is not empty)
    const int v = j - p0;
    int lo = 0, len = 0;
    if (in && v < V) {
        lo = a.start[j];
        len = (v + 1 < V ? a.start[j + 1] : p0 + a.stats[b * 4 + 1]) - lo;     // (the valid points lead the cloud's range)
    }
    if (in && v == 0) a.stats[b * 4] = V;
    if (in && v >= V) {                          // the tail behind the cloud's voxels
#pragma unroll
        for (int k = 0; k < 3; ++k) a.out_pc[k * a.out_ld + j] = 0.f;
        if (a.out_attr)
            for (int c = 0; c < a.channels; ++c) a.out_attr[c * a.oattr_ld + j] = 0.f;
        if (a.count) a.count[j] = 0;
        if (a.rep) a.rep[j] = -1;
    }
    if (len > 0 && len <= VX_SHORT) {            // the lane alone
        double s[3] = {0.0, 0.0, 0.0};
        for (int e = 0; e < len; ++e) {
            const int i = a.sval[lo + e];
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = s[k] + (double)a.pc[k * a.pc_ld + i];
        }
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (float)(s[k] / (double)len);
        int rep = a.sval[lo];
        float best = 0.f;
        for (int e = 0; e < len; ++e) {
            const int i = a.sval[lo + e];
            const float p[3] = {a.pc[i], a.pc[a.pc_ld + i], a.pc[2 * a.pc_ld + i]};
            const float d2 = d2_of(p, c);
            if (e == 0 || d2 < best) { best = d2; rep = i; }
        }
        write_voxel(a, j, len, c, rep);
        if (a.out_attr) {
            for (int ch = 0; ch < a.channels; ++ch) {
                const float *row = a.attr + ch * a.attr_ld;
                float o;
                if (a.mode) {
                    o = row[rep];
                } else {
                    double t = 0.0;
                    for (int e = 0; e < len; ++e) t = t + (double)row[a.sval[lo + e]];
                    o = (float)(t / (double)len);
                }
                a.out_attr[ch * a.oattr_ld + j] = o;
            }
        }
    }
    u64 todo = __ballot(len > VX_SHORT);
    while (todo) {                               // the whole wave, one long run after the other
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int lo_b = __shfl(lo, src), len_b = __shfl(len, src), at = __shfl(j, src);
        const float *const rows[3] = {a.pc, a.pc + a.pc_ld, a.pc + 2 * a.pc_ld};
        double s[3];
        wave_ordered_sum<3>(a.sval, lo_b, len_b, rows, lane, s);
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (float)(s[k] / (double)len_b);
        // the first member of the smallest d2: lane l looks at members l, l + 64, ..., then the lanes' (d2, place) meet
        float best = 0.f;
        int place = 0x7fffffff;
        for (int e = lane; e < len_b; e += 64) {
            const int i = a.sval[lo_b + e];
            const float p[3] = {a.pc[i], a.pc[a.pc_ld + i], a.pc[2 * a.pc_ld + i]};
            const float d2 = d2_of(p, c);
            if (place == 0x7fffffff || d2 < best) { best = d2; place = e; }
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const float ob = __shfl_xor(best, m);
            const int op = __shfl_xor(place, m);
            if (op != 0x7fffffff && (place == 0x7fffffff || ob < best || (ob == best && op < place))) { best = ob; place = op; }
        }
        const int rep = a.sval[lo_b + place];
        if (lane == 0) write_voxel(a, at, len_b, c, rep);
        if (a.out_attr) {
            for (int ch = 0; ch < a.channels; ++ch) {
                const float *const row[1] = {a.attr + ch * a.attr_ld};
                float o;
                if (a.mode) {
                    o = row[0][rep];
                } else {
                    double t[1];
                    wave_ordered_sum<1>(a.sval, lo_b, len_b, row, lane, t);
                    o = (float)(t[0] / (double)len_b);
                }
                if (lane == 0) a.out_attr[ch * a.oattr_ld + at] = o;
            }
        }
    }
}

int sort_bits(int batch) { return GRID_KEY_BITS + count_bits(batch - 1); }

// the sort and the scan share the room: enough for either
size_t temp_bytes(int64_t n) {
    size_t sc = 0;
    (void)rocprim::inclusive_scan(nullptr, sc, (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)n, rocprim::plus<int32_t>(),
                                  (hipStream_t) nullptr);
    const size_t ss = radix_temp_bytes<u64, int32_t>(n, 64u);
    return ss > sc ? ss : sc;
}

inline int64_t temp_room(int64_t n) { return room_all_pow2(n, temp_bytes); }

// workspace: key | sorted key | val | sorted val | heads | their inclusive sums | run starts | rocPRIM temporaries
struct Layout {                  // byte offsets
    int64_t key, skey, val, sval, flag, incl, start, bytes;
    explicit Layout(int64_t n) {
        Carver c;
        key = c.take(n * 8);
        skey = c.take(n * 8);
        val = c.take(n * 4);
        sval = c.take(n * 4);
        flag = c.take(n * 4);
        incl = c.take(n * 4);
        start = c.take(n * 4);
        bytes = c.bytes;
    }
};

int64_t workspace_bytes(int64_t n) { return Layout(n).bytes + temp_room(n); }

inline bool overlaps(const void *p, int64_t pn, const void *q, int64_t qn) {      // element counts of 4 bytes each
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && pn > 0 && qn > 0 && a < b + 4u * (uintptr_t)qn && b < a + 4u * (uintptr_t)pn;
}

inline int64_t extent(int rows, int64_t ld, int64_t n) { return rows > 0 && n > 0 ? (rows - 1) * ld + n : 0; }

}  // namespace

extern "C" int64_t hpl_voxel_downsample_workspace_bytes(int batch, int64_t n_total, int channels) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || channels < 0 || channels > VX_MAX_CHANNELS || n_total < 0 ||
        n_total >= CLOUD_MAX_POINTS)
        return -1;
    return workspace_bytes(n_total);
}

extern "C" int hpl_voxel_downsample(const float *pc, int64_t pc_ld, const float *attr, int64_t attr_ld, int channels, int batch,
                                    const int64_t *prefix, float voxel, const float *origin, int mode, float *out_pc,
                                    int64_t out_ld, float *out_attr, int64_t out_attr_ld, int32_t *count, int32_t *rep,
                                    int32_t *voxel_of, int32_t *stats, void *workspace, int64_t workspace_bytes_,
                                    hplStream stream) {
    const char *const op = "hpl_voxel_downsample";
    HPL_REQUIRE(pc && prefix && origin && out_pc && stats && workspace, "hpl_voxel_downsample: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(channels >= 0 && channels <= VX_MAX_CHANNELS, "hpl_voxel_downsample: channels = %d (0 .. %d)", channels,
                VX_MAX_CHANNELS);
    HPL_REQUIRE(attr || channels == 0, "hpl_voxel_downsample: null pointer (attr of %d channels)", channels);
    HPL_REQUIRE(mode == 0 || mode == 1, "hpl_voxel_downsample: mode = %d (0 centroid, 1 nearest)", mode);
    HPL_REQUIRE(voxel > 0.f && isfinite(voxel), "hpl_voxel_downsample: voxel must be finite and > 0");
    HPL_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), "hpl_voxel_downsample: origin must be finite");
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix", "cloud", prefix, batch));
    const int64_t N = prefix[batch];
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_CLOUD_CHECK(check_row_stride(op, pc_ld, N));
    HPL_CLOUD_CHECK(check_row_stride(op, out_ld, N));
    if (channels > 0) {
        HPL_CLOUD_CHECK(check_row_stride(op, attr_ld, N));
        if (out_attr) HPL_CLOUD_CHECK(check_row_stride(op, out_attr_ld, N));
    }
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, workspace_bytes(N)));
    HPL_CLOUD_CHECK(check_aligned4(op, {pc, attr, out_pc, out_attr, count, rep, voxel_of, stats}));
    {
        const int ach = channels > 0 ? channels : 0;
        const void *const ins[2] = {pc, ach ? attr : nullptr};
        const int64_t in_n[2] = {extent(3, pc_ld, N), extent(ach, attr_ld, N)};
        const void *const outs[6] = {out_pc, ach ? out_attr : nullptr, count, rep, voxel_of, stats};
        const int64_t out_n[6] = {extent(3, out_ld, N), extent(ach, out_attr_ld, N), N, N, N, 4 * (int64_t)batch};
        for (int o = 0; o < 6; ++o)
            for (int i = 0; i < 2; ++i)
                HPL_REQUIRE(!overlaps(outs[o], out_n[o], ins[i], in_n[i]), "hpl_voxel_downsample: an output overlaps an input");
    }
    if (N == 0) return HPL_OK;

    const Layout L(N);
    void *const temp = carved<char>(workspace, L.bytes);
    VxArgs a{};
    a.pc = pc; a.pc_ld = pc_ld; a.attr = attr; a.attr_ld = attr_ld;
    a.out_pc = out_pc; a.out_ld = out_ld; a.out_attr = channels > 0 ? out_attr : nullptr; a.oattr_ld = out_attr_ld;
    a.count = count; a.rep = rep; a.voxel_of = voxel_of; a.stats = stats;
    a.inv = 1.0 / (double)voxel;
    for (int k = 0; k < 3; ++k) a.org[k] = (double)origin[k];
    a.n = (int32_t)N; a.batch = batch; a.channels = channels; a.mode = mode;
    a.key = carved<u64>(workspace, L.key); a.skey = carved<u64>(workspace, L.skey);
    a.val = carved<int32_t>(workspace, L.val); a.sval = carved<int32_t>(workspace, L.sval);
    a.flag = carved<int32_t>(workspace, L.flag); a.incl = carved<int32_t>(workspace, L.incl);
    a.start = carved<int32_t>(workspace, L.start);
    narrow_prefix(prefix, batch, VX_BLOCK, a.pprefix, nullptr);

    hipStream_t s = to_stream(stream);
    if (hipMemsetAsync(stats, 0, sizeof(int32_t) * 4 * (size_t)batch, s) != hipSuccess) {
        set_error("hpl_voxel_downsample: clearing the counts failed: %s", hipGetErrorString(hipGetLastError()));
        return HPL_EHIP;
    }
    const unsigned grid = (unsigned)cdiv(N, VX_BLOCK);
    k_vx_keys<<<grid, VX_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_voxel_downsample (keys)");
    size_t tb = (size_t)temp_room(N);
    hipError_t e = rocprim::radix_sort_pairs(temp, tb, (const u64 *)a.key, a.skey, (const int32_t *)a.val, a.sval, (size_t)N, 0u,
                                             (unsigned)sort_bits(batch), s);
    if (e != hipSuccess) { set_error("hpl_voxel_downsample: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    k_vx_heads<<<grid, VX_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_voxel_downsample (heads)");
    tb = (size_t)temp_room(N);
    e = rocprim::inclusive_scan(temp, tb, (const int32_t *)a.flag, a.incl, (size_t)N, rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) { set_error("hpl_voxel_downsample: scan failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    k_vx_starts<<<grid, VX_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_voxel_downsample (starts)");
    k_vx_reduce<<<grid, VX_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_voxel_downsample (reduce)");
    return HPL_OK;
}
