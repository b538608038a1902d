// fps.hip -- farthest point sampling of a packed ragged batch of point clouds (hpl_fps): exactly m points per
// cloud (fewer only when the cloud runs out of distinct positions), in selection order, with the attribute channels that ride
// along, every sample's distance at the moment it was chosen, every point's final distance to its nearest sample and the
// per-cloud counts, without a host round trip or a floating-point atomic.
//
// Two paths give the same bits:
//
//   resident   k_fps_resident: one workgroup per cloud, all m rounds in ONE launch.  The cloud's coordinates and its D live in
//              registers: lane t owns the points t, t + BLOCK, ... (FPS_PPL of them, a compile-time count, every index static,
//              so nothing goes to scratch or LDS).  A round updates the owned points, takes the lane's largest key, reduces
//              the wave's 64 lanes by shuffles and the waves through one LDS line per wave -- the winner's coordinates travel
//              with its key --, double-buffered by the round's parity, so a round has ONE barrier.  Every lane reads the same
//              line, so the stop decision is the same in every lane and every barrier is reached by the whole workgroup.
//   rounds     k_fps_round: one launch per round over all clouds' points plus one closing launch, D in the workspace.  Launch
//              r's prologue folds the candidate keys that the cloud's workgroups stored in launch r - 1 (every workgroup folds
//              all of them, in one pass: a cloud has at most FPS_RBLOCK workgroups) -- that is sample r - 1 --, workgroup 0 of
//              the cloud writes the sample's outputs, and every workgroup updates its slice and stores its own candidate into
//              the other half of the candidate buffer.  No workgroup waits for another inside a launch: stream order is the
//              only synchronisation.  A cloud that has stopped stores zero candidates and returns.
//
// k_fps_fill clears the outputs first (idx -1, the rest 0, the path).  The sizes of all launches are host numbers (the
// prefix, m); nothing is read back.
//
// The arithmetic is part of the interface (include/hpl_bcl.h; tests/fps_oracle.py restates it in numpy).
#include "cloud_common.h"

#include <math.h>

using namespace hpl;

// The resident workgroup's shape, measured (profiles/fps_bench.txt): 512 x 32 runs a round in 2.33 us, 256 x 48 in 2.51,
// 1024 x 12 in 2.89; 1024 x 16 and 256 x 64 spill.  A build with another shape is for measuring it.
#ifndef HPL_FPS_BLOCK
#define HPL_FPS_BLOCK 512        // lanes of the resident workgroup
#endif
#ifndef HPL_FPS_PPL
#define HPL_FPS_PPL 32           // points a lane owns: 4 registers each
#endif

namespace {

constexpr int FPS_MAX_CHANNELS = 8;
constexpr int FPS_BLOCK = HPL_FPS_BLOCK;
constexpr int FPS_PPL = HPL_FPS_PPL;
constexpr int FPS_CAPACITY = FPS_BLOCK * FPS_PPL;
constexpr int FPS_WAVES = FPS_BLOCK / 64;
constexpr int FPS_RBLOCK = 256;          // lanes of a workgroup of the rounds path, and the most workgroups a cloud may have
constexpr int FPS_RMIN = 4;              // points per lane of the rounds path, at least
constexpr int FPS_FILL = 256;
static_assert(FPS_BLOCK % 64 == 0 && FPS_BLOCK >= 64 && FPS_BLOCK <= 1024 && FPS_PPL >= 1, "resident shape");

typedef unsigned long long u64;

struct FpsArgs {
    const float *pc;
    int64_t pc_ld;
    const float *attr;
    int64_t attr_ld;
    float *out_pc;
    int64_t out_ld;
    float *out_attr;
    int64_t oattr_ld;
    int32_t *idx;
    float *dist, *cover;
    int32_t *stats;
    float *D;                       // rounds: (N) the running distance, -1 a point that is not finite
    u64 *cand;                      // rounds: [2][slots] the workgroups' candidate keys by launch parity
    int32_t slots;
    int32_t batch, channels, m, path, ipl;      // ipl: rounds, the points per lane
    int32_t pprefix[CLOUD_MAX_BATCH + 1];
    int32_t bprefix[CLOUD_MAX_BATCH + 1];       // rounds: the first workgroup of every cloud
    int32_t start[CLOUD_MAX_BATCH];             // -1: none
};

// the key of a valid point of distance d >= +0 and cloud-local index i: larger d first, then the smaller index; 0 is no point
__device__ __forceinline__ u64 key_of(float d, int i) { return ((u64)__float_as_uint(d) << 32) | (u64)(0xFFFFFFFFu - (unsigned)i); }
__device__ __forceinline__ float key_dist(u64 k) { return __uint_as_float((unsigned)(k >> 32)); }
__device__ __forceinline__ int key_index(u64 k) { return (int)(0xFFFFFFFFu - (unsigned)k); }

__device__ __forceinline__ float d2_of(float x, float y, float z, float sx, float sy, float sz) {
    const float dx = x - sx, dy = y - sy, dz = z - sz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ u64 wave_max(u64 k) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const u64 o = __shfl_xor(k, s);
        k = o > k ? o : k;
    }
    return k;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the cloud's start: its index and coordinates when it is given and its point is finite, else index -1
struct Start {
    int i;
    float x, y, z;
};

__device__ __forceinline__ Start start_of(const FpsArgs &a, int b, int p0) {
    const int st = a.start[b], at = p0 + (st < 0 ? 0 : st);      // (a cloud that gets here is not empty)
    Start s{st, a.pc[at], a.pc[a.pc_ld + at], a.pc[2 * a.pc_ld + at]};
    if (!finite3(s.x, s.y, s.z)) s.i = -1;
    return s;
}

__global__ void __launch_bounds__(FPS_FILL) k_fps_fill(const FpsArgs a) {
    const int64_t total = (int64_t)a.batch * a.m;
    const int64_t j = (int64_t)blockIdx.x * FPS_FILL + threadIdx.x;
    if (j < a.batch) {
        a.stats[j * 4 + 0] = 0;
        a.stats[j * 4 + 1] = 0;
        a.stats[j * 4 + 2] = 0;
        a.stats[j * 4 + 3] = a.path;
    }
    if (j >= total) return;
    a.idx[j] = -1;
    a.dist[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.out_pc[k * a.out_ld + j] = 0.f;
    if (a.out_attr)
        for (int c = 0; c < a.channels; ++c) a.out_attr[c * a.oattr_ld + j] = 0.f;
}

// what sample j of cloud b leaves behind besides idx and dist: lane l < 3 + channels writes one row
__device__ __forceinline__ void gather_sample(const FpsArgs &a, int64_t col, int64_t src, int l) {
    if (l < 3) a.out_pc[l * a.out_ld + col] = a.pc[l * a.pc_ld + src];
    else if (a.out_attr && l < 3 + a.channels) a.out_attr[(l - 3) * a.oattr_ld + col] = a.attr[(l - 3) * a.attr_ld + src];
}

// ---------------------------------------------------------------------------------------------- the resident path
struct __align__(16) Line {              // a wave's candidate: its key and the point's coordinates
    u64 key;
    float x, y, z;
    int pad[3];
};

// One pass over the lane's points: with UPDATE, D <- min(D, d2 to s) first; then the lane's largest D (the first of equals: the
// owned indices ascend with k) as a key, and that point's coordinates.  (Skipping the rows past the cloud's end behind a
// uniform branch was measured slower from 8 192 points on: DESIGN.md §30.)
template <bool UPDATE>
__device__ __forceinline__ u64 scan_owned(const float (&x)[FPS_PPL], const float (&y)[FPS_PPL], const float (&z)[FPS_PPL],
                                          float (&D)[FPS_PPL], float sx, float sy, float sz, int t, float &cx, float &cy, float &cz) {
    float best = -1.f;
    int bk = 0;
#pragma unroll
    for (int k = 0; k < FPS_PPL; ++k) {
        if (UPDATE) D[k] = fminf(D[k], d2_of(x[k], y[k], z[k], sx, sy, sz));      // (a point that is not finite stays at -1)
        const bool up = D[k] > best;
        best = up ? D[k] : best;
        bk = up ? k : bk;
    }
    cx = x[0]; cy = y[0]; cz = z[0];
#pragma unroll
    for (int k = 1; k < FPS_PPL; ++k) {
        const bool is = bk == k;
        cx = is ? x[k] : cx;
        cy = is ? y[k] : cy;
        cz = is ? z[k] : cz;
    }
    return best >= 0.f ? key_of(best, bk * FPS_BLOCK + t) : 0;
}

__global__ void __launch_bounds__(FPS_BLOCK) k_fps_resident(const FpsArgs a) {
    __shared__ Line line[2][FPS_WAVES];
    __shared__ int wvalid[FPS_WAVES];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int p0 = a.pprefix[b], n = a.pprefix[b + 1] - p0;
    if (n == 0) return;                          // (the whole workgroup)
    float x[FPS_PPL], y[FPS_PPL], z[FPS_PPL], D[FPS_PPL];
    int nvalid = 0;
#pragma unroll
    for (int k = 0; k < FPS_PPL; ++k) {
        const int i = k * FPS_BLOCK + t;
        float px = NAN, py = NAN, pz = NAN;
        if (i < n) { px = a.pc[p0 + i]; py = a.pc[a.pc_ld + p0 + i]; pz = a.pc[2 * a.pc_ld + p0 + i]; }
        const bool ok = finite3(px, py, pz);
        x[k] = ok ? px : 0.f;
        y[k] = ok ? py : 0.f;
        z[k] = ok ? pz : 0.f;
        D[k] = ok ? INFINITY : -1.f;
        nvalid += ok ? 1 : 0;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) nvalid += __shfl_xor(nvalid, s);
    if (lane == 0) wvalid[wave] = nvalid;        // (read behind the first round's barrier)
    const Start st = start_of(a, b, p0);

    float sx = 0.f, sy = 0.f, sz = 0.f;          // the sample whose distances D does not hold yet
    bool pending = false;
    int count = 0;
    for (int j = 0; j < a.m; ++j) {
        float cx, cy, cz;
        const u64 key = j == 0 ? scan_owned<false>(x, y, z, D, 0.f, 0.f, 0.f, t, cx, cy, cz)
                               : scan_owned<true>(x, y, z, D, sx, sy, sz, t, cx, cy, cz);
        pending = false;
        const u64 top = wave_max(key);
        if (top ? key == top : lane == 0) {      // (non-zero keys differ in their index: one lane)
            Line &w = line[j & 1][wave];
            w.key = top; w.x = cx; w.y = cy; w.z = cz;
        }
        __syncthreads();
        u64 g = 0;
        int gw = 0;
#pragma unroll
        for (int w = 0; w < FPS_WAVES; ++w) {
            const u64 k = line[j & 1][w].key;
            const bool up = k > g;
            g = up ? k : g;
            gw = up ? w : gw;
        }
        if (g == 0) break;                       // no finite point (j == 0)
        float gd = key_dist(g);
        int gi = key_index(g);
        if (j > 0 && gd == 0.f) break;           // every remaining point coincides with a sample
        sx = line[j & 1][gw].x; sy = line[j & 1][gw].y; sz = line[j & 1][gw].z;
        if (j == 0 && st.i >= 0) { gi = st.i; sx = st.x; sy = st.y; sz = st.z; }
        if (t == 0) {
            a.idx[(int64_t)b * a.m + j] = gi;
            a.dist[(int64_t)b * a.m + j] = gd;
        }
        pending = true;
        count = j + 1;
    }
    if (a.cover) {
#pragma unroll
        for (int k = 0; k < FPS_PPL; ++k) {
            const int i = k * FPS_BLOCK + t;
            float d = D[k];
            if (pending) d = fminf(d, d2_of(x[k], y[k], z[k], sx, sy, sz));
            if (i < n) a.cover[p0 + i] = d < 0.f ? 0.f : d;
        }
    }
    if (t == 0) {
        int valid = 0;
        for (int w = 0; w < FPS_WAVES; ++w) valid += wvalid[w];
        a.stats[b * 4 + 0] = count;
        a.stats[b * 4 + 1] = valid;
        a.stats[b * 4 + 2] = n - valid;
    }
    __syncthreads();                             // this workgroup's idx, written by lane 0, is read back by the others
    const int rows = 3 + (a.out_attr ? a.channels : 0);
    for (int e = t; e < count * rows; e += FPS_BLOCK) {
        const int j = e / rows, l = e - j * rows;
        gather_sample(a, (int64_t)b * a.m + j, (int64_t)p0 + a.idx[(int64_t)b * a.m + j], l);
    }
}

// ---------------------------------------------------------------------------------------------- the rounds path
// the workgroup's largest key, in every lane
__device__ __forceinline__ u64 block_max(u64 k, u64 (&red)[FPS_RBLOCK / 64], int t) {
    k = wave_max(k);
    __syncthreads();                             // (red may still be read from the call before)
    if ((t & 63) == 0) red[t >> 6] = k;
    __syncthreads();
    u64 g = red[0];
#pragma unroll
    for (int w = 1; w < FPS_RBLOCK / 64; ++w) g = red[w] > g ? red[w] : g;
    return g;
}

// Launch r = 0 .. m of the rounds path (r == m closes).  A workgroup lies inside one cloud.
__global__ void __launch_bounds__(FPS_RBLOCK) k_fps_round(const FpsArgs a, const int r) {
    __shared__ u64 red[FPS_RBLOCK / 64];
    const int t = threadIdx.x, wg = blockIdx.x;
    const int b = group_of(a.bprefix, a.batch, wg);
    const int w = wg - a.bprefix[b], nw = a.bprefix[b + 1] - a.bprefix[b];
    const int p0 = a.pprefix[b], n = a.pprefix[b + 1] - p0;
    const int span = a.ipl * FPS_RBLOCK;
    const int lo = w * span, hi = (int)imin((int64_t)lo + span, n);       // the slice, cloud-local
    const bool last = r == a.m;
    u64 *const mine = a.cand + (int64_t)(r & 1) * a.slots + wg;

    if (r == 0) {                                // D and the first candidates: the smallest finite index has the largest key
        float best = -1.f;
        int bi = 0, nvalid = 0;
        for (int i = lo + t; i < hi; i += FPS_RBLOCK) {
            const bool ok = finite3(a.pc[p0 + i], a.pc[a.pc_ld + p0 + i], a.pc[2 * a.pc_ld + p0 + i]);
            a.D[p0 + i] = ok ? INFINITY : -1.f;
            nvalid += ok ? 1 : 0;
            if (ok && best < 0.f) { best = INFINITY; bi = i; }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) nvalid += __shfl_xor(nvalid, s);
        if ((t & 63) == 0 && nvalid) atomicAdd(&a.stats[b * 4 + 1], nvalid);      // (integers: any order, the same sum)
        const u64 g = block_max(best >= 0.f ? key_of(best, bi) : 0, red, t);
        if (t == 0) *mine = g;
        return;
    }

    // sample r - 1: the largest of the candidates of launch r - 1, folded by every workgroup of the cloud in the same order
    const u64 g = block_max(t < nw ? a.cand[(int64_t)((r - 1) & 1) * a.slots + a.bprefix[b] + t] : 0, red, t);
    float gd = key_dist(g);
    int gi = key_index(g);
    const bool stopped = g == 0 || (r >= 2 && gd == 0.f);
    if (w == 0 && t == 0) {
        if (r == 1) a.stats[b * 4 + 2] = n - a.stats[b * 4 + 1];                 // (launch 0 has finished counting)
        if (stopped && g != 0) a.stats[b * 4 + 0] = r - 1;       // (g == 0: stopped in an earlier launch, or nothing is finite)
    }
    if (stopped && !last) {
        if (t == 0) *mine = 0;
        return;
    }
    float s[3] = {0.f, 0.f, 0.f};
    if (!stopped) {
        if (r == 1) {
            const Start st = start_of(a, b, p0);
            if (st.i >= 0) gi = st.i;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = a.pc[k * a.pc_ld + p0 + gi];
        if (w == 0) {
            const int64_t col = (int64_t)b * a.m + (r - 1);
            if (t == 0) {
                a.idx[col] = gi;
                a.dist[col] = gd;
                if (last) a.stats[b * 4 + 0] = a.m;
            }
            gather_sample(a, col, (int64_t)p0 + gi, t);
        }
    }
    float best = -1.f;
    int bi = 0;
    for (int i = lo + t; i < hi; i += FPS_RBLOCK) {
        float d = a.D[p0 + i];
        if (!stopped && d >= 0.f) {
            d = fminf(d, d2_of(a.pc[p0 + i], a.pc[a.pc_ld + p0 + i], a.pc[2 * a.pc_ld + p0 + i], s[0], s[1], s[2]));
            if (!last) a.D[p0 + i] = d;
        }
        if (last && a.cover) a.cover[p0 + i] = d < 0.f ? 0.f : d;
        if (d > best) { best = d; bi = i; }      // (the lane's indices ascend: the first of equals stays)
    }
    if (last) return;
    const u64 c = block_max(best >= 0.f ? key_of(best, bi) : 0, red, t);
    if (t == 0) *mine = c;
}

// workspace of the rounds path: D | the candidate keys of both parities
struct Layout {                  // byte offsets
    int64_t D, cand, slots, bytes;
    explicit Layout(int64_t n, int batch) {
        Carver c;
        slots = cdiv(n, FPS_RMIN * FPS_RBLOCK) + batch;       // a cloud's last workgroup may be partial
        D = c.take(n * 4);
        cand = c.take(2 * slots * 8);
        bytes = c.bytes;
    }
};

inline bool overlaps(const void *p, int64_t pn, const void *q, int64_t qn) {      // element counts of 4 bytes each
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && pn > 0 && qn > 0 && a < b + 4u * (uintptr_t)qn && b < a + 4u * (uintptr_t)pn;
}

inline int64_t extent(int rows, int64_t ld, int64_t n) { return rows > 0 && n > 0 ? (rows - 1) * ld + n : 0; }

inline bool in_limits(int batch, int64_t n, int64_t m, int channels) {
    return batch >= 1 && batch <= CLOUD_MAX_BATCH && channels >= 0 && channels <= FPS_MAX_CHANNELS && n >= 0 && n < CLOUD_MAX_POINTS &&
           m >= 1 && m < CLOUD_MAX_POINTS && (int64_t)batch * m < CLOUD_MAX_POINTS;
}

}  // namespace

extern "C" int hpl_fps_resident_capacity(void) { return FPS_CAPACITY; }

extern "C" int64_t hpl_fps_workspace_bytes(int batch, int64_t n_total, int64_t m, int channels) {
    if (!in_limits(batch, n_total, m, channels)) return -1;
    return Layout(n_total, batch).bytes;
}

extern "C" int hpl_fps(const float *pc, int64_t pc_ld, const float *attr, int64_t attr_ld, int channels, int batch,
                       const int64_t *prefix, const int32_t *start, int64_t m, int path, int32_t *idx, float *dist, float *out_pc,
                       int64_t out_ld, float *out_attr, int64_t out_attr_ld, float *cover, int32_t *stats, void *workspace,
                       int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_fps";
    HPL_REQUIRE(pc && prefix && idx && dist && out_pc && stats && workspace, "hpl_fps: null pointer");
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(channels >= 0 && channels <= FPS_MAX_CHANNELS, "hpl_fps: channels = %d (0 .. %d)", channels, FPS_MAX_CHANNELS);
    HPL_REQUIRE(attr || channels == 0, "hpl_fps: null pointer (attr of %d channels)", channels);
    HPL_REQUIRE(path >= 0 && path <= 2, "hpl_fps: path = %d (0 auto, 1 resident, 2 rounds)", path);
    HPL_REQUIRE(m >= 1 && m < CLOUD_MAX_POINTS && (int64_t)batch * m < CLOUD_MAX_POINTS,
                "hpl_fps: m = %lld samples for each of %d clouds (m >= 1, batch * m < 2^31 / 3)", (long long)m, batch);
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix", "cloud", prefix, batch));
    const int64_t N = prefix[batch], M = (int64_t)batch * m;
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_CLOUD_CHECK(check_row_stride(op, pc_ld, N));
    HPL_CLOUD_CHECK(check_row_stride(op, out_ld, M));
    if (channels > 0) {
        HPL_CLOUD_CHECK(check_row_stride(op, attr_ld, N));
        if (out_attr) HPL_CLOUD_CHECK(check_row_stride(op, out_attr_ld, M));
    }
    int64_t largest = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t nb = prefix[b + 1] - prefix[b];
        largest = imax(largest, nb);
        if (start && nb > 0)
            HPL_REQUIRE(start[b] >= 0 && start[b] < nb, "hpl_fps: start %d of cloud %d outside its %lld points", (int)start[b], b,
                        (long long)nb);
    }
    if (path == HPL_FPS_RESIDENT)
        HPL_REQUIRE(largest <= FPS_CAPACITY, "hpl_fps: a cloud of %lld points passes the resident path's %d", (long long)largest,
                    FPS_CAPACITY);
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, Layout(N, batch).bytes));
    HPL_CLOUD_CHECK(check_aligned4(op, {pc, attr, idx, dist, out_pc, out_attr, cover, stats}));
    {
        const int ach = channels > 0 ? channels : 0;
        const void *const ins[2] = {pc, ach ? attr : nullptr};
        const int64_t in_n[2] = {extent(3, pc_ld, N), extent(ach, attr_ld, N)};
        const void *const outs[6] = {out_pc, ach ? out_attr : nullptr, idx, dist, cover, stats};
        const int64_t out_n[6] = {extent(3, out_ld, M), extent(ach, out_attr_ld, M), M, M, N, 4 * (int64_t)batch};
        for (int o = 0; o < 6; ++o)
            for (int i = 0; i < 2; ++i) HPL_REQUIRE(!overlaps(outs[o], out_n[o], ins[i], in_n[i]), "hpl_fps: an output overlaps an input");
    }
    if (N == 0) return HPL_OK;

    const Layout L(N, batch);
    FpsArgs a{};
    a.pc = pc; a.pc_ld = pc_ld; a.attr = attr; a.attr_ld = attr_ld;
    a.out_pc = out_pc; a.out_ld = out_ld; a.out_attr = channels > 0 ? out_attr : nullptr; a.oattr_ld = out_attr_ld;
    a.idx = idx; a.dist = dist; a.cover = cover; a.stats = stats;
    a.D = carved<float>(workspace, L.D); a.cand = carved<u64>(workspace, L.cand); a.slots = (int32_t)L.slots;
    a.batch = batch; a.channels = channels; a.m = (int32_t)m;
    a.path = path != HPL_FPS_AUTO ? path : largest <= FPS_CAPACITY ? HPL_FPS_RESIDENT : HPL_FPS_ROUNDS;
    a.ipl = (int32_t)imax(FPS_RMIN, cdiv(largest, (int64_t)FPS_RBLOCK * FPS_RBLOCK));     // at most FPS_RBLOCK workgroups a cloud
    const int64_t groups = narrow_prefix(prefix, batch, a.ipl * FPS_RBLOCK, a.pprefix, a.bprefix);
    for (int b = 0; b < batch; ++b) a.start[b] = start ? start[b] : -1;

    hipStream_t s = to_stream(stream);
    k_fps_fill<<<(unsigned)cdiv(M, FPS_FILL), FPS_FILL, 0, s>>>(a);
    HPL_CHECK_LAUNCH("hpl_fps (fill)");
    if (a.path == HPL_FPS_RESIDENT) {
        k_fps_resident<<<(unsigned)batch, FPS_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH("hpl_fps (resident)");
        return HPL_OK;
    }
    for (int r = 0; r <= a.m; ++r) {
        k_fps_round<<<(unsigned)groups, FPS_RBLOCK, 0, s>>>(a, r);
        HPL_CHECK_LAUNCH("hpl_fps (round)");
    }
    return HPL_OK;
}
