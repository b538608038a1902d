// render.hip -- maps from clouds (hpl_render_maps, hpl_maps_to_kitti): every point of a packed ragged batch of
// clouds is projected through its frame's pinhole camera -- the arithmetic of hpl_flow_metrics -- and a z-buffer keeps the
// nearest point per pixel.  hpl_render_maps returns the winner, its depth and attribute channels per pixel and which points the
// camera sees; hpl_maps_to_kitti is the inverse of hpl_frames_from_kitti: the raw uint16 values of KITTI's three PNGs.
//
//   k_render_clear   a lane per z-buffer word (all ones) and per counter (0)
//   k_render_splat   a lane per point: pixel_of, and the key (bits(zc) << 32) | local index offered to the pixels of its
//                    footprint with a no-return 64-bit atomicMin -- behind a look at the word, which only ever decreases
//   k_render_resolve a lane per pixel: winner, depth, the winner's channels; the covered count
//   k_render_visible a lane per point: zc against the depth at its own pixel
//   k_render_kitti   a lane per pixel: the five raw planes from the winner's two points
//
// A workgroup lies inside one cloud (or one frame), so the camera is uniform and the counts are one integer atomic a wave.
// The minimum of a set of integers does not depend on the order of the atomics: an output is the same bits alone, anywhere in a
// batch and beside other work.  The sizes of all launches are host numbers; nothing is read back, no lane waits for another.
//
// The arithmetic is part of the interface (include/hpl_bcl.h; tests/render_oracle.py restates it in numpy): float32, one
// rounding per operation, no contraction (-ffp-contract=off), the correctly rounded division.
#include "cloud_common.h"

#include <math.h>

using namespace hpl;

namespace {

constexpr int RD_BLOCK = 256;
constexpr int RD_MAX_FOOTPRINT = 4;
constexpr int RD_MAX_CHANNELS = 8;
constexpr float RD_KITTI_NEAR = 1e-3f;               // the near plane of hpl_maps_to_kitti (render_maps' default)
constexpr int64_t RD_MAX_LD = (int64_t)1 << 40;      // a row stride above it is refused: byte extents stay far inside 64 bits
constexpr unsigned long long RD_EMPTY = ~0ull;

struct RdArgs {
    const float *pc, *pc2, *attr;
    int64_t pc_ld, pc2_ld, attr_ld, attr_map_ld;
    unsigned long long *zbuf;
    int32_t *pixel_of, *winner, *stats;
    float *depth, *attr_map;
    uint8_t *visible;
    uint16_t *disp1, *disp2, *flow3;
    float near_z, rel1, abs_tol;                 // rel1 = 1 + rel_tol
    int32_t footprint, channels, batch, m_total;
    int32_t pprefix[CLOUD_MAX_BATCH + 1];        // points
    int32_t qprefix[CLOUD_MAX_BATCH + 1];        // pixels
    int32_t bprefix[CLOUD_MAX_BATCH + 1];        // workgroups of clouds (or frames) 0 .. b-1 of this launch
    int32_t height[CLOUD_MAX_BATCH], width[CLOUD_MAX_BATCH];
    float cam[CLOUD_MAX_BATCH][7];               // f, cx, cy, constx, consty, constz; KITTI: P00 * baseline
};

// utils/geometry.py:project_3d_to_2d, operation by operation (what k_flow_metrics computes)
__device__ __forceinline__ void project(const float (&c)[7], float x, float y, float z, float zc, float &u, float &v) {
    u = ((x * c[0] + c[1] * z) + c[3]) / zc;
    v = ((y * c[0] + c[2] * z) + c[4]) / zc;
}

__device__ __forceinline__ bool projectable(float x, float y, float z, float zc, float near_z) {
    return isfinite(x) && isfinite(y) && isfinite(z) && zc >= near_z;     // (a NaN zc fails)
}

// r = rintf(coordinate) is a pixel index of 0 .. n-1: decided on the floats (a float converts to double exactly), so a huge,
// infinite or NaN r is never cast; -0.0f passes and casts to 0
__device__ __forceinline__ bool in_range(float r, int n) { return r >= 0.f && (double)r <= (double)n - 1.0; }

__device__ __forceinline__ int wave_count(bool x) { return __popcll(__ballot(x)); }

__global__ void __launch_bounds__(RD_BLOCK) k_render_clear(const RdArgs a) {
    const int64_t i = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (i < a.m_total) a.zbuf[i] = RD_EMPTY;
    if (a.stats && i < 4 * a.batch) a.stats[i] = 0;
}

template <bool SKIP>
__global__ void __launch_bounds__(RD_BLOCK) k_render_splat(const RdArgs a) {
    const int b = block_group(a.bprefix, a.batch, (int)blockIdx.x);
    const int p0 = a.pprefix[b], n = a.pprefix[b + 1] - p0;
    const int local = ((int)blockIdx.x - a.bprefix[b]) * RD_BLOCK + (int)threadIdx.x;
    const bool live = local < n;
    const int H = a.height[b], W = a.width[b], r = a.footprint;
    bool ok = false, inside = false;
    int i = 0, j = 0;
    float zc = 0.f;
    if (live) {
        const int64_t g = (int64_t)p0 + local;
        const float x = a.pc[g], y = a.pc[a.pc_ld + g], z = a.pc[2 * a.pc_ld + g];
        zc = z + a.cam[b][5];
        ok = projectable(x, y, z, zc, a.near_z);
        if (ok) {
            float u, v;
            project(a.cam[b], x, y, z, zc, u, v);
            const float ru = rintf(u), rv = rintf(v);
            inside = in_range(ru, W) && in_range(rv, H);
            if (inside) { j = (int)ru; i = (int)rv; }
        }
        if (a.pixel_of) a.pixel_of[g] = inside ? i * W + j : -1;
    }
    if (a.stats) {
        const int n_in = wave_count(inside), n_bad = wave_count(live && !ok);
        if ((threadIdx.x & 63) == 0) {
            if (n_in) atomicAdd(a.stats + 4 * b, n_in);
            if (n_bad) atomicAdd(a.stats + 4 * b + 3, n_bad);
        }
    }
    if (!inside) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(zc) << 32) | (unsigned)local;
    unsigned long long *frame = a.zbuf + a.qprefix[b];
    const int i0 = max(i - r, 0), i1 = min(i + r, H - 1), j0 = max(j - r, 0), j1 = min(j + r, W - 1);
    for (int ii = i0; ii <= i1; ++ii)
        for (int jj = j0; jj <= j1; ++jj) {
            unsigned long long *word = frame + ((int64_t)ii * W + jj);
            if (SKIP && __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) continue;
            atomicMin(word, key);
        }
}

__global__ void __launch_bounds__(RD_BLOCK) k_render_resolve(const RdArgs a) {
    const int b = block_group(a.bprefix, a.batch, (int)blockIdx.x);
    const int q0 = a.qprefix[b], m = a.qprefix[b + 1] - q0;
    const int local = ((int)blockIdx.x - a.bprefix[b]) * RD_BLOCK + (int)threadIdx.x;
    bool covered = false;
    if (local < m) {
        const int64_t q = (int64_t)q0 + local;
        const unsigned long long word = a.zbuf[q];
        covered = word != RD_EMPTY;
        const int w = (int)(unsigned)word;
        a.winner[q] = covered ? w : -1;
        a.depth[q] = covered ? __uint_as_float((unsigned)(word >> 32)) : 0.f;
        if (a.attr_map) {
            const int64_t src = (int64_t)a.pprefix[b] + w;
            for (int c = 0; c < a.channels; ++c) a.attr_map[c * a.attr_map_ld + q] = covered ? a.attr[c * a.attr_ld + src] : 0.f;
        }
    }
    const int n_cov = wave_count(covered);
    if ((threadIdx.x & 63) == 0 && n_cov) atomicAdd(a.stats + 4 * b + 1, n_cov);
}

__global__ void __launch_bounds__(RD_BLOCK) k_render_visible(const RdArgs a) {
    const int b = block_group(a.bprefix, a.batch, (int)blockIdx.x);
    const int p0 = a.pprefix[b], n = a.pprefix[b + 1] - p0;
    const int local = ((int)blockIdx.x - a.bprefix[b]) * RD_BLOCK + (int)threadIdx.x;
    bool seen = false;
    if (local < n) {
        const int64_t g = (int64_t)p0 + local;
        const int pix = a.pixel_of[g];
        if (pix >= 0) {
            const float zc = a.pc[2 * a.pc_ld + g] + a.cam[b][5];
            const float zmin = __uint_as_float((unsigned)(a.zbuf[(int64_t)a.qprefix[b] + pix] >> 32));
            seen = zc <= (zmin * a.rel1) + a.abs_tol;
        }
        a.visible[g] = seen ? 1 : 0;
    }
    const int n_seen = wave_count(seen);
    if ((threadIdx.x & 63) == 0 && n_seen) atomicAdd(a.stats + 4 * b + 2, n_seen);
}

// rintf(x) clamped to lo .. hi as a uint16; a NaN gives lo
__device__ __forceinline__ uint16_t raw16(float x, float lo, float hi) {
    const float r = rintf(x);
    return (uint16_t)(int)(r >= lo ? (r <= hi ? r : hi) : lo);
}

__global__ void __launch_bounds__(RD_BLOCK) k_render_kitti(const RdArgs a) {
    const int b = block_group(a.bprefix, a.batch, (int)blockIdx.x);
    const int q0 = a.qprefix[b], m = a.qprefix[b + 1] - q0;
    const int local = ((int)blockIdx.x - a.bprefix[b]) * RD_BLOCK + (int)threadIdx.x;
    if (local >= m) return;
    const int64_t q = (int64_t)q0 + local;
    const unsigned long long word = a.zbuf[q];
    uint16_t r1 = 0, r2 = 0, ur = 0, vr = 0, mr = 0;
    if (word != RD_EMPTY) {
        const int W = a.width[b];
        const int i = local / W, j = local - i * W;
        const int64_t g = (int64_t)a.pprefix[b] + (int)(unsigned)word;
        const float fb = a.cam[b][6];
        const float z1 = a.pc[2 * a.pc_ld + g];
        const float x2 = a.pc2[g], y2 = a.pc2[a.pc2_ld + g], z2 = a.pc2[2 * a.pc2_ld + g];
        const float zc2 = z2 + a.cam[b][5];
        r1 = raw16((fb / z1 - 1e-5f) * 256.f, 1.f, 65535.f);
        if (projectable(x2, y2, z2, zc2, a.near_z)) {
            float px2, py2;
            project(a.cam[b], x2, y2, z2, zc2, px2, py2);
            r2 = raw16((fb / z2 - 1e-5f) * 256.f, 1.f, 65535.f);
            ur = raw16((px2 - (float)j) * 64.f + 32768.f, 0.f, 65535.f);
            vr = raw16((py2 - (float)i) * 64.f + 32768.f, 0.f, 65535.f);
            mr = 1;
        }
    }
    a.disp1[q] = r1;
    a.disp2[q] = r2;
    a.flow3[3 * q] = ur; a.flow3[3 * q + 1] = vr; a.flow3[3 * q + 2] = mr;
}

// workspace: the z-buffer, one 64-bit word per pixel
inline int64_t workspace_bytes(int64_t m) {
    Carver c;
    c.take(8 * m);
    return c.bytes;
}

inline bool overlaps(const void *p, int64_t pbytes, const void *q, int64_t qbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && pbytes > 0 && qbytes > 0 && a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}

inline int64_t rows_extent(int rows, int64_t ld, int64_t n) { return n > 0 && rows > 0 ? 4 * ((rows - 1) * ld + n) : 0; }

struct Piece { const void *p; int64_t bytes; int owner; };      // owner < 0: an input (whole extent), else an output's row

// No output row (or the workspace) overlaps an input or a row of another output: views that interleave inside one buffer stay legal.
int check_apart(const char *op, const Piece *pieces, int count) {
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j) {
            if (pieces[i].owner < 0 && pieces[j].owner < 0) continue;
            if (pieces[i].owner == pieces[j].owner) continue;
            const bool input = pieces[i].owner < 0 || pieces[j].owner < 0;
            HPL_REQUIRE(!overlaps(pieces[i].p, pieces[i].bytes, pieces[j].p, pieces[j].bytes),
                        input ? "%s: an output overlaps an input" : "%s: two outputs (or an output and the workspace) overlap", op);
        }
    return HPL_OK;
}

// the points' prefix and the frames' sizes and prefix; -> N, M
int check_shapes(const char *op, int batch, const int64_t *prefix, const int32_t *height, const int32_t *width,
                 const int64_t *pixel_prefix, int footprint, int64_t *n_out, int64_t *m_out) {
    HPL_REQUIRE(prefix && height && width && pixel_prefix, "%s: null pointer", op);
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix", "cloud", prefix, batch));
    HPL_CLOUD_CHECK(check_prefix(op, "the pixel prefix", "frame", pixel_prefix, batch));
    for (int b = 0; b < batch; ++b) {
        HPL_REQUIRE(height[b] >= 0 && width[b] >= 0, "%s: frame %d of %d x %d pixels", op, b, height[b], width[b]);
        HPL_REQUIRE(pixel_prefix[b + 1] - pixel_prefix[b] == (int64_t)height[b] * (int64_t)width[b],
                    "%s: the pixel prefix gives frame %d %lld pixels, its size %d x %d", op, b,
                    (long long)(pixel_prefix[b + 1] - pixel_prefix[b]), height[b], width[b]);
    }
    HPL_CLOUD_CHECK(check_points(op, prefix[batch]));
    HPL_REQUIRE(pixel_prefix[batch] < CLOUD_MAX_POINTS, "%s: %lld pixels pass the 32-bit element limit (M < 2^31 / 3)", op,
                (long long)pixel_prefix[batch]);
    HPL_REQUIRE(footprint >= 0 && footprint <= RD_MAX_FOOTPRINT, "%s: footprint %d (0 .. %d)", op, footprint, RD_MAX_FOOTPRINT);
    *n_out = prefix[batch];
    *m_out = pixel_prefix[batch];
    return HPL_OK;
}

int check_cloud(const char *op, const char *what, const float *pc, int64_t ld, int64_t n) {
    HPL_REQUIRE(pc || n == 0, "%s: null pointer", op);
    HPL_CLOUD_CHECK(check_row_stride(op, ld, n));
    HPL_REQUIRE(ld <= RD_MAX_LD, "%s: row stride %lld of %s above 2^40", op, (long long)ld, what);
    return HPL_OK;
}

void fill_shapes(RdArgs &a, int batch, const int64_t *prefix, const int32_t *height, const int32_t *width, const int64_t *pixel_prefix) {
    a.batch = batch;
    a.m_total = (int32_t)pixel_prefix[batch];
    for (int b = 0; b <= batch; ++b) {
        a.pprefix[b] = (int32_t)prefix[b];
        a.qprefix[b] = (int32_t)pixel_prefix[b];
        if (b < batch) { a.height[b] = height[b]; a.width[b] = width[b]; }
    }
}

// the workgroups of a launch with a lane per point (over = pprefix) or per pixel (over = qprefix)
unsigned span_blocks(RdArgs &a, const int32_t *over) {
    int64_t blocks = 0;
    for (int b = 0; b <= a.batch; ++b) {
        a.bprefix[b] = (int32_t)blocks;
        if (b < a.batch) blocks += cdiv((int64_t)over[b + 1] - over[b], RD_BLOCK);
    }
    return (unsigned)blocks;
}

#ifdef HPL_RENDER_NO_SKIP
constexpr bool RD_SKIP = false;                  // a measurement build: every offer pays its atomic (tools/render_bench.py)
#else
constexpr bool RD_SKIP = true;
#endif

// clear and splat: what both entries launch first
int launch_zbuffer(const char *op, RdArgs &a, int64_t N, int64_t M, hipStream_t s) {
    const int64_t cells = imax(M, a.stats ? 4 * (int64_t)a.batch : 0);
    if (cells > 0) {
        k_render_clear<<<(unsigned)cdiv(cells, RD_BLOCK), RD_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH(op);
    }
    if (N > 0) {
        const unsigned blocks = span_blocks(a, a.pprefix);
        k_render_splat<RD_SKIP><<<blocks, RD_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH(op);
    }
    return HPL_OK;
}

}  // namespace

extern "C" int64_t hpl_render_workspace_bytes(int batch, int64_t m_total) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || m_total < 0 || m_total >= CLOUD_MAX_POINTS) return -1;
    return workspace_bytes(m_total);
}

extern "C" int hpl_render_maps(const float *pc, int64_t pc_ld, const float *attr, int64_t attr_ld, int channels, int batch,
                               const int64_t *prefix, const float *camera, const int32_t *height, const int32_t *width,
                               const int64_t *pixel_prefix, int footprint, float rel_tol, float abs_tol, float near_z,
                               int32_t *pixel_of, int32_t *winner, float *depth, float *attr_map, int64_t attr_map_ld,
                               uint8_t *visible, int32_t *stats, void *workspace, int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_render_maps";
    int64_t N = 0, M = 0;
    HPL_REQUIRE(camera && stats && workspace, "%s: null pointer", op);
    HPL_CLOUD_CHECK(check_shapes(op, batch, prefix, height, width, pixel_prefix, footprint, &N, &M));
    HPL_REQUIRE(((pixel_of && visible) || N == 0) && ((winner && depth) || M == 0), "%s: null pointer", op);
    HPL_REQUIRE(channels >= 0 && channels <= RD_MAX_CHANNELS, "%s: %d channels (0 .. %d)", op, channels, RD_MAX_CHANNELS);
    HPL_REQUIRE(attr || channels == 0 || N == 0, "%s: null attr with %d channels", op, channels);
    HPL_CLOUD_CHECK(check_cloud(op, "pc", pc, pc_ld, N));
    if (channels) {
        HPL_CLOUD_CHECK(check_row_stride(op, attr_ld, N));
        HPL_REQUIRE(attr_ld <= RD_MAX_LD, "%s: row stride %lld of attr above 2^40", op, (long long)attr_ld);
        if (attr_map) {
            HPL_REQUIRE(attr_map_ld >= M && attr_map_ld <= RD_MAX_LD, "%s: row stride %lld of attr_map (%lld pixels .. 2^40)", op,
                        (long long)attr_map_ld, (long long)M);
        }
    }
    HPL_REQUIRE(isfinite(rel_tol) && rel_tol >= 0.f && isfinite(abs_tol) && abs_tol >= 0.f,
                "%s: tolerances %g (relative) / %g (absolute) must be finite and >= 0", op, (double)rel_tol, (double)abs_tol);
    HPL_REQUIRE(isfinite(near_z) && near_z > 0.f, "%s: near = %g (finite and > 0)", op, (double)near_z);
    for (int b = 0; b < batch; ++b)
        HPL_REQUIRE(camera[6 * b] != 0.f && isfinite(camera[6 * b]), "%s: f of camera %d must be finite and not zero", op, b);
    HPL_CLOUD_CHECK(check_aligned4(op, {pc, attr, pixel_of, winner, depth, attr_map, stats}));
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, workspace_bytes(M)));
    if (!channels) attr_map = nullptr;
    Piece pieces[8 + RD_MAX_CHANNELS];
    int count = 0;
    pieces[count++] = {pc, rows_extent(3, pc_ld, N), -1};
    pieces[count++] = {attr, rows_extent(channels, attr_ld, N), -1};
    pieces[count++] = {pixel_of, 4 * N, 0};
    pieces[count++] = {winner, 4 * M, 1};
    pieces[count++] = {depth, 4 * M, 2};
    pieces[count++] = {visible, N, 3};
    pieces[count++] = {stats, 16 * (int64_t)batch, 4};
    pieces[count++] = {workspace, workspace_bytes(M), 5};
    for (int c = 0; attr_map && c < channels; ++c) pieces[count++] = {attr_map + c * attr_map_ld, 4 * M, 6};
    HPL_CLOUD_CHECK(check_apart(op, pieces, count));
    if (N == 0 && M == 0) return HPL_OK;
    RdArgs a{};
    fill_shapes(a, batch, prefix, height, width, pixel_prefix);
    for (int b = 0; b < batch; ++b)
        for (int k = 0; k < 6; ++k) a.cam[b][k] = camera[6 * b + k];
    a.pc = pc; a.pc_ld = pc_ld; a.attr = attr; a.attr_ld = attr_ld; a.channels = channels;
    a.zbuf = carved<unsigned long long>(workspace, 0);
    a.pixel_of = pixel_of; a.winner = winner; a.depth = depth; a.attr_map = attr_map; a.attr_map_ld = attr_map_ld;
    a.visible = visible; a.stats = stats;
    a.footprint = footprint; a.near_z = near_z; a.rel1 = 1.f + rel_tol; a.abs_tol = abs_tol;
    hipStream_t s = to_stream(stream);
    HPL_CLOUD_CHECK(launch_zbuffer(op, a, N, M, s));
    if (M > 0) {
        const unsigned blocks = span_blocks(a, a.qprefix);
        k_render_resolve<<<blocks, RD_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH(op);
    }
    if (N > 0) {
        const unsigned blocks = span_blocks(a, a.pprefix);
        k_render_visible<<<blocks, RD_BLOCK, 0, s>>>(a);
        HPL_CHECK_LAUNCH(op);
    }
    return HPL_OK;
}

extern "C" int hpl_maps_to_kitti(const float *pc1, int64_t pc1_ld, const float *pc2, int64_t pc2_ld, int batch,
                                 const int64_t *prefix, const int32_t *height, const int32_t *width, const int64_t *pixel_prefix,
                                 const float *P, float baseline, int footprint, uint16_t *disp1, uint16_t *disp2, uint16_t *flow,
                                 void *workspace, int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_maps_to_kitti";
    int64_t N = 0, M = 0;
    HPL_REQUIRE(P && workspace, "%s: null pointer", op);
    HPL_CLOUD_CHECK(check_shapes(op, batch, prefix, height, width, pixel_prefix, footprint, &N, &M));
    HPL_REQUIRE((disp1 && disp2 && flow) || M == 0, "%s: null pointer", op);
    HPL_CLOUD_CHECK(check_cloud(op, "pc1", pc1, pc1_ld, N));
    HPL_CLOUD_CHECK(check_cloud(op, "pc2", pc2, pc2_ld, N));
    HPL_CLOUD_CHECK(check_aligned4(op, {pc1, pc2}));
    HPL_REQUIRE(((reinterpret_cast<uintptr_t>(disp1) | reinterpret_cast<uintptr_t>(disp2) | reinterpret_cast<uintptr_t>(flow)) & 1u) == 0,
                "%s: the uint16 arrays must be 2-byte aligned", op);
    HPL_REQUIRE(isfinite(baseline), "%s: baseline must be finite", op);
    RdArgs a{};
    for (int b = 0; b < batch; ++b) {
        const float *p = P + 12 * b;
        HPL_REQUIRE(p[1] == 0.f && p[4] == 0.f && p[8] == 0.f && p[9] == 0.f && p[0] == p[5],
                    "%s: P of frame %d is no rectified pinhole (P01, P10, P20, P21 must be 0 and P00 == P11)", op, b);
        HPL_REQUIRE(p[0] != 0.f && isfinite(p[0]), "%s: P00 of frame %d must be finite and not zero", op, b);
        a.cam[b][0] = -p[0]; a.cam[b][1] = p[2]; a.cam[b][2] = p[6]; a.cam[b][3] = p[3]; a.cam[b][4] = p[7]; a.cam[b][5] = p[11];
        a.cam[b][6] = p[0] * baseline;
    }
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 256, workspace_bytes_, workspace_bytes(M)));
    const Piece pieces[6] = {{pc1, rows_extent(3, pc1_ld, N), -1}, {pc2, rows_extent(3, pc2_ld, N), -2}, {disp1, 2 * M, 0},
                             {disp2, 2 * M, 1}, {flow, 6 * M, 2}, {workspace, workspace_bytes(M), 3}};
    HPL_CLOUD_CHECK(check_apart(op, pieces, 6));
    if (M == 0) return HPL_OK;
    fill_shapes(a, batch, prefix, height, width, pixel_prefix);
    a.pc = pc1; a.pc_ld = pc1_ld; a.pc2 = pc2; a.pc2_ld = pc2_ld;
    a.zbuf = carved<unsigned long long>(workspace, 0);
    a.disp1 = disp1; a.disp2 = disp2; a.flow3 = flow;
    a.footprint = footprint; a.near_z = RD_KITTI_NEAR;
    hipStream_t s = to_stream(stream);
    HPL_CLOUD_CHECK(launch_zbuffer(op, a, N, M, s));
    const unsigned blocks = span_blocks(a, a.qprefix);
    k_render_kitti<<<blocks, RD_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH(op);
    return HPL_OK;
}
