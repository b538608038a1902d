// frames.hip -- corresponding point clouds from raw disparity / optical-flow maps (hpl_frames_from_kitti, hpl_frames_from_ft3d,
// DESIGN.md §25): every pixel of a packed ragged batch of frames is back-projected in float32, and the valid correspondences
// of each frame are compacted to the front of its range in ascending pixel index -- the order of numpy's boolean-mask indexing,
// so a frame's result is the array the reference's preprocessing scripts save, transposed.  Also hpl_png_unfilter, the host-only
// inverse of the five PNG row filters for data.read_png.
//
//   k_frames_count   a workgroup per FR_SPAN pixels of one frame: the valid pixels it holds (an integer)
//   k_frames_scan    a workgroup per frame: its workgroups' counts become offsets, their sum counts[b] (the pattern of
//                    DESIGN.md §35; count and emit rank quads, not rows, and keep their text)
//   k_frames_emit    the same workgroups again: a valid pixel's two points and its index go to prefix[b] + its rank, and every
//                    position of the frame's range at or behind counts[b] is cleared (0 in the clouds, -1 in pixel)
//
// A lane takes four consecutive pixels whose first PACKED index is a multiple of four, so that with 16-byte aligned planes a
// quad inside its frame is one 4 / 8 / 16 / 24 / 32-byte group of vector loads whatever the frame's start; a quad that crosses
// its frame's ends, or whose address is not aligned, is read pixel by pixel.  The sizes of all launches are host numbers;
// nothing is read back, no lane waits for another, counts are integers and the rank of a pixel is its frame's own: a frame's
// outputs are the same bits alone, anywhere in a batch and beside other work.
//
// The arithmetic is part of the interface (include/hpl_bcl.h; tests/frames_oracle.py restates it in numpy): float32, one
// rounding per operation, no contraction (-ffp-contract=off), the correctly rounded division.
#include "cloud_common.h"

#include <math.h>
#include <stdlib.h>

using namespace hpl;

namespace {

constexpr int FR_BLOCK = 256;
constexpr int FR_WAVES = FR_BLOCK / 64;
constexpr int FR_QUAD = 4;                       // consecutive pixels of a lane
constexpr int FR_SPAN = FR_BLOCK * FR_QUAD;      // pixels of a workgroup
constexpr int FORM_KITTI = 0, FORM_FT3D = 1;
constexpr int64_t FR_MAX_LD = (int64_t)1 << 40;      // a row stride above it is refused: byte extents stay far inside 64 bits

struct FrArgs {
    const uint16_t *disp1, *disp2, *flow3;       // KITTI: raw PNG values, the flow interleaved (u, v, mask)
    const float *disp, *dchange, *flow2;         // FlyingThings3D: the flow interleaved (x, y)
    const uint8_t *occ1, *occ2;
    float *out1, *out2;
    int64_t ld1, ld2;
    int32_t *pixel, *counts, *blockoff;
    float nf, cx, cy, near_z;
    int32_t use_near, batch;
    int32_t pprefix[CLOUD_MAX_BATCH + 1];
    int32_t bprefix[CLOUD_MAX_BATCH + 1];        // workgroups of frames 0 .. b-1
    int32_t width[CLOUD_MAX_BATCH];
    float cam[CLOUD_MAX_BATCH][7];               // KITTI: P00, P02, P03, P12, P13, P23, P00 * baseline
};

// four pixels: KITTI a, b = the raw disparities, u, v = the raw flow; FlyingThings3D a, b = the disparities d1, d2, u, v = the flow
struct Quad {
    bool valid[FR_QUAD];
    float a[FR_QUAD], b[FR_QUAD], u[FR_QUAD], v[FR_QUAD];
};

__device__ __forceinline__ bool aligned_to(const void *p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

__device__ __forceinline__ void unpack4(const uint2 w, unsigned (&r)[4]) {
    r[0] = w.x & 0xffffu; r[1] = w.x >> 16; r[2] = w.y & 0xffffu; r[3] = w.y >> 16;
}

__device__ __forceinline__ void load_u16x4(const uint16_t *plane, int64_t i0, bool inside, int p0, int p1, unsigned (&r)[4]) {
    if (inside && aligned_to(plane + i0, 8)) {
        unpack4(*reinterpret_cast<const uint2 *>(plane + i0), r);
    } else {
#pragma unroll
        for (int k = 0; k < FR_QUAD; ++k) r[k] = (i0 + k >= p0 && i0 + k < p1) ? plane[i0 + k] : 0u;
    }
}

__device__ __forceinline__ void load_f32x4(const float *plane, int64_t i0, bool inside, int p0, int p1, float (&r)[4]) {
    if (inside && aligned_to(plane + i0, 16)) {
        const float4 w = *reinterpret_cast<const float4 *>(plane + i0);
        r[0] = w.x; r[1] = w.y; r[2] = w.z; r[3] = w.w;
    } else {
#pragma unroll
        for (int k = 0; k < FR_QUAD; ++k) r[k] = (i0 + k >= p0 && i0 + k < p1) ? plane[i0 + k] : 0.f;
    }
}

__device__ __forceinline__ void load_u8x4(const uint8_t *plane, int64_t i0, bool inside, int p0, int p1, unsigned (&r)[4]) {
    if (inside && aligned_to(plane + i0, 4)) {
        const unsigned w = *reinterpret_cast<const unsigned *>(plane + i0);
        r[0] = w & 0xffu; r[1] = (w >> 8) & 0xffu; r[2] = (w >> 16) & 0xffu; r[3] = w >> 24;
    } else {
#pragma unroll
        for (int k = 0; k < FR_QUAD; ++k) r[k] = (i0 + k >= p0 && i0 + k < p1) ? plane[i0 + k] : 1u;   // (outside: occluded)
    }
}

__device__ __forceinline__ float ft3d_depth(const FrArgs &a, float d) { return a.nf / d; }

// The quad of packed indices i0 .. i0 + 3 of the frame [p0, p1); a pixel outside the frame is not valid.  FULL: with the flow.
template <int FORM, bool FULL>
__device__ __forceinline__ void load_quad(const FrArgs &a, int64_t i0, int p0, int p1, Quad &q) {
    const bool inside = i0 >= p0 && i0 + FR_QUAD <= p1;
    if (FORM == FORM_KITTI) {
        unsigned r1[4], r2[4], fl[12];
        load_u16x4(a.disp1, i0, inside, p0, p1, r1);
        load_u16x4(a.disp2, i0, inside, p0, p1, r2);
        const uint16_t *f = a.flow3 + 3 * i0;
        if (inside && aligned_to(f, 8)) {
            unsigned w[3][4];
#pragma unroll
            for (int g = 0; g < 3; ++g) unpack4(*reinterpret_cast<const uint2 *>(f + 4 * g), w[g]);
#pragma unroll
            for (int e = 0; e < 12; ++e) fl[e] = w[e / 4][e % 4];
        } else {
#pragma unroll
            for (int k = 0; k < FR_QUAD; ++k) {
                const bool in = i0 + k >= p0 && i0 + k < p1;
                fl[3 * k + 2] = in ? f[3 * k + 2] : 0u;
                fl[3 * k] = (FULL && in) ? f[3 * k] : 0u;
                fl[3 * k + 1] = (FULL && in) ? f[3 * k + 1] : 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < FR_QUAD; ++k) {
            q.valid[k] = r1[k] > 0u && r2[k] > 0u && fl[3 * k + 2] == 1u;
            q.a[k] = (float)r1[k]; q.b[k] = (float)r2[k];
            q.u[k] = (float)fl[3 * k]; q.v[k] = (float)fl[3 * k + 1];
        }
    } else {
        unsigned o1[4], o2[4];
        float d[4], dc[4];
        load_u8x4(a.occ1, i0, inside, p0, p1, o1);
        load_u8x4(a.occ2, i0, inside, p0, p1, o2);
        const bool need_d = FULL || a.use_near;
        if (need_d) {
            load_f32x4(a.disp, i0, inside, p0, p1, d);
            load_f32x4(a.dchange, i0, inside, p0, p1, dc);
        }
        if (FULL) {
            const float *f = a.flow2 + 2 * i0;
            if (inside && aligned_to(f, 16)) {
                const float4 w0 = *reinterpret_cast<const float4 *>(f), w1 = *reinterpret_cast<const float4 *>(f + 4);
                q.u[0] = w0.x; q.v[0] = w0.y; q.u[1] = w0.z; q.v[1] = w0.w;
                q.u[2] = w1.x; q.v[2] = w1.y; q.u[3] = w1.z; q.v[3] = w1.w;
            } else {
#pragma unroll
                for (int k = 0; k < FR_QUAD; ++k) {
                    const bool in = i0 + k >= p0 && i0 + k < p1;
                    q.u[k] = in ? f[2 * k] : 0.f;
                    q.v[k] = in ? f[2 * k + 1] : 0.f;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < FR_QUAD; ++k) {
            bool ok = o1[k] == 0u && o2[k] == 0u;
            if (need_d) {
                q.a[k] = d[k];
                q.b[k] = d[k] + dc[k];
                if (a.use_near) ok = ok && ft3d_depth(a, q.a[k]) > a.near_z && ft3d_depth(a, q.b[k]) > a.near_z;   // (NaN: dropped)
            }
            q.valid[k] = ok;
        }
    }
}

// the first packed index of lane t's quad in workgroup blk of frame b: the frame's quads start at its start rounded down to 4
__device__ __forceinline__ int64_t quad_start(const FrArgs &a, int b, int blk, int t) {
    return (int64_t)(a.pprefix[b] & ~(FR_QUAD - 1)) + (int64_t)(blk - a.bprefix[b]) * FR_SPAN + (int64_t)t * FR_QUAD;
}

__device__ __forceinline__ int valid_count(const Quad &q) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < FR_QUAD; ++k) n += q.valid[k] ? 1 : 0;
    return n;
}

template <int FORM>
__global__ void __launch_bounds__(FR_BLOCK) k_frames_count(const FrArgs a) {
    __shared__ int wt[FR_WAVES];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = block_group(a.bprefix, a.batch, blk);
    Quad q;
    load_quad<FORM, false>(a, quad_start(a, b, blk, t), a.pprefix[b], a.pprefix[b + 1], q);
    int n = valid_count(q);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) n += __shfl_xor(n, m);
    if (lane == 0) wt[wave] = n;
    __syncthreads();
    if (t == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < FR_WAVES; ++w) s += wt[w];
        a.blockoff[blk] = s;
    }
}

__global__ void __launch_bounds__(FR_BLOCK) k_frames_scan(const FrArgs a) {
    // (k_ground_scan's text: as one function for both, this kernel's A/B fell outside the parent's span -- rule R)
    __shared__ int sc[FR_BLOCK];
    __shared__ int carry;
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b0 = a.bprefix[b], nb = a.bprefix[b + 1] - b0;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < nb; c0 += FR_BLOCK) {
        const int j = c0 + t;
        const int v = j < nb ? a.blockoff[b0 + j] : 0;
        sc[t] = v;
        __syncthreads();
        for (int w = 1; w < FR_BLOCK; w <<= 1) {             // inclusive sums of the chunk
            const int u = t >= w ? sc[t - w] : 0;
            __syncthreads();
            sc[t] += u;
            __syncthreads();
        }
        const int before = carry;
        if (j < nb) a.blockoff[b0 + j] = before + sc[t] - v;
        __syncthreads();
        if (t == FR_BLOCK - 1) carry = before + sc[t];
        __syncthreads();
    }
    if (t == 0) a.counts[b] = carry;
}

template <int FORM>
__global__ void __launch_bounds__(FR_BLOCK) k_frames_emit(const FrArgs a) {
    __shared__ int wt[FR_WAVES];
    const int blk = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = block_group(a.bprefix, a.batch, blk);
    const int p0 = a.pprefix[b], p1 = a.pprefix[b + 1], W = a.width[b];
    const int64_t i0 = quad_start(a, b, blk, t);
    const int total = a.counts[b];
    Quad q;
    load_quad<FORM, true>(a, i0, p0, p1, q);
    const int n = valid_count(q);
    int incl = n;                                // valid pixels of the wave up to and including this lane's
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wt[wave] = incl;
    __syncthreads();
    int rank = a.blockoff[blk] + incl - n;       // valid pixels of the frame before this lane's
#pragma unroll
    for (int w = 0; w < FR_WAVES; ++w) rank += w < wave ? wt[w] : 0;
#pragma unroll
    for (int k = 0; k < FR_QUAD; ++k) {
        const int64_t i = i0 + k;
        if (q.valid[k]) {
            const int local = (int)(i - p0);
            const int row = local / W, col = local - row * W;
            float x1, y1, z1, x2, y2, z2;
            if (FORM == FORM_KITTI) {
                const float P00 = a.cam[b][0], P02 = a.cam[b][1], P03 = a.cam[b][2], P12 = a.cam[b][3], P13 = a.cam[b][4],
                            P23 = a.cam[b][5], fb = a.cam[b][6];
                z1 = fb / (q.a[k] / 256.f + 1e-5f);
                z2 = fb / (q.b[k] / 256.f + 1e-5f);
                const float px1 = (float)col, py1 = (float)row;
                const float px2 = px1 + (q.u[k] - 32768.f) / 64.f, py2 = py1 + (q.v[k] - 32768.f) / 64.f;
                x1 = -(((px1 * (z1 + P23)) - ((P02 * z1) + P03)) / P00);
                y1 = -(((py1 * (z1 + P23)) - ((P12 * z1) + P13)) / P00);
                x2 = -(((px2 * (z2 + P23)) - ((P02 * z2) + P03)) / P00);
                y2 = -(((py2 * (z2 + P23)) - ((P12 * z2) + P13)) / P00);
            } else {
                const float pxc = (float)col - a.cx, pyc = (float)row - a.cy;
                z1 = ft3d_depth(a, q.a[k]);
                z2 = ft3d_depth(a, q.b[k]);
                x1 = (-pxc) / q.a[k];
                y1 = pyc / q.a[k];
                x2 = (-(pxc + q.u[k])) / q.b[k];
                y2 = (pyc + q.v[k]) / q.b[k];
            }
            const int64_t at = (int64_t)p0 + rank;
            a.out1[at] = x1; a.out1[a.ld1 + at] = y1; a.out1[2 * a.ld1 + at] = z1;
            a.out2[at] = x2; a.out2[a.ld2 + at] = y2; a.out2[2 * a.ld2 + at] = z2;
            if (a.pixel) a.pixel[at] = local;
            ++rank;
        }
        if (i >= p0 && i < p1 && i - p0 >= total) {          // (valid pixels land below `total`, these at or above it)
#pragma unroll
            for (int c = 0; c < 3; ++c) { a.out1[c * a.ld1 + i] = 0.f; a.out2[c * a.ld2 + i] = 0.f; }
            if (a.pixel) a.pixel[i] = -1;
        }
    }
}

inline int64_t frame_blocks(int64_t p0, int64_t p1) { return p1 > p0 ? cdiv(p1 - (p0 & ~(int64_t)(FR_QUAD - 1)), FR_SPAN) : 0; }

// workspace: the valid counts per workgroup, then their offsets (a frame owns at most n_b / FR_SPAN + 2 workgroups)
inline int64_t workspace_bytes(int batch, int64_t n) {
    Carver c;
    c.take((int64_t)sizeof(int32_t) * (cdiv(n, FR_SPAN) + 2 * (int64_t)batch));
    return c.bytes;
}

inline bool overlaps(const void *p, int64_t pbytes, const void *q, int64_t qbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && pbytes > 0 && qbytes > 0 && a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}

inline int64_t extent(int64_t ld, int64_t n) { return n > 0 ? 4 * (2 * ld + n) : 0; }     // bytes of a (3, n) float32 SoA

struct Input { const void *p; int per_pixel; };     // an input plane and its bytes per pixel

// what both entries check alike; -> N through *n_out
int check_common(const char *op, int batch, const int32_t *height, const int32_t *width, const int64_t *prefix, const float *out1,
                 int64_t ld1, const float *out2, int64_t ld2, const int32_t *pixel, const int32_t *counts, const void *workspace,
                 int64_t workspace_bytes_, const Input *ins, int n_ins, int64_t *n_out) {
    HPL_REQUIRE(height && width && prefix && out1 && out2 && counts && workspace, "%s: null pointer", op);
    for (int i = 0; i < n_ins; ++i) HPL_REQUIRE(ins[i].p, "%s: null pointer", op);
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_CLOUD_CHECK(check_prefix(op, "the prefix", "frame", prefix, batch));
    for (int b = 0; b < batch; ++b) {
        HPL_REQUIRE(height[b] >= 0 && width[b] >= 0, "%s: frame %d of %d x %d pixels", op, b, height[b], width[b]);
        HPL_REQUIRE(prefix[b + 1] - prefix[b] == (int64_t)height[b] * (int64_t)width[b],
                    "%s: the prefix gives frame %d %lld pixels, its size %d x %d", op, b, (long long)(prefix[b + 1] - prefix[b]),
                    height[b], width[b]);
    }
    const int64_t N = prefix[batch];
    HPL_CLOUD_CHECK(check_points(op, N));
    HPL_CLOUD_CHECK(check_row_stride(op, ld1, N));
    HPL_CLOUD_CHECK(check_row_stride(op, ld2, N));
    HPL_REQUIRE(ld1 <= FR_MAX_LD && ld2 <= FR_MAX_LD, "%s: row strides %lld / %lld above 2^40", op, (long long)ld1, (long long)ld2);
    HPL_CLOUD_CHECK(check_aligned4(op, {out1, out2, pixel, counts}));
    HPL_CLOUD_CHECK(check_workspace(op, workspace, 4, workspace_bytes_, workspace_bytes(batch, N)));
    const void *const outs[4] = {out1, out2, pixel, counts};
    const int64_t out_bytes[4] = {extent(ld1, N), extent(ld2, N), 4 * N, 4 * (int64_t)batch};
    for (int o = 0; o < 4; ++o)
        for (int i = 0; i < n_ins; ++i)
            HPL_REQUIRE(!overlaps(outs[o], out_bytes[o], ins[i].p, ins[i].per_pixel * N), "%s: an output overlaps an input", op);
    // the outputs among themselves and against the workspace, row by row: views that interleave inside one buffer stay legal
    const int64_t need = workspace_bytes(batch, N);
    struct Piece { const void *p; int64_t bytes; int owner; } pieces[9];
    for (int r = 0; r < 3; ++r) {
        pieces[r] = {out1 + r * ld1, 4 * N, 0};
        pieces[3 + r] = {out2 + r * ld2, 4 * N, 1};
    }
    pieces[6] = {pixel, 4 * N, 2};
    pieces[7] = {counts, 4 * (int64_t)batch, 3};
    pieces[8] = {workspace, need, 4};
    for (int i = 0; i < 9; ++i)
        for (int j = i + 1; j < 9; ++j)
            HPL_REQUIRE(pieces[i].owner == pieces[j].owner || N == 0 || !overlaps(pieces[i].p, pieces[i].bytes, pieces[j].p, pieces[j].bytes),
                        "%s: two outputs (or an output and the workspace) overlap", op);
    *n_out = N;
    return HPL_OK;
}

void fill_common(FrArgs &a, int batch, const int32_t *width, const int64_t *prefix, float *out1, int64_t ld1, float *out2, int64_t ld2,
                 int32_t *pixel, int32_t *counts, void *workspace, int64_t *blocks_out) {
    a.out1 = out1; a.ld1 = ld1; a.out2 = out2; a.ld2 = ld2;
    a.pixel = pixel; a.counts = counts;
    a.blockoff = carved<int32_t>(workspace, 0);
    a.batch = batch;
    int64_t blocks = 0;
    for (int b = 0; b <= batch; ++b) {
        a.pprefix[b] = (int32_t)prefix[b];
        a.bprefix[b] = (int32_t)blocks;
        if (b < batch) {
            a.width[b] = width[b];
            blocks += frame_blocks(prefix[b], prefix[b + 1]);
        }
    }
    *blocks_out = blocks;
}

template <int FORM>
int launch(const char *op, const FrArgs &a, int64_t blocks, hplStream stream) {
    hipStream_t s = to_stream(stream);
    k_frames_count<FORM><<<(unsigned)blocks, FR_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH(op);
    k_frames_scan<<<(unsigned)a.batch, FR_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH(op);
    k_frames_emit<FORM><<<(unsigned)blocks, FR_BLOCK, 0, s>>>(a);
    HPL_CHECK_LAUNCH(op);
    return HPL_OK;
}

}  // namespace

extern "C" int64_t hpl_frames_workspace_bytes(int batch, int64_t n_total) {
    if (batch < 1 || batch > CLOUD_MAX_BATCH || n_total < 0 || n_total >= CLOUD_MAX_POINTS) return -1;
    return workspace_bytes(batch, n_total);
}

extern "C" int hpl_frames_from_kitti(const uint16_t *disp1, const uint16_t *disp2, const uint16_t *flow, int batch,
                                     const int32_t *height, const int32_t *width, const int64_t *prefix, const float *P,
                                     float baseline, float *out_pc1, int64_t out1_ld, float *out_pc2, int64_t out2_ld,
                                     int32_t *pixel, int32_t *counts, void *workspace, int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_frames_from_kitti";
    HPL_REQUIRE(P, "%s: null pointer", op);
    const Input ins[3] = {{disp1, 2}, {disp2, 2}, {flow, 6}};
    int64_t N = 0;
    HPL_CLOUD_CHECK(check_common(op, batch, height, width, prefix, out_pc1, out1_ld, out_pc2, out2_ld, pixel, counts, workspace,
                                 workspace_bytes_, ins, 3, &N));
    HPL_REQUIRE(((reinterpret_cast<uintptr_t>(disp1) | reinterpret_cast<uintptr_t>(disp2) | reinterpret_cast<uintptr_t>(flow)) & 1u) == 0,
                "%s: the uint16 arrays must be 2-byte aligned", op);
    HPL_REQUIRE(isfinite(baseline), "%s: baseline must be finite", op);
    FrArgs a{};
    for (int b = 0; b < batch; ++b) {
        const float *p = P + 12 * b;
        HPL_REQUIRE(p[1] == 0.f && p[4] == 0.f && p[8] == 0.f && p[9] == 0.f && p[0] == p[5],
                    "%s: P of frame %d is no rectified pinhole (P01, P10, P20, P21 must be 0 and P00 == P11)", op, b);
        HPL_REQUIRE(p[0] != 0.f && isfinite(p[0]), "%s: P00 of frame %d must be finite and not zero", op, b);
        a.cam[b][0] = p[0]; a.cam[b][1] = p[2]; a.cam[b][2] = p[3]; a.cam[b][3] = p[6]; a.cam[b][4] = p[7]; a.cam[b][5] = p[11];
        a.cam[b][6] = p[0] * baseline;
    }
    if (N == 0) return HPL_OK;
    int64_t blocks = 0;
    fill_common(a, batch, width, prefix, out_pc1, out1_ld, out_pc2, out2_ld, pixel, counts, workspace, &blocks);
    a.disp1 = disp1; a.disp2 = disp2; a.flow3 = flow;
    return launch<FORM_KITTI>(op, a, blocks, stream);
}

extern "C" int hpl_frames_from_ft3d(const float *disp, const float *dchange, const float *flow, const uint8_t *occ1,
                                    const uint8_t *occ2, int batch, const int32_t *height, const int32_t *width,
                                    const int64_t *prefix, float f, float cx, float cy, int use_near, float near_z, float *out_pc1,
                                    int64_t out1_ld, float *out_pc2, int64_t out2_ld, int32_t *pixel, int32_t *counts,
                                    void *workspace, int64_t workspace_bytes_, hplStream stream) {
    const char *const op = "hpl_frames_from_ft3d";
    const Input ins[5] = {{disp, 4}, {dchange, 4}, {flow, 8}, {occ1, 1}, {occ2, 1}};
    int64_t N = 0;
    HPL_CLOUD_CHECK(check_common(op, batch, height, width, prefix, out_pc1, out1_ld, out_pc2, out2_ld, pixel, counts, workspace,
                                 workspace_bytes_, ins, 5, &N));
    HPL_CLOUD_CHECK(check_aligned4(op, {disp, dchange, flow}));
    HPL_REQUIRE(use_near == 0 || use_near == 1, "%s: use_near = %d (0 or 1)", op, use_near);
    HPL_REQUIRE(!use_near || !isnan(near_z), "%s: near must not be NaN", op);
    if (N == 0) return HPL_OK;
    FrArgs a{};
    int64_t blocks = 0;
    fill_common(a, batch, width, prefix, out_pc1, out1_ld, out_pc2, out2_ld, pixel, counts, workspace, &blocks);
    a.disp = disp; a.dchange = dchange; a.flow2 = flow; a.occ1 = occ1; a.occ2 = occ2;
    a.nf = (float)(-(double)f); a.cx = cx; a.cy = cy; a.use_near = use_near; a.near_z = near_z;
    return launch<FORM_FT3D>(op, a, blocks, stream);
}

// ---------------------------------------------------------------------------------------------- PNG row filters (host only)
extern "C" int hpl_png_unfilter(uint8_t *rows, int64_t height, int64_t stride, int bpp) {
    const char *const op = "hpl_png_unfilter";
    HPL_REQUIRE(height >= 0 && stride >= 1 && bpp >= 1 && bpp <= 8, "%s: height %lld, stride %lld, bpp %d (height >= 0, stride >= 1, bpp 1 .. 8)",
                op, (long long)height, (long long)stride, bpp);
    HPL_REQUIRE(rows || height == 0, "%s: null pointer", op);
    const int64_t n = stride - 1;                // data bytes of a row
    for (int64_t y = 0; y < height; ++y) {
        uint8_t *cur = rows + y * stride + 1;
        const uint8_t *up = y > 0 ? cur - stride : nullptr;
        const int filter = cur[-1];
        HPL_REQUIRE(filter <= 4, "%s: row %lld has filter type %d (0 .. 4)", op, (long long)y, filter);
        for (int64_t x = 0; x < n && filter != 0; ++x) {
            const int a = x >= bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
            int pred;
            if (filter == 1) pred = a;
            else if (filter == 2) pred = b;
            else if (filter == 3) pred = (a + b) >> 1;
            else {
                const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
                pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
            }
            cur[x] = (uint8_t)(cur[x] + pred);
        }
    }
    return HPL_OK;
}
