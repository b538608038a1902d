// transforms.hip -- the data transforms of one pair on the device (hpl_transform_pair): the reference's Augmentation /
// ProcessData (transforms/transforms.py:494-640) in front of the lattice build.
//
// Per point the reference's operations in its order: bias = shift + jitter1, a = p1.m + bias, b = p2.m + bias,
// b = b.m2^T + shift2, sf = b - a, b += jitter2 (unless NO_CORR); then the depth cut on the transformed clouds and the
// sampling.  numpy's float32 (M, 3) x (3, 3) product computes column c as fma(z, m[2][c], fma(y, m[1][c], x * m[0][c])):
// that chain is written with explicit fmaf (the library builds with -ffp-contract=off, nothing else is fused), so with the
// same draws the device gives the reference's bits.
//
// The random stream is our own, counter-based: Philox4x32-10 keyed by the 64-bit seed, counter (point index, call lo, call
// hi, purpose) -- purpose 0 / 1 the jitter of the clouds (Box-Muller on the four words, in fp64, three normals a point), 2 / 3
// the selection keys of cloud 1 / cloud 2.  A point's draws are a function of its index, so a kernel recomputes a point's
// transform wherever it needs it: nothing per point is stored but the flags and the selection keys.
//
// Sampling without replacement: every valid point gets a 63-bit key; the chosen set is the k smallest (key, index) pairs in
// ascending key order -- a uniformly random ordered k-subset, what rng.choice(replace=False) gives.  The (key, index) order
// is a stable LSD radix sort (rocPRIM) of the keys with the indices as values, invalid points keyed above every valid one.
// The valid points in index order (allow_less_points, num_points <= 0) are a rocPRIM select of the flags.  Which of the two
// is emitted, and how many, is decided on the device from the valid count: one enqueue, no host round trip.
#include "common.h"
#include "philox.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

using namespace hpl;

namespace {

constexpr int TT = 256;
constexpr unsigned long long INVALID_KEY = ~0ull;        // above every 63-bit key

// (Philox4x32-10 itself: philox.h)
__device__ inline u4 draw(const hpl_transform_params &P, int64_t i, uint32_t purpose) {
    return philox4x32_10(u4{(uint32_t)i, (uint32_t)P.counter, (uint32_t)(P.counter >> 32), purpose},
                         (uint32_t)P.seed, (uint32_t)(P.seed >> 32));
}

__device__ inline unsigned long long sel_key(const hpl_transform_params &P, int64_t i, uint32_t purpose) {
    const u4 w = draw(P, i, purpose);
    return (((unsigned long long)w.x << 32) | w.y) >> 1;
}

// clip(sigma * N(0, 1), -clip, clip) -> float32 for three components: Box-Muller in fp64 on uniforms (w + 1) / 2^32 in (0, 1]
// and w / 2^32 in [0, 1).  clip == 0: exactly -0 (x + -0 == x for every x, so the jitter changes nothing, as the reference's ±0).
__device__ inline void jitter(const hpl_transform_params &P, int64_t i, uint32_t purpose, double sigma, double clip,
                              const float *hook, float j[3]) {
    if (hook) {
        j[0] = hook[i * 3]; j[1] = hook[i * 3 + 1]; j[2] = hook[i * 3 + 2];
        return;
    }
    if (clip == 0.0) {
        j[0] = j[1] = j[2] = -0.0f;
        return;
    }
    const u4 w = draw(P, i, purpose);
    const double s32 = 2.3283064365386963e-10;          // 2^-32
    const double twopi = 6.283185307179586;
    const double r0 = sqrt(-2.0 * log(((double)w.x + 1.0) * s32)), t0 = twopi * ((double)w.y * s32);
    const double r1 = sqrt(-2.0 * log(((double)w.z + 1.0) * s32)), t1 = twopi * ((double)w.w * s32);
    const double n[3] = {r0 * cos(t0), r0 * sin(t0), r1 * cos(t1)};
#pragma unroll
    for (int c = 0; c < 3; ++c) j[c] = (float)fmin(fmax(sigma * n[c], -clip), clip);
}

// column c of p . m (m row-major 3 x 3): numpy's float32 chain
__device__ inline float dot_col(float x, float y, float z, const float *m, int c) {
    return fmaf(z, m[6 + c], fmaf(y, m[3 + c], x * m[c]));
}

// The transformed point i: a (cloud 1), b (cloud 2, after its jitter) and sf (before it).
__device__ inline void transform_point(const hpl_transform_params &P, const float *__restrict__ p1, const float *__restrict__ p2,
                                       const float *j1h, const float *j2h, int64_t i, float a[3], float b[3], float sf[3]) {
    const float x1 = p1[i * 3], y1 = p1[i * 3 + 1], z1 = p1[i * 3 + 2];
    const float x2 = p2[i * 3], y2 = p2[i * 3 + 1], z2 = p2[i * 3 + 2];
    if (!P.augment) {
        a[0] = x1; a[1] = y1; a[2] = z1;
        b[0] = x2; b[1] = y2; b[2] = z2;
#pragma unroll
        for (int c = 0; c < 3; ++c) sf[c] = b[c] - a[c];
        return;
    }
    float j[3], t[3];
    jitter(P, i, 0, P.jitter_sigma1, P.jitter_clip1, j1h, j);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float bias = P.shift[c] + j[c];
        a[c] = dot_col(x1, y1, z1, P.m, c) + bias;
        t[c] = dot_col(x2, y2, z2, P.m, c) + bias;
    }
    // b . m2^T: column c of m2^T is row c of m2
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = fmaf(t[2], P.m2[c * 3 + 2], fmaf(t[1], P.m2[c * 3 + 1], t[0] * P.m2[c * 3])) + P.shift2[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) sf[c] = b[c] - a[c];
    if (!P.no_corr) {
        jitter(P, i, 1, P.jitter_sigma2, P.jitter_clip2, j2h, j);
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] += j[c];
    }
}

// Pass 1: valid flag of every point (the depth cut) and, when the sampling is random, its selection key(s).
__global__ void __launch_bounds__(TT) k_tf_flags(const hpl_transform_params *__restrict__ Pp, const float *__restrict__ p1,
                                                 const float *__restrict__ p2, const float *j1h, const float *j2h, int64_t M,
                                                 uint8_t *__restrict__ flags, unsigned long long *__restrict__ key1,
                                                 unsigned long long *__restrict__ key2, int32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= M) return;
    const hpl_transform_params P = *Pp;
    float a[3], b[3], sf[3];
    transform_point(P, p1, p2, j1h, j2h, i, a, b, sf);
    const float T = P.depth_threshold;
    const bool valid = !(T > 0.0f) || (a[2] < T && b[2] < T);
    flags[i] = valid ? 1 : 0;
    if (key1) {
        key1[i] = valid ? sel_key(P, i, 2) : INVALID_KEY;
        vals[i] = (int32_t)i;
        if (key2) key2[i] = valid ? sel_key(P, i, 3) : INVALID_KEY;
    }
}

// Pass 2: decide the mode from the valid count, publish (valid, emitted), write the emitted rows as (3, emitted) SoA.
__global__ void __launch_bounds__(TT) k_tf_emit(const hpl_transform_params *__restrict__ Pp, const float *__restrict__ p1,
                                                const float *__restrict__ p2, const float *j1h, const float *j2h, int64_t M,
                                                const int32_t *__restrict__ valid_count, const int32_t *__restrict__ compact,
                                                const int32_t *__restrict__ sorted1, const int32_t *__restrict__ sorted2,
                                                const int32_t *__restrict__ sel1, const int32_t *__restrict__ sel2, int64_t n_sel,
                                                int64_t capacity, float *__restrict__ o1, float *__restrict__ o2,
                                                float *__restrict__ osf, int32_t *__restrict__ counts) {
    const hpl_transform_params P = *Pp;
    const int64_t V = *valid_count;
    // 0: rejected, 1: the k smallest keys, 2: every valid point in index order, 3: the test hook's indices
    int mode;
    int64_t k;
    if (V == 0) { mode = 0; k = 0; }                                           // the reference: len(indices) == 0 -> None
    else if (sel1) { mode = 3; k = n_sel; }
    else if (P.num_points <= 0) { mode = 2; k = V; }
    else if (V >= P.num_points) { mode = 1; k = P.num_points; }
    else if (P.allow_less_points) { mode = 2; k = V; }
    else { mode = 0; k = 0; }
    if (k > capacity) { mode = 0; k = 0; }                                     // excluded by the host's checks
    const int64_t j = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (j == 0) { counts[0] = (int32_t)V; counts[1] = (int32_t)k; }
    if (j >= k) return;
    int64_t i1, i2;
    if (mode == 1) { i1 = sorted1[j]; i2 = P.no_corr ? sorted2[j] : i1; }
    else if (mode == 2) { i1 = i2 = compact[j]; }
    else { i1 = sel1[j]; i2 = P.no_corr ? sel2[j] : i1; }
    float a[3], b[3], sf[3];
    const float nan = __builtin_nanf("");
    if (i1 >= 0 && i1 < M) {
        transform_point(P, p1, p2, j1h, j2h, i1, a, b, sf);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = sf[c] = nan;                          // a bad hook index reads nothing
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { o1[c * k + j] = a[c]; osf[c * k + j] = sf[c]; }
    if (i2 != i1) {
        if (i2 >= 0 && i2 < M) transform_point(P, p1, p2, j1h, j2h, i2, a, b, sf);
        else b[0] = b[1] = b[2] = nan;
    } else if (!(i1 >= 0 && i1 < M)) {
        b[0] = b[1] = b[2] = nan;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o2[c * k + j] = b[c];
}

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

size_t temp_bytes(int64_t M) {
    size_t sort = 0, sel = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                    (const int32_t *)nullptr, (int32_t *)nullptr, (unsigned)M, 0, 64, (hipStream_t) nullptr);
    (void)rocprim::select(nullptr, sel, rocprim::counting_iterator<int32_t>(0), (const uint8_t *)nullptr, (int32_t *)nullptr,
                          (int32_t *)nullptr, (size_t)M, (hipStream_t) nullptr);
    return sort > sel ? sort : sel;
}

// workspace: params | valid count | flags | compact | key1 | key2 | sorted keys | vals | sorted1 | sorted2 | rocPRIM temporaries
struct Layout {
    hpl_transform_params *params;
    int32_t *count, *compact, *vals, *sorted1, *sorted2;
    uint8_t *flags;
    unsigned long long *key1, *key2, *kout;
    void *temp;
    int64_t bytes;
    Layout(char *p, int64_t M) {
        char *b = p;
        params = reinterpret_cast<hpl_transform_params *>(p); p += align256(sizeof(hpl_transform_params));
        count = reinterpret_cast<int32_t *>(p); p += 256;
        flags = reinterpret_cast<uint8_t *>(p); p += align256(M);
        compact = reinterpret_cast<int32_t *>(p); p += align256(M * 4);
        key1 = reinterpret_cast<unsigned long long *>(p); p += align256(M * 8);
        key2 = reinterpret_cast<unsigned long long *>(p); p += align256(M * 8);
        kout = reinterpret_cast<unsigned long long *>(p); p += align256(M * 8);
        vals = reinterpret_cast<int32_t *>(p); p += align256(M * 4);
        sorted1 = reinterpret_cast<int32_t *>(p); p += align256(M * 4);
        sorted2 = reinterpret_cast<int32_t *>(p); p += align256(M * 4);
        temp = p; p += align256((int64_t)temp_bytes(M));
        bytes = p - b;
    }
};

}  // namespace

extern "C" int64_t hpl_transform_workspace_bytes(int64_t M) {
    if (M < 1 || M >= (int64_t)INT32_MAX) return 0;
    return Layout(nullptr, M).bytes;
}

extern "C" int hpl_transform_capacity(int64_t M, int num_points, int64_t *capacity) {
    HPL_REQUIRE(capacity, "hpl_transform_capacity: null argument");
    HPL_REQUIRE(M >= 1 && M < (int64_t)INT32_MAX, "hpl_transform_capacity: %lld points (1 .. 2^31 - 2)", (long long)M);
    *capacity = num_points > 0 ? imin(num_points, M) : M;
    return HPL_OK;
}

extern "C" int hpl_transform_pair(const float *pc1, const float *pc2, int64_t M, const hpl_transform_params *params,
                                  const float *jitter1, const float *jitter2, const int32_t *sel1, const int32_t *sel2,
                                  int64_t n_sel, float *out_pc1, float *out_pc2, float *out_sf, int64_t capacity,
                                  int32_t *counts, void *workspace, int64_t workspace_bytes, hplStream stream) {
    HPL_REQUIRE(pc1 && pc2 && params && out_pc1 && out_pc2 && out_sf && counts && workspace,
                "hpl_transform_pair: null argument");
    HPL_REQUIRE(M >= 1 && M < (int64_t)INT32_MAX, "hpl_transform_pair: %lld points (1 .. 2^31 - 2)", (long long)M);
    const uintptr_t mis = reinterpret_cast<uintptr_t>(pc1) | reinterpret_cast<uintptr_t>(pc2) |
                          reinterpret_cast<uintptr_t>(out_pc1) | reinterpret_cast<uintptr_t>(out_pc2) |
                          reinterpret_cast<uintptr_t>(out_sf) | reinterpret_cast<uintptr_t>(counts) |
                          reinterpret_cast<uintptr_t>(jitter1) | reinterpret_cast<uintptr_t>(jitter2) |
                          reinterpret_cast<uintptr_t>(sel1) | reinterpret_cast<uintptr_t>(sel2);
    HPL_REQUIRE((mis & 3u) == 0, "hpl_transform_pair: every array must be 4-byte aligned");
    HPL_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "hpl_transform_pair: workspace must be 256-byte aligned");
    HPL_REQUIRE(workspace_bytes >= hpl_transform_workspace_bytes(M), "hpl_transform_pair: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)hpl_transform_workspace_bytes(M));
    const hpl_transform_params &H = *params;
    const int64_t need = H.num_points > 0 ? imin(H.num_points, M) : M;
    HPL_REQUIRE(capacity >= need, "hpl_transform_pair: capacity %lld below the %lld rows num_points = %d can emit",
                (long long)capacity, (long long)need, H.num_points);
    HPL_REQUIRE((sel1 == nullptr) == (sel2 == nullptr) || (sel1 && !H.no_corr),
                "hpl_transform_pair: sel2 without sel1, or NO_CORR with sel1 but no sel2");
    HPL_REQUIRE(!sel1 || (n_sel >= 1 && n_sel <= capacity), "hpl_transform_pair: %lld hook indices (1 .. capacity %lld)",
                (long long)n_sel, (long long)capacity);
    HPL_REQUIRE(!(H.jitter_clip1 < 0.0) && !(H.jitter_clip2 < 0.0), "hpl_transform_pair: negative jitter clip");

    hipStream_t s = to_stream(stream);
    Layout L(reinterpret_cast<char *>(workspace), M);
    if (hipMemcpyAsync(L.params, params, sizeof(hpl_transform_params), hipMemcpyHostToDevice, s) != hipSuccess) {
        set_error("hpl_transform_pair: parameter copy failed: %s", hipGetErrorString(hipGetLastError()));
        return HPL_EHIP;
    }
    const bool random = !sel1 && H.num_points > 0;        // keys are needed only when the k smallest may be emitted
    const int grid = (int)cdiv(M, TT);
    k_tf_flags<<<grid, TT, 0, s>>>(L.params, pc1, pc2, jitter1, jitter2, M, L.flags, random ? L.key1 : nullptr,
                                   random && H.no_corr ? L.key2 : nullptr, L.vals);
    HPL_CHECK_LAUNCH("hpl_transform_pair");
    size_t tb = temp_bytes(M);
    hipError_t e = rocprim::select(L.temp, tb, rocprim::counting_iterator<int32_t>(0), L.flags, L.compact, L.count, (size_t)M, s);
    if (e != hipSuccess) { set_error("hpl_transform_pair: select failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
    if (random) {
        for (int c = 0; c < (H.no_corr ? 2 : 1); ++c) {
            tb = temp_bytes(M);
            e = rocprim::radix_sort_pairs(L.temp, tb, c ? L.key2 : L.key1, L.kout, L.vals, c ? L.sorted2 : L.sorted1, (unsigned)M,
                                          0u, 64u, s);
            if (e != hipSuccess) { set_error("hpl_transform_pair: radix sort failed: %s", hipGetErrorString(e)); return HPL_EHIP; }
        }
    }
    k_tf_emit<<<(int)cdiv(capacity, TT), TT, 0, s>>>(L.params, pc1, pc2, jitter1, jitter2, M, L.count, L.compact, L.sorted1,
                                                     L.sorted2, sel1, sel2, n_sel, capacity, out_pc1, out_pc2, out_sf, counts);
    HPL_CHECK_LAUNCH("hpl_transform_pair");
    return HPL_OK;
}

extern "C" int hpl_philox4x32_10(const uint32_t *counter /* HOST, 4 */, const uint32_t *key /* HOST, 2 */, uint32_t *out /* HOST, 4 */) {
    HPL_REQUIRE(counter && key && out, "hpl_philox4x32_10: null argument");
    const u4 r = philox4x32_10(u4{counter[0], counter[1], counter[2], counter[3]}, key[0], key[1]);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
    return HPL_OK;
}
