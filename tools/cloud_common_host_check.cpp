// Host-only check of csrc/cloud_common.h for a sanitizer build: the pair search against a linear scan, the Jacobi
// eigen-solver on symmetric 3x3 and 4x4 matrices, and the shared argument checks with fake addresses.  No device is needed.
// Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/cloud_common_host_check.cpp -o /tmp/cloud_common_host_check && /tmp/cloud_common_host_check
#include "../hplflownet_amd/csrc/cloud_common.h"

#include <string.h>

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links no library source)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace hpl

using namespace hpl;

static int failures = 0;

static void expect(bool ok, const char *what) {
    if (!ok) {
        ++failures;
        printf("FAILED: %s (last error: %s)\n", what, g_err);
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                      // xorshift64*: a fixed stream
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// group_of against a linear scan: every batch 1 .. 64, empty groups at the front, in the middle and at the back, every x
static void check_group_of() {
    for (int batch = 1; batch <= CLOUD_MAX_BATCH; ++batch)
        for (int rep = 0; rep < 8; ++rep) {
            int32_t prefix[CLOUD_MAX_BATCH + 1] = {0};
            const int front = rep & 1 ? (int)(rnd() % (unsigned)batch) : 0, back = rep & 2 ? (int)(rnd() % (unsigned)batch) : 0;
            for (int b = 0; b < batch; ++b) {
                int n = (int)(rnd() % 7u);
                if (rep & 4 && rnd() % 3u == 0) n = 0;                   // holes in the middle
                if (b < front || b >= batch - back) n = 0;
                prefix[b + 1] = prefix[b] + n;
            }
            for (int x = 0; x < prefix[batch]; ++x) {
                int want = 0;
                for (int b = 0; b < batch; ++b)
                    if (prefix[b] <= x) want = b;                        // the last group that starts at or before x
                const int got = group_of(prefix, batch, x);
                expect(got == want && prefix[got] <= x && x < prefix[got + 1], "group_of equals the linear scan");
            }
        }
}

// |A V - V diag| and |V^T V - I| (largest entry) <= 1e-13 |A|_F: 12 sweeps of a float64 Jacobi on at most 4x4 leave the
// off-diagonal weight below 1e-16 |A|_F (the stop rule) or converged quadratically far below it, and each of the at most 72
// rotations adds a few ulps (2.2e-16) of |A| to the residual and of 1 to the orthonormality: 72 * 4 * 2.2e-16 < 1e-13.
template <int N>
static void check_eigen(const double (&A0)[N][N], const char *what, bool finite) {
    double A[N][N], V[N][N];
    memcpy(A, A0, sizeof A);
    jacobi_eigen(A, V, 12);                  // (returning at all is the termination check)
    if (!finite) return;
    double norm = 0.0;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) norm += A0[i][j] * A0[i][j];
    norm = sqrt(norm);
    double res = 0.0, orth = 0.0;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            double av = 0.0, vv = 0.0;
            for (int k = 0; k < N; ++k) {
                av += A0[i][k] * V[k][j];
                vv += V[k][i] * V[k][j];
            }
            res = fmax(res, fabs(av - V[i][j] * A[j][j]));
            orth = fmax(orth, fabs(vv - (i == j ? 1.0 : 0.0)));
        }
    expect(res <= 1e-13 * norm && orth <= 1e-13, what);
}

static void check_jacobi() {
    const double z3[3][3] = {}, z4[4][4] = {};
    check_eigen(z3, "zero 3x3", true);
    check_eigen(z4, "zero 4x4", true);
    const double d3[3][3] = {{3, 0, 0}, {0, -1, 0}, {0, 0, 2}}, d4[4][4] = {{1, 0, 0, 0}, {0, 5, 0, 0}, {0, 0, -2, 0}, {0, 0, 0, 5}};
    check_eigen(d3, "diagonal 3x3", true);
    check_eigen(d4, "diagonal 4x4", true);
    const double r3[3][3] = {{2, 1, 1}, {1, 2, 1}, {1, 1, 2}};           // eigenvalues 1, 1, 4
    const double r4[4][4] = {{3, 1, 1, 1}, {1, 3, 1, 1}, {1, 1, 3, 1}, {1, 1, 1, 3}};     // 2, 2, 2, 6
    check_eigen(r3, "repeated eigenvalue 3x3", true);
    check_eigen(r4, "repeated eigenvalue 4x4", true);
    for (int rep = 0; rep < 200; ++rep) {
        double a3[3][3], a4[4][4];
        const double scale = rep % 3 == 0 ? 1e-9 : rep % 3 == 1 ? 1.0 : 1e12;
        for (int i = 0; i < 4; ++i)
            for (int j = i; j < 4; ++j) {
                const double v = scale * ((double)rnd() / 2147483648.0 - 1.0);
                a4[i][j] = a4[j][i] = v;
                if (j < 3) a3[i][j] = a3[j][i] = v;
            }
        check_eigen(a3, "random symmetric 3x3", true);
        check_eigen(a4, "random symmetric 4x4", true);
    }
    double n3[3][3] = {{2, 1, 1}, {1, 2, 1}, {1, 1, 2}}, n4[4][4] = {{3, 1, 1, 1}, {1, 3, 1, 1}, {1, 1, 3, 1}, {1, 1, 1, 3}};
    n3[0][1] = n3[1][0] = NAN;
    n4[2][2] = NAN;
    check_eigen(n3, "NaN 3x3", false);
    check_eigen(n4, "NaN 4x4", false);
    n4[2][2] = INFINITY;
    check_eigen(n4, "inf 4x4", false);
}

static void check_arguments() {
    const char *const op = "hpl_host_check";
    auto refused = [op](int rc) { return rc == HPL_EINVAL && strncmp(g_err, op, strlen(op)) == 0; };
    expect(refused(check_batch(op, 0)) && refused(check_batch(op, 65)) && refused(check_batch(op, -1)), "batch out of range");
    expect(check_batch(op, 1) == HPL_OK && check_batch(op, 64) == HPL_OK, "batch in range");

    int64_t p[66] = {0, 5, 5, 9};
    expect(check_prefix(op, "the prefix", "pair", p, 3) == HPL_OK, "a prefix with an empty pair");
    p[0] = 1;
    expect(refused(check_prefix(op, "the prefix", "pair", p, 3)) && strstr(g_err, "the prefix must start at 0"), "prefix from 1");
    p[0] = 0;
    p[2] = 4;
    expect(refused(check_prefix(op, "the prefix of pc1", "cloud", p, 3)) && strstr(g_err, "the prefix of pc1 decreases at cloud 1"),
           "prefix decreases");

    expect(check_points(op, 0) == HPL_OK && check_points(op, CLOUD_MAX_POINTS - 1) == HPL_OK, "points in range");
    expect(refused(check_points(op, CLOUD_MAX_POINTS)) && refused(check_points(op, (int64_t)1 << 60)), "points out of range");
    expect(3 * (CLOUD_MAX_POINTS - 1) < ((int64_t)1 << 31) && 3 * CLOUD_MAX_POINTS >= ((int64_t)1 << 31), "the point limit is 2^31 / 3");

    expect(check_row_stride(op, 100, 100) == HPL_OK && check_row_stride(op, 0, 0) == HPL_OK, "row stride");
    expect(refused(check_row_stride(op, 99, 100)), "short row stride");

    expect(check_flow_strides(op, 100, 1, 100) == HPL_OK && check_flow_strides(op, 1, 3, 100) == HPL_OK &&
               check_flow_strides(op, 1, 1, 1) == HPL_OK && check_flow_strides(op, 1, 1, 0) == HPL_OK &&
               check_flow_strides(op, 7, 40, 100) == HPL_OK, "flow strides that keep the elements apart");
    expect(refused(check_flow_strides(op, 0, 3, 100)) && refused(check_flow_strides(op, 1, 0, 100)) &&
               refused(check_flow_strides(op, 50, 1, 100)) && refused(check_flow_strides(op, 1, 2, 100)) &&
               refused(check_flow_strides(op, -1, 3, 100)), "flow strides that overlap");

    const void *const a = (const void *)0x10000, *const odd = (const void *)0x10002;
    expect(check_aligned4(op, {a, nullptr, (const void *)0x10004}) == HPL_OK, "aligned arrays, one absent");
    expect(refused(check_aligned4(op, {a, odd})) && refused(check_aligned4(op, {(const void *)0x10001})), "misaligned array");

    expect(check_workspace(op, (const void *)0x100000, 256, 4096, 4096) == HPL_OK &&
               check_workspace(op, (const void *)0x100008, 8, 4096, 0) == HPL_OK, "workspace");
    expect(refused(check_workspace(op, (const void *)0x100000, 256, 4095, 4096)), "short workspace");
    expect(refused(check_workspace(op, (const void *)0x100080, 256, 4096, 4096)) &&
               refused(check_workspace(op, (const void *)0x100004, 8, 4096, 4096)), "misaligned workspace");

    // the narrowed prefixes: empty pairs own no workgroup
    const int64_t q[5] = {0, 0, 1025, 1025, 3000};
    int32_t pp[CLOUD_MAX_BATCH + 1], bp[CLOUD_MAX_BATCH + 1];
    expect(narrow_prefix(q, 4, 1024, pp, bp) == 4 && pp[0] == 0 && pp[2] == 1025 && pp[4] == 3000 && bp[0] == 0 && bp[1] == 0 &&
               bp[2] == 2 && bp[3] == 2 && bp[4] == 4, "narrow_prefix with a workgroup prefix");
    memset(pp, -1, sizeof pp);
    expect(narrow_prefix(q, 4, 256, pp, nullptr) == 13 && pp[1] == 0 && pp[3] == 1025 && pp[4] == 3000 && pp[5] == -1,
           "narrow_prefix without one");
    for (int blk = 0; blk < 4; ++blk) expect(group_of(bp, 4, blk) == (blk < 2 ? 1 : 3), "workgroups of the non-empty pairs");

    expect(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512, "align256");
    expect(count_bits(0) == 1 && count_bits(1) == 1 && count_bits(2) == 2 && count_bits(255) == 8 && count_bits(256) == 9, "count_bits");
    Carver c;
    expect(c.take(1) == 0 && c.take(256) == 256 && c.take(0) == 512 && c.take(300) == 512 && c.bytes == 1024, "Carver");
    const uint32_t keys[6] = {1, 1, 4, 4, 4, 9};
    expect(lower_bound(keys, 6, 0u) == 0 && lower_bound(keys, 6, 1u) == 0 && lower_bound(keys, 6, 2u) == 2 &&
               lower_bound(keys, 6, 4u) == 2 && lower_bound(keys, 6, 9u) == 5 && lower_bound(keys, 6, 10u) == 6 &&
               lower_bound(keys, 0, 4u) == 0, "lower_bound");
}

int main() {
    check_group_of();
    check_jacobi();
    check_arguments();
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
