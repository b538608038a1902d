// Host-only check of csrc/grid_common.h for a sanitizer build: the key's packing, its order and its limits, the float64 cell
// of a point at the ends of the range, and the room helpers of the radix sort.  No device is needed.
// Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/grid_common_host_check.cpp -o /tmp/grid_common_host_check && /tmp/grid_common_host_check
#include "../hplflownet_amd/csrc/grid_common.h"

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
        printf("FAILED: %s\n", what);
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                      // xorshift64*: a fixed stream
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Fields {
    int b, c[3];
};

static Fields random_fields() {              // one field in four at an end of its range
    Fields f;
    f.b = rnd() % 4u == 0 ? (rnd() & 1 ? 0 : CLOUD_MAX_BATCH - 1) : (int)(rnd() % (unsigned)CLOUD_MAX_BATCH);
    for (int k = 0; k < 3; ++k) f.c[k] = rnd() % 4u == 0 ? (rnd() & 1 ? 0 : GRID_CELL_MASK) : (int)(rnd() & (unsigned)GRID_CELL_MASK);
    return f;
}

static int lexicographic(const Fields &p, const Fields &q) {
    if (p.b != q.b) return p.b < q.b ? -1 : 1;
    for (int k = 0; k < 3; ++k)
        if (p.c[k] != q.c[k]) return p.c[k] < q.c[k] ? -1 : 1;
    return 0;
}

static bool round_trips(const Fields &f) {
    int c[3];
    const u64 key = grid_key(f.b, f.c[0], f.c[1], f.c[2]);
    grid_cell(key, c);
    return grid_group(key) == f.b && c[0] == f.c[0] && c[1] == f.c[1] && c[2] == f.c[2];
}

static void check_key() {
    expect(GRID_CELL_BITS == 19 && GRID_CELL_BIAS == 1 << 18 && GRID_CELL_MASK == (1 << 19) - 1 && GRID_CELL_MAX == 262142.0 &&
               GRID_KEY_BITS == 57, "the constants");
    // a group below 64 leaves the top bit of the key clear: the key of all ones is nobody's, and no key + 1 wraps
    expect(count_bits(CLOUD_MAX_BATCH - 1) + GRID_KEY_BITS < 64, "the group digit fits above the cells");
    const Fields ends[4] = {{0, {0, 0, 0}}, {CLOUD_MAX_BATCH - 1, {GRID_CELL_MASK, GRID_CELL_MASK, GRID_CELL_MASK}},
                            {0, {GRID_CELL_MASK, 0, GRID_CELL_MASK}}, {CLOUD_MAX_BATCH - 1, {0, GRID_CELL_MASK, 0}}};
    for (const Fields &f : ends) expect(round_trips(f), "pack and unpack at the extremes");
    expect(grid_key(0, 0, 0, 0) == 0 && grid_key(1, 0, 0, 0) == (u64)1 << 57 && grid_key(0, 1, 0, 0) == (u64)1 << 38 &&
               grid_key(0, 0, 1, 0) == (u64)1 << 19 && grid_key(0, 0, 0, 1) == 1, "the fields' places");
    for (int rep = 0; rep < 200000; ++rep) {
        const Fields p = random_fields(), q = rep % 8 == 0 ? p : random_fields();
        expect(round_trips(p), "pack and unpack of random fields");
        const u64 kp = grid_key(p.b, p.c[0], p.c[1], p.c[2]), kq = grid_key(q.b, q.c[0], q.c[1], q.c[2]);
        const int want = lexicographic(p, q), got = kp < kq ? -1 : (kp > kq ? 1 : 0);
        expect(want == got, "the order of the keys is the lexicographic order of (b, cx, cy, cz)");
        expect(kp != ~0ull, "no key of a group below 64 is all ones");
    }
}

// cells at +-GRID_CELL_MAX: the 27 neighbours' fields stay inside 19 bits and inside group b, a biased cell never has a
// field of all ones (voxel_grid's "no cell"), and the 9 runs' bounds [klo, khi + 1) do not wrap
static void check_neighbours() {
    const int lo = GRID_CELL_BIAS - (int)GRID_CELL_MAX, hi = GRID_CELL_BIAS + (int)GRID_CELL_MAX;
    expect(lo == 2 && hi == GRID_CELL_MASK - 1, "the biased range is 2 .. 2^19 - 2");
    const int ends[2] = {lo, hi};
    for (int b : {0, 1, 31, CLOUD_MAX_BATCH - 1})
        for (int e = 0; e < 8; ++e) {
            const int c[3] = {ends[e & 1], ends[(e >> 1) & 1], ends[(e >> 2) & 1]};
            for (int d = 0; d < 27; ++d) {
                const Fields f = {b, {c[0] + d / 9 - 1, c[1] + d / 3 % 3 - 1, c[2] + d % 3 - 1}};
                bool inside = true;
                for (int k = 0; k < 3; ++k) inside = inside && f.c[k] >= 0 && f.c[k] <= GRID_CELL_MASK;
                expect(inside, "a neighbour's field stays inside 19 bits");
                expect(round_trips(f), "a neighbour's key stays inside group b");
            }
            for (int k = 0; k < 9; ++k) {
                const u64 klo = grid_key(b, c[0] + k / 3 - 1, c[1] + k % 3 - 1, c[2] - 1);
                const u64 khi = grid_key(b, c[0] + k / 3 - 1, c[1] + k % 3 - 1, c[2] + 1) + 1;
                expect(klo < khi && khi > grid_key(b, c[0] + k / 3 - 1, c[1] + k % 3 - 1, c[2] + 1) && khi <= grid_key(b + 1, 0, 0, 0),
                       "a run's bounds: first key below the key behind its last, no wrap, nothing of group b + 1");
            }
        }
}

// the largest float32 x with floor(x * inv) <= GRID_CELL_MAX, found by walking the floats from the real bound
static float last_inside(double inv) {
    float x = (float)((GRID_CELL_MAX + 1.0) / inv);
    while (floor((double)x * inv) > GRID_CELL_MAX) x = nextafterf(x, 0.f);
    while (floor((double)nextafterf(x, INFINITY) * inv) <= GRID_CELL_MAX) x = nextafterf(x, INFINITY);
    return x;
}

// the smallest (most negative) float32 x with floor(x * inv) >= -GRID_CELL_MAX
static float first_inside(double inv) {
    float x = (float)(-GRID_CELL_MAX / inv);
    while (floor((double)x * inv) < -GRID_CELL_MAX) x = nextafterf(x, 0.f);
    while (floor((double)nextafterf(x, -INFINITY) * inv) >= -GRID_CELL_MAX) x = nextafterf(x, -INFINITY);
    return x;
}

static void check_cell() {
    const double invs[4] = {1.0 / (GRID_CELL_MARGIN * 1.0), 1.0 / (GRID_CELL_MARGIN * 0.05), 1.0 / (GRID_CELL_MARGIN * 37.5), 1.0 / 0.1};
    for (double inv : invs) {
        int c[3] = {-1, -1, -1};
        expect(grid_cell_of(inv, 0.f, -0.f, 0.f, c) && c[0] == GRID_CELL_BIAS && c[1] == GRID_CELL_BIAS && c[2] == GRID_CELL_BIAS,
               "+-0 lies in the cell of the bias");
        const float tiny = -1e-30f;
        expect(grid_cell_of(inv, tiny, 0.f, 0.f, c) && c[0] == GRID_CELL_BIAS - 1, "a point just below 0 lies one cell down");
        const float bad[3] = {NAN, INFINITY, -INFINITY};
        for (float v : bad)
            for (int k = 0; k < 3; ++k) {
                float p[3] = {1.f, 2.f, 3.f};
                p[k] = v;
                expect(!grid_cell_of(inv, p[0], p[1], p[2], c), "a non-finite coordinate has no cell");
            }
        const float top = last_inside(inv), bottom = first_inside(inv);
        for (int k = 0; k < 3; ++k) {
            float p[3] = {0.f, 0.f, 0.f};
            p[k] = top;
            expect(grid_cell_of(inv, p[0], p[1], p[2], c) && c[k] == GRID_CELL_BIAS + (int)GRID_CELL_MAX && c[k] == GRID_CELL_MASK - 1,
                   "the last coordinate inside the range, upwards");
            p[k] = nextafterf(top, INFINITY);
            expect(!grid_cell_of(inv, p[0], p[1], p[2], c), "the first coordinate outside the range, upwards");
            p[k] = bottom;
            expect(grid_cell_of(inv, p[0], p[1], p[2], c) && c[k] == GRID_CELL_BIAS - (int)GRID_CELL_MAX && c[k] == 2,
                   "the last coordinate inside the range, downwards");
            p[k] = nextafterf(bottom, -INFINITY);
            expect(!grid_cell_of(inv, p[0], p[1], p[2], c), "the first coordinate outside the range, downwards");
        }
        expect(!grid_cell_of(inv, 3.0e38f, 0.f, 0.f, c) && !grid_cell_of(inv, 0.f, 0.f, -3.0e38f, c), "the largest floats have no cell");
    }
}

// The room helpers over one size query: 256-aligned and never below the query at n itself.  room_next_pow2 also covers the
// next power of two; room_all_pow2 covers that too and does not decrease over the sizes.  (room_next_pow2 makes no such
// promise and does not keep it: with the rocPRIM this was written against, which asks for nothing at 1025 and at 2048 pairs, its
// room is 256 bytes at 1024 pairs and 0 at 1025.  The sizes it gives are part of what callers cache, so it stays as it is.)
template <class TempBytes>
static void check_room(TempBytes temp_bytes, const char *what) {
    const int64_t sizes[8] = {0, 1, 255, 1024, 1025, 8193, 450000, (int64_t)1 << 27};
    int64_t last = 0;
    for (int64_t n : sizes) {
        int64_t cap = 1024;
        while (cap < n) cap <<= 1;
        const int64_t next = room_next_pow2(n, temp_bytes), all = room_all_pow2(n, temp_bytes);
        const int64_t ask = (int64_t)temp_bytes(n), ask_cap = (int64_t)temp_bytes(cap);
        const bool ok = next % 256 == 0 && all % 256 == 0 && next >= ask && next >= ask_cap && all >= next && all >= last;
        if (!ok)
            printf("n = %lld: room_next_pow2 %lld, room_all_pow2 %lld after %lld; the query asks for %lld, and %lld at %lld\n",
                   (long long)n, (long long)next, (long long)all, (long long)last, (long long)ask, (long long)ask_cap, (long long)cap);
        expect(ok, what);
        last = all;
    }
}

static void check_rooms() {
    check_room([](int64_t n) { return radix_temp_bytes<u64, GridRec>(n, 64u); }, "room of the (key, record) sort");
    check_room([](int64_t n) { return radix_temp_bytes<u64, int32_t>(n, 64u); }, "room of the (key, index) sort");
    check_room([](int64_t n) { return radix_temp_bytes<uint32_t, int32_t>(n, 32u); }, "room of the (object, index) sort");
    expect(sizeof(GridRec) == 16 && alignof(GridRec) == 16, "the record is 16 bytes, aligned to 16");
}

int main() {
    check_key();
    check_neighbours();
    check_cell();
    check_rooms();
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
