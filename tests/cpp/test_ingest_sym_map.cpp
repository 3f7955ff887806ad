// Stand-alone program over host/ingest_sym_map.hpp (the arithmetic k_ingest_sym and the copying calls' staging run), built by
// tests/test_ingest_sym_map.py with -fsanitize=address,undefined.  For every n = 1 .. 260 it replays one pull lane by lane, exactly as
// the kernel does, on heap buffers of exactly n x n doubles (an index outside the matrix is the sanitizer's), and checks:
//   - the predicate refuses exactly the odd n (the documented fallback: the linear pull), and nothing else;
//   - every (i, j) of the image is written exactly once;
//   - the image's (i, j) is the caller's (i, j) where tile(j) >= tile(i), the caller's (j, i) elsewhere (tiles of 16);
//   - the fetched bytes are 8 sum_i (n - 16 floor(i / 16)), every fetched unit is 16-byte aligned, and lies inside what the staging's
//     row segments copy (everything else of the arena holds a poison value that must not reach the image).
// Prints "ingest sym map ok".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../orcvio_amd/csrc/host/ingest_sym_map.hpp"

using namespace orcvio_amd;

static int fail(const char* what, int n, int i, int j) { std::printf("FAILED: %s (n = %d, i = %d, j = %d)\n", what, n, i, j); return 1; }

static int one_size(int n) {
    const bool want_ok = n >= 2 && n % 2 == 0;
    if (ingest_sym_ok(n) != want_ok) return fail("predicate", n, 0, 0);
    if (!want_ok) return 0;
    const size_t nn = (size_t)n * n;
    const double poison = -7.0;
    // the caller's matrix: every entry its own value, NOT symmetric, so the source of every image entry can be read off
    std::vector<double> P(nn), arena(nn, poison), image(nn, 0.0);
    std::vector<int> writes(nn, 0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) P[(size_t)i * n + j] = 1000.0 * i + j + 1.0;
    // the staging's row segments
    size_t staged = 0;
    for (int i = 0; i < n; ++i) {
        const int s = ingest_sym_seg_start(i), len = ingest_sym_seg_len(n, i);
        if (s != 16 * (i / 16) || len != n - 16 * (i / 16)) return fail("row segment", n, i, s);
        std::memcpy(&arena[(size_t)i * n + s], &P[(size_t)i * n + s], sizeof(double) * (size_t)len);
        staged += sizeof(double) * (size_t)len;
    }
    // the pull, lane by lane
    size_t fetched = 0;
    const unsigned lanes = ingest_sym_lanes(n);
    if (lanes != (unsigned)(nn / 2)) return fail("lane count", n, 0, 0);
    for (unsigned lane = 0; lane < lanes; ++lane) {
        int i = -1, j = -1;
        const bool live = ingest_sym_unit(n, lane, &i, &j);
        if (i != (int)(lane / (unsigned)(n / 2)) || j != 2 * (int)(lane % (unsigned)(n / 2))) return fail("lane order", n, i, j);   // consecutive lanes along the row
        if (live != (j >= 16 * (i / 16))) return fail("mask", n, i, j);
        if (!live) continue;
        const size_t o = (size_t)i * n + j;
        if ((o * sizeof(double)) % 16 != 0) return fail("unit alignment", n, i, j);
        const double x = arena[o], y = arena[o + 1];
        fetched += 16;
        image[o] = x; image[o + 1] = y;
        writes[o]++; writes[o + 1]++;
        const bool m = ingest_sym_mirrored(i, j);
        if (m != ingest_sym_mirrored(i, j + 1)) return fail("unit straddles the diagonal tile's edge", n, i, j);
        if (m != (j / 16 > i / 16)) return fail("mirror predicate", n, i, j);
        if (m) {
            image[(size_t)j * n + i] = x; image[(size_t)(j + 1) * n + i] = y;
            writes[(size_t)j * n + i]++; writes[(size_t)(j + 1) * n + i]++;
        }
    }
    size_t want_bytes = 0;
    for (int i = 0; i < n; ++i) want_bytes += 8 * (size_t)(n - 16 * (i / 16));
    if (fetched != want_bytes || ingest_sym_fetched_bytes(n) != want_bytes || staged != want_bytes) return fail("fetched bytes", n, (int)fetched, (int)want_bytes);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (writes[(size_t)i * n + j] != 1) return fail("written exactly once", n, i, j);
            const bool upper = j / 16 >= i / 16;
            const int si = upper ? i : j, sj = upper ? j : i;
            int hi, hj;
            ingest_sym_source(i, j, &hi, &hj);
            if (hi != si || hj != sj) return fail("ingest_sym_source", n, i, j);
            if (image[(size_t)i * n + j] != P[(size_t)si * n + sj]) return fail("source of the image", n, i, j);
        }
    return 0;
}

int main() {
    int fallbacks = 0;
    for (int n = 1; n <= 260; ++n) {
        if (one_size(n)) return 1;
        fallbacks += ingest_sym_ok(n) ? 0 : 1;
    }
    if (fallbacks != 130) { std::printf("FAILED: %d sizes fall back, 130 odd ones expected\n", fallbacks); return 1; }
    if (ingest_sym_ok(0) || ingest_sym_ok(-2)) { std::printf("FAILED: predicate at n <= 0\n"); return 1; }
    if (ingest_sym_fetched_bytes(202) != 8u * 202 * 202 - 150528u) { std::printf("FAILED: bytes at n = 202\n"); return 1; }
    std::printf("ingest sym map ok\n");
    return 0;
}
