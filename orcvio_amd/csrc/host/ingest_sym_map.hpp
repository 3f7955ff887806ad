// ingest_sym_map.hpp -- which entries of a symmetric prior P (n x n, row-major, FP64) cross the link when the device pulls it out of
// the pinned arena, and where each of them lands in HBM, in plain C++ that compiles for the host and for the device (the guard
// pattern of clone_choice_model.hpp).  k_ingest_sym (io_ops.hpp), the copying calls' staging (capi_update.inc: stage_prior) and
// tests/cpp/test_ingest_sym_map.cpp compile this one source.
//
// P is symmetric by contract (include/orcvio_msckf.h).  With T = 16 (the tile of the factorisations) row i travels as its contiguous
// suffix [T floor(i/T), n): the diagonal T x T tile whole, both triangles as the caller wrote them, and everything to the right of it.
// A fetched P[i][j] is stored to (i, j) and, when it lies to the right of the diagonal tile (j >= T (floor(i/T) + 1)), also to (j, i).
// Every element of the n x n image is written exactly once: (i, j) comes from the caller's (i, j) where tile(j) >= tile(i) and from
// the caller's (j, i) where tile(j) < tile(i).
//
// The unit of transfer is 16 bytes = two doubles.  A row starts at byte 8 i n and a suffix 128 floor(i/T) bytes into it, so the units
// are aligned, and rows end on a unit, exactly when n is even.  An ODD n (possible with extra states) takes the linear pull of the
// whole matrix: ingest_sym_ok is the one predicate for the kernel's launcher and the staging, and the only fallback case.
//
// Lanes: one per 16-byte unit of the WHOLE image, row by row (n / 2 per row); the lanes of a row's prefix are masked (they fetch and
// store nothing).  The lane count equals the linear pull's, so one round of loads covers the matrix as before.
#pragma once

#if defined(__HIPCC__)
#define ORC_ISM_HD __host__ __device__ inline
#else
#define ORC_ISM_HD inline
#endif

#include <stddef.h>

namespace orcvio_amd {

enum { INGEST_SYM_TILE = 16 };

// the trapezoid form applies: n even (and a matrix at all)
ORC_ISM_HD bool ingest_sym_ok(int n) { return n >= 2 && (n & 1) == 0; }
// first column of row i that travels, and how many do
ORC_ISM_HD int ingest_sym_seg_start(int i) { return i - i % INGEST_SYM_TILE; }
ORC_ISM_HD int ingest_sym_seg_len(int n, int i) { return n - ingest_sym_seg_start(i); }
// is a fetched (i, j), j >= ingest_sym_seg_start(i), stored to (j, i) as well?
ORC_ISM_HD bool ingest_sym_mirrored(int i, int j) { return j >= ingest_sym_seg_start(i) + INGEST_SYM_TILE; }
// lanes of one pull (masked ones included)
ORC_ISM_HD unsigned ingest_sym_lanes(int n) { return (unsigned)n * (unsigned)(n / 2); }
// lane -> the unit (i, j), (i, j + 1) it moves; false: a masked lane (the unit lies in the row's prefix)
ORC_ISM_HD bool ingest_sym_unit(int n, unsigned lane, int* i, int* j) {
    const unsigned upr = (unsigned)(n / 2);
    const unsigned r = lane / upr, u = lane - r * upr;
    *i = (int)r;
    *j = (int)(2u * u);
    return *j >= ingest_sym_seg_start((int)r);
}
// where the image's (i, j) comes from in the caller's matrix
ORC_ISM_HD void ingest_sym_source(int i, int j, int* si, int* sj) {
    const bool upper = j / INGEST_SYM_TILE >= i / INGEST_SYM_TILE;
    *si = upper ? i : j;
    *sj = upper ? j : i;
}
// bytes that cross the link: 8 sum_i (n - T floor(i/T))
ORC_ISM_HD size_t ingest_sym_fetched_bytes(int n) {
    size_t b = 0;
    for (int i = 0; i < n; ++i) b += sizeof(double) * (size_t)ingest_sym_seg_len(n, i);
    return b;
}

}  // namespace orcvio_amd
