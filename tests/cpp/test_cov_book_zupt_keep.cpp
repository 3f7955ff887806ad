// The bookkeeping of the fused zero-velocity update that writes only what stays (orcvio_amd/csrc/host/cov_book.hpp: zupt_keep,
// zupt_keep_done), built with -fsanitize=address,undefined by tests/test_cov_book_zupt_keep.py.  Every transition: applied with
// the factor following and without, a factor too wide for the reflectors, nuisance states, not applied (everything the prior's, its
// tail too), F = 0, the buffers never aliasing -- and the outcome equal to the separate edits' (gather, zupt, gather).  The
// expected values are written out here; none is computed by the code under test.  No device, no library.
#include <cstdio>

#include "../../orcvio_amd/csrc/host/cov_book.hpp"

using namespace orcvio_amd;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static double A[1], B[1], C[1], D[1];   // A / B the covariance pair, C / D the factor pair (only their addresses are used)

enum Factor { RIGHT, OTHER, NONE };
static CovBook start(int n, Factor f, int k, int ld, int tail) {
    CovBook b;
    b.d_Pres = A; b.d_Ptmp = B; b.d_Sres = C; b.d_Stmp = D;
    b.res_n = n; b.fac_n = f == OTHER ? n + 6 : n; b.fac_k = k; b.fac_ld = ld; b.fac_tail = tail; b.fac_valid = f != NONE;
    return b;
}
static bool cov_is(const CovBook& b, const double* res, const double* tmp, int n) { return b.d_Pres == res && b.d_Ptmp == tmp && b.res_n == n; }
static bool fac_is(const CovBook& b, const double* res, const double* tmp, int n, int k, int ld, int tail) {
    return b.fac_valid && b.d_Sres == res && b.d_Stmp == tmp && b.fac_n == n && b.fac_k == k && b.fac_ld == ld && b.fac_tail == tail;
}
static bool same(const CovBook& a, const CovBook& b) {
    return a.d_Pres == b.d_Pres && a.d_Ptmp == b.d_Ptmp && a.d_Sres == b.d_Sres && a.d_Stmp == b.d_Stmp && a.res_n == b.res_n && a.fac_n == b.fac_n &&
           a.fac_k == b.fac_k && a.fac_ld == b.fac_ld && a.fac_tail == b.fac_tail && a.fac_valid == b.fac_valid;
}
static bool apart(const CovBook& b) { return b.d_Pres != b.d_Ptmp && b.d_Sres != b.d_Stmp && b.d_Pres && b.d_Ptmp && b.d_Sres && b.d_Stmp; }

// n resident states, b = leg + 6 N of them no features, m kept, the factor's columns; ld_n / ld_m = round_up(. + 1, 16)
struct Row { int n, b, m, k, ld_n, ld_m; };
static const Row rows[] = {
    {35, 34, 28, 35, 48, 32},      // the smallest window, the previous clone leaves too
    {35, 34, 34, 29, 48, 48},      // ... stays; a factor that came through an augmentation (k < n)
    {64, 64, 58, 64, 80, 64},      // F = 0
    {64, 64, 64, 64, 80, 80},      // F = 0 and nothing marginalised: m == n
    {65, 64, 58, 71, 80, 64},      // k > n
    {64, 34, 28, 64, 80, 32},
    {232, 142, 136, 232, 240, 144},
    {232, 142, 136, 448, 240, 144},// k == kmax: the last the reflectors hold
};

static int transitions() {
    const int kmax = 448;
    for (const Row& r : rows)
        for (int tail : {15, 0})
            for (Factor f : {RIGHT, OTHER, NONE}) {
                const CovBook before = start(r.n, f, r.k, r.ld_n, tail);
                CHECK(CovBook::ld_for(r.n) == r.ld_n && CovBook::ld_for(r.m) == r.ld_m);
                {   // the record: what the launches read and write, and NOTHING changed by asking
                    CovBook b = before;
                    const CovEdit e = b.zupt_keep(r.m, true, kmax);
                    CHECK(same(b, before));
                    CHECK(e.P == A && e.Pout == B && e.S == C && e.Sout == D);
                    CHECK(e.n == r.n && e.m == r.m && e.fac_k == r.k && e.ld_in == r.ld_n && e.ld_out == r.ld_m);
                    CHECK(e.fac == (f == RIGHT));
                }
                {   // applied: P swapped to m; the factor adopted at (m, k, ld_for(m), tail 0) when it followed, dropped otherwise
                    CovBook b = before;
                    const CovEdit e = b.zupt_keep(r.m, true, kmax);
                    b.zupt_keep_done(e, true);
                    CHECK(cov_is(b, B, A, r.m) && apart(b));
                    if (f == RIGHT) CHECK(fac_is(b, D, C, r.m, r.k, r.ld_m, 0) && b.fac_follows());
                    else CHECK(!b.fac_valid && b.d_Sres == C && b.d_Stmp == D);
                    // ... the state the separate edits reach: the features leave, the update, the previous clone leaves (their
                    // buffers have changed roles three times, not once: shape, validity and tail are compared)
                    CovBook c = before;
                    if (r.b < r.n) c.gather(r.b);
                    c.zupt(true, kmax);
                    if (r.m < r.b) c.gather(r.m);
                    CHECK(c.res_n == b.res_n && c.fac_valid == b.fac_valid);
                    if (b.fac_valid) CHECK(c.fac_n == b.fac_n && c.fac_k == b.fac_k && c.fac_ld == b.fac_ld && c.fac_tail == b.fac_tail);
                }
                {   // applied with nuisance states declared, or a factor wider than the reflectors hold: the factor is dropped
                    CovBook b = before;
                    const CovEdit e = b.zupt_keep(r.m, false, kmax);
                    CHECK(!e.fac);
                    b.zupt_keep_done(e, true);
                    CHECK(cov_is(b, B, A, r.m) && !b.fac_valid && apart(b));
                    CovBook w = before;
                    const CovEdit ew = w.zupt_keep(r.m, true, r.k - 1);   // fac_k > kmax
                    CHECK(!ew.fac);
                    w.zupt_keep_done(ew, true);
                    CHECK(cov_is(w, B, A, r.m) && !w.fac_valid && w.d_Sres == C && w.d_Stmp == D);
                    CovBook x = before;
                    const CovEdit ex = x.zupt_keep(r.m, true, r.k);       // fac_k == kmax
                    CHECK(ex.fac == (f == RIGHT));
                }
                {   // not applied: no buffer changes roles, dimension, factor shape, validity and the prior's tail stand
                    CovBook b = before;
                    const CovEdit e = b.zupt_keep(r.m, true, kmax);
                    b.zupt_keep_done(e, false);
                    CHECK(same(b, before) && apart(b));
                    CHECK(cov_is(b, A, B, r.n));
                    if (f != NONE) CHECK(fac_is(b, C, D, f == OTHER ? r.n + 6 : r.n, r.k, r.ld_n, tail));
                }
            }
    return 0;
}

// A parked platform: prefactor, a frame refused on the device, then two applied frames (each: augment, the fused update)
static int chain() {
    CovBook b = start(64, NONE, 0, 0, 0);   // leg 22, 6 clones, 6 feature states
    b.prefactor(true);
    CHECK(cov_is(b, A, B, 64) && fac_is(b, D, C, 64, 64, 80, 15));
    b.augment();
    CHECK(cov_is(b, B, A, 70) && fac_is(b, C, D, 70, 64, 80, 0));
    CovEdit e = b.zupt_keep(58, true, 448);
    CHECK(e.P == B && e.Pout == A && e.S == C && e.Sout == D && e.fac);
    b.zupt_keep_done(e, false);
    CHECK(cov_is(b, B, A, 70) && fac_is(b, C, D, 70, 64, 80, 0));
    e = b.zupt_keep(58, true, 448);
    b.zupt_keep_done(e, true);
    CHECK(cov_is(b, A, B, 58) && fac_is(b, D, C, 58, 64, 64, 0));
    b.augment();
    CHECK(cov_is(b, B, A, 64) && fac_is(b, C, D, 64, 64, 80, 0));
    e = b.zupt_keep(58, true, 448);         // F = 0 now
    b.zupt_keep_done(e, true);
    CHECK(cov_is(b, A, B, 58) && fac_is(b, D, C, 58, 64, 64, 0) && apart(b));
    return 0;
}

int main() {
    if (transitions()) return 1;
    if (chain()) return 1;
    std::printf("cov book zupt keep ok\n");
    return 0;
}
