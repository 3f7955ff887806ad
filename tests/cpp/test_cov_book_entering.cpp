// The bookkeeping of features entering the state WITH the square-root factor carried along (orcvio_amd/csrc/host/cov_book.hpp:
// new_features_fac_follows, commit_new_features_fac), built with -fsanitize=address,undefined by tests/test_cov_book_entering.py.
// Every transition: the factor follows, it does not fit, the update's commit would not keep it, no factor stood before, a refused
// call (nothing changed), and the chain of a frame behind it.  The expected values are written out here; none is computed by the
// code under test.  No device, no library.
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
static bool fac_gone(const CovBook& b) { return !b.fac_valid && b.d_Sres == C && b.d_Stmp == D; }
static bool same(const CovBook& a, const CovBook& b) {
    return a.d_Pres == b.d_Pres && a.d_Ptmp == b.d_Ptmp && a.d_Sres == b.d_Sres && a.d_Stmp == b.d_Stmp && a.res_n == b.res_n && a.fac_n == b.fac_n &&
           a.fac_k == b.fac_k && a.fac_ld == b.fac_ld && a.fac_tail == b.fac_tail && a.fac_valid == b.fac_valid;
}

// n states, the update's factor has kf columns, sz new states; nt = n + sz, ld_t = round_up(nt + 1, 16); cols = the factor buffers' columns
struct Row { int n, kf, sz, nt, ld_t, cols; bool fits; };
static const Row rows[] = {
    {70, 70, 18, 88, 96, 304, true},     // kf == n
    {70, 64, 6, 76, 80, 304, true},      // kf < n: a factor that came through an augmentation
    {64, 70, 1, 65, 80, 304, true},      // kf > n: through a marginalisation; sz = 1
    {46, 46, 1, 47, 48, 304, true},      // nt = 47 = 15 (mod 16): ld = nt + 1
    {45, 45, 3, 48, 64, 304, true},      // nt = 48 = 0 (mod 16): ld jumps to nt + 16
    {220, 200, 60, 280, 288, 304, true}, // sz = 60
    {244, 244, 60, 304, 320, 304, true}, // kf + sz == cols: the last that fits
    {245, 245, 60, 305, 320, 304, false},// kf + sz == cols + 1
    {100, 290, 18, 118, 128, 304, false},// a wide factor on a small state
};

static int decision() {
    for (const Row& r : rows) {
        CHECK(CovBook::new_features_fac_follows(FacAfter::adopt, r.kf, r.sz, r.cols) == r.fits);
        CHECK(!CovBook::new_features_fac_follows(FacAfter::drop, r.kf, r.sz, r.cols));    // Schmidt states, the thin direct form
        CHECK(!CovBook::new_features_fac_follows(FacAfter::leave, r.kf, r.sz, r.cols));   // ORCVIO_OPT_RESIDENT_FACTOR off
        CHECK(CovBook::ld_for(r.nt) == r.ld_t);
    }
    return 0;
}

static int transitions() {
    for (const Row& r : rows)
        for (int tail : {15, 0})
            for (Factor f : {RIGHT, OTHER, NONE}) {   // what stood BEFORE does not matter: the update's own S+ is what is widened
                const int ld = CovBook::ld_for(r.n);
                {   // follows: P swapped to nt, the factor buffers swapped, kf + sz columns, ld_for(nt), tail 0
                    CovBook b = start(r.n, f, r.kf, ld, tail);
                    b.commit_new_features_fac(r.nt, r.kf, r.sz, true);
                    CHECK(cov_is(b, B, A, r.nt));
                    CHECK(fac_is(b, D, C, r.nt, r.kf + r.sz, r.ld_t, 0));
                    CHECK(b.fac_follows());
                }
                {   // does not follow (does not fit, or the commit would not keep S+): P swapped, the factor dropped, its buffers keep their roles
                    CovBook b = start(r.n, f, r.kf, ld, tail);
                    b.commit_new_features_fac(r.nt, r.kf, r.sz, false);
                    CHECK(cov_is(b, B, A, r.nt) && fac_gone(b));
                    CHECK(!b.fac_follows());
                    // ... which is what the call without the factor leaves
                    CovBook c = start(r.n, f, r.kf, ld, tail);
                    c.commit_new_features(r.nt);
                    CHECK(same(b, c));
                }
                {   // refused (capacity, no entering features, singular H_2): the call returns before the bookkeeping -- asking is free of effects
                    const CovBook before = start(r.n, f, r.kf, ld, tail);
                    CovBook b = before;
                    (void)CovBook::new_features_fac_follows(FacAfter::adopt, r.kf, r.sz, r.cols);
                    CHECK(same(b, before));
                }
            }
    return 0;
}

// A frame of the hybrid filter on the resident covariance: prefactor, first update committed with entering features, the second
// update's commit, the oldest clone marginalised.  n = 70 (leg 22, 8 clones), 2 features of width 3.
static int chain() {
    CovBook b = start(70, NONE, 0, 0, 0);
    b.prefactor(true);
    CHECK(cov_is(b, A, B, 70) && fac_is(b, D, C, 70, 70, 80, 15));
    b.commit_new_features_fac(76, 70, 6, true);            // S+ = sigma Z^T has the prior factor's 70 columns
    CHECK(cov_is(b, B, A, 76) && fac_is(b, C, D, 76, 76, 80, 0));
    b.commit_update(76, 76, 80, 0, false, FacAfter::adopt);   // the second update read the 76-column factor: kf = 76
    CHECK(cov_is(b, B, A, 76) && fac_is(b, D, C, 76, 76, 80, 0));
    b.gather(70);
    CHECK(cov_is(b, A, B, 70) && fac_is(b, C, D, 70, 76, 80, 0));
    b.commit_new_features_fac(73, 76, 3, true);            // the next frame: kf > n
    CHECK(cov_is(b, B, A, 73) && fac_is(b, D, C, 73, 79, 80, 0));
    b.commit_new_features_fac(76, 79, 3, false);           // ... and one that is dropped
    CHECK(cov_is(b, A, B, 76) && !b.fac_valid && b.d_Sres == D && b.d_Stmp == C);
    return 0;
}

int main() {
    if (decision()) return 1;
    if (transitions()) return 1;
    if (chain()) return 1;
    std::printf("cov book entering ok\n");
    return 0;
}
