// The bookkeeping of the resident covariance and of its square-root factor (orcvio_amd/csrc/host/cov_book.hpp) on its own, built with
// -fsanitize=address,undefined by tests/test_cov_book.py.  Every edit's rule, from start states with a factor of the right dimension,
// of another dimension and with none, fac_tail 15 and 0.  The expected values are written out here; none is computed by the code under
// test.  No device, no library.
#include <cstdio>

#include "../../orcvio_amd/csrc/host/cov_book.hpp"

using namespace orcvio_amd;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static double A[1], B[1], C[1], D[1];   // the four buffers: A / B the covariance pair, C / D the factor pair (only their addresses are used)

enum Factor { RIGHT, OTHER, NONE };
// n states resident in A, spare B; the factor (k columns, leading dimension ld) in C, spare D
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
static bool fac_gone(const CovBook& b) { return !b.fac_valid && b.d_Sres == C && b.d_Stmp == D; }   // (an invalid factor: the buffers keep their roles)
static bool same(const CovBook& a, const CovBook& b) {
    return a.d_Pres == b.d_Pres && a.d_Ptmp == b.d_Ptmp && a.d_Sres == b.d_Sres && a.d_Stmp == b.d_Stmp && a.res_n == b.res_n && a.fac_n == b.fac_n &&
           a.fac_k == b.fac_k && a.fac_ld == b.fac_ld && a.fac_tail == b.fac_tail && a.fac_valid == b.fac_valid;
}
static bool same_ints(const CovBook& a, const CovBook& b) {
    return a.res_n == b.res_n && a.fac_valid == b.fac_valid && (!a.fac_valid || (a.fac_n == b.fac_n && a.fac_k == b.fac_k && a.fac_ld == b.fac_ld && a.fac_tail == b.fac_tail));
}
// the record of an edit: what it reads and writes, as the buffers stood BEFORE it
static bool rec_is(const CovEdit& e, int n, int m, int k, int ld_in, int ld_out, bool fac) {
    return e.P == A && e.Pout == B && e.S == C && e.Sout == D && e.n == n && e.m == m && e.fac_k == k && e.ld_in == ld_in && e.ld_out == ld_out && e.fac == fac;
}

// n: resident dimension; ld: round_up(n + 1, 16); ld_aug: round_up(n + 7, 16); m: what a gather keeps; ld_m: round_up(m + 1, 16)
struct Dim { int n, k, ld, ld_aug, m, ld_m; };
static const Dim dims[] = {
    {46, 43, 48, 64, 40, 48},   // leg 46, no clone
    {34, 34, 48, 48, 28, 32},   // leg 22, two clones
    {58, 41, 64, 80, 52, 64},   // n + 7 = 65: one past a multiple of 16
    {69, 69, 80, 80, 63, 64},   // m + 1 = 64: the multiple itself
    {70, 55, 80, 80, 64, 80},   // m + 1 = 65
};

static int rows_of_the_table() {
    for (const Dim& d : dims)
        for (int tail : {15, 0}) {
            const int n = d.n, k = d.k;
            for (Factor f : {RIGHT, OTHER, NONE}) {
                const bool fac = f == RIGHT;
                {   // set(n'): P not swapped, no factor
                    CovBook b = start(n, f, k, d.ld, tail);
                    b.set(n + 3);
                    CHECK(cov_is(b, A, B, n + 3) && fac_gone(b));
                }
                {   // propagate: P swapped, no factor
                    CovBook b = start(n, f, k, d.ld, tail);
                    const CovEdit e = b.propagate();
                    CHECK(cov_is(b, B, A, n) && fac_gone(b));
                    CHECK(e.P == A && e.Pout == B && e.n == n && e.m == n && !e.fac);
                }
                {   // augment: n + 6; the factor follows with tail 0
                    CovBook b = start(n, f, k, d.ld, tail);
                    const CovEdit e = b.augment();
                    CHECK(cov_is(b, B, A, n + 6));
                    CHECK(fac ? fac_is(b, D, C, n + 6, k, d.ld_aug, 0) : fac_gone(b));
                    CHECK(rec_is(e, n, n + 6, k, d.ld, d.ld_aug, fac));
                }
                {   // gather to m states: the factor follows, tail kept
                    CovBook b = start(n, f, k, d.ld, tail);
                    const CovEdit e = b.gather(d.m);
                    CHECK(cov_is(b, B, A, d.m));
                    CHECK(fac ? fac_is(b, D, C, d.m, k, d.ld_m, tail) : fac_gone(b));
                    CHECK(rec_is(e, n, d.m, k, d.ld, d.ld_m, fac));
                }
                {   // permute: the leading dimension and the tail kept
                    CovBook b = start(n, f, k, d.ld, tail);
                    const CovEdit e = b.permute();
                    CHECK(cov_is(b, B, A, n));
                    CHECK(fac ? fac_is(b, D, C, n, k, d.ld, tail) : fac_gone(b));
                    CHECK(rec_is(e, n, n, k, d.ld, d.ld, fac));
                }
                {   // change of anchors: in place; a valid factor of another dimension becomes invalid
                    CovBook b = start(n, f, k, d.ld, tail);
                    const CovEdit e = b.change_anchors();
                    CHECK(cov_is(b, A, B, n));
                    CHECK(fac ? fac_is(b, C, D, n, k, d.ld, tail) : fac_gone(b));
                    CHECK(rec_is(e, n, n, k, d.ld, d.ld, fac));
                }
                {   // commit with entering features (3 features of dimension 3: n + 9)
                    CovBook b = start(n, f, k, d.ld, tail);
                    b.commit_new_features(n + 9);
                    CHECK(cov_is(b, B, A, n + 9) && fac_gone(b));
                }
                if (!fac)   // prefactor (asked for only without a factor of this dimension): P untouched, S swapped, n columns
                    for (bool rev : {true, false}) {
                        CovBook b = start(n, f, k, d.ld, tail);
                        CHECK(!b.fac_follows());
                        b.prefactor(rev);
                        CHECK(cov_is(b, A, B, n) && fac_is(b, D, C, n, n, d.ld, rev ? 15 : 0));
                    }
                else { const CovBook b = start(n, f, k, d.ld, tail); CHECK(b.fac_follows()); }
                // zero-velocity update: the factor follows only without nuisance states and with at most kmax columns; tail 0
                for (int variant = 0; variant < 3; ++variant) {
                    const bool no_nui = variant != 1;
                    const int kmax = variant == 2 ? k - 1 : k;
                    const bool follows = fac && variant == 0;
                    CovBook b = start(n, f, k, d.ld, tail);
                    const CovEdit e = b.zupt(no_nui, kmax);
                    CHECK(cov_is(b, B, A, n));
                    CHECK(follows ? fac_is(b, D, C, n, k, d.ld, 0) : fac_gone(b));
                    CHECK(rec_is(e, n, n, k, d.ld, d.ld, follows));
                    // ... refused on the device: the tail is put back only if the factor is still valid
                    b.zupt_refused(follows ? tail : 7);
                    CHECK(follows ? fac_is(b, D, C, n, k, d.ld, tail) : (fac_gone(b) && b.fac_tail == tail));
                }
                // the fused frame head: P swapped ONCE; m = n + 6 aug - d_lost; a propagation drops the factor, an augmentation its tail
                for (int prop = 0; prop < 2; ++prop)
                    for (int aug = 0; aug < 2; ++aug)
                        for (int lost : {0, n - d.m}) {
                            if (aug && lost) continue;   // (m = n + 6 - lost has no row in dims: the chains below cover it)
                            const int m = aug ? n + 6 : (lost ? d.m : n), ld_m = aug ? d.ld_aug : (lost ? d.ld_m : d.ld);
                            CovBook b = start(n, f, k, d.ld, tail);
                            const CovEdit e = b.head(prop != 0, aug != 0, lost);
                            CHECK(cov_is(b, B, A, m));
                            CHECK(fac && !prop ? fac_is(b, D, C, m, k, ld_m, aug ? 0 : tail) : fac_gone(b));
                            CHECK(rec_is(e, n, m, k, d.ld, ld_m, fac && !prop));
                        }
                // an update's commit: P+ in the spare buffer or in place; the factor adopted, dropped or left
                for (bool spare : {true, false}) {
                    CovBook b = start(n, f, k, d.ld, tail);
                    b.commit_update(d.m, d.m - 15, d.ld_m, 15, spare, FacAfter::adopt);
                    CHECK(spare ? cov_is(b, B, A, d.m) : cov_is(b, A, B, d.m));
                    CHECK(fac_is(b, D, C, d.m, d.m - 15, d.ld_m, 15));
                    b = start(n, f, k, d.ld, tail);
                    b.commit_update(d.m, d.m - 15, d.ld_m, 15, spare, FacAfter::drop);
                    CHECK((spare ? cov_is(b, B, A, d.m) : cov_is(b, A, B, d.m)) && fac_gone(b));
                    b = start(n, f, k, d.ld, tail);
                    b.commit_update(n, n, d.ld, 0, spare, FacAfter::leave);
                    CHECK(spare ? cov_is(b, B, A, n) : cov_is(b, A, B, n));
                    CHECK(f == NONE ? fac_gone(b) : fac_is(b, C, D, f == OTHER ? n + 6 : n, k, d.ld, tail));
                    // a dropping commit that refused itself on the device (the held-back prune update): the factor of the snapshot in
                    // front of it is kept -- buffers, shape, validity -- if it followed; the covariance stays as the commit left it
                    const CovBook before = start(n, f, k, d.ld, tail);
                    b = before;
                    b.commit_update(n, n - 15, d.ld_m, 15, spare, FacAfter::drop);
                    b.d_Sres = D; b.d_Stmp = C; b.fac_n = 1; b.fac_k = 2; b.fac_ld = 3; b.fac_tail = 4;   // (whatever stood there: none of it may survive)
                    b.keep_factor_of(before);
                    CHECK(spare ? cov_is(b, B, A, n) : cov_is(b, A, B, n));
                    if (fac) CHECK(fac_is(b, C, D, n, k, d.ld, tail));
                    else CHECK(!b.fac_valid && b.d_Sres == D && b.d_Stmp == C && b.fac_n == 1 && b.fac_k == 2 && b.fac_ld == 3 && b.fac_tail == 4);   // nothing done
                }
                // save -> any edit -> restore gives back all ten fields
                const CovBook saved = start(n, f, k, d.ld, tail);
                for (int edit = 0; edit < 9; ++edit) {
                    CovBook b = saved;
                    switch (edit) {
                        case 0: b.set(n + 3); break;
                        case 1: b.propagate(); break;
                        case 2: b.augment(); break;
                        case 3: b.gather(d.m); break;
                        case 4: b.permute(); break;
                        case 5: b.change_anchors(); break;
                        case 6: b.zupt(true, k); break;
                        case 7: b.head(false, true, 0); break;
                        default: b.commit_update(d.m, d.m, d.ld_m, 15, true, FacAfter::adopt); break;
                    }
                    b = saved;
                    CHECK(same(b, start(n, f, k, d.ld, tail)));
                }
            }
        }
    return 0;
}

// One frame as separate edits and as the fused head: the same integer fields.  The head swaps the covariance buffers once, the
// separate edits once each: three edits leave them in the SAME roles as the head (three swaps against one), two edits in opposite roles.
// n = 49: leg 46, no clone, three in-state features of dimension 1; k = 49, ld = round_up(50, 16) = 64.
static int chains() {
    for (int tail : {15, 0})
        for (Factor f : {RIGHT, OTHER, NONE}) {
            const bool fac = f == RIGHT;
            {   // propagation + augmentation + one lost feature: m = 49 + 6 - 1 = 54; no factor behind a propagation
                CovBook sep = start(49, f, 49, 64, tail), one = sep;
                sep.propagate(); sep.augment(); sep.gather(54);
                one.head(true, true, 1);
                CHECK(cov_is(sep, B, A, 54) && fac_gone(sep));
                CHECK(cov_is(one, B, A, 54) && fac_gone(one));
                CHECK(same_ints(sep, one));
            }
            {   // propagation + augmentation: m = 55; two swaps against one
                CovBook sep = start(49, f, 49, 64, tail), one = sep;
                sep.propagate(); sep.augment();
                one.head(true, true, 0);
                CHECK(cov_is(sep, A, B, 55) && fac_gone(sep));
                CHECK(cov_is(one, B, A, 55) && fac_gone(one));
                CHECK(same_ints(sep, one));
            }
            {   // no propagation, augmentation + one lost feature: the factor follows, ld = round_up(55, 16) = 64, tail 0
                CovBook sep = start(49, f, 49, 64, tail), one = sep;
                sep.augment(); sep.gather(54);
                one.head(false, true, 1);
                CHECK(cov_is(sep, A, B, 54) && (fac ? fac_is(sep, C, D, 54, 49, 64, 0) : fac_gone(sep)));
                CHECK(cov_is(one, B, A, 54) && (fac ? fac_is(one, D, C, 54, 49, 64, 0) : fac_gone(one)));
                CHECK(same_ints(sep, one));
            }
            {   // no propagation, no augmentation, one lost feature: m = 48, ld = round_up(49, 16) = 64, the tail kept
                CovBook sep = start(49, f, 49, 64, tail), one = sep;
                sep.gather(48);
                one.head(false, false, 1);
                CHECK(cov_is(sep, B, A, 48) && (fac ? fac_is(sep, D, C, 48, 49, 64, tail) : fac_gone(sep)));
                CHECK(same(sep, one));
            }
            {   // a zero-velocity frame: augmentation, update, the previous clone removed (n = 34 -> 40 -> 34), then the refusal
                CovBook b = start(34, f, 34, 48, tail);
                b.augment();
                const int tail_before = b.fac_tail;
                b.zupt(true, 64); b.gather(34);
                b.zupt_refused(tail_before);
                CHECK(cov_is(b, B, A, 34) && (fac ? fac_is(b, D, C, 34, 34, 48, 0) : fac_gone(b)));   // (the augmentation had set tail 0)
                CovBook c = start(34, f, 34, 48, tail);   // ... without the augmentation the tail comes back
                c.zupt(true, 64); c.gather(28);
                c.zupt_refused(tail);
                CHECK(cov_is(c, A, B, 28) && (fac ? fac_is(c, C, D, 28, 34, 32, tail) : fac_gone(c)));
            }
        }
    return 0;
}

int main() {
    if (rows_of_the_table()) return 1;
    if (chains()) return 1;
    std::printf("cov book ok\n");
    return 0;
}
