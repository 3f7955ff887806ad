// cov_book.hpp -- the bookkeeping of the device-resident covariance P and of its square-root factor S (P = S S^T), free of HIP.
//
// Both live in double-buffered pairs: an edit reads the resident buffer and writes the spare one, then the two change roles on the
// host.  S is fac_n x fac_k with leading dimension fac_ld (S(i, j) = d_Sres[j * fac_ld + i]), its last fac_tail columns zero in the
// rows >= 15.  Every edit of P decides the same three things -- does the factor follow (fac_valid && fac_n == res_n), which buffers
// change roles, what the new dimension is -- and each decision has ONE home here, a member function per edit.  The handle derives
// from CovBook; tests/cpp/test_cov_book.cpp asserts every transition on the CPU.  An edit that launches something returns a CovEdit:
// the pointers as they stood BEFORE the roles changed, so the launch may go out later than the bookkeeping (the step call).
#pragma once
#include <utility>

namespace orcvio_amd {

struct CovEdit {
    const double* P = nullptr;   // the covariance the edit reads [n][n]
    double* Pout = nullptr;      // the buffer it writes [m][m] (change of anchors: scratch, P itself is edited in place)
    const double* S = nullptr;   // the factor it reads (leading dimension ld_in)
    double* Sout = nullptr;      // the buffer the factor's edit writes (leading dimension ld_out)
    int n = 0, m = 0, fac_k = 0, ld_in = 0, ld_out = 0;
    bool fac = false;            // the factor follows: its launch goes out too
};

enum class FacAfter { adopt, drop, leave };   // what an update's commit does to the factor (CovBook::commit_update)

struct CovBook {
    double *d_Pres = nullptr, *d_Ptmp = nullptr;   // resident covariance, spare
    double *d_Sres = nullptr, *d_Stmp = nullptr;   // resident square-root factor, spare
    int res_n = 0;                                 // dimension of the resident covariance (0 = none)
    int fac_n = 0, fac_k = 0, fac_ld = 0, fac_tail = 0;
    bool fac_valid = false;

    static int ld_for(int m) { return (m + 16) / 16 * 16; }   // round_up(m + 1, 16)
    bool fac_follows() const { return fac_valid && fac_n == res_n; }

    // the factor a launch wrote into the spare buffer becomes the resident one (the ONE place the two factor buffers change roles)
    void fac_adopt(int n, int k, int ld, int tail) {
        std::swap(d_Sres, d_Stmp);
        fac_n = n; fac_k = k; fac_ld = ld; fac_tail = tail; fac_valid = true;
    }

    void set(int n) { res_n = n; fac_valid = false; }   // a new covariance in d_Pres: its factor is not known
    // P_LL <- Phi P_LL Phi^T + Q: the factor of the sum is not a row operation on S
    CovEdit propagate() { CovEdit e = edit(res_n, fac_ld); e.fac = false; swap_P(res_n); fac_valid = false; return e; }
    // a clone enters: its rows of S are copies of the IMU's (theta, p) rows, which are not zero in the trailing columns (tail 0)
    CovEdit augment() { const CovEdit e = edit(res_n + 6, ld_for(res_n + 6)); swap_P(e.m); follow(e, 0); return e; }
    // m of the states stay in their order (clones or features removed): rows of S deleted
    CovEdit gather(int m) { const CovEdit e = edit(m, ld_for(m)); swap_P(m); follow(e, fac_tail); return e; }
    // a symmetric permutation (clones to nuisance): rows of S moved
    CovEdit permute() { const CovEdit e = edit(res_n, fac_ld); swap_P(res_n); follow(e, fac_tail); return e; }
    // P <- T P T^T in place, S <- T S in place (T touches rows >= 15 only: fac_tail stays); a factor of another dimension is dropped
    CovEdit change_anchors() { const CovEdit e = edit(res_n, fac_ld); if (!e.fac) fac_valid = false; return e; }
    // an update's commit with entering features wrote the augmented covariance [nt][nt] into the spare buffer
    void commit_new_features(int nt) { swap_P(nt); fac_valid = false; }
    // ... with the factor carried along: S_aug = [[S+, 0], [-HH S+, sigma R^-1]] has the k columns of the update's S+ = sigma Z^T and
    // k_new more, one per new state.  It follows exactly when the update's own commit would adopt S+ (f) and the widened factor
    // fits the factor buffers (cols_max^2 doubles: k + k_new <= cols_max columns of ld_for(nt) <= cols_max) -- asked BEFORE the
    // launches, which write the spare factor buffer only then
    static bool new_features_fac_follows(FacAfter f, int k, int k_new, int cols_max) { return f == FacAfter::adopt && k + k_new <= cols_max; }
    // P roles change to nt; the factor is adopted with k + k_new columns, ld_for(nt), tail 0 (the new columns are not zero in the
    // rows >= 15), or dropped.  A refused call (singular H_2) does not come here: nothing changes
    void commit_new_features_fac(int nt, int k, int k_new, bool follows) {
        swap_P(nt);
        if (follows) fac_adopt(nt, k + k_new, ld_for(nt), 0); else fac_valid = false;
    }
    // P = L L^T has been factored into the spare factor buffer (the caller asks fac_follows() first) with leading dimension
    // ld_for(res_n); reversed: the rows >= 15 are zero in the last 15 columns
    void prefactor(bool reversed) { fac_adopt(res_n, res_n, ld_for(res_n), reversed ? 15 : 0); }
    // zero-velocity update: S+ by k_zupt_fac only without nuisance states and with at most kmax columns (tail 0: the rows >= 15 are
    // no longer zero in the trailing columns)
    CovEdit zupt(bool no_nuisance, int kmax) {
        CovEdit e = edit(res_n, fac_ld);
        e.fac = e.fac && no_nuisance && fac_k <= kmax;
        swap_P(res_n); follow(e, 0);
        return e;
    }
    // ... refused on the device: the spare buffers took bit copies of the prior and of its factor, whose trailing columns are still zero
    void zupt_refused(int tail_before) { if (fac_valid) fac_tail = tail_before; }
    // the zero-velocity update that writes only the m states that stay (the in-state features and the previous clone leave in the
    // same launch).  Whether it is applied is decided on the device and nothing is enqueued behind it before the wait, so this
    // changes NOTHING yet: the record goes to the launches and, with the outcome, to zupt_keep_done.  The factor follows by zupt's rule
    CovEdit zupt_keep(int m, bool no_nuisance, int kmax) const {
        CovEdit e = edit(m, ld_for(m));
        e.fac = e.fac && no_nuisance && fac_k <= kmax;
        return e;
    }
    // ... its outcome.  Applied: the P buffers change roles at m, the factor is adopted at (m, fac_k, ld_for(m), tail 0) or dropped.
    // Not applied (refused on the device, rejected by the check in front, or an outcome nobody could fetch): the spare buffers took
    // bit copies or nothing certain, the resident ones were only read -- no buffer changes roles, the factor's shape, validity and
    // fac_tail are the prior's, as cov_zupt leaves them
    void zupt_keep_done(const CovEdit& e, bool applied) {
        if (!applied) return;
        swap_P(e.m); follow(e, 0);
    }
    // the step call's fused frame head: propagation, augmentation and the removal of d_lost feature states in ONE launch, so the P
    // buffers change roles once (the separate edits: three times)
    CovEdit head(bool propagated, bool augmented, int d_lost) {
        CovEdit e = edit(res_n + (augmented ? 6 : 0) - d_lost, 0);
        e.ld_out = ld_for(e.m);
        if (propagated) e.fac = false;
        swap_P(e.m); follow(e, augmented ? 0 : fac_tail);
        return e;
    }
    // the commit of an update of dimension n whose factor S+ = sigma Z^T (k columns, leading dimension ld) stands in the spare factor
    // buffer; P_in_spare: P+ was written into the spare covariance buffer (otherwise into d_Pres itself)
    void commit_update(int n, int k, int ld, int tail, bool P_in_spare, FacAfter f) {
        if (P_in_spare) std::swap(d_Pres, d_Ptmp);
        if (f == FacAfter::adopt) fac_adopt(n, k, ld, tail);
        else if (f == FacAfter::drop) fac_valid = false;
        res_n = n;
    }
    // ... whose commit dropped the factor (FacAfter::drop, the direct form of a thin stack writes none) but refused itself on the device
    // (the step call's held-back prune update): the factor `before` that commit stands untouched where it was -- buffers, shape and
    // validity are `before`'s again if its factor followed; the covariance's buffers and dimension stay as the commit left them
    void keep_factor_of(const CovBook& before) {
        if (!before.fac_follows()) return;
        d_Sres = before.d_Sres; d_Stmp = before.d_Stmp;
        fac_n = before.fac_n; fac_k = before.fac_k; fac_ld = before.fac_ld; fac_tail = before.fac_tail; fac_valid = true;
    }

private:
    CovEdit edit(int m, int ld_out) const { return CovEdit{d_Pres, d_Ptmp, d_Sres, d_Stmp, res_n, m, fac_k, fac_ld, ld_out, fac_follows()}; }
    void swap_P(int m) { std::swap(d_Pres, d_Ptmp); res_n = m; }
    void follow(const CovEdit& e, int tail) { if (e.fac) fac_adopt(e.m, fac_k, e.ld_out, tail); else fac_valid = false; }
};

}  // namespace orcvio_amd
