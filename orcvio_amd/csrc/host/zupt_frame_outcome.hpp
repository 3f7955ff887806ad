// zupt_frame_outcome.hpp -- what the five zero-velocity calls on the resident covariance (orcvio_msckf_cov_zupt, _cov_zupt_frame,
// _cov_zupt_frame_hybrid, _cov_zupt_frame_checked, _cov_zupt_frame_checked_hybrid; capi_zupt.inc zupt_frame_run) plan before their
// launches and report behind their one wait: ONE plan and ONE outcome table, free of HIP and of the handle.
// tests/cpp/test_zupt_frame_outcome.cpp enumerates the table against a transcription of the five bodies it replaced.
//
// The plan (zupt_plan), by form:
//                    n_dx           bookkeeping   marginalisation            the update's `also`
//   update           n              deferred      none                       none
//   frame            n              eager         before the wait            imu_status when the handle is armed
//   frame_hybrid     leg + 6 N      deferred      inside the update launch   imu_status when the handle is armed
//   checked          n              eager         behind the wait, applied   zchk_status
//   checked_hybrid   leg + 6 N      deferred      inside the update launch   zchk_status
//   n: the dimension the update sees (resident + 6 with the augmentation).  eager: CovBook::zupt changes the roles when the update is
//   enqueued; deferred: CovBook::zupt_keep hands out the record, zupt_keep_done changes the roles with the outcome.  A checked form with
//   fewer than two selected samples has no check and no update: propagation, augmentation, one wait on the armed launch's status.
//
// The rows (zupt_frame_outcome), in the order they are tried (NOT_SPD = ORCVIO_ERR_NOT_SPD, the refusal of the device):
//   1. the head failed (hipSetDevice, the armed launch, propagation, augmentation): that code; nothing written, no bookkeeping.
//      From here on the checked forms write applied = 0 and n_after = n; rows 2-5 leave them so.
//   2. no update (checked, S < 2): the wait's code; else NOT_SPD "no propagation" when the armed launch refused Phi / Q; else OK.
//   3. the check's enqueue failed: that code.
//   4. the update's enqueue failed: that code; eager bookkeeping is restored.
//   5. the marginalisation before the wait or the wait failed: that code; bookkeeping by form (difference a below).
//      From here on applied = (status word == 0) is written by every form, n_after by every frame form (difference d).
//   6. applied: OK; deferred bookkeeping changes the roles now; checked: the marginalisation goes out now (zupt_frame_outcome_marg
//      takes its code: failed, the call returns it and n_after stays n).
//   7. not applied, unchecked forms: NOT_SPD; the message names the armed launch when it refused Phi / Q, else the update.
//   8. not applied, checked forms: the verdict's code when it was not evaluated; OK without a message when the check rejected (the
//      caller goes on with the moving frame); NOT_SPD when the check accepted and the update refused itself.
//      Rows 7, 8: eager bookkeeping gets the prior's fac_tail back (zupt_refused); deferred bookkeeping has changed nothing.
//
// Where the forms differ (kept as they were, each a row above; DESIGN.md lists them for a later decision):
//   a. behind a failed wait (row 5) `frame` voids the resident covariance (res_n = 0: the row deletion behind the update may have
//      overwritten the prior), `checked` restores the saved book and drops the factor, `update` and the hybrid forms leave everything.
//   b. `frame` marginalises the previous clone before the wait, even behind a refused update; `checked` behind the wait and only when
//      the update applied; the hybrid forms inside the update launch, which writes nothing that stays when it refuses.
//   c. the "not applied" message: "nothing applied" (update), "the update was not applied" (frame, both checked forms), "nothing
//      applied, no state has left" (frame_hybrid); the armed launch's refusal is named by the unchecked frames only (the checked ones
//      report it through the verdict: not evaluated), and with "no propagation" alone where there was no update.
//   d. *applied and *n_after on the error exits: the unchecked forms write neither in rows 1-5, the checked forms write 0 and n in
//      rows 2-5; `update` never writes n_after.
//   e. `frame` behind a refused update reports n_after without the previous clone (b), every other form n.
#pragma once
#include "cov_book.hpp"

namespace orcvio_amd {

enum class ZuptForm { update, frame, frame_hybrid, checked, checked_hybrid };
enum class ZuptMarg { none, before_wait, behind_wait, in_launch };   // where the previous clone is marginalised
enum class ZuptAlso { none, imu_status, zchk_status };               // the status block whose refusal the update takes on
enum class ZuptBook { nothing, restore, restore_drop_factor, void_resident, refused_tail, keep_done };
enum class ZuptMsg { none, stage, verdict, imu_no_propagation, imu_no_update, nothing_applied, not_applied, no_state_left };

inline bool zupt_checked(ZuptForm f) { return f == ZuptForm::checked || f == ZuptForm::checked_hybrid; }
inline bool zupt_hybrid(ZuptForm f) { return f == ZuptForm::frame_hybrid || f == ZuptForm::checked_hybrid; }

struct ZuptPlan {
    int n = 0, n_dx = 0;    // the dimension the update sees; the entries of dx
    bool armed = false;     // the head takes the handle's arming (k_imu_phi_q in front of the propagation launches)
    bool check = false, update = true;
    bool eager = false;
    ZuptMarg marg = ZuptMarg::none;
    ZuptAlso also = ZuptAlso::none;
};

// res_n: the resident dimension at the call; armed / S: the handle's arming and its selected samples
inline ZuptPlan zupt_plan(ZuptForm form, int res_n, bool augment, int leg_dim, int n_clones, bool armed, int S) {
    ZuptPlan p;
    p.n = res_n + (augment ? 6 : 0);
    p.n_dx = zupt_hybrid(form) ? leg_dim + 6 * n_clones : p.n;   // (hybrid: the features have left in front of K r)
    p.armed = armed && form != ZuptForm::update;
    p.check = zupt_checked(form) && S >= 2;   // (one selected sample: nothing to test with -- the frame is not a zero-velocity one)
    p.update = !zupt_checked(form) || p.check;
    p.eager = form == ZuptForm::frame || form == ZuptForm::checked;
    p.marg = form == ZuptForm::update ? ZuptMarg::none : form == ZuptForm::frame ? ZuptMarg::before_wait
           : form == ZuptForm::checked ? ZuptMarg::behind_wait : ZuptMarg::in_launch;
    p.also = zupt_checked(form) ? ZuptAlso::zchk_status : (p.armed ? ZuptAlso::imu_status : ZuptAlso::none);
    return p;
}

struct ZuptFacts {             // what is known at the exit; a stage that did not run keeps its code at OK
    ZuptForm form = ZuptForm::update;
    bool check_ran = false;    // S >= 2
    int rc_head = 0, rc_check = 0, rc_update = 0, rc_marg = 0, rc_wait = 0;   // rc_marg: the marginalisation enqueued before the wait
    int upd = 0;               // the update's status word
    bool evaluated = false, accept = false;   // the verdict ...
    int rc_verdict = 0;                       // ... and what zchk_verdict returned
    bool imu_refused = false;  // the armed launch refused Phi / Q (unchecked frames: the host-coherent word; no update: the fetched one)
    bool remove_previous = false;
};

struct ZuptOutcome {
    int ret = 0;
    bool write_applied = false, write_n_after = false;
    int applied = 0, n_after = 0;
    ZuptBook book = ZuptBook::nothing;
    bool keep_applied = false;   // ZuptBook::keep_done: zupt_keep_done's argument
    bool marg_behind = false;    // the marginalisation is enqueued now, behind the wait
    ZuptMsg msg = ZuptMsg::none; // stage / verdict: the message the failed stage / zchk_verdict left stands
};

// the text behind "<who>" (nullptr: the message stands as it is)
inline const char* zupt_message(ZuptMsg m) {
    switch (m) {
        case ZuptMsg::imu_no_propagation: return ": Phi or Q of the armed IMU propagation not finite: no propagation";
        case ZuptMsg::imu_no_update: return ": Phi or Q of the armed IMU propagation not finite: no propagation, no update";
        case ZuptMsg::nothing_applied: return ": H P H^T + R not positive definite, or a non-finite covariance: nothing applied";
        case ZuptMsg::not_applied: return ": H P H^T + R not positive definite, or a non-finite covariance: the update was not applied";
        case ZuptMsg::no_state_left: return ": H P H^T + R not positive definite, or a non-finite covariance: nothing applied, no state has left";
        default: return nullptr;
    }
}

// ok / not_spd: ORCVIO_OK / ORCVIO_ERR_NOT_SPD (passed in: the header stands without the C ABI's)
inline ZuptOutcome zupt_frame_outcome(const ZuptPlan& p, const ZuptFacts& f, int ok, int not_spd) {
    ZuptOutcome o;
    o.ret = ok;
    const bool checked = zupt_checked(f.form);
    auto failed = [&o](int rc, ZuptBook b) { o.ret = rc; o.msg = ZuptMsg::stage; o.book = b; return o; };
    if (f.rc_head != ok) return failed(f.rc_head, ZuptBook::nothing);                                      // row 1
    if (checked) { o.write_applied = o.write_n_after = true; o.applied = 0; o.n_after = p.n; }
    if (!p.update) {                                                                                       // row 2
        if (f.rc_wait != ok) return failed(f.rc_wait, ZuptBook::nothing);
        if (f.imu_refused) { o.ret = not_spd; o.msg = ZuptMsg::imu_no_propagation; }
        return o;
    }
    if (f.rc_check != ok) return failed(f.rc_check, ZuptBook::nothing);                                    // row 3
    if (f.rc_update != ok) return failed(f.rc_update, p.eager ? ZuptBook::restore : ZuptBook::nothing);    // row 4
    if (f.rc_marg != ok || f.rc_wait != ok)                                                                // row 5
        return failed(f.rc_marg != ok ? f.rc_marg : f.rc_wait, f.form == ZuptForm::frame     ? ZuptBook::void_resident
                                                               : f.form == ZuptForm::checked ? ZuptBook::restore_drop_factor
                                                                                             : ZuptBook::nothing);
    const bool applied = f.upd == 0;
    const int kept = (p.marg == ZuptMarg::in_launch ? p.n_dx : p.n) - (f.remove_previous ? 6 : 0);   // what stays behind an applied frame
    o.write_applied = true; o.applied = applied ? 1 : 0;
    o.write_n_after = f.form != ZuptForm::update;
    o.n_after = applied || p.marg == ZuptMarg::before_wait ? kept : p.n;
    if (p.eager) o.book = applied ? ZuptBook::nothing : ZuptBook::refused_tail;
    else { o.book = ZuptBook::keep_done; o.keep_applied = applied; }
    if (applied) {                                                                                         // row 6
        o.marg_behind = p.marg == ZuptMarg::behind_wait && f.remove_previous;
    } else if (!checked) {                                                                                 // row 7
        o.ret = not_spd;
        o.msg = f.imu_refused ? ZuptMsg::imu_no_update
              : f.form == ZuptForm::update ? ZuptMsg::nothing_applied : f.form == ZuptForm::frame ? ZuptMsg::not_applied : ZuptMsg::no_state_left;
    } else if (f.rc_verdict != ok) { o.ret = f.rc_verdict; o.msg = ZuptMsg::verdict; }                     // row 8
    else if (f.accept) { o.ret = not_spd; o.msg = ZuptMsg::not_applied; }
    return o;
}

// the outcome's bookkeeping.  before: the book as it stood in front of the update's enqueue; e: the record that enqueue got
inline void zupt_book_apply(CovBook& b, const CovBook& before, const CovEdit& e, const ZuptOutcome& o) {
    switch (o.book) {
        case ZuptBook::nothing: break;
        case ZuptBook::restore: b = before; break;
        case ZuptBook::restore_drop_factor: b = before; b.fac_valid = false; break;
        case ZuptBook::void_resident: b.res_n = 0; b.fac_valid = false; break;   // NOTHING is resident: the caller sets the covariance again
        case ZuptBook::refused_tail: b.zupt_refused(before.fac_tail); break;     // the spare buffers took bit copies, trailing columns still zero
        case ZuptBook::keep_done: b.zupt_keep_done(e, o.keep_applied); break;
    }
}

// ... with the code of the marginalisation enqueued behind the wait (only where marg_behind says so)
inline void zupt_frame_outcome_marg(const ZuptPlan& p, ZuptOutcome& o, int rc, int ok) {
    if (rc != ok) { o.ret = rc; o.msg = ZuptMsg::stage; o.n_after = p.n; }
}

}  // namespace orcvio_amd
