// The plan and the outcome table of the five zero-velocity calls (orcvio_amd/csrc/host/zupt_frame_outcome.hpp) on their own, built
// with -fsanitize=address,undefined by tests/test_zupt_frame_outcome.py.  The input space is enumerated against a literal
// transcription of the four bodies the table replaced (capi_zupt.inc and capi_zupt_check.inc of the commit in front of it; the line
// numbers are theirs), written as straight if chains form by form, with the stage codes injected and the bookkeeping run on a CovBook
// over four dummy buffers: return code, the *applied / *n_after writes and values, the message, both marginalisation decisions and
// every field of the book, pointers included -- with a following factor, a factor of another dimension and none.  The table's side
// walks the phases of zupt_frame_run on the same injected codes.  The plan, the messages' text and a few rows are asserted against
// constants written out here.  No device, no library.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../orcvio_amd/csrc/host/zupt_frame_outcome.hpp"

using namespace orcvio_amd;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

enum { OK = 0, HIP = 5, NOT_SPD = 6 };   // ORCVIO_OK, ORCVIO_ERR_HIP, ORCVIO_ERR_NOT_SPD (include/orcvio_msckf.h)
enum { LEG = 22, NCL = 3, B = LEG + 6 * NCL, FEAT = 5, KMAX = 448 };   // the window behind the augmentation: 40 states, hybrid 45
enum Msg { M_NONE, M_STAGE, M_VERDICT, M_IMU_NO_PROPAGATION, M_IMU_NO_UPDATE, M_NOTHING_APPLIED, M_NOT_APPLIED, M_NO_STATE_LEFT };
enum Imu { NOT_ARMED, ARMED, ARMED_REFUSED };         // the handle's arming and what k_imu_phi_q said of Phi / Q
enum Verdict { NOT_EVALUATED, REJECTED, ACCEPTED };   // zchk_verdict: evaluated / accept; it returns NOT_SPD when not evaluated
enum Factor { RIGHT, OTHER, NONE };

static double PA[1], PB[1], SC[1], SD[1];   // the covariance pair, the factor pair (only their addresses are used)

struct In {
    ZuptForm form;
    bool check_ran;   // S >= 2
    int rc_head, rc_check, rc_update, rc_marg, rc_wait, rc_marg_behind;   // what each stage returns IF it is reached
    int upd;          // the update's status word
    Verdict verdict;
    Imu imu;
    bool remove_previous;
};

struct Seen {   // what the caller can observe, and the book
    int ret = OK;
    bool w_applied = false, w_n_after = false;
    int applied = -1, n_after = -1;
    int msg = M_NONE;
    bool marg_before = false, marg_behind = false;   // a marginalisation was enqueued before / behind the wait
    CovBook book;
};
static bool same_book(const CovBook& a, const CovBook& b) {
    return a.d_Pres == b.d_Pres && a.d_Ptmp == b.d_Ptmp && a.d_Sres == b.d_Sres && a.d_Stmp == b.d_Stmp && a.res_n == b.res_n && a.fac_n == b.fac_n &&
           a.fac_k == b.fac_k && a.fac_ld == b.fac_ld && a.fac_tail == b.fac_tail && a.fac_valid == b.fac_valid;
}
static bool same(const Seen& a, const Seen& b) {
    return a.ret == b.ret && a.w_applied == b.w_applied && a.w_n_after == b.w_n_after && (!a.w_applied || a.applied == b.applied) &&
           (!a.w_n_after || a.n_after == b.n_after) && a.msg == b.msg && a.marg_before == b.marg_before && a.marg_behind == b.marg_behind &&
           same_book(a.book, b.book);
}

// the book behind the head (propagated, augmented): n states, a factor that came through the augmentation (k and ld are not n's)
static CovBook start(int n, Factor f) {
    CovBook b;
    b.d_Pres = PA; b.d_Ptmp = PB; b.d_Sres = SC; b.d_Stmp = SD;
    b.res_n = n; b.fac_n = f == OTHER ? n + 6 : n; b.fac_k = 46; b.fac_ld = 64; b.fac_tail = 15; b.fac_valid = f != NONE;
    return b;
}
// orcvio_msckf_cov_remove_clones of one clone: validated in front, it fails only in a HIP call -- modelled as leaving the book alone
static int remove_previous(CovBook& b, int rc) {
    if (rc == OK) b.gather(b.res_n - 6);
    return rc;
}
static Seen done(Seen s, const CovBook& b, int ret, int msg) { s.ret = ret; s.msg = msg; s.book = b; return s; }

// ---- the transcription ---------------------------------------------------------------------------------------------------------------
// capi_zupt.inc:52-68, orcvio_msckf_cov_zupt
static Seen t_update(const In& in, CovBook b) {
    Seen s;
    // 55: HIPCHK(hipSetDevice(h->device));
    if (in.rc_head != OK) return done(s, b, in.rc_head, M_STAGE);
    // 56: const CovState before = cov_state(h);
    const CovBook before = b;
    // 57: zupt_enqueue (34: h->zupt(...), then the launches); failed: cov_restore(h, before); return rc;
    b.zupt(true, KMAX);
    if (in.rc_update != OK) { b = before; return done(s, b, in.rc_update, M_STAGE); }
    // 60: zupt_collect failed: cov_restore(h, before); return rc;
    if (in.rc_wait != OK) { b = before; return done(s, b, in.rc_wait, M_STAGE); }
    const bool refused = in.upd != 0;
    // 61: *applied = refused ? 0 : 1;
    s.w_applied = true; s.applied = refused ? 0 : 1;
    // 62-66: if (refused) { cov_restore(h, before); g_last_error = "cov_zupt: ... nothing applied"; return ORCVIO_ERR_NOT_SPD; }
    if (refused) { b = before; return done(s, b, NOT_SPD, M_NOTHING_APPLIED); }
    return done(s, b, OK, M_NONE);
}

// capi_zupt.inc:92-126, orcvio_msckf_cov_zupt_frame
static Seen t_frame(const In& in, CovBook b) {
    Seen s;
    const bool armed = in.imu != NOT_ARMED, imu_refused = in.imu == ARMED_REFUSED;
    // 101-102: int rc = zupt_frame_head(h, f, armed); if (rc != ORCVIO_OK) return rc;
    if (in.rc_head != OK) return done(s, b, in.rc_head, M_STAGE);
    // 103: const CovState before = cov_state(h);
    const CovBook before = b;
    // 104-105: rc = zupt_enqueue(...); if (rc != ORCVIO_OK) { cov_restore(h, before); return rc; }
    b.zupt(true, KMAX);
    if (in.rc_update != OK) { b = before; return done(s, b, in.rc_update, M_STAGE); }
    int rc = OK;
    // 106-109: if (f->remove_previous) rc = orcvio_msckf_cov_remove_clones(h, z->leg_dim, &prev, 1);
    if (in.remove_previous) { s.marg_before = true; rc = remove_previous(b, in.rc_marg); }
    // 111: if (rc == ORCVIO_OK) rc = zupt_collect(h, n, dx, &refused);
    if (rc == OK) rc = in.rc_wait;
    // 112-116: if (rc != ORCVIO_OK) { h->res_n = 0; h->fac_valid = false; return rc; }
    if (rc != OK) { b.res_n = 0; b.fac_valid = false; return done(s, b, rc, M_STAGE); }
    const bool refused = in.upd != 0;
    // 117-118: *n_after = h->res_n; *applied = refused ? 0 : 1;
    s.w_n_after = true; s.n_after = b.res_n;
    s.w_applied = true; s.applied = refused ? 0 : 1;
    // 119-124: if (refused) { h->zupt_refused(before.fac_tail); g_last_error = armed && imu_refused(h) ? "...: no propagation, no
    // update" : "...: the update was not applied"; return ORCVIO_ERR_NOT_SPD; }
    if (refused) {
        b.zupt_refused(before.fac_tail);
        return done(s, b, NOT_SPD, armed && imu_refused ? M_IMU_NO_UPDATE : M_NOT_APPLIED);
    }
    return done(s, b, OK, M_NONE);
}

// capi_zupt.inc:164-192, orcvio_msckf_cov_zupt_frame_hybrid
static Seen t_frame_hybrid(const In& in, CovBook b) {
    Seen s;
    const bool armed = in.imu != NOT_ARMED, imu_refused = in.imu == ARMED_REFUSED;
    // 174-175: int rc = zupt_frame_head(h, f, armed); if (rc != ORCVIO_OK) return rc;
    if (in.rc_head != OK) return done(s, b, in.rc_head, M_STAGE);
    // 177-178: rc = zupt_keep_enqueue(...) (153: kp.m = a.b - (remove_previous ? 6 : 0); 155: e = h->zupt_keep(kp.m, ...)); failed: return rc;
    const CovEdit e = b.zupt_keep(B - (in.remove_previous ? 6 : 0), true, KMAX);
    if (in.rc_update != OK) return done(s, b, in.rc_update, M_STAGE);
    // 181-182: rc = zupt_collect(...); if (rc != ORCVIO_OK) return rc;
    if (in.rc_wait != OK) return done(s, b, in.rc_wait, M_STAGE);
    const bool refused = in.upd != 0;
    // 183-185: h->zupt_keep_done(e, !refused); *n_after = h->res_n; *applied = refused ? 0 : 1;
    b.zupt_keep_done(e, !refused);
    s.w_n_after = true; s.n_after = b.res_n;
    s.w_applied = true; s.applied = refused ? 0 : 1;
    // 186-190: if (refused) { g_last_error = armed && imu_refused(h) ? "...: no propagation, no update" : "...: nothing applied, no
    // state has left"; return ORCVIO_ERR_NOT_SPD; }
    if (refused) return done(s, b, NOT_SPD, armed && imu_refused ? M_IMU_NO_UPDATE : M_NO_STATE_LEFT);
    return done(s, b, OK, M_NONE);
}

// capi_zupt_check.inc:121-194, zupt_frame_checked: hy == false orcvio_msckf_cov_zupt_frame_checked, true _checked_hybrid
static Seen t_checked(const In& in, CovBook b, bool hy) {
    Seen s;
    // 136: const bool check = S >= 2;
    const bool check = in.check_ran;
    // 147-150: imu_consume, launch_cov_propagate, cov_augment; if (rc != ORCVIO_OK) return rc;
    if (in.rc_head != OK) return done(s, b, in.rc_head, M_STAGE);
    // 151-152: *n_after = h->res_n; *applied = 0;
    s.w_n_after = true; s.n_after = b.res_n;
    s.w_applied = true; s.applied = 0;
    // 153-161: if (!check) { dx zeroed; one wait on imu_status; failed: return rc; refused: "...: no propagation", NOT_SPD; return OK; }
    if (!check) {
        if (in.rc_wait != OK) return done(s, b, in.rc_wait, M_STAGE);
        if (in.imu == ARMED_REFUSED) return done(s, b, NOT_SPD, M_IMU_NO_PROPAGATION);
        return done(s, b, OK, M_NONE);
    }
    // 162-163: rc = zchk_enqueue(...); if (rc != ORCVIO_OK) return rc;
    if (in.rc_check != OK) return done(s, b, in.rc_check, M_STAGE);
    // 164-165: const CovState before = cov_state(h); CovEdit kept;
    const CovBook before = b;
    CovEdit kept;
    // 166-167: rc = hy ? zupt_keep_enqueue(..., &kept) : zupt_enqueue(...); if (rc != ORCVIO_OK) { cov_restore(h, before); return rc; }
    if (hy) kept = b.zupt_keep(B - (in.remove_previous ? 6 : 0), true, KMAX); else b.zupt(true, KMAX);
    if (in.rc_update != OK) { b = before; return done(s, b, in.rc_update, M_STAGE); }
    // 171-176: rc = fetch_copies(...); if (rc != ORCVIO_OK) { cov_restore(h, before); if (!hy) h->fac_valid = false; return rc; }
    if (in.rc_wait != OK) { b = before; if (!hy) b.fac_valid = false; return done(s, b, in.rc_wait, M_STAGE); }
    // 177: const int rv = zchk_verdict(...);   (not evaluated: it sets the message and returns ORCVIO_ERR_NOT_SPD)
    const int rv = in.verdict == NOT_EVALUATED ? NOT_SPD : OK;
    const bool accept = in.verdict == ACCEPTED;
    // 178-184: if (upd != 0) { if (!hy) h->zupt_refused(before.fac_tail); if (rv != ORCVIO_OK) return rv; if (!verdict->accept) return
    // ORCVIO_OK; g_last_error = who + ": ... the update was not applied"; return ORCVIO_ERR_NOT_SPD; }
    if (in.upd != 0) {
        if (!hy) b.zupt_refused(before.fac_tail);
        if (rv != OK) return done(s, b, rv, M_VERDICT);
        if (!accept) return done(s, b, OK, M_NONE);
        return done(s, b, NOT_SPD, M_NOT_APPLIED);
    }
    // 185-186: *applied = 1; if (hy) h->zupt_keep_done(kept, true);
    s.applied = 1;
    if (hy) b.zupt_keep_done(kept, true);
    // 187-191: if (!hy && f->remove_previous) { rc = orcvio_msckf_cov_remove_clones(...); if (rc != ORCVIO_OK) return rc; }
    if (!hy && in.remove_previous) {
        s.marg_behind = true;
        const int rc = remove_previous(b, in.rc_marg_behind);
        if (rc != OK) return done(s, b, rc, M_STAGE);
    }
    // 192-193: *n_after = h->res_n; return ORCVIO_OK;
    s.n_after = b.res_n;
    return done(s, b, OK, M_NONE);
}

static Seen transcription(const In& in, const CovBook& b) {
    switch (in.form) {
        case ZuptForm::update: return t_update(in, b);
        case ZuptForm::frame: return t_frame(in, b);
        case ZuptForm::frame_hybrid: return t_frame_hybrid(in, b);
        case ZuptForm::checked: return t_checked(in, b, false);
        default: return t_checked(in, b, true);
    }
}

// ---- the table, walked as zupt_frame_run walks it (capi_zupt.inc: phases 2-8 on the injected codes) ------------------------------------
static int msg_id(ZuptMsg m) {
    switch (m) {
        case ZuptMsg::none: return M_NONE;
        case ZuptMsg::stage: return M_STAGE;
        case ZuptMsg::verdict: return M_VERDICT;
        case ZuptMsg::imu_no_propagation: return M_IMU_NO_PROPAGATION;
        case ZuptMsg::imu_no_update: return M_IMU_NO_UPDATE;
        case ZuptMsg::nothing_applied: return M_NOTHING_APPLIED;
        case ZuptMsg::not_applied: return M_NOT_APPLIED;
        default: return M_NO_STATE_LEFT;
    }
}

static Seen through_table(const In& in, CovBook b) {
    Seen s;
    const bool augment = in.form != ZuptForm::update;
    const ZuptPlan p = zupt_plan(in.form, b.res_n - (augment ? 6 : 0), augment, LEG, NCL, in.imu != NOT_ARMED, in.check_ran ? 2 : 1);
    ZuptFacts f;
    f.form = in.form; f.check_ran = p.check; f.remove_previous = in.remove_previous;
    int rc = f.rc_head = in.rc_head;
    if (rc == OK && p.check) rc = f.rc_check = in.rc_check;
    const CovBook before = b;
    CovEdit e;
    if (rc == OK && p.update) {   // zupt_enqueue: the record in front of the launches
        const bool fused = p.marg == ZuptMarg::in_launch;
        e = p.eager ? b.zupt(true, KMAX) : b.zupt_keep(fused ? B - (in.remove_previous ? 6 : 0) : b.res_n, true, KMAX);
        if (!p.eager && !fused) e.ld_out = e.ld_in;
        rc = f.rc_update = in.rc_update;
    }
    if (rc == OK && p.marg == ZuptMarg::before_wait && in.remove_previous) { s.marg_before = true; rc = f.rc_marg = remove_previous(b, in.rc_marg); }
    if (rc == OK) rc = f.rc_wait = in.rc_wait;
    if (rc == OK) {
        f.upd = p.update ? in.upd : 0;
        f.imu_refused = p.update ? p.also == ZuptAlso::imu_status && in.imu == ARMED_REFUSED : in.imu == ARMED_REFUSED;
        if (p.check) { f.evaluated = in.verdict != NOT_EVALUATED; f.accept = in.verdict == ACCEPTED; f.rc_verdict = f.evaluated ? OK : NOT_SPD; }
    }
    ZuptOutcome o = zupt_frame_outcome(p, f, OK, NOT_SPD);
    zupt_book_apply(b, before, e, o);
    if (o.marg_behind) { s.marg_behind = true; zupt_frame_outcome_marg(p, o, remove_previous(b, in.rc_marg_behind), OK); }
    s.w_applied = o.write_applied; s.applied = o.applied;
    s.w_n_after = o.write_n_after; s.n_after = o.n_after;
    return done(s, b, o.ret, msg_id(o.msg));
}

// ---- what no call can reach: skipped, and counted -------------------------------------------------------------------------------------
static bool unreachable(const In& in) {
    // orcvio_msckf_cov_zupt has no frame flags: nothing to marginalise
    if (in.form == ZuptForm::update && in.remove_previous) return true;
    // a checked form is refused in front of every launch on a handle that is not armed
    if (zupt_checked(in.form) && in.imu == NOT_ARMED) return true;
    // a checked update reads the check's status block (`also`): it applies itself only behind an accepting verdict
    if (zupt_checked(in.form) && in.check_ran && in.upd == 0 && in.verdict != ACCEPTED) return true;
    return false;
}
// (NOT skipped, and so compared: a verdict or S >= 2 on an unchecked form, an arming on orcvio_msckf_cov_zupt, codes of stages a form
// does not have or does not reach -- the table has to ignore them as the bodies did)

static int enumerate(int* compared, int* skipped) {
    const ZuptForm forms[5] = {ZuptForm::update, ZuptForm::frame, ZuptForm::frame_hybrid, ZuptForm::checked, ZuptForm::checked_hybrid};
    int bad = 0;
    for (ZuptForm form : forms) for (int check = 0; check < 2; ++check) for (int codes = 0; codes < 64; ++codes)
        for (int upd : {0, 1}) for (Verdict v : {NOT_EVALUATED, REJECTED, ACCEPTED}) for (Imu imu : {NOT_ARMED, ARMED, ARMED_REFUSED})
            for (int rem = 0; rem < 2; ++rem) {
                const In in{form, check != 0, codes & 1 ? HIP : OK, codes & 2 ? HIP : OK, codes & 4 ? HIP : OK, codes & 8 ? HIP : OK,
                            codes & 16 ? HIP : OK, codes & 32 ? HIP : OK, upd, v, imu, rem != 0};
                if (unreachable(in)) { ++*skipped; continue; }
                ++*compared;
                for (Factor fac : {RIGHT, OTHER, NONE}) {
                    const CovBook b = start(zupt_hybrid(form) ? B + FEAT : B, fac);
                    if (!same(through_table(in, b), transcription(in, b))) {
                        if (++bad <= 10) std::printf("differs: form %d check %d codes %d upd %d verdict %d imu %d remove %d factor %d\n", (int)form, check, codes, upd, (int)v, (int)imu, rem, (int)fac);
                    }
                }
            }
    return bad;
}

// ---- constants written out --------------------------------------------------------------------------------------------------------------
static int the_plan() {
    struct Row { ZuptForm form; int res_n; bool augment, armed; int S; int n, n_dx; bool hd_armed, check, update, eager; ZuptMarg marg; ZuptAlso also; };
    const Row rows[] = {
        {ZuptForm::update, 40, false, false, 0, 40, 40, false, false, true, false, ZuptMarg::none, ZuptAlso::none},
        {ZuptForm::update, 40, false, true, 9, 40, 40, false, false, true, false, ZuptMarg::none, ZuptAlso::none},   // the arming is not the update's
        {ZuptForm::frame, 34, true, false, 0, 40, 40, false, false, true, true, ZuptMarg::before_wait, ZuptAlso::none},
        {ZuptForm::frame, 40, false, true, 1, 40, 40, true, false, true, true, ZuptMarg::before_wait, ZuptAlso::imu_status},
        {ZuptForm::frame_hybrid, 39, true, false, 0, 45, 40, false, false, true, false, ZuptMarg::in_launch, ZuptAlso::none},
        {ZuptForm::frame_hybrid, 39, true, true, 5, 45, 40, true, false, true, false, ZuptMarg::in_launch, ZuptAlso::imu_status},
        {ZuptForm::checked, 34, true, true, 2, 40, 40, true, true, true, true, ZuptMarg::behind_wait, ZuptAlso::zchk_status},
        {ZuptForm::checked, 34, true, true, 1, 40, 40, true, false, false, true, ZuptMarg::behind_wait, ZuptAlso::zchk_status},
        {ZuptForm::checked_hybrid, 39, true, true, 128, 45, 40, true, true, true, false, ZuptMarg::in_launch, ZuptAlso::zchk_status},
        {ZuptForm::checked_hybrid, 39, true, true, 0, 45, 40, true, false, false, false, ZuptMarg::in_launch, ZuptAlso::zchk_status},
    };
    for (const Row& r : rows) {
        const ZuptPlan p = zupt_plan(r.form, r.res_n, r.augment, LEG, NCL, r.armed, r.S);
        CHECK(p.n == r.n && p.n_dx == r.n_dx && p.armed == r.hd_armed && p.check == r.check && p.update == r.update && p.eager == r.eager);
        CHECK(p.marg == r.marg && p.also == r.also);
    }
    return 0;
}

static int the_messages() {
    CHECK(!zupt_message(ZuptMsg::none) && !zupt_message(ZuptMsg::stage) && !zupt_message(ZuptMsg::verdict));
    CHECK(!std::strcmp(zupt_message(ZuptMsg::imu_no_propagation), ": Phi or Q of the armed IMU propagation not finite: no propagation"));
    CHECK(!std::strcmp(zupt_message(ZuptMsg::imu_no_update), ": Phi or Q of the armed IMU propagation not finite: no propagation, no update"));
    CHECK(!std::strcmp(zupt_message(ZuptMsg::nothing_applied), ": H P H^T + R not positive definite, or a non-finite covariance: nothing applied"));
    CHECK(!std::strcmp(zupt_message(ZuptMsg::not_applied), ": H P H^T + R not positive definite, or a non-finite covariance: the update was not applied"));
    CHECK(!std::strcmp(zupt_message(ZuptMsg::no_state_left),
                       ": H P H^T + R not positive definite, or a non-finite covariance: nothing applied, no state has left"));
    return 0;
}

static const In QUIET{ZuptForm::frame, true, OK, OK, OK, OK, OK, OK, 0, ACCEPTED, ARMED, true};

// the differences between the forms the header lists, each with its numbers
static int named_rows() {
    {   // a. a failed wait: `frame` voids the resident covariance ...
        In in = QUIET; in.rc_wait = HIP;
        Seen s = through_table(in, start(40, RIGHT));
        CHECK(s.ret == HIP && !s.w_applied && !s.w_n_after && s.msg == M_STAGE && s.book.res_n == 0 && !s.book.fac_valid);
        in.form = ZuptForm::checked;   // ... `checked` restores the book and drops the factor, applied = 0 and n_after = 40 written ...
        s = through_table(in, start(40, RIGHT));
        CHECK(s.ret == HIP && s.w_applied && s.applied == 0 && s.w_n_after && s.n_after == 40);
        CHECK(s.book.res_n == 40 && !s.book.fac_valid && s.book.d_Pres == PA && s.book.d_Sres == SC && s.book.fac_tail == 15);
        for (ZuptForm form : {ZuptForm::update, ZuptForm::frame_hybrid, ZuptForm::checked_hybrid}) {   // ... the others leave everything
            in.form = form; in.remove_previous = form != ZuptForm::update;
            const CovBook b = start(form == ZuptForm::update ? 40 : 45, RIGHT);
            s = through_table(in, b);
            CHECK(s.ret == HIP && same_book(s.book, b) && s.book.fac_valid && s.w_applied == (form == ZuptForm::checked_hybrid));
        }
    }
    {   // b. / e. a refused update: `frame` has marginalised all the same (n_after 34), the prior's tail is back
        In in = QUIET; in.upd = 1;
        Seen s = through_table(in, start(40, RIGHT));
        CHECK(s.ret == NOT_SPD && s.applied == 0 && s.n_after == 34 && s.marg_before && s.book.res_n == 34 && s.book.fac_valid && s.book.fac_tail == 15);
        CHECK(s.msg == M_NOT_APPLIED);
        in.imu = ARMED_REFUSED;
        CHECK(through_table(in, start(40, RIGHT)).msg == M_IMU_NO_UPDATE);
        in.form = ZuptForm::checked; in.verdict = REJECTED;   // rejected by the check: OK, no message, nothing marginalised
        s = through_table(in, start(40, RIGHT));
        CHECK(s.ret == OK && s.applied == 0 && s.n_after == 40 && !s.marg_behind && !s.marg_before && s.msg == M_NONE && s.book.res_n == 40);
        CHECK(s.book.d_Pres == PB && s.book.d_Sres == SD && s.book.fac_tail == 15);   // (the bit copies are resident in the swapped buffers)
        in.form = ZuptForm::checked_hybrid;
        const CovBook b = start(45, RIGHT);
        s = through_table(in, b);
        CHECK(s.ret == OK && s.applied == 0 && s.n_after == 45 && same_book(s.book, b));
        in.verdict = NOT_EVALUATED;
        s = through_table(in, b);
        CHECK(s.ret == NOT_SPD && s.msg == M_VERDICT && same_book(s.book, b));
    }
    {   // applied: the dimensions and the factor behind every form
        In in = QUIET;
        Seen s = through_table(in, start(40, RIGHT));
        CHECK(s.ret == OK && s.applied == 1 && s.n_after == 34 && s.book.res_n == 34 && s.book.fac_n == 34 && s.book.fac_ld == 48 && s.book.fac_tail == 0);
        in.form = ZuptForm::checked;
        s = through_table(in, start(40, RIGHT));
        CHECK(s.ret == OK && s.applied == 1 && s.n_after == 34 && s.marg_behind && s.book.res_n == 34 && s.book.fac_tail == 0);
        in.rc_marg_behind = HIP;   // ... its marginalisation fails: that code, applied stays 1, n_after stays 40
        s = through_table(in, start(40, RIGHT));
        CHECK(s.ret == HIP && s.applied == 1 && s.n_after == 40 && s.msg == M_STAGE);
        in = QUIET; in.form = ZuptForm::checked_hybrid;
        s = through_table(in, start(45, RIGHT));
        CHECK(s.ret == OK && s.applied == 1 && s.n_after == 34 && s.book.res_n == 34 && s.book.d_Pres == PB && s.book.d_Sres == SD && s.book.fac_ld == 48);
        in.remove_previous = false; in.form = ZuptForm::frame_hybrid;
        s = through_table(in, start(45, OTHER));
        CHECK(s.ret == OK && s.n_after == 40 && s.book.res_n == 40 && !s.book.fac_valid);
        in.form = ZuptForm::update;   // the update alone: S+ keeps the factor's leading dimension, n_after is not written
        s = through_table(in, start(40, RIGHT));
        CHECK(s.ret == OK && s.applied == 1 && !s.w_n_after && s.book.res_n == 40 && s.book.d_Pres == PB && s.book.d_Sres == SD);
        CHECK(s.book.fac_valid && s.book.fac_n == 40 && s.book.fac_k == 46 && s.book.fac_ld == 64 && s.book.fac_tail == 0);
    }
    {   // one selected sample: no check, no update -- OK, or the armed launch's refusal
        In in = QUIET; in.form = ZuptForm::checked; in.check_ran = false; in.upd = 1; in.verdict = NOT_EVALUATED;
        const CovBook b = start(40, RIGHT);
        Seen s = through_table(in, b);
        CHECK(s.ret == OK && s.w_applied && s.applied == 0 && s.n_after == 40 && s.msg == M_NONE && same_book(s.book, b));
        in.imu = ARMED_REFUSED;
        s = through_table(in, b);
        CHECK(s.ret == NOT_SPD && s.applied == 0 && s.msg == M_IMU_NO_PROPAGATION && same_book(s.book, b));
    }
    return 0;
}

int main() {
    int compared = 0, skipped = 0;
    const int bad = enumerate(&compared, &skipped);
    std::printf("compared %d combinations (each with three factors), skipped %d, %d differ from the transcription\n", compared, skipped, bad);
    CHECK(bad == 0);
    CHECK(compared + skipped == 5 * 2 * 64 * 2 * 3 * 3 * 2);
    if (the_plan() || the_messages() || named_rows()) return 1;
    std::printf("zupt frame outcome ok\n");
    return 0;
}
