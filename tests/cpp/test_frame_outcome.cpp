// The outcome table of the one-call filter frame (orcvio_amd/csrc/host/frame_outcome.hpp) on its own, built plainly and with
// -fsanitize=address,undefined by tests/test_frame_outcome.py.  The whole input space is enumerated against a second, literal
// transcription of the two code paths the table replaced (capi_step.inc of the commit in front of it: lines 657-677 the one-pass
// outcomes, lines 616-655 the end of the repair path), written as straight if chains; the rows the header documents are asserted by
// name; three flipped rows show that the comparison sees a flip.  No device, no library.
#include <cstdio>
#include <initializer_list>

#include "../../orcvio_amd/csrc/host/frame_outcome.hpp"

using namespace orcvio_amd;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

enum { OK = 0, NOT_SPD = 6, TIMEOUT = 7 };   // ORCVIO_OK, ORCVIO_ERR_NOT_SPD, ORCVIO_ERR_TIMEOUT (include/orcvio_msckf.h)
static const int CODES[3] = {OK, NOT_SPD, TIMEOUT};

struct Seen {   // what the caller of either path can observe
    int status_first, status_prune, ret;
    bool clear_stats3, clear_prune_stats3, evaluated_second;
};
static bool same(const Seen& a, const Seen& b) {
    return a.status_first == b.status_first && a.status_prune == b.status_prune && a.ret == b.ret && a.clear_stats3 == b.clear_stats3 &&
           a.clear_prune_stats3 == b.clear_prune_stats3 && a.evaluated_second == b.evaluated_second;
}

// second_code: what feature_outcome_view of the second update gives (one pass) / what its safe repeat returns (repaired)
static Seen transcription(const FrameFacts& f, int second_code) {
    Seen s{OK, OK, OK, false, false, false};
    if (!f.repaired) {
        // 658: res->status_first = first ? feature_outcome_view(h, vA, soA, res->stats) : ORCVIO_OK;
        s.status_first = f.first ? f.first_code : OK;
        // 659: if (imu_bad) { res->status_first = ORCVIO_ERR_NOT_SPD; ... }
        if (f.imu_bad) s.status_first = NOT_SPD;
        // 660: if (res->status_first != ORCVIO_OK) res->stats[3] = 0;
        if (s.status_first != OK) s.clear_stats3 = true;
        // 661: const int sc_changes = changes_status();
        const int sc_changes = f.changes;
        // 662: if (second) {
        if (f.second) {
            // 663: if (rcB != ORCVIO_OK) res->status_prune = rcB;
            if (f.rcB != OK) s.status_prune = f.rcB;
            // 664: else if (res->status_first != ORCVIO_OK) { res->status_prune = res->status_first; res->prune_stats[3] = 0; }
            else if (s.status_first != OK) { s.status_prune = s.status_first; s.clear_prune_stats3 = true; }
            // 665: else if (sc_changes != ORCVIO_OK) { res->status_prune = sc_changes; res->prune_stats[3] = 0; }
            else if (sc_changes != OK) { s.status_prune = sc_changes; s.clear_prune_stats3 = true; }
            // 666: else if (held) { (void)feature_outcome_view(h, vB, soB, res->prune_stats); res->status_prune = ORCVIO_OK; res->prune_stats[3] = 0; }
            else if (f.held) { s.evaluated_second = true; s.status_prune = OK; s.clear_prune_stats3 = true; }
            // 667-670: else { res->status_prune = feature_outcome_view(h, vB, soB, res->prune_stats); if (res->status_prune != ORCVIO_OK) res->prune_stats[3] = 0; }
            else {
                s.evaluated_second = true;
                s.status_prune = second_code;
                if (s.status_prune != OK) s.clear_prune_stats3 = true;
            }
        }
        // 675: if (rcR != ORCVIO_OK) return leave(rcR);
        if (f.rcR != OK) { s.ret = f.rcR; return s; }
        // 676: if (!second && rcB != ORCVIO_OK) return leave(rcB);
        if (!f.second && f.rcB != OK) { s.ret = f.rcB; return s; }
        // 677: return leave(res->status_first != ORCVIO_OK ? res->status_first : (res->status_prune != ORCVIO_OK ? res->status_prune : sc_changes));
        s.ret = s.status_first != OK ? s.status_first : (s.status_prune != OK ? s.status_prune : sc_changes);
        return s;
    }
    // 610 / 613 (the first update lost): rc = imu_bad ? ORCVIO_ERR_NOT_SPD : io_run_forked(...); res->status_first = rc;
    // 617-618 (the second lost): res->status_first = first ? feature_outcome_view(...) : ORCVIO_OK; if (imu_bad) res->status_first = ORCVIO_ERR_NOT_SPD;
    s.status_first = f.first ? f.first_code : OK;
    if (f.imu_bad) s.status_first = NOT_SPD;
    // 636: if (second) {
    if (f.second) {
        // 638-639: if (res->status_first != ORCVIO_OK) { res->status_prune = res->status_first; }
        if (s.status_first != OK) s.status_prune = s.status_first;
        // 640-643: else { rcB = step_second_update(h, fl, N, sb, true, res->prune_stats, who); ... res->status_prune = rcB;
        else { s.evaluated_second = true; s.status_prune = second_code; }
    }
    // 652: if (st->n_remove > 0 && !held) { rcR = step_remove(...); if (rcR != ORCVIO_OK) return leave(rcR); }
    if (f.rcR != OK) { s.ret = f.rcR; return s; }
    // 654: const int sc = changes_status();
    const int sc = f.changes;
    // 655: return leave(res->status_first != ORCVIO_OK ? res->status_first : (res->status_prune != ORCVIO_OK ? res->status_prune : sc));
    s.ret = s.status_first != OK ? s.status_first : (s.status_prune != OK ? s.status_prune : sc);
    return s;
}

typedef FrameOutcome (*Table)(const FrameFacts&, int, int);
typedef void (*Fold)(const FrameFacts&, FrameOutcome&, int, int);

static Seen through(Table table, Fold fold, const FrameFacts& f, int second_code) {
    FrameOutcome o = table(f, OK, NOT_SPD);
    if (o.eval_second) fold(f, o, second_code, OK);
    return Seen{o.status_first, o.status_prune, o.ret, o.clear_stats3, o.clear_prune_stats3, o.eval_second};
}

// combinations in which the table and the transcription differ
static int mismatches(Table table, Fold fold, int* total = nullptr) {
    int bad = 0, all = 0;
    for (int bits = 0; bits < 32; ++bits)
        for (int fc : CODES) for (int ch : {OK, NOT_SPD}) for (int rb : CODES) for (int rr : CODES) for (int sc : CODES) {
            FrameFacts f;
            f.repaired = bits & 1; f.first = bits & 2; f.second = bits & 4; f.held = bits & 8; f.imu_bad = bits & 16;
            f.first_code = fc; f.changes = ch; f.rcB = rb; f.rcR = rr;
            ++all;
            if (!same(through(table, fold, f, sc), transcription(f, sc))) ++bad;
        }
    if (total) *total = all;
    return bad;
}

// three flipped rows
static FrameOutcome flip_held_is_an_error(const FrameFacts& f, int ok, int ns) {   // row 4 reports the outcome instead of OK
    FrameFacts g = f; g.held = false;
    FrameOutcome o = frame_outcome(g, ok, ns);
    return o;
}
static void fold_held_is_an_error(const FrameFacts& f, FrameOutcome& o, int code, int ok) { FrameFacts g = f; g.held = false; frame_outcome_second(g, o, code, ok); }
static FrameOutcome flip_repair_clears(const FrameFacts& f, int ok, int ns) {   // difference a: the repair path clears stats[3] too
    FrameFacts g = f; g.repaired = false;
    FrameOutcome o = frame_outcome(g, ok, ns), p = frame_outcome(f, ok, ns);
    p.clear_stats3 = o.clear_stats3;
    return p;
}
static FrameOutcome flip_changes_before_first(const FrameFacts& f, int ok, int ns) {   // the return value prefers the changes' status
    FrameOutcome o = frame_outcome(f, ok, ns);
    if (f.rcR == ok && f.changes != ok && o.ret != f.rcB) o.ret = f.changes;
    return o;
}

static int named_rows() {
    {   // a refused Phi / Q: both updates NOT_SPD, both [3] cleared, the call returns NOT_SPD
        FrameFacts f; f.first = true; f.second = true; f.imu_bad = true;
        const FrameOutcome o = frame_outcome(f, OK, NOT_SPD);
        CHECK(o.status_first == NOT_SPD && o.status_prune == NOT_SPD && o.clear_stats3 && o.clear_prune_stats3 && !o.eval_second && o.ret == NOT_SPD);
    }
    {   // held back: status_prune OK, prune_stats[3] = 0, the call returns OK -- whatever the second update's own outcome says
        FrameFacts f; f.first = true; f.second = true; f.held = true;
        for (int code : CODES) {
            FrameOutcome o = frame_outcome(f, OK, NOT_SPD);
            CHECK(o.eval_second);
            frame_outcome_second(f, o, code, OK);
            CHECK(o.status_first == OK && o.status_prune == OK && !o.clear_stats3 && o.clear_prune_stats3 && o.ret == OK);
        }
    }
    {   // refused changes: status_changes (the caller's, = facts.changes) = status_prune = NOT_SPD
        FrameFacts f; f.first = true; f.second = true; f.changes = NOT_SPD;
        const FrameOutcome o = frame_outcome(f, OK, NOT_SPD);
        CHECK(o.status_first == OK && o.status_prune == NOT_SPD && o.clear_prune_stats3 && !o.eval_second && o.ret == NOT_SPD);
    }
    {   // a prune update without a valid track is not an error: its outcome is OK (prune_stats[3] = 0 is the device's), nothing cleared here
        FrameFacts f; f.first = true; f.second = true;
        FrameOutcome o = frame_outcome(f, OK, NOT_SPD);
        CHECK(o.eval_second);
        frame_outcome_second(f, o, OK, OK);
        CHECK(o.status_prune == OK && !o.clear_prune_stats3 && o.ret == OK);
    }
    {   // a frame without a first update: OK, and the second update is evaluated
        FrameFacts f; f.second = true; f.first_code = NOT_SPD;
        const FrameOutcome o = frame_outcome(f, OK, NOT_SPD);
        CHECK(o.status_first == OK && o.eval_second);
    }
    {   // the differences a and d of the header: repaired, nothing is cleared and the one-pass enqueue code is not looked at
        FrameFacts f; f.repaired = true; f.first = true; f.second = true; f.first_code = NOT_SPD; f.rcB = TIMEOUT;
        const FrameOutcome o = frame_outcome(f, OK, NOT_SPD);
        CHECK(o.status_first == NOT_SPD && o.status_prune == NOT_SPD && !o.clear_stats3 && !o.clear_prune_stats3 && !o.eval_second && o.ret == NOT_SPD);
    }
    return 0;
}

int main() {
    int total = 0;
    const int bad = mismatches(frame_outcome, frame_outcome_second, &total);
    std::printf("%d combinations, %d differ from the transcription\n", total, bad);
    CHECK(total == 32 * 3 * 2 * 3 * 3 * 3 && bad == 0);
    if (named_rows()) return 1;
    const int seen[3] = {mismatches(flip_held_is_an_error, fold_held_is_an_error), mismatches(flip_repair_clears, frame_outcome_second),
                         mismatches(flip_changes_before_first, frame_outcome_second)};
    std::printf("flipped rows seen in %d, %d, %d combinations\n", seen[0], seen[1], seen[2]);
    CHECK(seen[0] > 0 && seen[1] > 0 && seen[2] > 0);
    std::printf("frame outcome ok\n");
    return 0;
}
