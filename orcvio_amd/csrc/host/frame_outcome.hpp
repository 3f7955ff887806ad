// frame_outcome.hpp -- what a one-call filter frame (orcvio_msckf_io_step_frame / _ex, capi_step.inc) reports once its results are on the
// host: ONE table for the one-pass path and for the repair path, free of HIP and of the handle.  tests/cpp/test_frame_outcome.cpp
// enumerates it against a transcription of the two code paths it replaced.
//
// The rows, in the order they are tried (NOT_SPD = ORCVIO_ERR_NOT_SPD, the refusal of the device):
//   status_first   a refused Phi / Q of the armed IMU propagation: NOT_SPD.  Otherwise the first update's own outcome; a frame
//                  without a first update: OK.
//   status_prune   (frames with a second update)
//     1. its enqueue failed (one pass only): that code; its outcome is not evaluated.
//     2. the first update was refused: the second refused its commit on the kept status words -- status_first; not evaluated.
//     3. the changes were refused (one pass only): their status; not evaluated.
//     4. held back by the choice of the clones that leave (one pass only): evaluated -- the outcome's side effects are today's --, but
//        not an error: OK, prune_stats[3] = 0.
//     5. otherwise its own outcome.  A prune update that was refused on the device for want of a valid track reports OK with
//        prune_stats[3] = 0 of its own: not an error.
//   stats[3] / prune_stats[3] are cleared where the update was refused or held back -- on the one-pass path only.
//   the call returns: a failed marginalisation's code; else (one pass, no second update) the failed anchor-change launch's code; else
//   the first of status_first, status_prune, the changes' status that is not OK.
//
// Where the two paths differ (kept as they were, each a row above; DESIGN.md 3.6 lists them for a later decision):
//   a. one pass clears stats[3] behind a refused first update and prune_stats[3] in rows 2-5; the repair path takes io_run_forked's
//      stats as they come.
//   b. one pass lets refused changes refuse the prune update (row 3); repaired, the second update's safe form reads the changes' word
//      before its update goes out and returns NOT_SPD itself (row 5), prune_stats untouched.
//   c. a held-back frame's prune update is OK with prune_stats[3] = 0 by row 4 in one pass; repaired, the second update's safe form
//      returns OK with zeroed results itself (row 5).
//   d. the one-pass codes of a failed enqueue (rows 1 and the return value's second clause) are not looked at behind a repair: the
//      repair has run those launches again and returned on their failure itself.
#pragma once

namespace orcvio_amd {

struct FrameFacts {         // what is known once the results are on the host
    bool repaired = false;  // the lost-hand-off path ran (capi_step.inc frame_repair)
    bool first = false;     // the frame has a first update
    bool second = false;    // ... a second (prune) update
    bool held = false;      // the choice of the clones that leave disagreed: the second half was held back
    bool imu_bad = false;   // the armed IMU launch refused Phi / Q
    int first_code = 0;     // the first update's own outcome (feature_outcome_view, or the repeat's io_run_forked); ignored without one
    int changes = 0;        // the changes' status
    int rcB = 0;            // one pass: what enqueueing the second half returned
    int rcR = 0;            // what enqueueing the marginalisation returned
};

struct FrameOutcome {
    int status_first = 0, status_prune = 0;
    bool clear_stats3 = false, clear_prune_stats3 = false;
    bool eval_second = false;   // the second update's own outcome is to be evaluated (repaired: the update is to be run again) and
                                // handed to frame_outcome_second -- in exactly these cases: evaluating has side effects
    int ret = 0;                // what the call returns
};

// the call's return value from an outcome and the facts AS THEY STAND: two of them may have moved on since frame_outcome was asked --
// rcR (the marginalisation behind an agreed choice goes out behind the outcomes) and, repaired, the changes' status (read last)
inline int frame_outcome_return(const FrameFacts& f, const FrameOutcome& o, int ok) {
    if (f.rcR != ok) return f.rcR;
    if (!f.repaired && !f.second && f.rcB != ok) return f.rcB;
    return o.status_first != ok ? o.status_first : (o.status_prune != ok ? o.status_prune : f.changes);
}

// ok / not_spd: ORCVIO_OK / ORCVIO_ERR_NOT_SPD (passed in: the header stands without the C ABI's)
inline FrameOutcome frame_outcome(const FrameFacts& f, int ok, int not_spd) {
    FrameOutcome o;
    o.status_first = f.imu_bad ? not_spd : (f.first ? f.first_code : ok);
    o.status_prune = ok;
    o.clear_stats3 = !f.repaired && o.status_first != ok;
    if (f.second) {
        if (!f.repaired && f.rcB != ok) o.status_prune = f.rcB;                                                   // row 1
        else if (o.status_first != ok) { o.status_prune = o.status_first; o.clear_prune_stats3 = !f.repaired; }   // row 2
        else if (!f.repaired && f.changes != ok) { o.status_prune = f.changes; o.clear_prune_stats3 = true; }      // row 3
        else if (!f.repaired && f.held) { o.eval_second = true; o.clear_prune_stats3 = true; }                     // row 4
        else o.eval_second = true;                                                                                // row 5
    }
    o.ret = frame_outcome_return(f, o, ok);
    return o;
}

// ... with the second update's own outcome (only where eval_second says so)
inline void frame_outcome_second(const FrameFacts& f, FrameOutcome& o, int code, int ok) {
    if (f.repaired || !f.held) {   // (row 4: held back is not an error whatever the outcome says)
        o.status_prune = code;
        if (!f.repaired && code != ok) o.clear_prune_stats3 = true;
    }
    o.ret = frame_outcome_return(f, o, ok);
}

}  // namespace orcvio_amd
