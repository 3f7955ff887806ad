"""GPU: features entering the state with the resident square-root factor carried along (orcvio_msckf_cov_commit_new_features_fac:
k_aug_rows, k_aug_finish), block by block at the edge shapes.  P_aug and dx_new against entering_cases.tail_ext fed with what the
device itself read back (TAIL_TOL); the factor against entering_factor_cases.s_aug_ext fed with the S+ a twin handle's cov_commit
leaves after the same update (G_TOL, RINV_TOL: 100 x the float64 restatement's own worst error, tests/test_entering_factor_cases.py,
never what the device returns), its old rows and zeros bit for bit; the payoff: the next update starts from the widened factor.

Shapes beyond entering_cases.TAIL_CASES (sz = 1: small_d1_k1; sz = 60: small_d3_k20; n + 1 > 256: wide_*):
    small_d1_k13   n + sz = 111 = 15 (mod 16): the leading dimension is n + sz + 1, and the old one (112)
    small_d1_k14   n + sz = 112 =  0 (mod 16): the leading dimension jumps to 128
    small_d3_k2    the same jump for d = 3 (106 -> 112)
and three ROUTES of the prior's factor to the update: 'prefactored' (kf = n), 'augmented' (cov_augment behind the factorisation:
kf = n - 6 < n), 'marginalised' (cov_remove_clones behind it: kf = n + 6 > n); 'none': the update factors its prior itself."""
import contextlib
import ctypes as C
import dataclasses

import numpy as np
import pytest

from orcvio_amd import capi, synth
from oracle import mirror
from helpers import rel
import entering_cases as ec
import entering_factor_cases as fc

pytestmark = pytest.mark.gpu

MAX_CLONES = 40
CAPACITY = 46 + 6 * MAX_CLONES          # states the handle's resident covariance can hold
UPDATE_TOL = 1e-6

EDGE_CASES = [ec.CaseId('small', 1, 13), ec.CaseId('small', 1, 14), ec.CaseId('small', 3, 2)]
TAIL_CASES = [c for c in ec.CASES if ec.make_case(c).win.n + c.d * c.k <= CAPACITY]
# (case, route): every case with the update's own factorisation or the prefactored prior in turn, the routes on the 6-feature cases
RUNS = ([(c, 'none' if i % 2 else 'prefactored') for i, c in enumerate(TAIL_CASES + EDGE_CASES)] +
        [(ec.CaseId('small', d, 6), r) for d in (1, 3) for r in ('augmented', 'marginalised')] +
        [(ec.CaseId('small', 3, 20), 'augmented'), (ec.CaseId('small', 1, 14), 'marginalised')])
RUN_IDS = ['%s-%s' % (c, r) for c, r in RUNS]


def _new(max_clones=MAX_CLONES):
    return capi.MsckfUpdater(device=0, max_clones=max_clones, max_features=512, max_observations=16384, debug_hooks=True)


@pytest.fixture(scope='module')
def upd(built):
    u = _new()
    yield u
    u.close()


@pytest.fixture(scope='module')
def twin(built):
    u = _new()
    yield u
    u.close()


@contextlib.contextmanager
def options(u, case):
    w = case.win
    u.set_extra_states(w.n_extra)
    u.set_schmidt_states(w.n_nui)
    u.set_ekf_rows_mode(True)
    u.set_ref_h2_ldlt(case.cid.ldlt)
    try:
        yield
    finally:
        u.set_ref_h2_ldlt(False)
        u.set_ekf_rows_mode(False)
        u.set_schmidt_states(0)
        u.set_extra_states(0)


def np_augment(P, pose):
    """stateAugmentation in numpy: the new clone copies the IMU's (theta, p) rows and columns, inserted at `pose`"""
    n = P.shape[0]
    src = np.concatenate([np.arange(pose), [0, 1, 2, 6, 7, 8], np.arange(pose, n)])
    return np.ascontiguousarray(P[np.ix_(src, src)])


def prepare(u, case, route):
    """The resident covariance (dimension case.win.n) and its factor by `route`; inside options() (cov_augment reads the extra states)."""
    w = case.win
    leg, pose = w.flags.leg_dim, w.flags.leg_dim + 6 * w.N
    if route in ('none', 'prefactored'):
        u.cov_set(w.P)
        if route == 'prefactored':
            u.cov_prefactor()
    elif route == 'augmented':
        keep = np.concatenate([np.arange(pose - 6), np.arange(pose, w.n)])
        u.cov_set(w.P[np.ix_(keep, keep)])
        u.cov_prefactor()
        u.cov_augment()
    else:
        assert route == 'marginalised'
        u.cov_set(np_augment(w.P, pose))
        u.cov_prefactor()
        u.cov_remove_clones(leg, [0])
    st = capi.debug_factor_state(u)
    assert st['res_n'] == w.n, st
    return st


def stage_and_run(u, case, entering=True):
    w = case.win
    u.upload(w, resident_cov=True)
    if w.n_nui:
        u.upload_nuisance_poses(w.nui)
    u.upload_slam_features(case.cid.d, case.slam)
    if entering:
        u.upload_new_features(w, case.cid.d, case.new)
    u.run_update()
    u.sync()
    return u.download()


@dataclasses.dataclass
class Outcome:
    got: dict          # the update's dx, P_new, ...
    blocks: tuple      # H_1, H_2, r_1 as the device holds them
    dx_new: np.ndarray
    P_aug: np.ndarray
    st: dict
    S_aug: object      # the resident factor afterwards, or None
    S_twin: object     # what the twin's cov_commit left, or None (Schmidt: no factor behind the update)
    st_before: dict


def run_case(u, tw, case, route):
    """The update on both handles, cov_commit on the twin, the new call on `u`."""
    with options(u, case):
        st0 = prepare(u, case, route)
        got = stage_and_run(u, case)
        blocks = u.download_new_feature_blocks()
        dx_new = u.cov_commit_new_features_fac()
        P_aug = u.cov_get()
        st = capi.debug_factor_state(u)
        S_aug = capi.debug_factor(u) if st['fac_valid'] else None
    S_twin = None
    if tw is not None:
        with options(tw, case):
            prepare(tw, case, route)
            got2 = stage_and_run(tw, case)
            tw.cov_commit()
            st2 = capi.debug_factor_state(tw)
            if st2['fac_valid']:
                S_twin = capi.debug_factor(tw)
        assert np.array_equal(got2['dx'], got['dx']) and np.array_equal(got2['P_new'], got['P_new'])
    return Outcome(got, blocks, dx_new, P_aug, st, S_aug, S_twin, st0)


def check_P(case, o):
    """P_aug's new blocks and dx_new against the extended tail within TAIL_TOL, the moved blocks bit for bit, exact symmetry"""
    cid, w, tail = case.cid, case.win, case.tail
    n, sz = w.n, cid.d * cid.k
    H_1, H_2, r_1 = o.blocks
    assert o.got['updated']
    ref = ec.tail_ext(H_1, H_2, r_1, o.got['dx'], o.got['P_new'], w.flags.noise_feature ** 2, tail, ref_ldlt=cid.ldlt)
    assert o.P_aug.shape == (n + sz, n + sz) and o.dx_new.shape == (sz,)
    gb, rb = ec.tail_blocks(o.P_aug, n, sz, tail), ec.tail_blocks(ref['P_aug'], n, sz, tail)
    err = {q: ec.block_err(gb[q], rb[q]) for q in gb if q.startswith('P2')}
    err['dx_new'] = float(np.abs(o.dx_new.astype(ec.LD) - ref['dx_new']).max() / ref['dx_scale'])
    print('entering factor %s: P %s (bound %.1e)' % (cid, {q: '%.2e' % v for q, v in err.items()}, ec.TAIL_TOL))
    assert set(err) == ({'P21_front', 'P21_behind', 'P22', 'dx_new'} if tail else {'P21_front', 'P22', 'dx_new'})
    for q, v in err.items():
        assert v <= ec.TAIL_TOL, (q, v)
    n0 = n - tail
    keep = np.concatenate([np.arange(n0), np.arange(n0 + sz, n + sz)])
    assert np.array_equal(o.P_aug[np.ix_(keep, keep)], 0.5 * (o.got['P_new'] + o.got['P_new'].T))
    assert np.array_equal(o.P_aug, o.P_aug.T)
    assert o.st['res_n'] == n + sz


def check_S(case, o, kf_expected=None):
    """the widened factor: state, old rows and zeros bit for bit, G and sigma R^-1 within their bars, S S^T against the device's P_aug"""
    cid, w = case.cid, case.win
    n, sz = w.n, cid.d * cid.k
    H_1, H_2, r_1 = o.blocks
    assert o.S_twin is not None and o.S_aug is not None
    kf = o.S_twin.shape[1]
    if kf_expected is not None:
        assert kf == kf_expected, (kf, kf_expected)
    assert o.st == dict(fac_valid=1, fac_n=n + sz, fac_k=kf + sz, res_n=n + sz), o.st
    ref = fc.s_aug_ext(H_1, H_2, r_1, o.S_twin, w.flags.noise_feature, 0, cid.ldlt)
    bad, fig = fc.violations(o.S_aug, o.S_twin, ref, cid.d)
    fig['SSt'] = rel(o.S_aug @ o.S_aug.T, o.P_aug)
    print('entering factor %s: kf %d S %s (bounds G %.1e own %.1e)' % (cid, kf, {q: '%.2e' % v for q, v in fig.items()}, fc.G_TOL, fc.RINV_TOL))
    assert not bad, (bad, fig)
    assert fig['SSt'] < 1e-12, fig   # (the figure tests/test_gpu_cov_edits.py uses for a committed factor)


@pytest.mark.parametrize('cid,route', RUNS, ids=RUN_IDS)
def test_augmented_covariance_and_factor_block_by_block(upd, twin, cid, route):
    case = ec.make_case(cid)
    n = case.win.n
    o = run_case(upd, twin, case, route)
    check_P(case, o)
    if case.win.n_nui:   # a Schmidt update leaves no factor: dropped, P as above
        assert o.st['fac_valid'] == 0 and o.S_twin is None
        return
    if route != 'none' and n <= 224:   # (beyond 224 states there is no prefactorisation: the update factors its prior itself)
        assert o.st_before['fac_valid'] == 1 and o.st_before['fac_k'] == {'prefactored': n, 'augmented': n - 6, 'marginalised': n + 6}[route]
        check_S(case, o, o.st_before['fac_k'])
    else:
        assert o.st_before['fac_valid'] == 0
        check_S(case, o, n)


def test_the_case_list_reaches_the_edges():
    by = {str(c): ec.make_case(c).win.n for c, _ in RUNS}
    assert by['small_d1_k1'] + 1 == 99 and by['small_d3_k20'] + 60 == 166 and by['wide_d3_k1'] == 280
    ld = lambda m: (m + 16) // 16 * 16                                                 # CovBook::ld_for
    assert by['small_d1_k13'] + 13 == 111 and ld(111) == 112 == ld(98)
    assert by['small_d1_k14'] + 14 == 112 and ld(112) == 128 != ld(98)
    assert by['small_d3_k2'] + 6 == 112 and ld(106) == 112
    assert ld(124) == 128 != ld(106)                                            # small_d3_k6: old and new leading dimensions differ
    assert {r for _, r in RUNS} == {'none', 'prefactored', 'augmented', 'marginalised'}
    assert any(ec.make_case(c).win.n_nui for c, _ in RUNS)


def test_a_factor_that_does_not_fit_is_dropped(built):
    """A handle of 13 clones (124 states, factor buffers of 128 columns): n = 106, sz = 18, and the marginalised route's kf = 112 --
    the augmented state fits the handle, the 130 columns of the widened factor do not.  fac_valid == 0, P as everywhere; the
    prefactored route (124 columns) fits on the same handle."""
    case = ec.make_case(ec.CaseId('small', 3, 6))
    u = _new(max_clones=13)
    try:
        o = run_case(u, None, case, 'marginalised')
        assert o.st_before['fac_valid'] == 1 and o.st_before['fac_k'] == 112
        check_P(case, o)
        assert o.st['fac_valid'] == 0 and o.st['res_n'] == 124
        o = run_case(u, None, case, 'prefactored')
        check_P(case, o)
        assert o.st == dict(fac_valid=1, fac_n=124, fac_k=124, res_n=124)
        assert rel(o.S_aug @ o.S_aug.T, o.P_aug) < 1e-12
    finally:
        u.close()


def test_resident_factor_switched_off_drops_it(upd):
    case = ec.make_case(ec.CaseId('small', 3, 6))
    upd._chk(upd.lib.orcvio_msckf_set_option(upd.h, 7, 0), 'set_option')   # ORCVIO_OPT_RESIDENT_FACTOR off
    try:
        o = run_case(upd, None, case, 'none')
        check_P(case, o)
        assert o.st['fac_valid'] == 0
    finally:
        upd._chk(upd.lib.orcvio_msckf_set_option(upd.h, 7, 1), 'set_option')


def commit_rc(u, sz):
    """the bare call: its status, whatever the wrapper remembers of earlier uploads"""
    buf = np.zeros(max(sz, 1))
    u.lib.orcvio_msckf_cov_commit_new_features_fac.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    return u.lib.orcvio_msckf_cov_commit_new_features_fac(u.h, buf.ctypes.data_as(C.POINTER(C.c_double)))


def test_refusals_leave_the_covariance_and_factor_unchanged(upd):
    ERR_INVALID, ERR_CAPACITY = 1, 3
    assert capi.STATUS[ERR_INVALID] == 'ERR_INVALID' and capi.STATUS[ERR_CAPACITY] == 'ERR_CAPACITY'

    def snapshot():
        st = capi.debug_factor_state(upd)
        return upd.cov_get(), st, (capi.debug_factor(upd) if st['fac_valid'] else None)

    def unchanged(before, what):
        now = snapshot()
        assert np.array_equal(now[0], before[0]) and now[1] == before[1], what
        assert (now[2] is None) == (before[2] is None) and (now[2] is None or np.array_equal(now[2], before[2])), what

    # the augmented state exceeds the handle's capacity
    case = ec.make_case(ec.CaseId('wide', 3, 6))
    assert case.win.n <= CAPACITY < case.win.n + 18
    with options(upd, case):
        prepare(upd, case, 'none')
        assert stage_and_run(upd, case)['updated']
        before = snapshot()
        assert commit_rc(upd, 18) == ERR_CAPACITY
        unchanged(before, 'capacity')
    assert np.array_equal(before[0], case.win.P) and before[1]['res_n'] == case.win.n

    # no entering features uploaded (the prefactored factor stands); a second call after a success (the widened factor stands)
    case = ec.make_case(ec.CaseId('small', 3, 6))
    with options(upd, case):
        prepare(upd, case, 'prefactored')
        assert stage_and_run(upd, case, entering=False)['updated']
        before = snapshot()
        assert before[1]['fac_valid'] == 1
        assert commit_rc(upd, 18) == ERR_INVALID
        unchanged(before, 'no entering features')
        stage_and_run(upd, case)
        upd.cov_commit_new_features_fac()
        before = snapshot()
        assert before[1] == dict(fac_valid=1, fac_n=case.win.n + 18, fac_k=case.win.n + 18, res_n=case.win.n + 18)
        assert commit_rc(upd, 18) == ERR_INVALID
        unchanged(before, 'second call')


def next_update(u, P, N, leg, seed):
    """the frame's next update on the resident covariance (40 tracks: more than the 16 projected rows up to which an update may take the
    direct form), everything behind the clones as extra states; committed"""
    extra = P.shape[0] - leg - 6 * N
    w = synth.make_window(N=N, F=40, seed=seed, track_len=(3, min(N, 12)), flags=synth.Flags(leg_dim=leg))
    w = dataclasses.replace(w, P=np.ascontiguousarray(P), n_extra=extra)
    u.set_extra_states(extra)
    try:
        got = u.update_features(w, resident_cov=True, want_P=True)
        u.cov_commit()
    finally:
        u.set_extra_states(0)
    assert got['updated'] and got['stats'][0] > 16
    return w, got


@pytest.mark.parametrize('cid,route', [(ec.CaseId('small', 3, 6), 'augmented'), (ec.CaseId('small', 1, 1), 'marginalised'),
                                       (ec.CaseId('small', 3, 20), 'prefactored'), (ec.CaseId('wide', 3, 1), 'none')],
                         ids=lambda v: str(v))
def test_the_next_update_starts_from_the_widened_factor(upd, twin, cid, route):
    """The payoff.  This handle: the new call, then an update that reads the widened factor (fac_k = kf + sz behind its commit: with
    kf != n that is not the dimension a factorisation of the augmented prior would leave).  The other handle: the old call, then the
    same update, which factors its prior.  Both against the numpy restatement, and against each other."""
    case = ec.make_case(cid)
    w, sz = case.win, cid.d * cid.k
    n, N, leg = w.n, w.N, w.flags.leg_dim
    o = run_case(upd, None, case, route)
    kf = o.st['fac_k'] - sz
    assert o.st['fac_valid'] == 1 and o.st['fac_n'] == o.st['res_n'] == n + sz
    if n <= 224:
        assert kf == {'prefactored': n, 'augmented': n - 6, 'marginalised': n + 6}[route]
    w2, got = next_update(upd, o.P_aug, N, leg, seed=5 + sz)
    after = capi.debug_factor_state(upd)
    assert after == dict(fac_valid=1, fac_n=n + sz, fac_k=kf + sz, res_n=n + sz), after
    with options(twin, case):
        prepare(twin, case, route)
        stage_and_run(twin, case)
        twin.cov_commit_new_features()
        P_old = twin.cov_get()
        assert capi.debug_factor_state(twin)['fac_valid'] == 0
    assert rel(P_old, o.P_aug) < 1e-12
    _, got_old = next_update(twin, P_old, N, leg, seed=5 + sz)
    ref = mirror.msckf_update(w2)
    fig = dict(new_dx=rel(got['dx'], ref['dx']), new_P=rel(got['P_new'], ref['P_new']), old_dx=rel(got_old['dx'], ref['dx']),
               old_P=rel(got_old['P_new'], ref['P_new']), both_dx=rel(got['dx'], got_old['dx']), both_P=rel(got['P_new'], got_old['P_new']))
    print('entering factor payoff %s %s: %s' % (cid, route, {q: '%.2e' % v for q, v in fig.items()}))
    assert np.array_equal(got['accept'], got_old['accept'])
    for q, v in fig.items():
        assert v < UPDATE_TOL, (q, v)


def test_a_handle_that_held_a_larger_state_gives_the_same_bits(upd, built):
    """`upd` first carries the factor of the 280-state case through the call (both factor buffers written at the leading dimension 288),
    then runs a small case; a fresh handle runs only the small one.  dx_new, P_aug, S_aug and the next update bit for bit."""
    big = ec.make_case(ec.CaseId('wide', 3, 1))
    o = run_case(upd, None, big, 'none')
    assert o.st['fac_valid'] == 1 and o.st['fac_n'] == 283
    next_update(upd, o.P_aug, big.win.N, 46, seed=2)
    case = ec.make_case(ec.CaseId('small', 3, 6))
    fresh = _new()
    try:
        outs = []
        for u in (upd, fresh):
            o = run_case(u, None, case, 'augmented')
            _, got = next_update(u, o.P_aug, case.win.N, 22, seed=9)
            outs.append((o.dx_new, o.P_aug, o.S_aug, got['dx'], got['P_new'], capi.debug_factor(u), o.st))
        for a, b in zip(*outs):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    finally:
        fresh.close()
