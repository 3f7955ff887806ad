"""The cases and the reference chain of the armed prune update (tests/prune_tri_cases.py) on the numpy mirror alone: the conditions every
case must meet, that mode ORCVIO_TRI_ALL_MOTION_BUT_LAST is neither of its neighbours on these inputs, the two-observation track, and
that the checks of tests/test_gpu_prune_tri.py catch the three ways of getting the chain wrong.  No device."""
import numpy as np
import pytest

from orcvio_amd import synth
from oracle import mirror_triangulate as mt
from helpers import rel
import prune_tri_cases as pc
import tri_io_cases as tc

TOL = tc.TOL


@pytest.mark.parametrize('case', pc.CASES, ids=pc.case_id)
def test_every_case_meets_its_conditions(case):
    ch = pc.reference(case)   # (check_conditions runs where the reference is made)
    wn, fs, rm, ap = case
    w = pc.window(wn, fs)
    sp, remove = ch['sp'], pc.remove_sets(w.N)[rm]
    assert sp['tri'].F == sp['prune'].F == len(ch['keep']) > 0
    # the tri list: the prune tracks in full, ending at the newest clone; the prune list: their observations in the clones that leave
    assert tc.ends_at_newest(sp['tri']).all()
    assert np.isin(sp['prune'].obs_clone, remove).all() and (np.diff(sp['prune'].obs_ptr) == 2).all()
    for j in range(sp['tri'].F):
        full = sp['tri'].obs_clone[sp['tri'].obs_ptr[j]:sp['tri'].obs_ptr[j + 1]]
        assert (np.diff(full) > 0).all() and np.isin(remove, full).all() and len(full) <= 32
    assert 0 < sp['first'].F <= pc.MAX_FIRST and ch['ref']['dx'] is not None
    assert ch['ref']['n_after'] == w.n - 12


def test_the_set_has_every_kind_of_failure():
    bits = pc.failure_kinds()
    assert bits & mt.FLAG_NO_MOTION and bits & (mt.FLAG_NEG_DEPTH | mt.FLAG_BIG_PROJ), bits


def test_mode_3_differs_from_its_neighbours_on_the_set():
    """ALL checks the motion on the LAST entry, ALL_BUT_LAST triangulates without it: were either wired in instead, some case would show."""
    differs = {tc.ALL: 0, tc.ALL_BUT_LAST: 0}
    for case in pc.CASES:
        ch = pc.reference(case)
        for md in differs:
            other = pc.prune_tri(ch['win2'], np.full(len(ch['keep']), md, np.int32))
            both = ch['keep'] & (other['valid'] == 1)
            if not np.array_equal(other['valid'], ch['tri']['valid']) or (both.any() and rel(other['p_w'][both], ch['tri']['p_w'][both]) > 100 * TOL):
                differs[md] += 1
    print('cases in which mode 3 differs from', differs)
    assert differs[tc.ALL] >= 1 and differs[tc.ALL_BUT_LAST] >= 1


def test_a_two_observation_track_has_no_motion():
    w = synth.make_window(N=6, F=6, seed=8, track_len=2)
    tri = pc.prune_tri(w, cfg=mt.OptimizationConfig(translation_threshold=0.0))
    assert (tri['motion'] == 0.0).all() and (tri['flags'] == mt.FLAG_NO_MOTION).all() and not tri['valid'].any()
    # ... where ALL finds motion between the two and triangulates
    assert tc.mirror_tri(w, cfg=mt.OptimizationConfig(translation_threshold=0.05))['valid'].any()


def _caught(ch, mut):
    """Would check() of the GPU tests see the mutated chain as a failure?"""
    if not np.array_equal(mut['tri']['valid'], ch['tri']['valid']) or not np.array_equal(mut['tri']['flags'], ch['tri']['flags']):
        return True
    k = ch['keep']
    return rel(mut['tri']['p_w'][k], ch['tri']['p_w'][k]) >= TOL or rel(mut['ref']['prune_dx'], ch['ref']['prune_dx']) >= TOL or rel(mut['ref']['P'], ch['ref']['P']) >= TOL


def test_mutations_of_the_chain_are_caught():
    w = pc.window('n12', 'euroc')
    slow = pc.window('n12_slow', 'euroc')
    newest = pc.remove_sets(w.N)['newest']
    good, good_slow = pc.reference(('n12', 'euroc', 'newest', 1)), pc.reference(('n12_slow', 'euroc', 'newest', 1))
    # the motion check on the last entry (ORCVIO_TRI_ALL's): the slowed window's short tracks pass it
    assert _caught(good_slow, pc.chain(slow, newest, 1, motion_last=-1))
    # the triangulation without the last entry (ORCVIO_TRI_ALL_BUT_LAST's)
    assert _caught(good, pc.chain(w, newest, 1, drop_last=True))
    # the poses of the first update NOT incremented although prune_apply_dx = 1
    assert _caught(good, pc.chain(w, newest, 1, increment=False))
    # ... and the chain itself is not caught
    assert not _caught(good, pc.chain(w, newest, 1))
