"""Preconditions of the inputs of test_gpu_io_triangulate*.py, stated with the mirror alone (no GPU): every window and frame keeps
enough tracks, the mixed ones drop some, no kept track's gate decision can flip on rounding, and the ALL_BUT_LAST case is exercised
(triangulating those tracks over all their observations moves a position by far more than the tolerance)."""
import numpy as np
import pytest

import tri_io_cases as tc
from oracle import mirror_triangulate as mt

MARGIN = 1e-3


@pytest.mark.parametrize('name', tc.window_names())
def test_windows_keep_enough_drop_some_and_gate_clear_of_the_threshold(name):
    w, mode, mixed = tc.window_case(name)
    ref = tc.window_reference(name)
    keep = ref['keep']
    print(name, 'kept', int(keep.sum()), 'of', w.F)
    assert keep.sum() >= 10
    if mixed:
        assert (~keep).sum() >= 3
    margin = tc.gate_margin(tc.kept_window(w, ref['tri']), ref['upd']['gamma'], ref['upd']['accept'], w.flags.chi2_prob)
    print(name, 'smallest gate margin', margin)
    assert margin > MARGIN


@pytest.mark.parametrize('variant', ['abl', 'keep'])
@pytest.mark.parametrize('name', ['config1', 'mixed80', 'small24'])
def test_mode_variants_of_the_windows(name, variant):
    w, mode = tc.with_modes(name, variant)
    ref = tc.window_reference(name, variant)
    assert ref['keep'].sum() >= 10
    margin = tc.gate_margin(tc.kept_window(w, ref['tri']), ref['upd']['gamma'], ref['upd']['accept'], w.flags.chi2_prob)
    print(name, variant, 'kept', int(ref['keep'].sum()), 'of', w.F, 'smallest gate margin', margin)
    assert margin > MARGIN


def test_all_but_last_is_exercised():
    w, mode, _ = tc.window_case('small24_abl')
    abl = mode == tc.ALL_BUT_LAST
    assert abl.sum() >= 3
    ref = tc.window_reference('small24_abl')['tri']
    full = mt.triangulate_tracks(w)
    both = abl & (ref['valid'] == 1) & (full['valid'] == 1)
    assert both.any()
    moved = np.linalg.norm(full['p_w'][both] - ref['p_w'][both], axis=1) / np.linalg.norm(ref['p_w'][both], axis=1)
    print('ALL_BUT_LAST tracks', int(abl.sum()), 'largest relative move over all observations', float(moved.max()))
    assert moved.max() > 100 * tc.TOL


@pytest.mark.parametrize('name', list(tc.FLAG_SETS))
def test_stream_frames(name):
    frames, _ = tc.stream(name)
    refs = tc.stream_reference(name)
    for it, (fr, r) in enumerate(zip(frames, refs)):
        keep = r['keep']
        w = fr['w']
        print(name, 'frame', it, 'kept', int(keep.sum()), 'of', w.F)
        assert keep.sum() >= 10
        margin = tc.gate_margin(r['wk'], r['ref']['gamma'], r['ref']['accept'], w.flags.chi2_prob)
        print(name, 'frame', it, 'smallest gate margin', margin)
        assert margin > MARGIN
        if it < 3:   # the mixed frames; frame 3 is the all-valid one
            assert (~keep).sum() >= 3
    assert refs[3]['keep'].all()
