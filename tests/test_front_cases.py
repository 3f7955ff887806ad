"""CPU: the references, inputs and bars of tests/front_cases.py -- the two evaluations of the reference against each other and against
oracle.mp_reference.msckf_update_mp, the conditions on the inputs, the gate-edge sides, the recorded restatement figures behind K_G and
K_GAMMA, the float64 stand-in through the very checkers the device test uses, and five mutations each of which must fail its bar."""
import numpy as np
import pytest

import front_cases as fc
from oracle import mirror
from oracle import mp_reference as mpr

SHORT = ['a_leg22_N4', 'c_N8', 'd_N9_0111', 'e_N9', 'f_N20_F17']


@pytest.mark.parametrize('cid', SHORT)
def test_two_evaluations_of_gamma_agree(cid):
    """E = H_x P H_x^T in mp and in np.longdouble (the form the long tracks take): within 1/100 of the bar of gamma."""
    case = fc.make_case(cid)
    worst = 0.0
    for j in sorted(set(int(case.rep[j]) for j in fc.live_tracks(case))):
        a, b = fc.reference(case, j, 'mp')['gamma'], fc.reference(case, j, 'ld')['gamma']
        worst = max(worst, abs(a - b) / (fc.U * a))
    print('front-cases %s: mp against longdouble E, worst %.2f u (bar / 100 = %.0f u)' % (cid, worst, fc.K_GAMMA / 100))
    assert worst < fc.K_GAMMA / 100


def test_reference_against_the_whole_update_in_mp():
    """gamma_j of the projector form equals the gamma of oracle.mp_reference.msckf_update_mp (explicit null-space basis from an mp QR)
    to the last bit of a double, and the accept masks agree."""
    case = fc.make_case('a_leg22_N4')
    ref = mpr.msckf_update_mp(case.win, digits=fc.DIGITS)
    _, _, acc, gam = fc.window_reference(case.cid)
    assert np.array_equal(ref['accept'], acc)
    assert np.abs(ref['gamma'] - gam).max() <= 2 * fc.U * np.abs(gam).max()


def test_bars_come_from_the_recorded_figures():
    assert fc.K_G == 10 * max(fc.REF_FIGURES['mirror_G'], fc.REF_FIGURES['oracle_G'])
    assert fc.K_GAMMA == 10 * max(fc.REF_FIGURES['mirror_gamma'], fc.REF_FIGURES['oracle_gamma'])
    assert fc.K_G * fc.U < 3e-13 and fc.K_GAMMA * fc.U < 4e-12     # six decades below the whole-update bars


@pytest.mark.parametrize('cid', fc.CASES)
def test_inputs_and_restatements(cid):
    """Every track is further than 1e-6 thr from the gate (group e: at 1e-8, on the intended side by at least 1e-9), the mask is the
    one the builder wanted, groups b, d, f hold accepted and rejected tracks, and the two float64 restatements stay within the recorded
    figures (twice them: another LAPACK rounds the mirror's SVD differently)."""
    case = fc.make_case(cid)
    win = case.win
    _, _, acc, gam = fc.window_reference(cid)
    live = fc.live_tracks(case)
    assert np.array_equal(acc[live], case.want[live])
    assert all(case.want[j] == -1 and np.isnan(gam[j]) and acc[j] == 0 for j in range(win.F) if j not in live)
    for j in live:
        thr = fc.reference(case, j)['thr']
        if j in case.edge:
            assert case.edge[j] * (gam[j] - thr) >= 1e-9 * thr and abs(gam[j] - thr) <= 1.1 * fc.EDGE_REL * thr
        else:
            assert abs(gam[j] - thr) > 1e-6 * thr
    if cid[0] in 'bdf':
        assert 0 < acc.sum() < len(live)
    if cid[0] == 'e':
        assert sorted(case.edge) == live and [len(range(*win.obs_ptr[j:j + 2])) for j in live] == [m for m in fc.EDGE_LENGTHS for _ in (0, 1)]
    assert all(len(set(win.obs_clone[win.obs_ptr[j]:win.obs_ptr[j + 1]])) == win.obs_ptr[j + 1] - win.obs_ptr[j] for j in range(win.F))
    f = fc.restatement_figures(case)
    print('front-cases %s: restatements %s' % (cid, {k: '%.0f' % v for k, v in f.items()}))
    for k, v in f.items():
        assert v <= 2 * fc.REF_FIGURES[k], (k, v)


def test_the_shapes_are_the_ones_asked_for():
    by = {c: fc.make_case(c) for c in ('a_leg22_N9', 'a_leg22_N20', 'a_leg22_N31', 'a_leg46_N29', 'a_leg22_N41', 'a_leg22_N42', 'a_leg46_N60', 'c_N8', 'b_N32')}
    assert (by['a_leg22_N9'].NA, by['a_leg22_N9'].NAP) == (61, 64)
    assert (by['a_leg22_N20'].NA, by['a_leg22_N20'].NAP) == (127, 128)          # no padding column behind the right-hand side
    assert by['a_leg22_N31'].NA == 193 and by['a_leg22_N31'].routes == ('forked', 'inlaunch')
    assert by['a_leg46_N29'].win.n == 220 and by['a_leg46_N29'].routes == ('forked', 'inlaunch')
    assert by['a_leg22_N41'].NAP == 256 and by['a_leg22_N41'].routes == ('forked',)
    assert (by['a_leg22_N42'].NAP + 63) // 64 == 5 and (by['a_leg46_N60'].NAP, (by['a_leg46_N60'].NAP + 63) // 64) == (400, 7)
    c = by['c_N8'].win
    assert 5 not in set(c.obs_clone) and {0, 1}.issubset(set(np.diff(c.obs_ptr)))
    assert list(c.obs_clone[c.obs_ptr[1]:c.obs_ptr[2]]) == [6, 4, 2, 1] and list(c.obs_clone[:3]) == [0, 3, 7]
    assert sorted(np.diff(by['b_N32'].win.obs_ptr)) == sorted(fc.B_ACCEPTED + fc.B_REJECTED)
    # row chunks: one and two on either route, five on the forked one
    assert [fc.forked_chunks(F)[0] for F in (341, 342, 1366)] == [1, 2, 5] and [fc.fused_chunks(F)[0] for F in (213, 214)] == [1, 2]
    assert (3 * 341, 3 * 342, 3 * 213, 3 * 214) == (1023, 1026, 639, 642)
    assert fc.make_case('f_N4_F1366').routes == ('forked',) and fc.make_case('f_N4_F342').routes == ('forked', 'deferred')
    assert set(fc.make_case('f_N20_F17').win.obs_clone) == set(range(20))


def test_thresholds_of_the_library_are_the_references(built):
    """The gate-edge tracks stand 1e-8 thr from the threshold: the library's table must be scipy's to far less than that."""
    from orcvio_amd import capi
    for dof in sorted({2 * m - 3 for m in range(2, 33)}):
        assert abs(capi.chi2_quantile(dof) - mirror.chi2_threshold(dof)) <= 1e-12 * mirror.chi2_threshold(dof), dof


MODEL_CASES = ['a_leg22_N4', 'a_leg22_N20', 'c_N8', 'd_N9_0111', 'f_N4_F342']


@pytest.mark.parametrize('cid', MODEL_CASES)
def test_the_float64_stand_in_passes_the_checkers(cid):
    case = fc.make_case(cid)
    m = fc.model_front(case)
    f1, bad1 = fc.check_tracks(case, m)
    f2, bad2 = fc.check_window(case, m, 'forked')
    print('front-cases %s: stand-in %s %s' % (cid, {k: '%.1f' % v for k, v in f1.items()}, {k: '%.2f' % v for k, v in f2.items()}))
    assert not bad1 and not bad2, (bad1, bad2)


def _kinds(bad):
    return {b[0] for b in bad}


def test_mutation_a_lost_row_at_a_chunk_boundary():
    case = fc.make_case('f_N4_F342')
    m = fc.model_front(case)
    assert m['chunks'] == 2
    row = m['rows_per_chunk'] - 1           # the last row of the first chunk: a row of an accepted track
    assert m['T3'][row].any()
    m['S'], m['Gpart'] = fc.model_grams(case, m['Xobs'], m['T3'], m['chunks'], m['rows_per_chunk'], drop_row=row)
    m['A'] = fc.assemble_model(case, m['S'], m['Gpart'])
    assert {'Gpart', 'A'} <= _kinds(fc.check_window(case, m, 'forked')[1])


def test_mutation_two_clones_tiles_swapped():
    case = fc.make_case('a_leg22_N20')
    m = fc.model_front(case)
    live = [c for c in range(case.win.N) if m['S'][c].any()]
    m['S'][[live[0], live[1]]] = m['S'][[live[1], live[0]]]
    m['A'] = fc.assemble_model(case, m['S'], m['Gpart'])
    assert {'S', 'A'} <= _kinds(fc.check_window(case, m, 'forked')[1])


def test_mutation_one_entry_of_xobs_off_by_1e_9():
    case = fc.make_case('c_N8')
    m = fc.model_front(case)
    assert not fc.check_tracks(case, m)[1]
    r = int(np.nonzero(m['Xobs'].any(axis=1))[0][3])
    c = int(np.abs(m['Xobs'][r]).argmax())          # (the leading entry of the row)
    m['Xobs'][r, c] += 1e-9 * abs(m['Xobs'][r, c])
    assert 'gram' in _kinds(fc.check_tracks(case, m)[1])


def test_mutation_td_column_zeroed():
    case = fc.make_case('d_N9_0111')
    m = fc.model_front(case)
    assert m['Xobs'][:, 6].any() and m['T3'][:, 6].any()
    m['Xobs'][:, 6] = 0.0
    m['T3'][:, 6] = 0.0
    m['Hs'][:, 6] = 0.0
    assert {'gram', 'Hs'} <= _kinds(fc.check_tracks(case, m)[1])
    S, G = fc.model_grams(case, m['Xobs'], m['T3'], m['chunks'], m['rows_per_chunk'])
    m.update(S=S, Gpart=G, A=fc.assemble_model(case, S, G))
    assert 'A' in _kinds(fc.check_window(case, m, 'forked')[1])


def test_mutation_right_hand_side_read_from_the_column_in_front():
    """N = 20: NA + 1 == NAP, the right-hand side is the last column of the last pass."""
    case = fc.make_case('a_leg22_N20')
    m = fc.model_front(case)
    m['A'] = fc.assemble_model(case, m['S'], m['Gpart'], rhs_e=12)
    assert 'A' in _kinds(fc.check_window(case, m, 'forked')[1])


def test_summation_term_is_derived_from_the_row_counts():
    """c for the benchmark-like shapes, by hand: N = 4, F = 1366 forked -- a clone holds at most 2 x 1025 rows (tracks of two and three
    observations over four clones), 16 wavefronts: rw = 132 rows, 4 x 17 + 1 + 4 = 73; + 1 + 3 over the clones; T3: 824 rows per chunk,
    rw = 52, 4 x 7 + 1 + 4 = 33; + 2 + 2 over five chunks; + 2."""
    assert fc.gram_chain(64, 16) == 4 + 1 + 4 and fc.gram_chain(0, 8) == 0 and fc.gram_chain(640, 8) == 40 + 1 + 3
    case = fc.make_case('f_N4_F1366')
    rows = int(fc.clone_rows(case.win).max())
    assert fc.summation_c(case, 'forked') == fc.gram_chain(rows, 16) + 1 + 3 + 33 + 2 + 2 + 2
    assert fc.summation_c(case, 'forked') < fc.K_G / 10      # (the per-track term carries the bar of A)
