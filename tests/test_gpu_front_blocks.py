"""GPU: the feature front end -- feature_body (k_feature, k_front), the Grams (k_gram_pair, the Gram items of k_front) and the assembly
of A (k_assemble_A, assemble_entry inside k_front, the assembly deferred behind k_front) -- TRACK BY TRACK and element by element against
the 60-digit reference of tests/front_cases.py, at the shapes where each mechanism takes another path, on every route the shape admits:
    forked     set_fused_front(False): k_feature, k_gram_pair, k_assemble_A
    deferred   k_front leaves the Grams, A is assembled by the consumer (read here with debug_read 'A': the same assemble_entry)
    inlaunch   k_front assembles A itself (NA > 192)
The route that ran is read from the handle (debug_read 'front': would the upload take k_front, is A still to be assembled) with
front_fallbacks unchanged, and must be the one asked for.  The bars (front_cases.K_G, K_GAMMA, summation_c) come from the float64
restatements and from the summation trees of the code; nothing measured on the device enters them.

Bit for bit between the routes.  k_feature and k_front both instantiate the ONE template feature_body<NPASS, PAD_BARRIERS>
(msckf_kernels.hpp); PAD_BARRIERS changes the kind of store (st_pub), the barriers an absent track keeps company, and nothing of the
arithmetic; k_front's second team runs the body on the threads (local + 128) & 255, i.e. tid 0..255 again.  gamma, T3 and Xobs of the
two routes are therefore compared bit for bit; A, whose summation trees differ (16 wavefronts against 8, other row chunks), only
through the reference.

Diagnostics build with the stack materialised (debug_read 'T3', 'Xobs', 'obs_pos', 'S', 'Gpart', 'Hs', 'A'); gamma and the accept mask
are checked on the product build too."""
import numpy as np
import pytest

from orcvio_amd import capi
import front_cases as fc

pytestmark = pytest.mark.gpu

class Front:
    """One handle of the diagnostics build; the first run of every (case, route) is kept and shared."""

    def __init__(self):
        self.upd = capi.MsckfUpdater(device=0, max_clones=60, max_features=1400, max_observations=8192, debug_hooks=True)
        self.upd.set_materialize_stack(True)
        self.done = {}

    def run(self, cid, route):
        """everything the front end of one update_features left, and the route it took"""
        case = fc.make_case(cid)
        upd = self.upd
        upd.set_fused_front(route != 'forked')
        before = upd.counters()['front_fallbacks']
        out = upd.update_features(case.win)
        fr = capi.debug_read(upd, 'front')            # (before 'A': reading A assembles a deferred one)
        assert upd.counters()['front_fallbacks'] == before, 'the fused front end fell back to the forked route'
        ran = 'forked' if not fr['fused'] else ('deferred' if fr['deferred'] else 'inlaunch')
        assert ran == route, (cid, route, fr)
        assert (fr['F'], fr['N'], fr['nobs']) == (case.win.F, case.win.N, int(case.win.obs_ptr[-1]))
        assert (fr['chunks'], fr['rows_per_chunk']) == (fc.forked_chunks(case.win.F) if route == 'forked' else fc.fused_chunks(case.win.F))
        got = dict(gamma=out['gamma'].copy(), accept=out['accept'].copy(), chunks=fr['chunks'], rows_per_chunk=fr['rows_per_chunk'])
        for k in ('T3', 'Xobs', 'obs_pos', 'S', 'Gpart', 'Hs', 'A'):
            got[k] = capi.debug_read(upd, k)
        assert got['Hs'].shape[0] == fc.row_ptr(case.win)[-1]
        return got

    def first(self, cid, route):
        if (cid, route) not in self.done:
            self.done[(cid, route)] = self.run(cid, route)
        return self.done[(cid, route)]


@pytest.fixture(scope='module')
def front(built):
    f = Front()
    yield f
    f.upd.close()


@pytest.fixture(scope='module')
def product(built):
    u = capi.MsckfUpdater(device=0, max_clones=60, max_features=1400, max_observations=8192)
    yield u
    u.close()


def _check(cid, route, got, tag):
    case = fc.make_case(cid)
    f1, bad1 = fc.check_tracks(case, got)
    f2, bad2 = fc.check_window(case, got, route)
    print('front-blocks %s %s%s: gamma %.1f u (bar %.0f), X^T X - T3^T T3 %.1f, Hs^T Hs %.1f u B (bar %.0f), A %.1f u sum B (bar %.0f), '
          'S %.3f, sum Gpart %.3f of their summation bars' % (cid, route, tag, f1['gamma'], fc.K_GAMMA, f1['gram'], f1['Hs'], fc.K_G, f2['A'],
                                                              f2['A_bar'], f2['S'], f2['Gpart']))
    assert not bad1, bad1[:5]
    assert not bad2, bad2[:5]


def _same_bits(a, b, keys):
    return [k for k in keys if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


@pytest.mark.parametrize('cid,route', [(c, r) for c in fc.CASES for r in fc.routes_of(c)])
def test_front_end_track_by_track(front, cid, route):
    """Every track's accept, gamma, X^T X - T3^T T3 and Hs^T Hs; the rows of the rejected and of the short tracks exactly zero; S, the
    partial Grams and A element by element; and a second run of the same input on the same route to the bit."""
    got = front.first(cid, route)
    _check(cid, route, got, '')
    again = front.run(cid, route)
    assert not _same_bits(got, again, ('gamma', 'T3', 'Xobs', 'A'))


@pytest.mark.parametrize('cid', [c for c in fc.CASES if len(fc.routes_of(c)) == 2])
def test_routes_agree_to_the_bit_in_what_feature_body_writes(front, cid):
    a, b = (front.first(cid, r) for r in fc.routes_of(cid))
    assert np.array_equal(a['accept'], b['accept'])
    assert not _same_bits(a, b, ('gamma', 'T3', 'Xobs'))


@pytest.mark.parametrize('route', fc.routes_of(fc.LEFTOVER_PAIR[1]))
def test_nothing_is_left_of_a_larger_window(front, route):
    """F = 1366 (five partial Grams, 3415 observations) and then the N = 4 window of six tracks on the same handle: every check of the
    small one, whose Xobs, T3, S and Gpart stand where the large one's stood."""
    big, small = fc.LEFTOVER_PAIR
    front.run(big, 'forked')
    _check(small, route, front.run(small, route), ' behind ' + big)


@pytest.mark.parametrize('cid', fc.CASES)
def test_gamma_and_mask_on_the_product_build(product, cid):
    """update_features of the product library on its default route: accept identical, every gamma within K_GAMMA u of its own
    reference, NaN and 0 below two observations."""
    case = fc.make_case(cid)
    out = product.update_features(case.win)
    f, bad = fc.check_tracks(case, out, need=('gamma',))
    print('front-blocks %s product: gamma %.1f u (bar %.0f)' % (cid, f['gamma'], fc.K_GAMMA))
    assert not bad, bad[:5]
