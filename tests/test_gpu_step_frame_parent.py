"""The one-call frames against the PARENT of the commit that split step_frame_impl into phases (tests/golden/step_frame_parent.npz,
recorded by scripts/make_golden_step_frame.py on a build of that parent): every stream of tests/step_frame_parent_cases.py, in every
launch form, gives the same integers and the same bytes -- results, NaN positions, the covariance behind each frame.  No tolerance:
no kernel changed, so a difference is a finding about the host's sequence of launches and copies."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
import step_frame_parent_cases as sc

pytestmark = pytest.mark.gpu
COLS = sc.INTS + tuple('stats[%d]' % i for i in range(8)) + tuple('prune_stats[%d]' % i for i in range(8)) + ('evaluated', 'agree', 'chosen[0]', 'chosen[1]')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'step_frame_parent.npz'))


def test_the_golden_holds_every_stream_in_every_form(golden):
    assert sorted(k for k in golden.files if k.endswith('/ints')) == sorted('%s/%s/ints' % (n, m) for n in sc.STREAMS for m in sc.MODES)
    for n in sc.STREAMS:
        for m in sc.MODES:
            assert golden['%s/%s/ints' % (n, m)].shape == (8, len(COLS)) and golden['%s/%s/hash' % (n, m)].shape == (8, len(sc.HASHED), 8)


@pytest.mark.parametrize('mode', sc.MODES)
@pytest.mark.parametrize('name', list(sc.STREAMS))
def test_stream_equals_the_parent_build(built, golden, name, mode):
    got = sc.run_stream(name, mode)
    ints, hashes = golden['%s/%s/ints' % (name, mode)], golden['%s/%s/hash' % (name, mode)]
    assert got['ints'].shape == ints.shape
    for it in range(len(ints)):
        bad = [(COLS[j], int(got['ints'][it, j]), int(ints[it, j])) for j in range(len(COLS)) if got['ints'][it, j] != ints[it, j]]
        assert not bad, (name, mode, 'frame', it, '(field, got, parent)', bad)
        bad = [k for j, k in enumerate(sc.HASHED) if not np.array_equal(got['hash'][it, j], hashes[it, j])]
        assert not bad, (name, mode, 'frame', it, 'bytes differ from the parent build in', bad)
    if mode == 'product':   # (implied by the hashes; here so that a mismatch can be read)
        assert np.array_equal(got['last_dx'], golden['%s/last_dx' % name], equal_nan=True)
        assert np.array_equal(got['last_diag'], golden['%s/last_diag' % name])
