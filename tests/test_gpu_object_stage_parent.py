"""The object update against the PARENT of the commit that moved its host staging into csrc/host/object_stage.hpp
(tests/golden/object_stage_parent.npz, recorded by scripts/make_golden_object_stage.py on a build of that parent): every case of
tests/object_stage_parent_cases.py through every entry point on every handle gives the same integers, and float arrays that are the
parent's bytes -- or, where the parent itself did not give the same bytes five times over (atomics), its first run's values element by
element within four times the spread the PARENT showed over its five runs (the result's run being a sixth draw)."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
import object_stage_parent_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'object_stage_parent.npz'))


@pytest.fixture(scope='module')
def handles(built):
    hs = {}

    def get(mode):
        if mode not in hs:
            hs[mode] = oc.handle(mode)
        return hs[mode]
    yield get
    for u in hs.values():
        u.close()


def test_the_golden_holds_every_case_on_every_handle(golden):
    n = len(oc.keys())
    assert n == len(oc.MODES) * ((len(oc.CASES) - 1) * len(oc.ENTRIES) + 2)
    assert golden['ints'].shape == (n, len(oc.INTS)) and golden['hash'].shape == (n, len(oc.FLOATS), 8)


@pytest.mark.parametrize('mode', oc.MODES)
@pytest.mark.parametrize('case', list(oc.CASES))
def test_case_equals_the_parent_build(handles, golden, case, mode):
    got = oc.run_case(handles(mode), case)
    rows = {e: i for i, (c, m, e) in enumerate(oc.keys()) if (c, m) == (case, mode)}
    assert sorted(got) == sorted(rows)
    for entry, i in rows.items():
        key, g = '%s/%s/%s' % (case, mode, entry), got[entry]
        ints = golden['ints'][i]
        bad = [(oc.INTS[j], int(g['ints'][j]), int(ints[j])) for j in range(len(oc.INTS)) if g['ints'][j] != ints[j]]
        assert not bad, (key, '(field, got, parent)', bad)
        for j, name in enumerate(oc.FLOATS):
            raw = '%s/raw/%s' % (key, name)
            if raw not in golden.files:
                assert np.array_equal(oc.digest(g[name]), golden['hash'][i, j]), (key, 'bytes differ from the parent build in', name)
                continue
            ref, bound = golden[raw], 4.0 * float(golden['%s/spread/%s' % (key, name)])
            assert g[name].shape == ref.shape, (key, name)
            err = float(np.abs(g[name] - ref).max())   # (NaN fails)
            print('%s %s: max |got - parent| %.3e, bound 4 x parent spread %.3e' % (key, name, err, bound))
            assert err <= bound, (key, name, err, bound)
