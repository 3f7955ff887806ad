"""orcvio_msckf_zupt_check_feat -- checkZUPTFeat's decision (src/orcvio.cpp:3081-3100) on the pixel distances the front end computed --
through ctypes against np.sort(d)[-9]: host arithmetic, no handle, no device."""
import ctypes as C

import numpy as np
import pytest

from orcvio_amd import capi


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.mark.parametrize('n', [0, 19, 20, 21, 200])
def test_the_ninth_largest_distance_decides(built, n):
    rng = np.random.default_rng(n)
    d = rng.uniform(0.0, 5.0, n)
    for max_dis in (0.5, 2.5, 4.9, 6.0):
        got = capi.zupt_check_feat(d, max_dis)
        if n < 20:   # :3082-3086: too few features
            assert got['accept'] == 0 and np.isnan(got['kth'])
        else:
            kth = np.sort(d)[-9]
            assert got['kth'] == kth
            assert got['accept'] == int(kth < max_dis)
    assert d.shape == (n,)


def test_ties_at_the_ninth_largest_and_the_strict_comparison(built):
    d = np.concatenate([np.full(12, 2.0), np.full(5, 3.0), np.linspace(0.1, 1.0, 10)])   # sorted tail: ... 2 2 2 2 | 3 3 3 3 3
    np.random.default_rng(3).shuffle(d)
    kth = np.sort(d)[-9]
    assert kth == 2.0
    got = capi.zupt_check_feat(d, 2.0)
    assert got['kth'] == 2.0 and got['accept'] == 0          # a threshold EQUAL to the ninth largest: kth < max_dis is strict
    assert capi.zupt_check_feat(d, np.nextafter(2.0, 3.0))['accept'] == 1
    assert capi.zupt_check_feat(d, np.nextafter(2.0, 0.0))['accept'] == 0
    before = d.copy()
    capi.zupt_check_feat(d, 1.0)
    assert np.array_equal(d, before)                          # (the selection runs on a copy)


def test_refusals(built):
    lib = capi.load()
    d = np.linspace(0.0, 1.0, 30)
    acc, kth = C.c_int32(7), np.full(1, 7.0)
    call = lib.orcvio_msckf_zupt_check_feat
    assert call(_dp(d), 30, 1.0, C.byref(acc), _dp(kth)) == 0 and acc.value == 1 and kth[0] == np.sort(d)[-9]
    assert call(None, 30, 1.0, C.byref(acc), _dp(kth)) == 1
    assert call(_dp(d), 30, 1.0, None, _dp(kth)) == 1
    assert call(_dp(d), 30, 1.0, C.byref(acc), None) == 1
    assert call(_dp(d), -1, 1.0, C.byref(acc), _dp(kth)) == 1
    for bad in (np.nan, np.inf, -np.inf):
        assert call(_dp(d), 30, bad, C.byref(acc), _dp(kth)) == 1
        e = d.copy()
        e[17] = bad
        assert call(_dp(e), 30, 1.0, C.byref(acc), _dp(kth)) == 1
        with pytest.raises(capi.MsckfError):
            capi.zupt_check_feat(e, 1.0)
    assert call(None, 0, 1.0, C.byref(acc), _dp(kth)) == 0 and acc.value == 0 and np.isnan(kth[0])   # n = 0 needs no list
