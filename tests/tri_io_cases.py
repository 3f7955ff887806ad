"""Inputs and the reference chain of the armed in-place update (orcvio_msckf_io_triangulate): the mirror's triangulation with a mode
per track, the invalid tracks removed, then the mirror's update or frame at the mirror's positions.  Shared by
test_tri_io_inputs.py (CPU: the preconditions of the cases) and test_gpu_io_triangulate*.py; every reference is computed once."""
import dataclasses

import numpy as np

from orcvio_amd import synth
from oracle import mirror, mirror_frame, mirror_triangulate as mt, oracle

KEEP, ALL, ALL_BUT_LAST = 0, 1, 2
TOL = 1e-6   # tests/test_gpu_triangulate.py's
EUROC = dict(use_larvio=1)
KITTI = dict(use_larvio=0, use_left_perturbation=0, noise_feature=1.0, discard_large_update=1)
FLAG_SETS = {'euroc': (EUROC, None), 'kitti': (KITTI, 0.008)}   # tests/test_gpu_step_oracle.py's
NSLAM = 12
_CACHE = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ends_at_newest(w):
    """Tracks whose last listed observation is on the newest clone: the reference's if_tracked_now."""
    last = w.obs_clone[np.maximum(w.obs_ptr[1:] - 1, 0)]
    return (np.diff(w.obs_ptr) > 0) & (last == w.N - 1)


def select_tracks(w, keep, p_w=None, drop_last=None):
    """The window with the tracks of `keep` only (at positions p_w); drop_last: tracks that lose their last listed observation."""
    F = w.F
    keep = np.ones(F, bool) if keep is None else np.asarray(keep, bool)
    drop = np.zeros(F, bool) if drop_last is None else np.asarray(drop_last, bool)
    ptr, idx = [0], []
    for j in np.flatnonzero(keep):
        lo, hi = int(w.obs_ptr[j]), int(w.obs_ptr[j + 1]) - (1 if drop[j] else 0)
        idx += list(range(lo, max(hi, lo)))
        ptr.append(len(idx))
    idx = np.array(idx, np.int64)
    pw = w.p_w if p_w is None else p_w
    return dataclasses.replace(w, p_w=np.ascontiguousarray(pw[keep]).reshape(-1, 3), obs_ptr=np.array(ptr, np.int32),
                               obs_clone=np.ascontiguousarray(w.obs_clone[idx]), obs_z=np.ascontiguousarray(w.obs_z[idx]).reshape(-1, 2),
                               obs_zvel=np.ascontiguousarray(w.obs_zvel[idx]).reshape(-1, 2))


def mirror_tri(w, mode=None, cfg=None):
    """oracle/mirror_triangulate.py with a mode per track: KEEP tracks valid at their given position, ALL_BUT_LAST tracks
    triangulated without their last listed observation."""
    mode = np.full(w.F, ALL, np.int32) if mode is None else np.asarray(mode, np.int32)
    out = mt.triangulate_tracks(select_tracks(w, None, drop_last=mode == ALL_BUT_LAST), cfg)
    k = mode == KEEP
    out['valid'][k] = 1; out['flags'][k] = 0; out['p_w'][k] = w.p_w[k]
    out['solution'][k] = np.nan; out['cost'][k] = np.nan
    return out


def kept_window(w, tri):
    return select_tracks(w, tri['valid'] == 1, tri['p_w'])


# ---- the windows of the io_update tests: name -> (window, mode or None, mixed) -----------------------------------------------
def _windows():
    a = synth.config_window(1)
    b = synth.make_window(N=12, F=80, seed=17, track_len=(2, 10), outlier_frac=0.2)
    c = synth.make_window(N=6, F=24, seed=4, track_len=(2, 6), outlier_frac=0.2)
    return {'config1': (a, None, True), 'mixed80': (b, None, True), 'small24': (c, None, True),
            'small24_abl': (c, np.where(ends_at_newest(c), ALL_BUT_LAST, ALL).astype(np.int32), True)}


def window_case(name):
    return cached(('win', name), _windows)[name]


def window_names():
    return ['config1', 'mixed80', 'small24', 'small24_abl']


def with_modes(name, variant):
    """(window, mode): variant 'all' = the case's own modes; 'abl' = ALL_BUT_LAST on tracks ending at the newest clone; 'keep' = every
    second track KEEP at its given position."""
    w, mode, _ = window_case(name)
    base = np.full(w.F, ALL, np.int32) if mode is None else mode.copy()
    if variant == 'abl':
        base = np.where(ends_at_newest(w), ALL_BUT_LAST, ALL).astype(np.int32)
    elif variant == 'keep':
        base[::2] = KEEP
    return w, base


def window_reference(name, variant='all'):
    """dict(tri, keep, upd): the mirror's triangulation, its valid mask and the oracle's update of the kept tracks."""
    def make():
        w, mode = with_modes(name, variant)
        tri = mirror_tri(w, mode)
        return dict(tri=tri, keep=tri['valid'] == 1, upd=oracle.msckf_update(kept_window(w, tri), want_blocks=False, want_K=False))
    return cached(('ref', name, variant), make)


def gate_margin(w_kept, gamma, accept, prob):
    """Smallest relative distance of a kept track's gamma to its chi-square threshold (2M - 3 degrees of freedom)."""
    table = mirror.chi2_table(prob)
    dof = 2 * np.diff(w_kept.obs_ptr) - 3
    ok = dof > 0
    thr = table[dof[ok]]
    g = np.asarray(gamma)[ok]
    fin = np.isfinite(g)
    return float(np.min(np.abs(g[fin] - thr[fin]) / thr[fin])) if fin.any() else np.inf


# ---- the stream frames of the frame-call tests --------------------------------------------------------------------------------
def stream(name):
    def make():
        fl, sigma_px = FLAG_SETS[name]
        return synth.make_stream(synth.Flags(**fl), sigma_px=sigma_px, cycle=4)
    return cached(('stream', name), make)


def stream_reference(name, apply_dx=0):
    """Per frame: dict(tri, keep, ref) with ref = mirror_frame.step_frame on the kept tracks at the mirror's positions, the
    covariance carried from frame to frame."""
    def make():
        frames, P0 = stream(name)
        table = mirror.chi2_table(frames[0]['w'].flags.chi2_prob)
        P, out = P0, []
        for fr in frames:
            tri = mirror_tri(fr['w'])
            wk = kept_window(fr['w'], tri)
            ref = mirror_frame.step_frame(P, dict(fr, w=wk), 1, apply_dx, table=table)
            out.append(dict(tri=tri, keep=tri['valid'] == 1, ref=ref, wk=wk))
            P = ref['P']
        return out
    return cached(('stream_ref', name, apply_dx), make)


def gamma_err(got, ref):
    from helpers import rel
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    return rel(got[~nan], ref[~nan]) if (~nan).any() else 0.0
