"""Bit-level fingerprint of the object mapper's six calls (GPU): orcvio_msckf_object_lm / _object_init / _object_init_lm and their
_lite forms run over the edge shapes of the GPU tests (tests/test_gpu_object_{lm,init,lite}.py, taken from the case modules under
tests/), and every call and case leaves ONE sha256 over the raw bytes of its result arrays and its statistics.  Two builds compute the
same thing exactly when their tables are equal: a refactor of the kernels or of the staging is checked by running this file in a
checkout of the parent and in the new tree (it uses nothing but the public capi API and the case modules, so the same file runs in
both) and comparing with --against.
usage: python scripts/gpu_object_mapper_bits.py [--out FILE] [--against FILE_OF_THE_OTHER_BUILD]"""
import argparse
import dataclasses
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from orcvio_amd import capi  # noqa: E402
from orcvio_amd import build as b  # noqa: E402
import object_lm_cases as oc  # noqa: E402
import object_lite_cases as lc  # noqa: E402

TWENTY = [(1, 1), (1, 9), (2, 3), (3, 17), (4, 2), (4, 33), (5, 5), (6, 12), (7, 1), (8, 64), (9, 4), (10, 31), (11, 7), (12, 30),
          (12, 65), (13, 2), (14, 16), (15, 3), (16, 8), (16, 128)]
LITE_FRAMES = [(0, 2, 1), (0, 16, 2), (0, 17, 2), (0, 65, 1), (0, 128, 2), (2, 2, 2), (2, 17, 2), (2, 65, 2), (2, 128, 1)]   # (new_bbox, F, seed)
STAT_KEYS = ('cost0', 'cost', 'iterations', 'evaluations', 'status')


def digest(parts):
    h = hashlib.sha256()
    for p in parts:
        a = np.ascontiguousarray(p)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def lm_parts(tracks, stats):
    parts = []
    for t, s in zip(tracks, stats):
        parts += [np.asarray(t.wTo, dtype=np.float64), np.asarray(t.shape, dtype=np.float64), np.asarray(t.kps, dtype=np.float64),
                  np.array([s['cost0'], s['cost']], dtype=np.float64), np.array([s[k] for k in STAT_KEYS[2:]], dtype=np.int64)]
    return parts


def init_parts(inits):
    parts = []
    for r in inits:
        parts += [np.asarray(r[k]) for k in ('wTo', 'kps_world', 'kp_used', 'kp_obs', 'kp_cond', 'R', 't', 'sigma')]
        parts += [np.array([r['scale']], dtype=np.float64), np.array([r['n_used'], r['status']], dtype=np.int64)]
    return parts


def lite_init_parts(inits):
    parts = []
    for r in inits:
        parts += [np.asarray(r['wTo'], dtype=np.float64), np.array([r['d']], dtype=np.float64), np.array([r['status']], dtype=np.int64)]
    return parts


def unzip(cases):
    return tuple([c[i] for c in cases] for i in range(len(cases[0])))


def degenerate():
    """A box without width in front of an identity camera: the lite start is not finite, the optimiser behind it skips the object."""
    obj, ms = lc.synthetic(2, 1)
    frames = [dict(obj.frames[0], wTc=np.eye(4), bbox=np.array([0.25, -0.125, 0.25, 0.125]))] + list(obj.frames[1:])
    return dataclasses.replace(obj, frames=frames), ms


def run(upd):
    table = {}
    # ---- object_lm: the one_car cases (F = 1, NaN detections among them), left / right, new_bbox 0 and 2, both weightings
    for name, c in oc.CASES.items():
        for left in (True, False):
            obj, ms, mk = oc.one_car(c['n_frames'], c['nan_case'], c['starts'][0])
            table['object_lm/%s/%s' % (name, 'left' if left else 'right')] = digest(lm_parts(*upd.object_lm([obj], [ms], [mk], left, c['new_bbox'], c['weights'])))
    for n_frames, nan_case in ((1, 0), (2, 1), (2, 2)):
        for left in (True, False):
            for new_bbox in (0, 2):
                for wname, w in (('refw', oc.WEIGHTS_REF), ('unitw', oc.WEIGHTS_UNIT)):
                    obj, ms, mk = oc.one_car(n_frames, nan_case, 2)
                    key = 'object_lm/grid/f%d-nan%d-%s-bbox%d-%s' % (n_frames, nan_case, 'left' if left else 'right', new_bbox, wname)
                    table[key] = digest(lm_parts(*upd.object_lm([obj], [ms], [mk], left, new_bbox, w)))
    for K, F, w in ((1, 5, oc.WEIGHTS_UNIT), (16, 4, oc.WEIGHTS_UNIT), (12, 65, oc.WEIGHTS_REF), (5, 128, oc.WEIGHTS_REF)):
        obj, ms, mk = oc.synthetic(K, F, 1, start_scale=0.3, start=0)
        table['object_lm/synthetic/K%d-F%d' % (K, F)] = digest(lm_parts(*upd.object_lm([obj], [ms], [mk], True, 0, w)))
    twenty = [oc.synthetic(K, F, seed=3 + i) for i, (K, F) in enumerate(TWENTY)]
    objs, mss, mks = unzip(twenty)
    table['object_lm/batch-of-twenty'] = digest(lm_parts(*upd.object_lm(objs, mss, mks, True, 0, oc.WEIGHTS_UNIT)))
    # ---- object_init and object_init_lm: the car, the synthetic shapes, the batch; the three pose forms
    init_cases = {'car_f4': oc.one_car(4), 'car_f5': oc.one_car(5), 'car_f47': oc.one_car(47), 'K4_F64': oc.synthetic(4, 64, 2),
                  'K12_F65': oc.synthetic(12, 65, 1), 'K16_F128': oc.synthetic(16, 128, 1), 'car_f2_nan': oc.one_car(2, 2, 0)}
    for form in (0, 1, 2):
        for name, (obj, ms, mk) in init_cases.items():
            table['object_init/%s/form%d' % (name, form)] = digest(init_parts(upd.object_init([obj], [mk], pose_form=form)))
        table['object_init/batch-of-twenty/form%d' % form] = digest(init_parts(upd.object_init(objs, mks, pose_form=form)))
        both = [oc.one_car(33), oc.one_car(47), oc.one_car(2, 2, 0)] + twenty[:8]   # (a failed start among them: the skip word)
        o2, ms2, mk2 = unzip(both)
        inits, tracks, stats = upd.object_init_lm(o2, ms2, mk2, True, 0, oc.WEIGHTS_REF, pose_form=form)
        table['object_init_lm/batch/form%d' % form] = digest(init_parts(inits) + lm_parts(tracks, stats))
    # ---- the lite calls: F = 1, 2, 16, 17, 65, 128; the weights and the regulariser's repeats; the batch of five
    for new_bbox, F, seed in LITE_FRAMES:
        obj, ms = lc.synthetic(F, seed)
        table['object_lm_lite/bbox%d-F%d-s%d' % (new_bbox, F, seed)] = digest(lm_parts(*upd.object_lm_lite([obj], [ms], True, new_bbox, max_iter=lc.MAX_ITER)))
    for seed, new_bbox in ((2, 0), (1, 2)):
        obj, ms = lc.synthetic(1, seed)
        for left in (True, False):
            key = 'object_lm_lite/F1-s%d-bbox%d-%s' % (seed, new_bbox, 'left' if left else 'right')
            table[key] = digest(lm_parts(*upd.object_lm_lite([obj], [ms], left, new_bbox, max_iter=lc.MAX_ITER)))
    for F in (2, 17):
        for new_bbox in (0, 2):
            for wname, w in (('unitw', lc.UNIT), ('refw', lc.REFW)):
                for reg in (0, 1):
                    obj, ms = lc.synthetic(F, 2)
                    key = 'object_lm_lite/grid/F%d-bbox%d-%s-reg%d' % (F, new_bbox, wname, reg)
                    table[key] = digest(lm_parts(*upd.object_lm_lite([obj], [ms], False, new_bbox, w, reg, max_iter=lc.MAX_ITER)))
    five = [lc.synthetic(F, seed) for F, seed in ((1, 2), (2, 2), (17, 2), (65, 1), (128, 2))]
    o5, ms5 = unzip(five)
    table['object_lm_lite/batch-of-five'] = digest(lm_parts(*upd.object_lm_lite(o5, ms5, True, 0, max_iter=lc.MAX_ITER)))
    table['object_lm_lite/one_car-f47'] = digest(lm_parts(*upd.object_lm_lite([lc.one_car(47, 2)[0]], [lc.one_car(47, 2)[1]], True, 0, lc.REFW, max_iter=lc.MAX_ITER)))
    starts = [lc.one_car(47)] + [lc.synthetic(F, seed) for F, seed in ((2, 1), (17, 2), (65, 1))]
    for form in (0, 1, 2):
        os_, mss_ = unzip(starts + [degenerate()])
        table['object_init_lite/batch/form%d' % form] = digest(lite_init_parts(upd.object_init_lite(os_, mss_, form, (1.1, 0.9, 1.2))))
        for new_bbox in (0, 2):
            o6, ms6 = unzip(starts[:3] + [degenerate()] + [lc.synthetic(17, 1)])
            inits, tracks, stats = upd.object_init_lm_lite(o6, ms6, True, new_bbox, max_iter=lc.MAX_ITER, pose_form=form)
            table['object_init_lm_lite/batch/form%d-bbox%d' % (form, new_bbox)] = digest(lite_init_parts(inits) + lm_parts(tracks, stats))
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--against', default=None, help='the table of another build: every digest must be equal')
    args = ap.parse_args()
    upd = capi.MsckfUpdater(device=0, max_clones=48, max_features=64, max_observations=1024)
    try:
        table = run(upd)
    finally:
        upd.close()
    rec = dict(source_sha16=b.source_sha16(), n=len(table), digests=table)
    rc = 0
    if args.against:
        other = json.load(open(args.against))
        diff = sorted(k for k in set(table) | set(other['digests']) if table.get(k) != other['digests'].get(k))
        rec['against'] = dict(source_sha16=other['source_sha16'], n=other['n'], differing=diff, verdict='equal' if not diff else 'DIFFERENT')
        rc = 0 if not diff else 1
    line = json.dumps(rec, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(json.dumps(dict(n=rec['n'], source_sha16=rec['source_sha16'], against=rec.get('against'))))
    return rc


if __name__ == '__main__':
    sys.exit(main())
