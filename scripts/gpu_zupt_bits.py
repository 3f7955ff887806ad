"""cov_zupt and cov_zupt_frame on fixed inputs with the library of ONE checkout, the results to an npz -- to compare the bits of two
builds (this tree's against a parent commit's, after a change to zupt_ops.hpp that moves the kernels' instruction streams):
  python scripts/gpu_zupt_bits.py run  ROOT OUT.npz     the package under ROOT (a checkout whose library is built), in a process of its own
  python scripts/gpu_zupt_bits.py diff A.npz B.npz      the arrays that differ (exit status 1 if any does)
Nine shapes (leg 22 / 46, the tile edges, 3-d feature states, a nuisance block, 20 and 30 clones), each without and with a resident
factor: the update, a second update on its result (which reads the factor k_zupt_fac wrote), and the frame call -- 108 arrays."""
import sys

import numpy as np


def spd(n, seed):
    g = np.random.default_rng(seed)
    A = g.standard_normal((n, n)) / np.sqrt(n)
    P = 1e-3 * (A @ A.T) + np.diag(g.uniform(1e-4, 1e-2, n))
    return 0.5 * (P + P.T)


def run(root, out):
    sys.path.insert(0, root)
    from orcvio_amd import capi, synth
    assert capi.__file__.startswith(root), capi.__file__
    u = capi.MsckfUpdater(device=0, max_clones=40, max_features=256, max_observations=4096)
    res = {}
    for leg, N, extra, nui in ((22, 2, 0, 0), (46, 2, 0, 0), (22, 7, 0, 0), (22, 7, 1, 0), (22, 3, 9, 0), (22, 4, 6, 1), (22, 20, 0, 0),
                               (22, 20, 12, 0), (46, 30, 0, 0)):
        n = leg + 6 * N + extra
        g = np.random.default_rng(n)
        r = 1e-3 * g.standard_normal(9)
        Phi = np.ascontiguousarray(np.eye(leg) + 1e-3 * g.standard_normal((leg, leg)))
        G = g.standard_normal((leg, 12))
        Q = np.ascontiguousarray(1e-8 * G @ G.T)
        for fac in (0, 1):
            u.set_extra_states(extra)
            u.set_schmidt_states(nui)
            u.cov_set(spd(n, n))
            if fac:
                u.cov_prefactor()
            key = f'{leg}_{N}_{extra}_{nui}_{fac}'
            got = u.cov_zupt(leg, N, r, synth.ZUPT_NOISES)
            res[key + '_dx'], res[key + '_P'] = got['dx'], u.cov_get()
            got = u.cov_zupt(leg, N, 0.5 * r, synth.ZUPT_NOISES)
            res[key + '_dx2'], res[key + '_P2'] = got['dx'], u.cov_get()
            u.cov_set(spd(n - 6, n + 1))
            if fac:
                u.cov_prefactor()
            got = u.cov_zupt_frame(leg, N, r, synth.ZUPT_NOISES, None if fac else Phi, None if fac else Q, True, True)
            res[key + '_fdx'], res[key + '_fP'] = got['dx'], u.cov_get()
    u.set_extra_states(0)
    u.set_schmidt_states(0)
    u.close()
    np.savez(out, **res)
    print('wrote', out, len(res), 'arrays')


def diff(a, b):
    a, b = np.load(a), np.load(b)
    assert sorted(a.files) == sorted(b.files)
    bad = [k for k in a.files if not np.array_equal(a[k], b[k])]
    print('arrays', len(a.files), 'differing', bad)
    for k in bad:
        print(k, float(np.abs(a[k] - b[k]).max()), float(np.abs(a[k]).max()))
    return 1 if bad else 0


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(sys.argv[2], sys.argv[3])
    else:
        sys.exit(diff(sys.argv[2], sys.argv[3]))
