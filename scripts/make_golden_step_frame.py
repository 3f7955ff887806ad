"""Records tests/golden/step_frame_parent.npz: every stream of tests/step_frame_parent_cases.py through orcvio_msckf_io_step_frame /
_ex on the build in the tree, in the three launch forms (product, ORCVIO_STEP_FUSED=0 on the diagnostics build, ORCVIO_LA_SPIN=0).
Run on an MI355X from the repo root, ON A BUILD OF THE COMMIT WHOSE BEHAVIOUR IS TO BE KEPT, once:
    timeout -k 10 900 python scripts/make_golden_step_frame.py [out.npz]
Every stream runs twice on fresh handles; a stream that is not the same bytes both times is reported and left out (it could pin nothing).
tests/test_gpu_step_frame_parent.py replays the file."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import step_frame_parent_cases as sc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'step_frame_parent.npz')
    data, unstable = {}, []
    for name in sc.STREAMS:
        for mode in sc.MODES:
            t0 = time.time()
            a, b = sc.run_stream(name, mode), sc.run_stream(name, mode)
            same = all(np.array_equal(a[k], b[k]) for k in ('ints', 'hash'))
            ints = a['ints']
            print('%-18s %-8s frames %d  rc %s  first %s  prune %s  changes %s  repaired %s  n_after %s  %s  %.1f s' % (
                name, mode, len(ints), ints[:, 0].tolist(), ints[:, 1].tolist(), ints[:, 2].tolist(), ints[:, 3].tolist(), ints[:, 4].tolist(),
                ints[:, 5].tolist(), 'same twice' if same else 'DIFFERS BETWEEN TWO RUNS', time.time() - t0), flush=True)
            if not same:
                unstable.append((name, mode))
                continue
            data['%s/%s/ints' % (name, mode)] = a['ints']
            data['%s/%s/hash' % (name, mode)] = a['hash']
            if mode == 'product':
                data['%s/last_dx' % name] = a['last_dx']
                data['%s/last_diag' % name] = a['last_diag']
    np.savez_compressed(out, **data)
    print('wrote', out, os.path.getsize(out), 'bytes;', 'not reproducible:', unstable)
    assert os.path.getsize(out) < 100 * 1024


if __name__ == '__main__':
    main()
