"""Records tests/golden/object_stage_parent.npz: every case of tests/object_stage_parent_cases.py through its six entry points on the
four handles, on the build in the tree.  Run on an MI355X from the repo root, ON A BUILD OF THE COMMIT WHOSE BEHAVIOUR IS TO BE KEPT, once:
    timeout -k 10 600 python scripts/make_golden_object_stage.py [out.npz]
The object kernels accumulate with atomics, so every (case, mode, entry) runs RUNS = 5 times.  The integers must be the same five times
(else the run stops: they could pin nothing).  A float array whose five hashes agree is stored as its hash; one whose hashes differ is
stored raw (the first run) with the largest element-wise spread over the five runs, max - min, measured here on this build; the replay
compares it element by element within four times that spread.  tests/test_gpu_object_stage_parent.py replays the file."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import object_stage_parent_cases as oc  # noqa: E402

RUNS = 5


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'object_stage_parent.npz')
    ints, hashes, data, loose = [], [], {}, []
    for mode in oc.MODES:
        u = oc.handle(mode)
        try:
            for case in oc.CASES:
                runs = [oc.run_case(u, case) for _ in range(RUNS)]
                for entry, first in runs[0].items():
                    key = '%s/%s/%s' % (case, mode, entry)
                    assert all(np.array_equal(r[entry]['ints'], first['ints']) for r in runs), (key, [r[entry]['ints'].tolist() for r in runs])
                    ints.append(first['ints'])
                    hashes.append(np.stack([oc.digest(first[name]) for name in oc.FLOATS]))
                    for name in oc.FLOATS:
                        if all(np.array_equal(oc.digest(r[entry][name]), oc.digest(first[name])) for r in runs):
                            continue
                        stack = np.stack([r[entry][name] for r in runs])
                        assert np.isfinite(stack).all(), key
                        spread = float((stack.max(axis=0) - stack.min(axis=0)).max())
                        data['%s/raw/%s' % (key, name)] = first[name]
                        data['%s/spread/%s' % (key, name)] = np.array(spread)
                        loose.append((key, name, spread))
                    print('%-44s ints %s' % (key, first['ints'].tolist()), flush=True)
        finally:
            u.close()
    assert len(ints) == len(oc.keys())
    np.savez_compressed(out, ints=np.array(ints, np.int32), hash=np.stack(hashes), **data)
    print('wrote', out, os.path.getsize(out), 'bytes; (case, array) pairs', len(ints) * len(oc.FLOATS), 'of which not the same bytes five times:', len(loose))
    for key, name, spread in loose:
        print('  by value: %-44s %-6s spread %.3e' % (key, name, spread))
    assert os.path.getsize(out) < 100 * 1024


if __name__ == '__main__':
    main()
