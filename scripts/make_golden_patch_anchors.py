"""Records where integration/orcvio_msckf.patch anchors in the reference tree: for every hunk of the patch, its position and the
sha256 of the reference lines it replaces (its context), into tests/golden/integration_anchors.json.  tests/test_integration_patch.py
checks the patch against these digests, so the test needs the reference tree only when the fixture is made.

usage: python scripts/make_golden_patch_anchors.py <reference-tree>
Refuses to write the fixture if `git apply --check` does not accept the patch in that tree."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from test_integration_patch import PATCH, ANCHORS, _preimages  # noqa: E402


def main():
    ref = os.path.abspath(sys.argv[1])
    r = subprocess.run(['git', 'apply', '--check', '-p1', PATCH], cwd=ref, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit('the patch does not apply to %s:\n%s' % (ref, r.stdout + r.stderr))
    out = {}
    for path, hunks in _preimages().items():
        with open(os.path.join(ref, path), 'rb') as f:
            data = f.read()
        lines = data.decode().split('\n')
        rows = []
        for start, length, pre in hunks:
            text = '\n'.join(lines[start - 1:start - 1 + length])
            assert text == '\n'.join(pre), (path, start)
            rows.append(dict(old_start=start, old_len=length, sha256=hashlib.sha256(text.encode()).hexdigest()))
        out[path] = dict(file_sha256=hashlib.sha256(data).hexdigest(), lines=len(lines), hunks=rows)
    with open(ANCHORS, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('anchors ->', os.path.relpath(ANCHORS, ROOT))


if __name__ == '__main__':
    main()
