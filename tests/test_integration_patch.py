"""integration/orcvio_msckf.patch: the call-site patch INTEGRATION.md describes, as a file that applies.  Its anchors
-- src/orcvio.cpp :2154-2193 removeLostObjects, :2497-2560 removeLostFeatures, :2803-2851 pruneImuStateBuffer,
include/orcvio/orcvio.h:200-214, CMakeLists.txt -- must still match the reference text: tests/golden/integration_anchors.json holds
the position of every hunk in the reference tree and the sha256 of the reference lines there (scripts/make_golden_patch_anchors.py
records it from a reference tree, after `git apply --check` accepted the patch there), so the check needs no copy of the reference.
Everything the patch adds to the C++ sources sits inside #ifdef ORCVIO_USE_AMD_MSCKF, so the reference builds and behaves as before
without the definition, and it names only entry points include/orcvio_msckf.h declares."""
import hashlib
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, 'integration', 'orcvio_msckf.patch')
ANCHORS = os.path.join(ROOT, 'tests', 'golden', 'integration_anchors.json')


def _hunks():
    files, cur = {}, None
    for line in open(PATCH).read().splitlines():
        if line.startswith('+++ '):
            cur = line[4:].split('\t')[0]
            cur = cur[2:] if cur.startswith('b/') else cur
            files[cur] = []
        elif line.startswith('--- ') or line.startswith('@@'):
            if cur is not None and line.startswith('@@'):
                files[cur].append([])
        elif cur is not None and files[cur]:
            files[cur][-1].append(line)
    return files


def test_patch_touches_the_three_call_sites_and_nothing_else():
    files = _hunks()
    assert set(files) == {'CMakeLists.txt', 'include/orcvio/orcvio.h', 'src/orcvio.cpp'}
    added = '\n'.join(l[1:] for h in files['src/orcvio.cpp'] for l in h if l.startswith('+'))
    for name in ('gpuFeatureUpdate(msckf_feature_ids, nullptr)', 'gpuFeatureUpdate(used_IDs, &rm_imu_state_ids)', 'gpuObjectUpdate(H_x, H_f, res)'):
        assert name in added, name
    # no line of the reference is removed: the reference path stays, behind the #else
    assert not any(l.startswith('-') for hs in files.values() for h in hs for l in h if isinstance(l, str) and len(l) > 0)


def test_everything_added_to_the_sources_is_behind_the_definition():
    files = _hunks()
    for f in ('include/orcvio/orcvio.h', 'src/orcvio.cpp'):
        for h in files[f]:
            depth = 0
            for l in h:
                if not l.startswith('+'):
                    assert depth == 0 or l.strip() in ('', ' '), (f, l)   # (context lines sit outside the guarded blocks)
                    continue
                t = l[1:].strip()
                if t.startswith('#ifdef ORCVIO_USE_AMD_MSCKF'):
                    depth += 1
                elif t.startswith('#endif'):
                    depth -= 1
                    assert depth >= 0
                else:
                    assert depth > 0 or t == '', (f, l)
            assert depth == 0, f


def test_patch_calls_only_declared_entry_points():
    header = open(os.path.join(ROOT, 'include', 'orcvio_msckf.h')).read()
    declared = set(re.findall(r'\b(orcvio_msckf_\w+)\s*\(', header)) | set(re.findall(r'\b(orcvio_msckf_\w+)\b', header))
    used = set(re.findall(r'\b(orcvio_msckf_\w+)\b', '\n'.join(l[1:] for l in open(PATCH).read().splitlines() if l.startswith('+') and not l.startswith('+++'))))
    used -= {'orcvio_msckf_h'}
    lib_names = {u for u in used if not u.endswith('.so')}
    assert lib_names <= declared | {'orcvio_msckf'}, lib_names - declared


def _preimages():
    """{file: [(old_start, old_len, the lines the hunk expects there)]} -- what `git apply` looks for in the tree it patches."""
    files, cur, left = {}, None, 0
    for line in open(PATCH).read().splitlines():
        if left > 0 and line[:1] in (' ', '-', ''):   # (a hunk's own lines: context and removed lines, counted by its header)
            files[cur][-1][2].append(line[1:])
            left -= 1
        elif line.startswith('+++ '):
            cur = line[4:].split('\t')[0]
            cur = cur[2:] if cur.startswith('b/') else cur
            files[cur] = []
        elif line.startswith('@@') and cur is not None:
            m = re.match(r'@@ -(\d+)(?:,(\d+))? \+', line)
            left = int(m.group(2) or 1)
            files[cur].append((int(m.group(1)), left, []))
    return files


def test_patch_applies_to_the_reference_tree(tmp_path):
    """Every hunk's context is the reference text at the recorded position (sha256), and `git apply --check` accepts the patch on a
    stand-in tree that holds exactly that text there (hunk headers, line counts, order)."""
    anchors = json.load(open(ANCHORS))
    pre = _preimages()
    assert set(pre) == set(anchors)
    for path, hunks in pre.items():
        rec = anchors[path]['hunks']
        assert [(h['old_start'], h['old_len']) for h in rec] == [(s, n) for s, n, _ in hunks], path
        lines = ['/* stand-in line %d */' % (i + 1) for i in range(anchors[path]['lines'])]
        for (start, n, body), h in zip(hunks, rec):
            assert len(body) == n, (path, start)
            assert hashlib.sha256('\n'.join(body).encode()).hexdigest() == h['sha256'], (path, start, 'context differs from the reference')
            lines[start - 1:start - 1 + n] = body
        os.makedirs(os.path.dirname(os.path.join(tmp_path, path)), exist_ok=True)
        with open(os.path.join(tmp_path, path), 'w') as f:
            f.write('\n'.join(lines))
    r = subprocess.run(['git', 'apply', '--check', '-p1', '--verbose', PATCH], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
