"""Compares the gfx950 code objects of two builds of the library, kernel by kernel:
    python scripts/compare_code_objects.py PARENT.so RESULT.so [out.txt]
Every function of the device code is disassembled (llvm-objdump) and compared as its instruction stream with encodings, addresses and
comment lines stripped; the resource table (VGPRs, SGPRs, scratch, LDS, kernarg bytes per kernel, from the code object's metadata
note) is compared and written out.  Exit status 1 if anything differs.  No device needed."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')


def code_object(lib, tmp):
    fat, co = os.path.join(tmp, 'fat.bin'), os.path.join(tmp, os.path.basename(lib) + '.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', lib, fat])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', '--unbundle', '--input=' + fat,
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co])
    return co


def functions(co):
    """{symbol: [instruction with its encoding, ...]}"""
    text = subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-leading-addr', co], text=True)
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r'^(?:[0-9a-f]+ )?<(.+)>:$', ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.strip() and not ln.lstrip().startswith(('//', ';')):
            cur.append(re.sub(r'\s+', ' ', re.sub(r'//\s*[0-9A-Fa-f]+:', '//', ln)).strip())
    return out


def resources(co):
    """{kernel: (vgpr, sgpr, scratch bytes, lds bytes, kernarg bytes)}"""
    note = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    out = {}
    for blk in re.split(r'\n\s+- \.agpr_count:', note)[1:]:
        get = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        out[re.search(r'\.name:\s+(\S+)', blk).group(1)] = (get('vgpr_count'), get('sgpr_count'), get('private_segment_fixed_size'),
                                                           get('group_segment_fixed_size'), get('kernarg_segment_size'))
    return out


def main():
    parent, result = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ca, cb = code_object(parent, ta), code_object(result, tb)
        fa, fb, ra, rb = functions(ca), functions(cb), resources(ca), resources(cb)
    lines = ['%s against %s: %d / %d functions, %d / %d kernels' % (parent, result, len(fa), len(fb), len(ra), len(rb))]
    bad = sorted(set(fa) ^ set(fb)) + sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
    bad_res = sorted(set(ra) ^ set(rb)) + sorted(k for k in set(ra) & set(rb) if ra[k] != rb[k])
    lines.append('instruction streams that differ: %s' % (bad or 'none'))
    lines.append('resource lines that differ: %s' % (bad_res or 'none'))
    lines.append('%-100s %5s %5s %8s %7s %8s' % ('kernel (result)', 'VGPR', 'SGPR', 'scratch', 'LDS', 'kernarg'))
    for k in sorted(rb):
        lines.append('%-100s %5d %5d %8d %7d %8d' % ((k[:100],) + rb[k]))
    text = '\n'.join(lines) + '\n'
    if len(sys.argv) > 3:
        with open(sys.argv[3], 'w') as f:
            f.write(text)
    print('\n'.join(lines[:3]))
    sys.exit(1 if bad or bad_res else 0)


if __name__ == '__main__':
    main()
