"""The bookkeeping of the fused zero-velocity update that writes only what stays (orcvio_amd/csrc/host/cov_book.hpp: zupt_keep,
zupt_keep_done) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU
(tests/cpp/test_cov_book_zupt_keep.cpp): applied with and without a following factor, a factor too wide, not applied with the
prior's tail standing, F = 0, the buffers never aliasing."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_fused_update_keeps_or_drops_the_factor_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'test_cov_book_zupt_keep')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_cov_book_zupt_keep.cpp')])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'cov book zupt keep ok' in out.stdout
